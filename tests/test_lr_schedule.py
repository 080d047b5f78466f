"""``lr_schedule`` on the CPU engine: the adaptive rule (ops/oracle.lr_adapt) against a hand-worked table, the linear
formula, the torch worker against hand-driven grad / apply loops, the record's fields, refusals, the CLI flags,
resume and a 2-rank gloo run.  Shapes: tests/test_target_kl.py.

The engineered rates (seed 3, ``dppo`` preset, HalfCheetah-v2 48 x 6 full batch, ``lr_kl_target`` 0.008, so the
thresholds are 0.016 and 0.004).  The hand-driven adaptive loop's per-step KL of the first iteration:

    lr 3e-3   kl = 0, 4.1e-2, 8.0e-2, 9.2e-2, ...: up at step 0 (the first KL of an iteration is 0), down from step 1 on
    lr 1e-6   every kl below 2.5e-5: up at every step

``assert_lr_margin`` holds every probed KL a factor 1.5 away from both thresholds: the worker and the hand loop are
two paths of one engine and agree bit for bit, so the margin only keeps the predicted steps from depending on the
last bits of a BLAS (relative differences of 1e-6 between machines, far inside 1.5).
"""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from pytorch_dppo_amd.config import Params, dppo_preset, params_from_args
from pytorch_dppo_amd.ops import oracle
from pytorch_dppo_amd.parallel.dist import DistContext
from pytorch_dppo_amd.runtime.launcher import free_port, run_worker
from pytorch_dppo_amd.runtime.worker import DPPOWorker
from test_target_kl import CHEETAH, PENDULUM_MB, ROOT, cpu_worker, same_floats

F = np.float32
NAN = float("nan")
T = 0.008
HI, LO = float(F(2) * F(T)), float(F(0.5) * F(T))          # the thresholds as the kernel forms them
ADAPT = dict(lr_schedule="adaptive", lr_kl_target=T)
LR_HIGH, LR_TINY = 3e-3, 1e-6
MARGIN = 1.5


def f(x):
    return float(F(x))


# (lr, kl, kl_target, factor, lr_min, lr_max) -> lr'; the expected values are worked out by hand in numpy float32
LR_TABLE = [
    ((3e-4, 0.02, T, 1.5, 1e-6, 1e-2), f(F(3e-4) / F(1.5))),                       # above 2 x target: down
    ((3e-4, 0.001, T, 1.5, 1e-6, 1e-2), f(F(3e-4) * F(1.5))),                      # below half: up
    ((3e-4, 0.008, T, 1.5, 1e-6, 1e-2), f(3e-4)),                                  # in between
    ((3e-4, HI, T, 1.5, 1e-6, 1e-2), f(3e-4)),                                     # exactly 2 x target: unchanged
    ((3e-4, LO, T, 1.5, 1e-6, 1e-2), f(3e-4)),                                     # exactly half: unchanged
    ((3e-4, float(np.nextafter(F(HI), F(1))), T, 1.5, 1e-6, 1e-2), f(F(3e-4) / F(1.5))),   # the float above: down
    ((3e-4, float(np.nextafter(F(LO), F(0))), T, 1.5, 1e-6, 1e-2), f(F(3e-4) * F(1.5))),   # the float below: up
    ((1.2e-6, 1.0, T, 1.5, 1e-6, 1e-2), f(1e-6)),                                  # the clamp at lr_min
    ((9e-3, 0.0, T, 1.5, 1e-6, 1e-2), f(1e-2)),                                    # the clamp at lr_max
    ((3e-4, NAN, T, 1.5, 1e-6, 1e-2), f(3e-4)),                                    # a NaN: unchanged
    ((3e-4, -1e-9, T, 1.5, 1e-6, 1e-2), f(F(3e-4) * F(1.5))),                      # a tiny negative first KL: up
    ((7e-4, 0.05, 0.01, 2.0, 1e-5, 1e-3), f(F(7e-4) / F(2))),                      # other operands
    ((1e-3, 1.0, T, 3.0, 1e-6, 1e-2), f(F(1e-3) / F(3))),                          # a divide that rounds
]
LR_DIRS = [-1, 1, 0, 0, 0, -1, 1, -1, 1, 0, 1, -1, -1]


@pytest.mark.parametrize("case", range(len(LR_TABLE)))
def test_oracle_lr_adapt_table(case):
    args, want = LR_TABLE[case]
    got = oracle.lr_adapt(*args)
    assert same_floats([got], [want]), (got, want)
    assert same_floats([oracle.lr_adapt(torch.tensor(args[0]), torch.tensor(args[1]), *args[2:])], [want])
    assert oracle.lr_adapt_dir(args[1], args[2]) == LR_DIRS[case]


# ---- the linear rate ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("frac", [0.0, 0.1])
@pytest.mark.parametrize("bound", ["max_iters", "total_env_steps"])
def test_linear_rate_formula(frac, bound):
    n = 7
    kw = dict(max_iters=n) if bound == "max_iters" else dict(total_env_steps=288 * 2 * (n - 1) + 5)
    p = dppo_preset(lr=3e-4, lr_schedule="linear", lr_final_frac=frac, **dict(CHEETAH, **kw))
    world = 1 if bound == "max_iters" else 2
    assert p.schedule_iters(world) == n
    for i, want in ((0, 3e-4), (1, 3e-4 * (1 - (1 - frac) * 1 / 7)), (n - 1, 3e-4 * (1 - (1 - frac) * 6 / 7)),
                    (n, 3e-4 * frac), (n + 5, 3e-4 * frac)):
        assert p.linear_lr(i, world) == pytest.approx(want, rel=1e-12, abs=1e-30)
    assert p.linear_lr(0, world) == 3e-4 and p.linear_lr(n, world) == 3e-4 * (1.0 - (1.0 - frac))


# ---- hand-driven loops -----------------------------------------------------------------------------------------
def hand_iterations(w, iters, rate_of=None, adapt=None, gate_target=float("inf")):
    """``iters`` iterations of worker ``w`` (schedule constant) driven by hand through the engine's phases: grad /
    apply at the rate this loop sets / oracle.kl_gate / oracle.lr_adapt.  ``rate_of(i)``: the rate of iteration i
    (linear); ``adapt``: dict(lr, kl_target, factor, lr_min, lr_max), the rate persists over the iterations.
    Returns [(iteration, step, kl, rate the step ran at, applied)]."""
    p, eng = w.p, w.engine
    lr = f(adapt["lr"]) if adapt else None
    log = []
    for _ in range(iters):
        w.init_stats()
        ro = eng.rollout()
        w._merge_stats(ro["count"], ro["s1"], ro["s2"], ro["shift"], count_uniform=True)
        eng.values()
        eng.gae()
        if rate_of is not None:
            eng.lr = rate_of(w.iteration)
        eng.begin_update()
        N, mb, nmb = w._minibatch_plan()
        w._perm_gen.manual_seed((p.seed * 1000003 + w.ctx.rank * 7919 + w.iteration) & 0x7FFFFFFF)
        gate, s = [0.0, 0.0, 0.0, 0.0], 0
        for epoch in range(p.num_epoch):
            perm = None if (mb >= N and nmb == 1) else torch.randperm(N, generator=w._perm_gen)
            for b in range(nmb):
                idx = None if perm is None else perm[(b * mb) % N:(b * mb) % N + mb]
                eng.grad(idx)
                if adapt:
                    eng.lr = lr
                    if gate[0] == 0.0:
                        eng.apply()
                    M = float(mb)
                    kl_sum = float(F(eng._last["approx_kl"]) * F(M))
                    gate, applied = oracle.kl_gate(kl_sum, M, gate_target, gate)
                    log.append((w.iteration, s, gate[3], lr, applied))
                    if applied:
                        lr = oracle.lr_adapt(lr, gate[3], adapt["kl_target"], adapt["factor"], adapt["lr_min"],
                                             adapt["lr_max"])
                else:
                    eng.apply()
                    log.append((w.iteration, s, eng._last["approx_kl"], eng.lr, True))
                s += 1
        w.iteration += 1
    return log, lr


def adapt_of(p):
    return dict(lr=p.lr, kl_target=p.lr_kl_target, factor=p.lr_adapt_factor, lr_min=p.lr_min, lr_max=p.lr_max)


def assert_lr_margin(kls, target=T):
    """every probed KL is a factor MARGIN away from both thresholds: the decisions do not hang on last bits"""
    for k in kls:
        for thr in (2 * target, 0.5 * target):
            assert k <= thr / MARGIN or k >= thr * MARGIN, (k, thr)


def same_engine_state(a, b):
    return (torch.equal(a.model.flat.data, b.model.flat.data) and torch.equal(a.engine.adam_m, b.engine.adam_m)
            and torch.equal(a.engine.adam_v, b.engine.adam_v) and a.engine.adam_step == b.engine.adam_step)


@pytest.mark.parametrize("shape", ["cheetah", "pendulum_minibatch"])
def test_adaptive_worker_equals_hand_loop(shape):
    kw = dict({"cheetah": CHEETAH, "pendulum_minibatch": PENDULUM_MB}[shape], num_epoch=4)
    w = cpu_worker(**ADAPT, **kw)
    ms = [w.iteration_step(), w.iteration_step()]
    ref = cpu_worker(**kw)
    log, lr = hand_iterations(ref, 2, adapt=adapt_of(w.p))
    assert same_engine_state(w, ref)
    assert same_floats([w.engine.lr], [lr]) and same_floats([w.engine.lr_state[0]], [lr])
    # the rate persists over the boundary: iteration 1's first step ran at the rate iteration 0 left
    first1 = next(e for e in log if e[0] == 1)
    last0 = [e for e in log if e[0] == 0][-1]
    assert first1[3] == oracle.lr_adapt(last0[3], last0[2], T, 1.5, 1e-6, 1e-2) != f(w.p.lr)
    downs = sum(oracle.lr_adapt_dir(e[2], T) < 0 for e in log)
    ups = sum(oracle.lr_adapt_dir(e[2], T) > 0 for e in log)
    assert ms[1]["lr"] == lr and ms[1]["lr_downs"] == downs and ms[1]["lr_ups"] == ups and ups >= 2
    assert ms[1]["kl_stopped"] is False and ms[1]["steps_applied"] == len(log) // 2 and ms[1]["updates"] == len(log)


_probe = {}


def probe(lr):
    """the hand-driven adaptive loop's first iteration at initial rate ``lr`` (once per rate)"""
    if lr not in _probe:
        ref = cpu_worker(lr=lr, **CHEETAH)
        p = dppo_preset(lr=lr, **ADAPT, **CHEETAH)
        _probe[lr] = (hand_iterations(ref, 1, adapt=adapt_of(p)), ref)
    return _probe[lr]


def test_engineered_high_rate_goes_down_at_the_predicted_steps():
    (log, lr_end), ref = probe(LR_HIGH)
    kls = [e[2] for e in log]
    print("kl", ["%.3e" % k for k in kls], "rates", ["%.3e" % e[3] for e in log])
    assert_lr_margin(kls)
    dirs = [oracle.lr_adapt_dir(k, T) for k in kls]
    assert dirs[0] == 1 and dirs[1] == -1 and dirs.count(-1) >= 2       # the first KL of an iteration is 0
    w = cpu_worker(lr=LR_HIGH, **ADAPT, **CHEETAH)
    rates = []
    orig = w.engine.apply

    def apply(extra=0.0):
        rates.append(w.engine.lr)
        return orig(extra)
    w.engine.apply = apply
    m = w.iteration_step()
    assert rates == [e[3] for e in log]                                  # every step ran at the predicted rate
    for s in range(len(log) - 1):
        want = {1: min(f(F(rates[s]) * F(1.5)), f(1e-2)), -1: max(f(F(rates[s]) / F(1.5)), f(1e-6)), 0: rates[s]}[dirs[s]]
        assert rates[s + 1] == want, s
    assert m["lr"] == lr_end < f(LR_HIGH) and m["lr_downs"] == dirs.count(-1) and m["lr_ups"] == dirs.count(1)
    assert same_engine_state(w, ref)


def test_engineered_tiny_rate_goes_up():
    (log, lr_end), ref = probe(LR_TINY)
    kls = [e[2] for e in log]
    print("kl", ["%.3e" % k for k in kls])
    assert_lr_margin(kls)
    assert all(oracle.lr_adapt_dir(k, T) == 1 for k in kls)
    w = cpu_worker(lr=LR_TINY, **ADAPT, **CHEETAH)
    m = w.iteration_step()
    want = f(LR_TINY)
    for _ in range(10):
        want = f(F(want) * F(1.5))
    assert m["lr"] == want == lr_end and m["lr_ups"] == 10 and m["lr_downs"] == 0
    assert same_engine_state(w, ref)


def test_adaptive_with_target_kl_the_tripping_step_adapts_the_stopped_do_not():
    (log, _), _ = probe(LR_HIGH)
    kls = [e[2] for e in log]
    # a gate target between the KLs of steps 1 and 2 of the probe (4.1e-2 and 8.0e-2: their geometric mean leaves a
    # factor 1.3 on both sides, against last-bit differences of 1e-6): step 2 trips
    target_kl = math.sqrt(kls[1] * kls[2])
    assert kls[1] * 1.3 <= target_kl <= kls[2] / 1.3 and kls[2] >= HI * MARGIN
    w = cpu_worker(lr=LR_HIGH, target_kl=target_kl, **ADAPT, **CHEETAH)
    m = w.iteration_step()
    ref = cpu_worker(lr=LR_HIGH, **CHEETAH)
    p = dppo_preset(lr=LR_HIGH, **ADAPT, **CHEETAH)
    glog, lr_end = hand_iterations(ref, 1, adapt=adapt_of(p), gate_target=target_kl)
    assert [e[4] for e in glog] == [True] * 3 + [False] * 7
    assert same_engine_state(w, ref) and w.engine.adam_step == 3
    assert m["kl_stopped"] is True and m["steps_applied"] == 3
    # three decisions: up (kl 0), down, down (the tripping step) - and nothing from the seven stopped steps
    assert m["lr_ups"] == 1 and m["lr_downs"] == 2 and m["lr"] == lr_end
    assert m["lr"] == f(F(f(F(f(F(LR_HIGH) * F(1.5))) / F(1.5))) / F(1.5))


def test_nan_kl_stops_the_iteration_and_leaves_the_rate():
    w = cpu_worker(**ADAPT, **CHEETAH)
    orig = w.engine.grad
    calls = []

    def grad(idx):
        out = orig(idx)
        calls.append(1)
        if len(calls) == 3:
            w.engine.kl_pair = torch.tensor([NAN, 288.0])
        return out
    w.engine.grad = grad
    m = w.iteration_step()
    assert m["kl_stopped"] is True and m["steps_applied"] == 3 and math.isnan(m["kl_trip"])
    assert m["lr_ups"] + m["lr_downs"] <= 2        # the NaN step and the stopped steps decided nothing


# ---- linear / constant ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("frac", [0.0, 0.1])
def test_linear_worker_equals_hand_loop_fed_the_formula(frac):
    kw = dict(CHEETAH, num_epoch=2, max_iters=3)
    w = cpu_worker(lr_schedule="linear", lr_final_frac=frac, **kw)
    ms = [w.iteration_step() for _ in range(3)]
    ref = cpu_worker(**kw)
    rate = lambda i: 3e-4 * (1.0 - (1.0 - frac) * min(i, 3) / 3)     # noqa: E731
    hand_iterations(ref, 3, rate_of=rate)
    assert same_engine_state(w, ref)
    assert [m["lr"] for m in ms] == [rate(0), rate(1), rate(2)] and rate(2) < rate(0)
    assert "lr_downs" not in ms[0] and "kl_stopped" not in ms[0] and w.engine.gate is None
    const = cpu_worker(**kw)
    for _ in range(3):
        const.iteration_step()
    assert not torch.equal(const.model.flat.data, w.model.flat.data)


def test_constant_is_the_flag_omitted_bit_for_bit():
    off, on = cpu_worker(**CHEETAH), cpu_worker(lr_schedule="constant", **CHEETAH)
    for _ in range(2):
        m0, m1 = off.iteration_step(), on.iteration_step()
    assert same_engine_state(off, on)
    assert m0["loss"] == m1["loss"] and m0["grad_norm"] == m1["grad_norm"]
    assert not any(k in m1 for k in ("lr", "lr_downs", "lr_ups", "kl_stopped"))
    assert on.engine.lr_state is None and on.engine.gate is None


# ---- refusals, CLI ---------------------------------------------------------------------------------------------
def test_refusals():
    with pytest.raises(ValueError, match="lr_schedule must be"):
        Params(lr_schedule="cosine")
    with pytest.raises(ValueError, match="max_iters or total_env_steps"):
        Params(lr_schedule="linear")
    Params(lr_schedule="linear", max_iters=3)
    Params(lr_schedule="linear", total_env_steps=10 ** 6, loss="dppo_ref", compat=True, overlap_rollout=True,
           overlap_value_epochs=True, target_kl=0.0)
    Params(lr_schedule="linear", max_iters=3, target_kl=0.01)
    for bad in (dict(lr_kl_target=0.0), dict(lr_kl_target=-1.0), dict(lr_kl_target=NAN), dict(lr_adapt_factor=1.0),
                dict(lr_adapt_factor=0.5), dict(lr_min=1e-2, lr_max=1e-3), dict(lr=1e-1), dict(lr=1e-7),
                dict(lr_min=0.0)):
        with pytest.raises(ValueError, match="lr_"):
            Params(lr_schedule="adaptive", **bad)
    with pytest.raises(ValueError, match="dppo_ref"):
        Params(lr_schedule="adaptive", loss="dppo_ref")
    with pytest.raises(ValueError, match="compat"):
        Params(lr_schedule="adaptive", compat=True)
    with pytest.raises(ValueError, match="overlap_rollout"):
        Params(lr_schedule="adaptive", overlap_rollout=True)
    with pytest.raises(ValueError, match="overlap_value_epochs"):
        Params(lr_schedule="adaptive", overlap_value_epochs=True)
    # the adaptive operands are not checked while the schedule is off; everything else composes
    Params(lr_adapt_factor=0.5, lr_min=1.0, lr=5.0)
    p = Params(lr_schedule="adaptive", target_kl=0.02, reward_norm=True, bootstrap_time_limit=True, normalize_adv=True,
               max_grad_norm=0.5, fused_apply=False, grad_comm="process_group", update_kernels="tile", dtype="fp8",
               grad_reduce="mean")
    assert p.gated() and p.gate_target() == 0.02 and Params(lr_schedule="adaptive").gate_target() == float("inf")
    assert not Params().gated() and Params(target_kl=0.01).gated()


def test_cli_flags():
    p = params_from_args([])
    assert (p.lr_schedule, p.lr_final_frac, p.lr_kl_target, p.lr_adapt_factor, p.lr_min, p.lr_max) == \
        ("constant", 0.0, 0.008, 1.5, 1e-6, 1e-2)
    p = params_from_args(["--lr-schedule", "adaptive", "--lr-kl-target", "0.01", "--lr-adapt-factor", "2", "--lr-min",
                          "1e-5", "--lr-max", "1e-3"])
    assert (p.lr_schedule, p.lr_kl_target, p.lr_adapt_factor, p.lr_min, p.lr_max) == ("adaptive", 0.01, 2.0, 1e-5, 1e-3)
    assert Params.from_dict(p.to_dict()).lr_schedule == "adaptive"
    p = params_from_args(["--lr-schedule", "linear", "--lr-final-frac", "0.1", "--max-iters", "5"])
    assert p.lr_schedule == "linear" and p.lr_final_frac == 0.1
    with pytest.raises(ValueError):
        params_from_args(["--lr-schedule", "linear"])
    with pytest.raises(ValueError):
        params_from_args(["--lr-schedule", "adaptive", "--overlap-rollout", "true"])


# ---- checkpoints ---------------------------------------------------------------------------------------------
def _run(stop_after=None, **kw):
    """a 3-iteration run (the bound the linear rate anneals to), stopped after ``stop_after`` iterations"""
    base = dict(num_processes=1, num_epoch=3, max_iters=3, **CHEETAH)
    base.update(kw)
    return run_worker(dppo_preset(**base), DistContext(), max_iters=stop_after, evaluator=False, quiet=True)[0]


@pytest.mark.parametrize("schedule", ["adaptive", "linear"])
def test_resume_is_bit_identical(tmp_path, schedule):
    kw = dict(lr_schedule=schedule, lr_final_frac=0.1, lr=LR_HIGH if schedule == "adaptive" else 3e-4)
    ck = str(tmp_path / "ck")
    w_full = _run(**kw)
    w_two = _run(stop_after=2, checkpoint_dir=ck, **kw)
    assert w_two.iteration == 2
    st = torch.load(os.path.join(ck, "trainer_state.pt"), weights_only=True)
    assert ("lr_state" in st) == (schedule == "adaptive")
    if schedule == "adaptive":
        assert same_floats(st["lr_state"].tolist(), w_two.engine.lr_state) and st["lr_state"][0] != f(LR_HIGH)
        assert st["lr_state"].dtype == torch.float32 and st["lr_state"].numel() == 4
    # the rate is a function of the iteration index and the run's bound: the resumed run continues on the same line
    w_res = _run(resume=ck, checkpoint_dir="", **kw)
    assert w_res.iteration == 3 and same_engine_state(w_full, w_res)
    assert w_res.last_metrics["lr"] == w_full.last_metrics["lr"]
    if schedule == "adaptive":
        assert same_floats(w_res.engine.lr_state, w_full.engine.lr_state)
        assert w_res.last_metrics["lr_downs"] == w_full.last_metrics["lr_downs"] > 0
    else:
        assert w_full.last_metrics["lr"] == 3e-4 * (1.0 - 0.9 * 2 / 3)


def test_train_py_logs_the_fields(tmp_path):
    path, csv = tmp_path / "train.jsonl", tmp_path / "train.csv"
    cmd = [sys.executable, "train.py", "--env-name", "HalfCheetah-v2", "--max-iters", "2", "--num-processes", "1",
           "--num-envs", "48", "--exploration-size", "288", "--batch-size", "288", "--seed", "3", "--lr-schedule",
           "adaptive", "--num-epoch", "3", "--log-jsonl", str(path), "--log-csv", str(csv)]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=170)
    assert r.returncode == 0, r.stderr[-3000:]
    recs = [json.loads(l) for l in path.read_text().splitlines()]
    assert len(recs) == 2
    for rec in recs:
        assert 1e-6 <= rec["lr"] <= 1e-2 and rec["lr_ups"] >= 1 and rec["lr_downs"] >= 0
        assert rec["kl_stopped"] is False and rec["steps_applied"] == 3 and rec["kl_trip"] is None
    assert recs[1]["lr_ups"] >= recs[0]["lr_ups"] and recs[1]["updates"] == 6
    head = csv.read_text().splitlines()[0]
    assert not any(k in head.split(",") for k in ("lr", "lr_downs", "lr_ups", "kl_stopped"))   # the CSV columns are fixed
    assert "lr_ups" not in r.stdout and "lr_downs" not in r.stdout


# ---- two ranks -----------------------------------------------------------------------------------------------
def _rank_main(rank, world, port, out_dir):
    from pytorch_dppo_amd.parallel.dist import init_distributed
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.set_num_threads(1)
    ctx = init_distributed("cpu", rank=rank, world_size=world, timeout_s=60.0)
    kw = dict(CHEETAH, num_processes=world, verify_sync_every=1, num_epoch=4, lr=LR_HIGH, **ADAPT)
    w = DPPOWorker(dppo_preset(**kw), ctx)
    ms = [w.iteration_step(), w.iteration_step()]
    torch.save({"lr_state": list(w.engine.lr_state), "lr": [m["lr"] for m in ms], "downs": ms[1]["lr_downs"],
                "ups": ms[1]["lr_ups"], "in_sync": all(bool(m["replicas_in_sync"]) for m in ms),
                "flat": w.model.flat.data.clone(), "rewards": w.engine.rewards.clone()},
               os.path.join(out_dir, f"r{rank}.pt"))
    ctx.destroy()


@pytest.mark.slow
def test_two_ranks_keep_one_rate(tmp_path):
    import torch.multiprocessing as mp
    port = free_port()
    mpc = mp.get_context("spawn")
    procs = [mpc.Process(target=_rank_main, args=(r, 2, port, str(tmp_path))) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(240)
    for p in procs:
        if p.is_alive():
            p.terminate()
    assert [p.exitcode for p in procs] == [0, 0]
    r0 = torch.load(tmp_path / "r0.pt", weights_only=True)
    r1 = torch.load(tmp_path / "r1.pt", weights_only=True)
    assert not torch.equal(r0["rewards"], r1["rewards"])                           # per-rank seeds: different data
    assert same_floats(r0["lr_state"], r1["lr_state"]) and r0["lr"] == r1["lr"]
    assert r0["downs"] == r1["downs"] > 0 and r0["ups"] == r1["ups"] >= 2
    assert r0["in_sync"] and r1["in_sync"] and torch.equal(r0["flat"], r1["flat"])
