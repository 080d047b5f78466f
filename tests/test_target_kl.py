"""``target_kl`` on the CPU engine: the gate (ops/oracle.kl_gate) against a table, the torch worker against a
hand-driven grad / apply loop, the record's fields, refusals, the CLI flag, resume and a 2-rank gloo run.

The shapes of the engine comparisons (seed 3, ``dppo`` preset), the CPU engine's per-step KL of the first
iteration and the targets:

    HalfCheetah-v2 48 x 6 full batch   kl = 0, 4.011e-4, 1.625e-3   target 8.07e-4   trip at step 2, 3 applied
    Humanoid-v2   256 x 8 full batch   kl = 0, 1.207e-3, 4.895e-3   target 2.43e-3   trip at step 2, 3 applied

Where two engines are compared the reference's own sequence must leave a factor >= 2 on both sides of the target
(``assert_margin``).  kl_2 / kl_1 is 4.05 at both shapes, so only targets within 0.7 % of the geometric mean of
kl_1 and kl_2 do: the targets are those means to three digits.  (The round figures 8e-4 and 2.4e-3 put kl_1 =
4.011e-4 / 1.207e-3 just above target / 2 = 4.000e-4 / 1.200e-3 and fail the factor-2 rule on the low side.)
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHEETAH = dict(env_name="HalfCheetah-v2", num_envs=48, exploration_size=48 * 6, batch_size=48 * 6, seed=3)
HUMANOID = dict(env_name="Humanoid-v2", num_envs=256, exploration_size=256 * 8, batch_size=256 * 8, seed=3)
PENDULUM_MB = dict(env_name="Pendulum-v0", num_envs=64, exploration_size=64 * 16, batch_size=256, seed=3)
TABLE_TARGET = {"HalfCheetah-v2": 8.07e-4, "Humanoid-v2": 2.43e-3}

# ---- the gate ------------------------------------------------------------------------------------------------
F = np.float32
T01 = float(F(0.01))                       # the target as the kernel sees it
ABOVE = float(np.nextafter(F(0.01), F(1)))
NAN = float("nan")
# (kl sum, count, target, gate before) -> (gate after, applied); the expected values are worked out by hand in
# numpy float32, not by the function under test
GATE_TABLE = [
    # kl == target does not trip
    ((T01, 1.0, 0.01, [0, 0, 0, 0]), ([0, 1, 0, T01], True)),
    # the float just above it does
    ((ABOVE, 1.0, 0.01, [0, 4, 0, 0.003]), ([1, 5, ABOVE, ABOVE], True)),
    # a NaN trips
    ((NAN, 288.0, 0.01, [0, 0, 0, 0]), ([1, 1, NAN, NAN], True)),
    # a count of 0 gives kl 0 (no 0 / 0)
    ((0.0, 0.0, 0.01, [0, 2, 0, 0.004]), ([0, 3, 0, 0.0], True)),
    # a tiny negative first KL (rounding of (ratio - 1) - log ratio) does not trip
    ((float(F(-1e-9) * F(64)), 64.0, 0.01, [0, 0, 0, 0]), ([0, 1, 0, float(F(F(-1e-9) * F(64)) / F(64))], True)),
    # a quotient: fl32(0.9 / 300) = 0.003 stays under, fl32(3.3 / 300) = 0.011 trips
    ((0.9, 300.0, 0.01, [0, 1, 0, 0]), ([0, 2, 0, float(F(0.9) / F(300))], True)),
    ((3.3, 300.0, 0.01, [0, 1, 0, 0]), ([1, 2, float(F(3.3) / F(300)), float(F(3.3) / F(300))], True)),
    # a set stop stays set under a small KL, and applies nothing
    ((0.3, 300.0, 0.01, [1, 3, float(F(0.02)), float(F(0.02))]), ([1, 3, float(F(0.02)), float(F(0.3) / F(300))], False)),
    # ... and under a NaN
    ((NAN, 300.0, 0.01, [1, 3, float(F(0.02)), 0.0]), ([1, 3, float(F(0.02)), NAN], False)),
]


def same_floats(a, b):
    """equal as fp32 bit patterns (a NaN equals a NaN)"""
    return all((math.isnan(x) and math.isnan(y)) or F(x) == F(y) for x, y in zip(a, b)) and len(a) == len(b)


@pytest.mark.parametrize("case", range(len(GATE_TABLE)))
def test_oracle_gate_table(case):
    (kl_sum, count, target, gate), (want, want_applied) = GATE_TABLE[case]
    got, applied = oracle.kl_gate(kl_sum, count, target, gate)
    assert applied is want_applied
    assert same_floats(got, want), (got, want)
    # tensors go in as well as floats
    got_t, _ = oracle.kl_gate(torch.tensor(kl_sum), torch.tensor(count), target, gate)
    assert same_floats(got_t, want)


# ---- the worker against a hand-driven loop -------------------------------------------------------------------
def cpu_worker(**kw):
    return DPPOWorker(dppo_preset(**kw), DistContext())


def hand_iteration(w, n_apply):
    """one iteration of worker ``w`` (flag off) driven by hand through the engine's phases: every step calls
    ``grad``, only the first ``n_apply`` call ``apply``.  Returns the per-step approx_kl."""
    p, eng = w.p, w.engine
    w.init_stats()
    ro = eng.rollout()
    w._merge_stats(ro["count"], ro["s1"], ro["s2"], ro["shift"], count_uniform=True)
    eng.values()
    eng.gae()
    eng.begin_update()
    N, mb, nmb = w._minibatch_plan()
    w._perm_gen.manual_seed((p.seed * 1000003 + w.ctx.rank * 7919 + w.iteration) & 0x7FFFFFFF)
    kls = []
    for epoch in range(p.num_epoch):
        perm = None if (mb >= N and nmb == 1) else torch.randperm(N, generator=w._perm_gen)
        for b in range(nmb):
            idx = None if perm is None else perm[(b * mb) % N:(b * mb) % N + mb]
            kls.append(eng.grad(idx)["approx_kl"])
            if len(kls) <= n_apply:
                eng.apply()
    w.iteration += 1
    return kls


def assert_margin(kls, target, trip):
    """the reference's own KL sequence leaves a factor >= 2 on both sides of the target: a rounding
    difference between two engines cannot move the trip"""
    print("kl", ["%.3e" % k for k in kls[:trip + 1]], "target", target)
    assert all(k <= target / 2 for k in kls[:trip]) and kls[trip] >= 2 * target


_probe_cache = {}


def probe_kls(tag, kw):
    """the ungated per-step KL sequence of the first iteration (computed once per shape)"""
    if tag not in _probe_cache:
        _probe_cache[tag] = hand_iteration(cpu_worker(**kw), 10 ** 9)
    return _probe_cache[tag]


@pytest.mark.parametrize("shape", ["cheetah", "humanoid", "pendulum_minibatch"])
def test_gated_worker_equals_hand_loop(shape):
    kw = {"cheetah": CHEETAH, "humanoid": HUMANOID, "pendulum_minibatch": PENDULUM_MB}[shape]
    kls = probe_kls(shape, kw)
    if shape == "pendulum_minibatch":
        # two paths of one engine: bit-exact, no margin needed; the trip falls inside the first epoch
        target = math.sqrt(kls[1] * kls[2])
        assert kls[1] < target < kls[2] and dppo_preset(**kw).num_minibatches() == 4
    else:
        target = TABLE_TARGET[kw["env_name"]]
        assert_margin(kls, target, 2)
    w = cpu_worker(target_kl=target, **kw)
    m = w.iteration_step()
    ref = cpu_worker(**kw)
    hand_iteration(ref, 3)
    a, b = w.engine, ref.engine
    assert a.adam_step == b.adam_step == 3
    assert torch.equal(w.model.flat.data, ref.model.flat.data)
    assert torch.equal(a.adam_m, b.adam_m) and torch.equal(a.adam_v, b.adam_v)
    assert m["kl_stopped"] is True and m["steps_applied"] == 3 and m["updates"] == 3
    assert m["kl_trip"] == pytest.approx(kls[2], rel=1e-5)
    # the logged losses are the last step's, measured at the parameters the iteration ends with
    assert m["approx_kl"] == pytest.approx(a._last["approx_kl"]) and m["approx_kl"] > target
    assert m["grad_norm"] == pytest.approx(float(torch.linalg.vector_norm(a.grad_flat)), rel=1e-6)
    # the ungated run went on
    full = cpu_worker(**kw)
    full.iteration_step()
    assert full.engine.adam_step == full.p.num_epoch * full.p.num_minibatches()
    assert not torch.equal(full.model.flat.data, w.model.flat.data)


def test_huge_target_is_the_flag_off_bit_for_bit():
    off, on = cpu_worker(**CHEETAH), cpu_worker(target_kl=1e9, **CHEETAH)
    for _ in range(2):
        m0, m1 = off.iteration_step(), on.iteration_step()
    assert torch.equal(off.model.flat.data, on.model.flat.data)
    assert torch.equal(off.engine.adam_m, on.engine.adam_m) and torch.equal(off.engine.adam_v, on.engine.adam_v)
    assert off.engine.adam_step == on.engine.adam_step == 20
    assert m1["kl_stopped"] is False and m1["kl_trip"] is None and m1["steps_applied"] == 10
    assert m1["updates"] == m0["updates"] == 20
    assert m0["loss"] == m1["loss"] and m0["grad_norm"] == m1["grad_norm"]
    # the flag off holds no state and logs no field
    assert off.engine.gate is None and not any(k in m0 for k in ("kl_stopped", "steps_applied", "kl_trip"))


def test_record_fields_over_two_iterations():
    w = cpu_worker(target_kl=TABLE_TARGET["HalfCheetah-v2"], **CHEETAH)
    m1 = w.iteration_step()
    m2 = w.iteration_step()
    assert m1["kl_stopped"] and m1["steps_applied"] == 3 and m1["updates"] == 3
    assert 1 <= m2["steps_applied"] <= 10
    assert m2["updates"] == 3 + m2["steps_applied"] == w.engine.adam_step == w.updates      # cumulative, applied only
    assert (m2["kl_trip"] is None) == (not m2["kl_stopped"])
    json.dumps(m2)


# ---- refusals, CLI -------------------------------------------------------------------------------------------
def test_refusals():
    with pytest.raises(ValueError, match="target_kl must be >= 0"):
        Params(target_kl=-0.01)
    with pytest.raises(ValueError, match="target_kl must be >= 0"):
        Params(target_kl=float("nan"))
    with pytest.raises(ValueError, match="dppo_ref.*approx_kl = 0"):
        Params(target_kl=0.01, loss="dppo_ref")
    with pytest.raises(ValueError, match="compat"):
        Params(target_kl=0.01, compat=True)
    with pytest.raises(ValueError, match="overlap_rollout.*side stream"):
        Params(target_kl=0.01, overlap_rollout=True)
    with pytest.raises(ValueError, match="overlap_value_epochs.*device counter"):
        Params(target_kl=0.01, overlap_value_epochs=True)
    # 0 is off and refuses nothing; everything else composes
    Params(target_kl=0.0, loss="dppo_ref", compat=True, overlap_rollout=True, overlap_value_epochs=True)
    p = Params(target_kl=0.01, reward_norm=True, bootstrap_time_limit=True, normalize_adv=True, max_grad_norm=0.5,
               fused_apply=False, grad_comm="process_group", update_kernels="tile", dtype="fp8", grad_reduce="mean")
    assert p.target_kl == 0.01 and Params().target_kl == 0.0


def test_cli_flag():
    assert params_from_args([]).target_kl == 0.0
    p = params_from_args(["--target-kl", "0.015"])
    assert p.target_kl == 0.015 and Params.from_dict(p.to_dict()).target_kl == 0.015
    with pytest.raises(ValueError):
        params_from_args(["--target-kl", "0.01", "--overlap-rollout", "true"])


# ---- checkpoints ---------------------------------------------------------------------------------------------
def _run(**kw):
    base = dict(num_processes=1, target_kl=TABLE_TARGET["HalfCheetah-v2"], **CHEETAH)
    base.update(kw)
    return run_worker(dppo_preset(**base), DistContext(), evaluator=False, quiet=True)[0]


def test_resume_after_a_stopped_iteration_is_bit_identical(tmp_path):
    ck = str(tmp_path / "ck")
    w_full = _run(max_iters=3)
    w_two = _run(max_iters=2, checkpoint_dir=ck)
    st = torch.load(os.path.join(ck, "trainer_state.pt"), weights_only=True)
    assert w_two.last_metrics["kl_stopped"] is True                   # the checkpoint follows a stopped iteration
    assert st["adam_step"] == st["updates"] == w_two.engine.adam_step < 20     # the applied count
    w_res = _run(max_iters=3, resume=ck, checkpoint_dir="")
    assert w_res.iteration == 3 and w_res.engine.adam_step == w_full.engine.adam_step
    assert w_res.last_metrics["updates"] == w_full.last_metrics["updates"] == w_full.engine.adam_step
    for a, b in ((w_full.model.flat.data, w_res.model.flat.data), (w_full.engine.adam_m, w_res.engine.adam_m),
                 (w_full.engine.adam_v, w_res.engine.adam_v)):
        assert torch.equal(a, b)


def test_train_py_logs_the_fields(tmp_path):
    path, csv = tmp_path / "train.jsonl", tmp_path / "train.csv"
    cmd = [sys.executable, "train.py", "--env-name", "HalfCheetah-v2", "--max-iters", "2", "--num-processes", "1",
           "--num-envs", "48", "--exploration-size", "288", "--batch-size", "288", "--seed", "3", "--target-kl", "8.07e-4",
           "--log-jsonl", str(path), "--log-csv", str(csv)]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=170)
    assert r.returncode == 0, r.stderr[-3000:]
    recs = [json.loads(l) for l in path.read_text().splitlines()]
    assert len(recs) == 2 and recs[0]["kl_stopped"] is True and recs[0]["steps_applied"] == 3 and recs[0]["updates"] == 3
    assert recs[0]["kl_trip"] == pytest.approx(1.63e-3, rel=0.01)
    assert recs[1]["updates"] == 3 + recs[1]["steps_applied"]
    head = csv.read_text().splitlines()[0]
    assert not any(k in head for k in ("kl_stopped", "steps_applied", "kl_trip"))      # the CSV columns are fixed
    assert "kl_stopped" not in r.stdout and "steps_applied" not in r.stdout


# ---- two ranks -----------------------------------------------------------------------------------------------
# the summed KL of the 2-rank probe is 0, 3.408e-4, 1.374e-3: their geometric mean, to three digits
TWO_RANK_TARGET = 6.84e-4


def _rank_main(rank, world, port, out_dir):
    from pytorch_dppo_amd.parallel.dist import init_distributed
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.set_num_threads(1)
    ctx = init_distributed("cpu", rank=rank, world_size=world, timeout_s=60.0)
    kw = dict(CHEETAH, num_processes=world, verify_sync_every=1)
    # the probe: the per-rank (KL sum, count) pairs of an ungated iteration, every step applied
    w = DPPOWorker(dppo_preset(**kw), ctx)
    pairs = []
    orig = w.engine.grad

    def grad(idx):
        out = orig(idx)
        pairs.append((out["approx_kl"] * 288.0, 288.0))
        return out
    w.engine.grad = grad
    w.iteration_step()
    g = DPPOWorker(dppo_preset(target_kl=TWO_RANK_TARGET, **kw), ctx)
    m = g.iteration_step()
    torch.save({"pairs": pairs, "steps_applied": m["steps_applied"], "kl_trip": m["kl_trip"], "updates": m["updates"],
                "in_sync": bool(m["replicas_in_sync"]), "flat": g.model.flat.data.clone(),
                "rewards": g.engine.rewards.clone()}, os.path.join(out_dir, f"r{rank}.pt"))
    ctx.destroy()


@pytest.mark.slow
def test_two_ranks_take_the_same_decision_from_the_summed_pairs(tmp_path):
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
    # the global KL of step s = (sum of both ranks' KL sums) / (sum of the counts)
    kls = [(a[0] + b[0]) / (a[1] + b[1]) for a, b in zip(r0["pairs"], r1["pairs"])]
    print("summed kl", ["%.3e" % k for k in kls])
    trip = next(s for s, k in enumerate(kls) if not k <= TWO_RANK_TARGET)
    assert all(k <= TWO_RANK_TARGET / 2 for k in kls[:trip]) and kls[trip] >= 2 * TWO_RANK_TARGET    # factor 2 of room on both sides
    assert r0["steps_applied"] == r1["steps_applied"] == trip + 1 == r0["updates"]
    assert r0["kl_trip"] == r1["kl_trip"] == pytest.approx(kls[trip], rel=1e-4)
    assert r0["in_sync"] and r1["in_sync"] and torch.equal(r0["flat"], r1["flat"])
