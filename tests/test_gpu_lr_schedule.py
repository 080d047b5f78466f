"""``lr_schedule`` on the GPU engine: the rate block of the gate kernel (csrc/optim.hip kl_gate_kernel) against the
oracle's table, the gated Adam launches reading the rate from device memory against the same launches given it by
the host, an adaptive engine step by step against ops/oracle.lr_adapt and against a twin engine whose host rate the
test sets, the linear schedule, and the plumbing: no host sync, resume, two ranks, ``train.py``.  No learning-curve
comparison between engines: their KLs differ in the last bits, and a threshold crossing may not."""
import json
import math
import os
import subprocess
import sys

import pytest
import torch

from pytorch_dppo_amd.config import dppo_preset
from pytorch_dppo_amd.ops import oracle
from pytorch_dppo_amd.parallel.dist import DistContext
from test_gpu_target_kl import (DEV, FORM_CASES, PATHS, ROOT, SMALL, _ext, _sync_mode_raises, assert_same, bits, gpu_worker,
                                moved, prep, step_kl)
from test_lr_schedule import LR_DIRS, LR_TABLE, NAN, T, f
from test_target_kl import HUMANOID, same_floats

pytestmark = pytest.mark.gpu

ADAPT = dict(lr_schedule="adaptive", lr_kl_target=T)
RULE = (T, 1.5, 1e-6, 1e-2)
F32 = dict(dtype=torch.float32, device=DEV)


def rate_of(eng):
    """lr_state as python floats (a host sync)"""
    return eng.lr_state.tolist()


# ---- the gate kernel's rate block ------------------------------------------------------------------------------
def run_gate(kl, lr, rule, gate0=(0.0, 0.0, 0.0, 0.0), target=float("inf"), block=True):
    sums = torch.full((8,), -3.0, device=DEV)
    sums[3], sums[5] = kl, 1.0
    gate = torch.tensor(gate0, **F32)
    state = torch.tensor([5.0, 5.0, 7.5, -1.0], device=DEV)
    lr_state = torch.tensor([lr, 3.0, 5.0, -7.0], **F32)
    if block:
        _ext().kl_gate(sums, gate, state, target, lr_state, *rule)
    else:
        _ext().kl_gate(sums, gate, state, target)
    torch.cuda.synchronize()
    return gate, state, lr_state


@pytest.mark.parametrize("case", range(len(LR_TABLE)))
def test_kl_gate_rate_block_is_the_oracle(case):
    (lr, kl, *rule), _ = LR_TABLE[case]
    want = oracle.lr_adapt(lr, kl, *rule)
    gate, state, lr_state = run_gate(kl, lr, rule)
    got = lr_state.tolist()
    assert torch.equal(lr_state[0:1].cpu().view(torch.int32), torch.tensor([want], dtype=torch.float32).view(torch.int32))
    d = LR_DIRS[case]
    assert got[1:] == [3.0 + (d < 0), 5.0 + (d > 0), -7.0]                 # cumulative counts; the reserved slot stays
    # the gate itself is the oracle's, as without the block; +inf trips on a NaN alone
    want_gate, _ = oracle.kl_gate(kl, 1.0, float("inf"), [0.0] * 4)
    assert same_floats(gate.tolist(), want_gate) and (want_gate[0] == 1.0) == math.isnan(kl)
    assert state.tolist() == [6.0, 6.0, 7.5, -1.0]
    gate_n, state_n, lr_n = run_gate(kl, lr, rule, block=False)
    assert torch.equal(bits(gate_n), bits(gate)) and torch.equal(state_n, state)
    assert lr_n.tolist() == [f(lr), 3.0, 5.0, -7.0]


def test_kl_gate_stopped_step_adapts_nothing_and_the_tripping_step_adapts():
    lr = 3e-4
    _, state, lr_state = run_gate(1.0, lr, RULE, gate0=(1.0, 2.0, 0.5, 0.5), target=0.01)
    assert lr_state.tolist() == [f(lr), 3.0, 5.0, -7.0] and state.tolist() == [5.0, 5.0, 7.5, -1.0]
    gate, state, lr_state = run_gate(1.0, lr, RULE, target=0.01)             # open, trips now: applied, so it adapts
    assert gate.tolist()[:3] == [1.0, 1.0, 1.0] and state.tolist()[0] == 6.0
    assert lr_state.tolist() == [oracle.lr_adapt(lr, 1.0, *RULE), 4.0, 5.0, -7.0]


def test_kl_gate_rate_block_refusals():
    ext = _ext()
    z = lambda n, **k: torch.zeros(n, device=k.pop("device", DEV), **k)   # noqa: E731
    ok = (T, 1.5, 1e-6, 1e-2)
    ext.kl_gate(z(8), z(4), z(4), 0.01, torch.full((4,), 3e-4, **F32), *ok)
    ext.kl_gate(z(8), z(4), z(4), 0.01, torch.empty(0, **F32), 0.0, 0.0, 0.0, 0.0)    # an empty block: the gate alone
    for lr_state, rule in ((z(3), ok), (z(5), ok), (z(4, dtype=torch.float64), ok), (z(4, device="cpu"), ok),
                           (z(4), (0.0, 1.5, 1e-6, 1e-2)), (z(4), (-T, 1.5, 1e-6, 1e-2)), (z(4), (NAN, 1.5, 1e-6, 1e-2)),
                           (z(4), (T, 1.0, 1e-6, 1e-2)), (z(4), (T, 0.5, 1e-6, 1e-2)), (z(4), (T, 1.5, 1e-2, 1e-3))):
        with pytest.raises(RuntimeError):
            ext.kl_gate(z(8), z(4), z(4), 0.01, lr_state, *rule)
    torch.cuda.synchronize()


# ---- the gated Adam launches: device rate against host rate ------------------------------------------------------
N_FLAT = 300
X_RATE = 4.4444e-4
STORAGE = {0: torch.float32, 1: torch.bfloat16, 2: torch.uint8, 3: torch.int32}


def flat_case(dt):
    """a flat vector of 300 parameters, every one mapped into an image of 2 x 300 entries (the second half of
    the vector also into a transposed entry), with non-trivial optimizer state"""
    n = N_FLAT
    gen = torch.Generator().manual_seed(5)
    i32 = dict(dtype=torch.int32, device=DEV)
    c = {"p": torch.randn(n, generator=gen).to(DEV), "g": torch.randn(n, generator=gen).to(DEV),
         "m": (torch.randn(n, generator=gen) * 1e-2).to(DEV), "v": (torch.rand(n, generator=gen) * 1e-4).to(DEV),
         "wimg": torch.zeros(2 * n, dtype=STORAGE[dt], device=DEV), "w_map": torch.arange(n, **i32)}
    wt = n + torch.arange(n, **i32)
    wt[:n // 2] = -1
    c["wt_map"] = wt
    return c


def launch(form, dt, c, gate, lr, lr_dev):
    ext, n = _ext(), N_FLAT
    i32 = dict(dtype=torch.int32, device=DEV)
    no_q, no_i, no_u8 = torch.empty(0, **F32), torch.empty(0, **i32), torch.empty(0, dtype=torch.uint8, device=DEV)
    state = torch.tensor([4.0, 4.0, 0.0, 0.0], **F32)
    if form == "gather_adam":
        # one reduce item (partial column 0 -> loss_out[0]) and one slab run: every element is slab[0], one chunk
        ext.gather_adam(torch.full((1,), 0.37, **F32), torch.zeros(n, **i32), torch.full((n,), 32, **i32),
                        torch.ones(1, **F32), 1, 1, torch.zeros(1, **i32), torch.full((1,), -1, **i32), [0, n], 1.0,
                        torch.zeros(8, **F32), c["g"], c["p"], c["m"], c["v"], lr, 0.9, 0.999, 1e-8, 0, state,
                        torch.zeros(3, **F32), c["wimg"], c["w_map"], c["wt_map"], dt, no_q, no_u8, no_i, no_q, gate, lr_dev)
    else:
        ext.adam(c["p"], c["g"], c["m"], c["v"], lr, 0.9, 0.999, 1e-8, 0.5 if form == "clip_pair" else 0.0, state,
                 torch.zeros(2, **F32), c["wimg"], c["w_map"], c["wt_map"], dt, no_q, 0, no_u8, no_i, no_q, gate, lr_dev)
    torch.cuda.synchronize()
    assert state.tolist()[:2] == [4.0, 4.0]                    # a gated launch never writes the counter
    return {k: c[k].clone() for k in ("p", "m", "v", "wimg", "g")}


@pytest.mark.parametrize("stopped", [False, True])
@pytest.mark.parametrize("dt", [0, 1, 2, 3])
@pytest.mark.parametrize("form", ["gather_adam", "adam_noclip", "clip_pair"])
def test_device_rate_equals_host_rate(form, dt, stopped):
    gate = torch.tensor([1.0 if stopped else 0.0, 0.0, 0.0, 0.0], **F32)
    start = flat_case(dt)
    host = launch(form, dt, flat_case(dt), gate, X_RATE, torch.empty(0, **F32))
    lr_state = torch.tensor([X_RATE, 0.0, 0.0, 0.0], **F32)
    dev = launch(form, dt, flat_case(dt), gate, 123.0, lr_state)            # (the host float is unread)
    assert_same(host, dev)
    assert lr_state.tolist() == [f(X_RATE), 0.0, 0.0, 0.0]                   # read only
    none = launch(form, dt, flat_case(dt), gate, X_RATE, None)               # no operand at all: the host rate
    assert_same(host, none)
    assert torch.equal(host["p"], start["p"]) == stopped and torch.equal(bits(host["wimg"]), bits(start["wimg"])) == stopped
    if not stopped:
        other = launch(form, dt, flat_case(dt), gate, 123.0, torch.tensor([2 * X_RATE, 0.0, 0.0, 0.0], **F32))
        assert not torch.equal(other["p"], host["p"])


def test_lr_dev_without_a_gate_is_refused():
    c = flat_case(0)
    p0 = c["p"].clone()
    lr_state = torch.tensor([X_RATE, 0.0, 0.0, 0.0], **F32)
    for form in ("gather_adam", "adam_noclip", "clip_pair"):
        with pytest.raises(RuntimeError, match="lr_dev needs a gate"):
            launch(form, 0, c, torch.empty(0, **F32), X_RATE, lr_state)
    gate = torch.zeros(4, **F32)
    for bad in (torch.zeros(3, **F32), torch.zeros(5, **F32), torch.zeros(4, dtype=torch.float64, device=DEV), torch.zeros(4)):
        with pytest.raises(RuntimeError, match="lr_state"):
            launch("adam_noclip", 0, c, gate, X_RATE, bad)
    torch.cuda.synchronize()
    assert torch.equal(c["p"], p0)


# ---- the engine, step by step --------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,path", FORM_CASES)
def test_adaptive_engine_step_by_step(dtype, path):
    """an initial rate of 3e-3 moves in both directions within a few steps (up after the zero KL that opens an
    iteration, down once the KL is past 0.016); whichever way each step goes, the device took the oracle's decision
    on its own KL bits, and a twin engine handed every step's rate by the host lands on the same bits"""
    kw = dict(SMALL, dtype=dtype, lr=3e-3, **PATHS[path])
    wa, wt = gpu_worker(**ADAPT, **kw), gpu_worker(target_kl=1e9, **kw)
    ea, et = wa.engine, wt.engine
    assert ea.heads == et.heads == (PATHS[path]["update_kernels"] == "heads")
    assert ea.gate is not None and ea._grad_sums is not None and et.lr_state is None
    lr = f(3e-3)
    assert rate_of(ea) == [lr, 0.0, 0.0, 0.0]
    downs = ups = 0
    rates = []
    for it in range(2):
        prep(wa)
        prep(wt)
        ea.begin_update()
        et.begin_update()
        assert rate_of(ea)[0] == lr                       # begin_update() does not reset the rate
        for s in range(3):
            rates.append(lr)
            et.lr = lr
            ea.step(None)
            et.step(None)
            ea.finish_steps()
            et.finish_steps()
            torch.cuda.synchronize()
            kl = step_kl(ea)
            assert kl == ea.gate.tolist()[3]
            if s == 0 and dtype != "fp8":       # the opening KL: 0 up to rounding (fp8: the update's e4m3 forward image differs
                assert abs(kl) < 1e-6           # from the rollout's weights, profiles/r4/fp8_heads.md)
            lr = oracle.lr_adapt(lr, kl, *RULE)
            d = oracle.lr_adapt_dir(kl, T)
            downs, ups = downs + (d < 0), ups + (d > 0)
            got = rate_of(ea)
            assert same_floats(got[:1], [lr]) and got[1:] == [float(downs), float(ups), 0.0], (it, s, kl, got)
        assert_same(moved(ea), moved(et))
        assert torch.equal(ea.gate, et.gate) and ea.adam_state.tolist()[:2] == et.adam_state.tolist()[:2] == [3.0 * (it + 1)] * 2
    print("rates", rates, "downs", downs, "ups", ups)
    assert ups >= 2 and len(set(rates)) > 1


def test_adaptive_with_target_kl_on_the_device():
    """the tripping step adapts, the stopped steps do not (the gate's own rule: tests/test_gpu_target_kl.py)"""
    kw = dict(SMALL, dtype="bf16x3", lr=3e-3, num_epoch=5)
    probe = gpu_worker(**ADAPT, **kw)
    prep(probe)
    probe.engine.begin_update()
    kls = []
    for _ in range(3):
        probe.engine.step(None)
        torch.cuda.synchronize()
        kls.append(step_kl(probe.engine))
    assert abs(kls[0]) < 1e-6 < kls[1] < kls[2]
    target = math.sqrt(kls[1] * kls[2])                  # two runs of one engine: bit-exact, no margin needed
    w = gpu_worker(target_kl=target, **ADAPT, **kw)
    m = w.iteration_step()
    assert m["kl_stopped"] is True and m["steps_applied"] == 3 and m["kl_trip"] == kls[2]
    lr = f(3e-3)
    for k in kls:
        lr = oracle.lr_adapt(lr, k, *RULE)
    dirs = [oracle.lr_adapt_dir(k, T) for k in kls]
    assert rate_of(w.engine) == [lr, float(dirs.count(-1)), float(dirs.count(1)), 0.0]
    assert m["lr"] == lr and m["lr_downs"] == dirs.count(-1) and m["lr_ups"] == dirs.count(1)


# ---- linear --------------------------------------------------------------------------------------------------------
def test_linear_gpu_worker_equals_a_worker_fed_the_rate_by_hand():
    kw = dict(SMALL, dtype="bf16x3", num_epoch=2, max_iters=3)
    wl, wh, wc = gpu_worker(lr_schedule="linear", lr_final_frac=0.1, **kw), gpu_worker(**kw), gpu_worker(**kw)
    assert wl.engine.lr_state is None and wl.engine.gate is None and wl.engine.metrics_buf.numel() == 12
    for i in range(3):
        rate = 3e-4 * (1.0 - (1.0 - 0.1) * min(i, 3) / 3)
        wh.engine.lr = rate
        ml = wl.iteration_step()
        wh.iteration_step()
        wc.iteration_step()
        assert ml["lr"] == rate and "lr_downs" not in ml and "kl_stopped" not in ml
    assert_same(moved(wl.engine), moved(wh.engine))
    assert not torch.equal(wl.model.flat.data, wc.model.flat.data)
    assert wc.engine.metrics_buf.numel() == 11 and wc.engine.lr_state is None


# ---- plumbing --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["joint", "unfused", "clip"])
def test_deferred_adaptive_iteration_does_not_sync(path):
    kw = dict(HUMANOID, dtype="bf16x3", phase_timing=0, **ADAPT, **PATHS[path])
    w = gpu_worker(**kw)
    w.iteration_step(defer=True)                 # (first call: allocations, kernel loads)
    torch.cuda.synchronize()
    if not _sync_mode_raises():
        pytest.skip("torch.cuda.set_sync_debug_mode('error') does not raise on .item() in this build")
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        m = w.iteration_step(defer=True)
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    torch.cuda.synchronize()
    assert m["kl_stopped"] is False and m["steps_applied"] == m["updates"] == 10
    assert 1e-6 <= m["lr"] <= 1e-2 and m["lr_ups"] >= 1 and m["lr_ups"] + m["lr_downs"] <= 10
    m2 = w.finish_metrics()
    got = rate_of(w.engine)
    assert [m2["lr"], float(m2["lr_downs"]), float(m2["lr_ups"])] == got[:3] and m2["updates"] == 20


def test_resume_is_bit_identical(tmp_path):
    from pytorch_dppo_amd.runtime.launcher import run_worker
    base = dict(SMALL, device="gpu", num_processes=1, dtype="bf16x3", update_kernels="heads", lr=3e-3, num_epoch=3,
                max_iters=3, **ADAPT)
    ctx = DistContext(device=DEV)
    w_full, _ = run_worker(dppo_preset(**base), ctx, evaluator=False, quiet=True)
    ck = str(tmp_path / "ck")
    w_two, _ = run_worker(dppo_preset(checkpoint_dir=ck, **base), ctx, max_iters=2, evaluator=False, quiet=True)
    st = torch.load(os.path.join(ck, "trainer_state.pt"), weights_only=True)
    assert st["lr_state"].tolist() == rate_of(w_two.engine) and st["lr_state"].tolist()[0] != f(3e-3)
    assert st["adam_step"] == 6
    w_res, _ = run_worker(dppo_preset(resume=ck, **base), ctx, evaluator=False, quiet=True)
    assert w_res.iteration == 3 and w_res.engine.adam_step == w_full.engine.adam_step == 9
    assert_same(moved(w_full.engine), moved(w_res.engine))
    assert torch.equal(w_full.engine.lr_state, w_res.engine.lr_state)
    assert w_res.last_metrics["lr"] == w_full.last_metrics["lr"] == rate_of(w_full.engine)[0]


def _train_py(tmp_path, *flags):
    path = tmp_path / "train.jsonl"
    cmd = [sys.executable, "train.py", "--device", "gpu", "--env-name", "Humanoid-v2", "--num-processes", "1",
           "--num-envs", "64", "--exploration-size", "256", "--batch-size", "256", "--seed", "3", "--dtype", "bf16x3",
           "--num-epoch", "3", "--log-jsonl", str(path), *flags]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=170)
    assert r.returncode == 0, r.stderr[-3000:]
    recs = [json.loads(l) for l in path.read_text().splitlines()]
    assert all(math.isfinite(x[k]) for x in recs for k in ("loss", "grad_norm", "approx_kl", "lr"))
    return recs


def test_train_py_adaptive_logs_the_fields(tmp_path):
    recs = _train_py(tmp_path, "--lr-schedule", "adaptive", "--max-iters", "2")
    assert len(recs) == 2 and recs[1]["updates"] == 6
    for rec in recs:
        assert 1e-6 <= rec["lr"] <= 1e-2 and rec["lr_ups"] >= 1 and rec["lr_downs"] >= 0
        assert rec["kl_stopped"] is False and rec["steps_applied"] == 3 and rec["kl_trip"] is None
    assert recs[1]["lr_ups"] + recs[1]["lr_downs"] >= recs[0]["lr_ups"] + recs[0]["lr_downs"]


def test_train_py_linear_logs_the_rate(tmp_path):
    recs = _train_py(tmp_path, "--lr-schedule", "linear", "--max-iters", "3")
    assert [r["lr"] for r in recs] == [3e-4 * (1.0 - i / 3) for i in range(3)]
    assert not any(k in recs[0] for k in ("lr_downs", "lr_ups", "kl_stopped"))


# ---- two ranks -------------------------------------------------------------------------------------------------------
def _two_rank_child(rank, world, port, out_dir):
    """one of 2 ranks sharing cuda:0 over gloo (per-rank seeds): per gradient comm, two adaptive iterations"""
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.set_num_threads(2)
    from pytorch_dppo_amd.parallel.dist import init_distributed
    base = init_distributed("gpu", rank=rank, world_size=world, backend="gloo", timeout_s=120)
    common = dict(SMALL, dtype="bf16x3", num_epoch=3, lr=3e-3, num_processes=world, dist_backend="gloo",
                  verify_sync_every=1, update_kernels="heads", **ADAPT)
    out = {}
    for gc in ("auto", "process_group"):
        c = DistContext(rank=rank, world_size=world, local_rank=0, backend="gloo", device=base.device, timeout_s=120,
                        grad_comm=gc)
        w = gpu_worker(c, grad_comm=gc, **common)
        ms = [w.iteration_step(), w.iteration_step()]
        torch.cuda.synchronize()
        out[gc] = {"lr_state": w.engine.lr_state.cpu(), "flat": w.model.flat.data.cpu(), "m": w.engine.adam_m.cpu(),
                   "in_sync": all(bool(m["replicas_in_sync"]) for m in ms), "native": c.native is not None,
                   "lr": [m["lr"] for m in ms], "rewards": w.engine.rewards.cpu()}
    torch.save(out, os.path.join(out_dir, f"lr{rank}.pt"))
    base.destroy()


def test_two_ranks_end_with_equal_lr_state(tmp_path):
    import torch.multiprocessing as mp
    from pytorch_dppo_amd.runtime.launcher import free_port
    port = free_port()
    ctxm = mp.get_context("spawn")
    procs = [ctxm.Process(target=_two_rank_child, args=(r, 2, port, str(tmp_path))) for r in range(2)]
    for p_ in procs:
        p_.start()
    for p_ in procs:
        p_.join(115)
    codes = [p_.exitcode for p_ in procs]
    for p_ in procs:
        if p_.is_alive():
            p_.kill()
    assert codes == [0, 0], codes
    r0 = torch.load(tmp_path / "lr0.pt", weights_only=True)
    r1 = torch.load(tmp_path / "lr1.pt", weights_only=True)
    for gc in ("auto", "process_group"):
        a, b = r0[gc], r1[gc]
        print(gc, "lr_state", a["lr_state"].tolist())
        assert not torch.equal(a["rewards"], b["rewards"])                     # per-rank data
        assert a["native"] == (gc == "auto")                                   # the in-stream branch / the process group
        assert torch.equal(a["lr_state"], b["lr_state"]) and a["lr"] == b["lr"]
        assert torch.equal(a["flat"], b["flat"]) and torch.equal(a["m"], b["m"]) and a["in_sync"] and b["in_sync"]
        s = a["lr_state"].tolist()
        assert s[0] != f(3e-3) and s[1] + s[2] >= 2 and s[2] >= 2             # the rate moved (every iteration opens with an up)
    # the two comm paths agree bit for bit
    assert torch.equal(r0["auto"]["lr_state"], r0["process_group"]["lr_state"])
    assert torch.equal(r0["auto"]["flat"], r0["process_group"]["flat"])
