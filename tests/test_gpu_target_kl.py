"""``target_kl`` on the GPU engine: the gate kernel (csrc/optim.hip kl_gate_kernel) against the oracle's table, the
gated forms of the three Adam launches against the ungated ones, the exact end-to-end oracle (a gated 10-epoch
iteration that trips at step 2 == an ungated 3-epoch iteration, bit for bit), the GPU worker against the CPU worker,
and the plumbing: no host sync, resume, two ranks, ``train.py``.  Shapes and targets: tests/test_target_kl.py."""
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
from pytorch_dppo_amd.runtime.worker import DPPOWorker
from test_target_kl import (CHEETAH, GATE_TABLE, HUMANOID, PENDULUM_MB, TABLE_TARGET, assert_margin, cpu_worker,
                            probe_kls, same_floats)

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0) if torch.cuda.is_available() else None
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = dict(env_name="Humanoid-v2", num_envs=64, exploration_size=64 * 4, batch_size=64 * 4, seed=3, num_epoch=1)


def _ext():
    from pytorch_dppo_amd.ops import native
    return native.load()


def gpu_worker(ctx=None, **kw):
    return DPPOWorker(dppo_preset(device="gpu", **kw), ctx if ctx is not None else DistContext(device=DEV))


def prep(w):
    """rollout -> statistics -> values -> GAE: the engine is ready for begin_update() / step()"""
    eng = w.engine
    w.init_stats()
    ro = eng.rollout()
    w._merge_stats(ro["count"], ro["s1"], ro["s2"], ro["shift"])
    eng.values()
    eng.gae()


def moved(eng):
    """everything a stopped step must leave alone: p, m, v, the weight images, the e4m3 shadow, the counter"""
    torch.cuda.synchronize()
    out = {"p": eng.model.flat.data, "m": eng.adam_m, "v": eng.adam_v, "wimg": eng.wimg, "step": eng.adam_state[0:1]}
    if eng.fp8:
        out["wimg_fwd"] = eng.wimg_fwd
    return {k: v.detach().clone() for k, v in out.items()}


def bits(t):
    return t.view(torch.uint8) if t.element_size() == 1 else t.contiguous().view(-1).view(torch.uint8)


def assert_same(a, b, keys=None):
    for k in (keys or a.keys()):
        assert torch.equal(bits(a[k]), bits(b[k])), k


def step_kl(eng):
    s = eng.loss_sums.tolist()
    return float(torch.tensor(s[3], dtype=torch.float32) / max(torch.tensor(s[5], dtype=torch.float32), 1.0))


def minibatch_indices(w):
    """the worker's loop order of one iteration: the index tensor of every step (None: full batch)"""
    p = w.p
    N, mb, nmb = w._minibatch_plan()
    w._perm_gen.manual_seed((p.seed * 1000003 + w.ctx.rank * 7919 + w.iteration) & 0x7FFFFFFF)
    out = []
    for epoch in range(p.num_epoch):
        perm = None if (mb >= N and nmb == 1) else torch.randperm(N, generator=w._perm_gen)
        out += [None if perm is None else perm[(b * mb) % N:(b * mb) % N + mb] for b in range(nmb)]
    return out


def hand_steps(w, n_steps, allreduce=None):
    """the first ``n_steps`` steps of worker ``w``'s iteration through eng.step; returns each step's KL"""
    eng = w.engine
    prep(w)
    eng.begin_update()
    kls = []
    for idx in minibatch_indices(w)[:n_steps]:
        eng.step(idx, allreduce=allreduce)
        eng.finish_steps()
        kls.append(step_kl(eng))
    torch.cuda.synchronize()
    return kls


# ---- the gate kernel -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", range(len(GATE_TABLE)))
def test_kl_gate_kernel_is_the_oracle(case):
    (kl_sum, count, target, gate0), _ = GATE_TABLE[case]
    want, applied = oracle.kl_gate(kl_sum, count, target, gate0)
    sums = torch.full((8,), -3.0, device=DEV)
    sums[3], sums[5] = kl_sum, count
    gate = torch.tensor(gate0, dtype=torch.float32, device=DEV)
    state = torch.tensor([5.0, 5.0, 7.5, -1.0], device=DEV)
    _ext().kl_gate(sums, gate, state, target)
    torch.cuda.synchronize()
    got = gate.tolist()
    assert same_floats(got, want), (got, want)
    assert state.tolist() == ([6.0, 6.0, 7.5, -1.0] if applied else [5.0, 5.0, 7.5, -1.0])
    # bitwise where the value is a number
    w32 = torch.tensor(want, dtype=torch.float32)
    ok = ~torch.isnan(w32)
    assert torch.equal(gate.cpu().view(torch.int32)[ok], w32.view(torch.int32)[ok])
    assert sums.tolist()[0] == -3.0                                           # the sums are read only


def test_kl_gate_binding_refusals():
    ext = _ext()
    z = lambda n, **k: torch.zeros(n, device=k.pop("device", DEV), **k)   # noqa: E731
    ext.kl_gate(z(8), z(4), z(4), 0.01)
    for sums, gate, state, target in ((z(7), z(4), z(4), 0.01), (z(8), z(3), z(4), 0.01), (z(8), z(5), z(4), 0.01),
                                      (z(8), z(4), z(3), 0.01), (z(8), z(4, device="cpu"), z(4), 0.01),
                                      (z(8), z(4, dtype=torch.float64), z(4), 0.01), (z(8), z(4), z(4), 0.0),
                                      (z(8, device="cpu"), z(4), z(4), 0.01)):
        with pytest.raises(RuntimeError):
            ext.kl_gate(sums, gate, state, target)
    torch.cuda.synchronize()


def test_adam_binding_gate_argument_and_refusals():
    """``adam`` / ``gather_adam`` on a flat vector of 300 parameters with an fp32 image nobody is mapped into: an
    empty gate is the ungated launch (which counts the step), a well-formed gate the gated one (the counter belongs
    to kl_gate), and a malformed gate — or no gate and no host step number for the fused launch — raises before
    anything is launched."""
    ext, n = _ext(), 300
    f32, i32 = dict(dtype=torch.float32, device=DEV), dict(dtype=torch.int32, device=DEV)
    gen = torch.Generator().manual_seed(5)
    p0 = torch.randn(n, generator=gen).to(DEV)
    p, g, m, v = p0.clone(), torch.randn(n, generator=gen).to(DEV), torch.zeros(n, **f32), torch.zeros(n, **f32)
    state, wimg, no_map = torch.zeros(4, **f32), torch.zeros(32, **f32), torch.full((n,), -1, **i32)
    no_q, no_i, no_u8 = torch.empty(0, **f32), torch.empty(0, **i32), torch.empty(0, dtype=torch.uint8, device=DEV)

    def adam(gate, host_step, max_norm, nblk):
        ext.adam(p, g, m, v, 1e-3, 0.9, 0.999, 1e-8, max_norm, state, torch.zeros(nblk, **f32), wimg, no_map, no_map,
                 0, no_q, host_step, no_u8, no_i, no_q, gate)

    def gather_adam(gate, step):
        # one reduce item (partial column 0 -> loss_out[0]) and one slab run: every element is slab[0], one chunk
        ext.gather_adam(torch.ones(1, **f32), torch.zeros(n, **i32), torch.full((n,), 32, **i32), torch.ones(1, **f32),
                        1, 1, torch.zeros(1, **i32), torch.full((1,), -1, **i32), [0, n], 1.0, torch.zeros(8, **f32),
                        g, p, m, v, 1e-3, 0.9, 0.999, 1e-8, step, state, torch.zeros(2, **f32), wimg, no_map, no_map,
                        0, no_q, no_u8, no_i, no_q, gate)

    adam(no_q, 1, 0.0, 1)                      # ungated, no clipping: one launch, which writes the counter
    torch.cuda.synchronize()
    assert state.tolist()[0] == 1.0 and not torch.equal(p, p0)
    p1 = p.clone()
    adam(torch.zeros(4, **f32), 0, 0.5, 2)     # gated and open: applied, the counter is left to kl_gate
    torch.cuda.synchronize()
    assert state.tolist()[:2] == [1.0, 1.0] and not torch.equal(p, p1)
    p2 = p.clone()
    bad = (torch.zeros(3, **f32), torch.zeros(5, **f32), torch.zeros(4, dtype=torch.float64, device=DEV),
           torch.zeros(4))
    for gate in bad:
        with pytest.raises(RuntimeError, match="gate"):
            adam(gate, 1, 0.0, 1)
        with pytest.raises(RuntimeError, match="gate"):
            gather_adam(gate, 1)
    with pytest.raises(RuntimeError, match="host step number"):
        gather_adam(no_q, 0)
    torch.cuda.synchronize()
    assert torch.equal(p, p2) and state.tolist()[:2] == [1.0, 1.0]


# ---- the gated Adam forms --------------------------------------------------------------------------------------
PATHS = {"joint": dict(update_kernels="heads"), "unfused": dict(update_kernels="heads", fused_apply=False),
         "tile": dict(update_kernels="tile"), "tile_unfused": dict(update_kernels="tile", fused_apply=False),
         "clip": dict(update_kernels="heads", max_grad_norm=0.5), "tile_clip": dict(update_kernels="tile", max_grad_norm=0.5)}
FORM_CASES = [(d, p) for d in ("bf16x3", "bf16", "fp8") for p in ("joint", "unfused", "tile", "clip")] + \
             [("fp32", p) for p in ("tile", "tile_unfused", "tile_clip")]


@pytest.mark.parametrize("dtype,path", FORM_CASES)
def test_gated_adam_forms(dtype, path):
    kw = dict(SMALL, dtype=dtype, **PATHS[path])
    wu, wg = gpu_worker(**kw), gpu_worker(target_kl=1e9, **kw)
    eu, eg = wu.engine, wg.engine
    assert eg.heads == eu.heads == (PATHS[path]["update_kernels"] == "heads")
    prep(wu)
    prep(wg)
    gen = torch.Generator().manual_seed(11)
    m0, v0 = torch.randn(eu.adam_m.numel(), generator=gen) * 1e-2, torch.rand(eu.adam_v.numel(), generator=gen) * 1e-4
    for e in (eu, eg):
        e.adam_m.copy_(m0)
        e.adam_v.copy_(v0)
    # the twin's gradient at the shared parameters
    eu.begin_update()
    eu.grad(None)
    torch.cuda.synchronize()
    g_ref, sums_ref = eu.grad_flat.clone(), eu.loss_sums.clone()
    # ---- stop = 1: nothing moves; the gradient, the loss sums and the norm partials are still written
    eg.begin_update()
    eg.adam_step = 4
    eg.gate[0] = 1.0
    before = moved(eg)
    eg.grad_flat.fill_(float("nan"))
    eg.loss_sums.fill_(float("nan"))
    eg.norm_part.fill_(float("nan"))
    eg.adam_state[2] = -1.0
    eg.step(None)
    after = moved(eg)
    assert_same(before, after)
    assert float(after["step"]) == 4.0 and eg.adam_state.tolist()[1] == 4.0
    assert torch.equal(eg.grad_flat, g_ref) and torch.equal(eg.loss_sums, sums_ref)
    gate = eg.gate.tolist()
    assert gate[:3] == [1.0, 0.0, 0.0] and gate[3] == step_kl(eg)
    norm = float(torch.linalg.vector_norm(g_ref.double()))
    assert float(eg.norm_part[:eg._norm_n].double().sum().sqrt()) == pytest.approx(norm, rel=1e-5)
    if "clip" in path:
        assert eg.adam_state.tolist()[2] == pytest.approx(norm, rel=1e-5)
    # ---- stop = 0 with adam_state[0] = 4: the bits of the ungated step with host step 5
    eg.begin_update()
    assert eg.gate.tolist() == [0.0] * 4
    eg.step(None)
    eu.begin_update()
    eu.adam_step = 4
    eu.adam_state[0] = 4.0              # (the ungated clip pair stages its step number from the device counter)
    eu.step(None)
    eu.finish_steps()
    a, b = moved(eg), moved(eu)
    assert float(a["step"]) == 5.0 and eg.gate.tolist()[:3] == [0.0, 1.0, 0.0]
    assert_same(a, b, [k for k in a if k != "step"])
    assert not torch.equal(a["p"], before["p"]) and not torch.equal(bits(a["wimg"]), bits(before["wimg"]))
    assert torch.equal(eg.grad_flat, eu.grad_flat) and torch.equal(eg.loss_sums, eu.loss_sums)
    assert eg.adam_step == 5 and eu.adam_step == 5


# ---- the exact end-to-end oracle ---------------------------------------------------------------------------------
E2E = [("bf16x3", HUMANOID, "heads"), ("bf16", HUMANOID, "heads"), ("fp8", HUMANOID, "heads"), ("fp32", CHEETAH, "tile")]


@pytest.mark.parametrize("dtype,shape,kernels", E2E)
def test_gated_iteration_is_the_ungated_three_epoch_iteration(dtype, shape, kernels):
    kw = dict(shape, dtype=dtype, update_kernels=kernels)
    target = TABLE_TARGET[shape["env_name"]]
    wg = gpu_worker(target_kl=target, num_epoch=10, **kw)
    m = wg.iteration_step()
    print("gpu kl_trip", m["kl_trip"], "target", target)
    assert m["kl_stopped"] is True and m["steps_applied"] == 3 and m["updates"] == 3
    assert wg.engine.gate.tolist()[:2] == [1.0, 3.0] and wg.engine.adam_state.tolist()[:2] == [3.0, 3.0]
    w3 = gpu_worker(num_epoch=3, **kw)
    w3.iteration_step()
    assert w3.engine.heads == wg.engine.heads == (kernels == "heads")
    assert_same(moved(wg.engine), moved(w3.engine))
    assert wg.engine.adam_step == w3.engine.adam_step == 3
    # the same gated iteration without the joint gather + Adam launch: identical bits
    wf = gpu_worker(target_kl=target, num_epoch=10, fused_apply=False, **kw)
    mf = wf.iteration_step()
    assert_same(moved(wg.engine), moved(wf.engine))
    assert torch.equal(wg.engine.gate, wf.engine.gate) and mf["kl_trip"] == m["kl_trip"]
    assert mf["loss"] == m["loss"] and mf["approx_kl"] == m["approx_kl"]
    assert mf["grad_norm"] == pytest.approx(m["grad_norm"], rel=1e-5)     # (block partials of two grids)
    # the logged losses are the last step's, at the parameters the iteration ends with: above the target
    assert m["approx_kl"] > target


def test_minibatched_iteration_trips_inside_an_epoch():
    kw = dict(PENDULUM_MB, dtype="bf16x3", num_epoch=2)
    kls = hand_steps(gpu_worker(**kw), 3)
    print("gpu kl", kls)
    assert kls[0] < kls[1] < kls[2] and kls[1] > 0
    target = math.sqrt(kls[1] * kls[2])          # two paths of one engine: bit-exact, no margin needed
    wg = gpu_worker(target_kl=target, **kw)
    assert wg.p.num_minibatches() == 4
    m = wg.iteration_step()
    assert m["kl_stopped"] and m["steps_applied"] == 3 and m["kl_trip"] == kls[2]
    ref = gpu_worker(**kw)
    hand_steps(ref, 3)                           # steps 0 .. trip applied, nothing after
    assert_same(moved(wg.engine), moved(ref.engine))


# ---- against the CPU worker --------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,shape,tag", [("fp32", CHEETAH, "cheetah"), ("bf16x3", HUMANOID, "humanoid")])
def test_gpu_worker_trips_where_the_cpu_worker_does(dtype, shape, tag):
    target = TABLE_TARGET[shape["env_name"]]
    assert_margin(probe_kls(tag, shape), target, 2)              # on the reference alone
    wc = cpu_worker(target_kl=target, **shape)
    wg = gpu_worker(target_kl=target, dtype=dtype, **shape)
    assert torch.equal(wg.model.flat.data.cpu(), wc.model.flat.data)
    mc, mg = wc.iteration_step(), wg.iteration_step()
    print("kl_trip cpu", mc["kl_trip"], "gpu", mg["kl_trip"])
    assert mc["kl_stopped"] and mg["kl_stopped"] and mc["steps_applied"] == mg["steps_applied"] == 3
    assert mg["updates"] == mc["updates"] == 3
    # test_engine_iteration_matches_torch_engine_fp32's bounds, with 3 steps
    d = (wg.model.flat.data.cpu() - wc.model.flat.data).abs()
    print("max |dp|", d.max().item(), "frac > 1e-5", (d > 1e-5).float().mean().item())
    assert d.max().item() <= 2 * wg.p.lr * 3 + 1e-6
    assert (d > 1e-5).float().mean().item() < 0.01
    assert abs(mg["loss_value"] - mc["loss_value"]) < 1e-3 * (1 + abs(mc["loss_value"]))


# ---- flag off / never tripping ----------------------------------------------------------------------------------
def test_huge_target_is_the_flag_off_and_flag_off_holds_no_gate():
    kw = dict(SMALL, dtype="bf16x3", num_epoch=2)
    off, on = gpu_worker(**kw), gpu_worker(target_kl=1e9, **kw)
    for _ in range(2):
        m0, m1 = off.iteration_step(), on.iteration_step()
    assert_same(moved(off.engine), moved(on.engine), ["p", "m", "v", "wimg"])
    assert off.engine.adam_step == on.engine.adam_step == 4 and m0["updates"] == m1["updates"] == 4
    assert m1["kl_stopped"] is False and m1["kl_trip"] is None and m1["steps_applied"] == 2
    assert m0["loss"] == m1["loss"]
    eng = off.engine
    assert eng.gate is None and eng._grad_sums is None and eng.metrics_buf.numel() == 11
    assert eng.grad_flat.numel() == eng.model.num_params and eng.loss_sums.numel() == 8
    assert eng.loss_sums.data_ptr() != eng.grad_flat.data_ptr() + 4 * eng.grad_flat.numel()
    assert not any(k in m0 for k in ("kl_stopped", "steps_applied", "kl_trip"))
    assert on.engine.metrics_buf.numel() == 15 and on.engine.loss_sums.data_ptr() == on.engine._grad_sums[-8:].data_ptr()


def _sync_mode_raises():
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        torch.ones(1, device=DEV).item()
        return False
    except RuntimeError:
        return True
    finally:
        torch.cuda.set_sync_debug_mode(prev)


@pytest.mark.parametrize("path", ["joint", "unfused", "clip"])
def test_deferred_gated_iteration_does_not_sync(path):
    kw = dict(HUMANOID, dtype="bf16x3", phase_timing=0, target_kl=TABLE_TARGET["Humanoid-v2"], **PATHS[path])
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
    assert m["kl_stopped"] is True and m["steps_applied"] == m["updates"] < 10
    m2 = w.finish_metrics()
    assert m2["updates"] == m["updates"] + m2["steps_applied"] == w.engine.adam_step


def test_resume_after_a_stopped_iteration_is_bit_identical(tmp_path):
    from pytorch_dppo_amd.runtime.launcher import run_worker
    base = dict(device="gpu", num_processes=1, dtype="bf16x3", update_kernels="heads",
                target_kl=TABLE_TARGET["Humanoid-v2"], **HUMANOID)
    ctx = DistContext(device=DEV)
    w_full, _ = run_worker(dppo_preset(max_iters=3, **base), ctx, evaluator=False, quiet=True)
    ck = str(tmp_path / "ck")
    w_two, _ = run_worker(dppo_preset(max_iters=2, checkpoint_dir=ck, **base), ctx, evaluator=False, quiet=True)
    st = torch.load(os.path.join(ck, "trainer_state.pt"), weights_only=True)
    assert w_two.last_metrics["kl_stopped"] is True
    assert st["adam_step"] == st["updates"] == w_two.engine.adam_step < 20
    w_res, _ = run_worker(dppo_preset(max_iters=3, resume=ck, **base), ctx, evaluator=False, quiet=True)
    assert w_res.iteration == 3 and w_res.engine.adam_step == w_full.engine.adam_step > st["adam_step"]
    assert_same(moved(w_full.engine), moved(w_res.engine))
    assert w_res.last_metrics["updates"] == w_full.last_metrics["updates"] == w_full.engine.adam_step


def test_train_py_runs_and_logs_the_fields(tmp_path):
    path = tmp_path / "train.jsonl"
    cmd = [sys.executable, "train.py", "--device", "gpu", "--env-name", "Humanoid-v2", "--max-iters", "2",
           "--num-processes", "1", "--num-envs", "256", "--exploration-size", "2048", "--batch-size", "2048", "--seed", "3",
           "--dtype", "bf16x3", "--target-kl", "2.43e-3", "--log-jsonl", str(path)]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=170)
    assert r.returncode == 0, r.stderr[-3000:]
    recs = [json.loads(l) for l in path.read_text().splitlines()]
    assert len(recs) == 2 and recs[0]["kl_stopped"] is True and recs[0]["steps_applied"] == 3 and recs[0]["updates"] == 3
    assert recs[0]["kl_trip"] > 2.43e-3 and recs[1]["updates"] == 3 + recs[1]["steps_applied"]
    assert all(math.isfinite(x[k]) for x in recs for k in ("loss", "grad_norm", "approx_kl"))


# ---- two ranks ---------------------------------------------------------------------------------------------------
def _two_rank_child(rank, world, port, out_dir):
    """one of 2 ranks sharing cuda:0 over gloo (per-rank seeds): per gradient comm, an ungated 4-step probe whose
    first KLs, summed over the ranks, give the target, then one gated iteration"""
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.set_num_threads(2)
    import torch.distributed as dist
    from pytorch_dppo_amd.parallel.dist import init_distributed
    base = init_distributed("gpu", rank=rank, world_size=world, backend="gloo", timeout_s=120)
    common = dict(HUMANOID, dtype="bf16x3", num_epoch=4, num_processes=world, dist_backend="gloo", verify_sync_every=1,
                  update_kernels="heads")
    out = {}
    for gc in ("auto", "process_group"):
        def ctx():
            return DistContext(rank=rank, world_size=world, local_rank=0, backend="gloo", device=base.device,
                               timeout_s=120, grad_comm=gc)
        c = ctx()
        probe = gpu_worker(c, grad_comm=gc, **common)
        eng = probe.engine
        prep(probe)
        eng.begin_update()
        kls = []
        for _ in range(4):
            eng.step(None, allreduce=c.grad_allreduce_fn(False))
            eng.finish_steps()
            pair = eng.loss_sums[[3, 5]].clone()
            dist.all_reduce(pair)
            kls.append(float(pair[0] / pair[1]))
        target = math.sqrt(kls[1] * kls[2])
        c = ctx()
        w = gpu_worker(c, grad_comm=gc, target_kl=target, **common)
        m = w.iteration_step()
        torch.cuda.synchronize()
        out[gc] = {"kls": kls, "gate": w.engine.gate.cpu(), "flat": w.model.flat.data.cpu(), "m": w.engine.adam_m.cpu(),
                   "ungated": probe.model.flat.data.cpu(), "in_sync": bool(m["replicas_in_sync"]),
                   "native": c.native is not None, "applied": m["steps_applied"], "loss": m["loss"],
                   "rewards": w.engine.rewards.cpu()}
    torch.save(out, os.path.join(out_dir, f"kl{rank}.pt"))
    base.destroy()


def test_two_ranks_gate_on_the_summed_kl(tmp_path):
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
    r0 = torch.load(tmp_path / "kl0.pt", weights_only=True)
    r1 = torch.load(tmp_path / "kl1.pt", weights_only=True)
    for gc in ("auto", "process_group"):
        a, b = r0[gc], r1[gc]
        print(gc, "summed kl", a["kls"], "gate", a["gate"].tolist())
        assert not torch.equal(a["rewards"], b["rewards"])                     # per-rank data
        assert a["kls"] == b["kls"] and a["kls"][1] < a["kls"][2]
        assert a["native"] == (gc == "auto")                                   # the in-stream branch / the process group
        assert torch.equal(a["gate"], b["gate"]) and torch.equal(a["flat"], b["flat"]) and torch.equal(a["m"], b["m"])
        assert a["in_sync"] and b["in_sync"]
        assert a["gate"].tolist()[:2] == [1.0, 3.0] and a["applied"] == b["applied"] == 3
        assert a["gate"].tolist()[2] == pytest.approx(a["kls"][2], rel=1e-5)   # the gate saw the summed pair
        assert a["loss"] == b["loss"]                                          # ... and the logged sums are global
        assert not torch.equal(a["flat"], a["ungated"])                        # the 4th step was not applied
    # the two comm paths agree bit for bit
    assert torch.equal(r0["auto"]["flat"], r0["process_group"]["flat"])
    assert torch.equal(r0["auto"]["gate"], r0["process_group"]["gate"])
