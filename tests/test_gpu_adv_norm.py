"""``adv_norm_scope`` global | minibatch on the GPU engine: the statistics kernels (csrc/advnorm.hip) against the
oracle, the advantage operand of the three update kernels against the same launch on a pre-normalised buffer, an
engine iteration against a twin engine fed that buffer, the GPU worker against the CPU worker, and the plumbing: no
host sync, flag off, resume, two ranks, ``train.py``."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from pytorch_dppo_amd.config import dppo_preset
from pytorch_dppo_amd.ops import oracle
from pytorch_dppo_amd.parallel.dist import DistContext
from test_adv_norm import same_bits
from test_gpu_target_kl import (DEV, PATHS, ROOT, SMALL, _ext, _sync_mode_raises, assert_same, bits, gpu_worker,
                                minibatch_indices, moved, prep)
from test_target_kl import CHEETAH, HUMANOID, PENDULUM_MB, cpu_worker

pytestmark = pytest.mark.gpu

F32 = dict(dtype=torch.float32, device=DEV)
F64 = dict(dtype=torch.float64, device=DEV)
ON = dict(normalize_adv=True, adv_norm_scope="global")
WG_ROWS = 1024            # rows per workgroup of adv_stats_kernel; its 256 threads take 4 each
ONE_PASS = 256 * WG_ROWS  # rows whose partials one pass of adv_moments_kernel's 256 threads covers


# ---- the statistics kernels ----------------------------------------------------------------------------------------
def stats(adv, ret, idx, n, n_total=None, block=True, split=False):
    """(sums fp64[4], block fp32[4]) of the two-launch form, or with ``split`` of the three-launch one"""
    ext = _ext()
    part = torch.full((4 * int(ext.adv_stats_nblk(n)),), float("nan"), **F64)
    sums, blk = torch.full((4,), float("nan"), **F64), torch.full((4,), float("nan"), **F32)
    empty_i, none = torch.empty(0, dtype=torch.int32, device=DEV), torch.empty(0, **F32)
    nt = float(n if n_total is None else n_total)
    ext.adv_stats(adv, none if ret is None else ret, empty_i if idx is None else idx, n, part, sums, nt,
                  blk if (block and not split) else none)
    if split:
        ext.adv_block(sums, nt, blk)
    torch.cuda.synchronize()
    return sums.cpu(), blk.cpu()


SIZES = [2, 255, 256, 257, WG_ROWS - 1, WG_ROWS, WG_ROWS + 1, 65537, ONE_PASS + 1]


def data(kind, n, seed):
    g = torch.Generator().manual_seed(seed)
    if kind == "randn":
        return torch.randn(n, generator=g) * 3, torch.randn(n, generator=g) + 0.5
    if kind == "offset":
        return 1e3 + 1e-2 * torch.randn(n, generator=g), -1e3 + 1e-2 * torch.randn(n, generator=g)
    return torch.full((n,), 0.3), torch.full((n,), -7.25)


@pytest.mark.parametrize("kind", ["randn", "offset", "equal"])
@pytest.mark.parametrize("order", ["identity", "descending_duplicates"])
def test_statistics_kernels_against_the_oracle(kind, order):
    ext = _ext()
    assert ext.adv_stats_nblk(WG_ROWS) == 1 and ext.adv_stats_nblk(WG_ROWS + 1) == 2
    assert ext.adv_stats_nblk(ONE_PASS) == 256 and ext.adv_stats_nblk(ONE_PASS + 1) == 257
    for n in SIZES:
        adv, ret = data(kind, n, n)
        idx = None if order == "identity" else torch.flip(torch.arange(n) // 2, [0])     # rows (n-1)//2 .. 0, each twice
        want = oracle.adv_sums(adv, ret, idx)
        idx_d = None if idx is None else idx.to(DEV, torch.int32)
        sums, block = stats(adv.to(DEV), ret.to(DEV), idx_d, n)
        a = (adv if idx is None else adv[idx]).double()
        r = (ret if idx is None else ret[idx]).double()
        u = n * 2.0 ** -53
        bound = [u * float(a.abs().sum()), u * float((a * a).sum()), u * float(r.abs().sum()), u * float((r * r).sum())]
        err = (sums - want).abs().tolist()
        print(kind, order, n, "err", err, "bound", bound)
        assert all(e <= b for e, b in zip(err, bound)), (n, err, bound)
        # the block is the oracle's arithmetic on the kernel's own sums, bit for bit
        assert same_bits(block.numpy(), oracle.adv_block(sums, n).numpy()), (n, block, oracle.adv_block(sums, n))
        # the three-launch form (the sums alone, then the finish): the same bits
        sums3, block3 = stats(adv.to(DEV), ret.to(DEV), idx_d, n, split=True)
        assert torch.equal(sums3, sums) and same_bits(block3.numpy(), block.numpy())
        # a count of its own (the all-reduced form's n_total) and no return
        sums_a, block_a = stats(adv.to(DEV), None, idx_d, n, n_total=3 * n)
        assert torch.equal(sums_a[:2], sums[:2]) and sums_a[2:].tolist() == [0.0, 0.0]
        assert same_bits(block_a.numpy(), oracle.adv_block(sums_a, 3 * n).numpy()) and math.isnan(float(block_a[3]))
        if kind == "equal":
            assert float(block[2]) == 0.0 and float(block[1]) == float(np.float32(1e8))
            assert float(block[0]) == float(np.float32(0.3)) and math.isnan(float(block[3]))
        if kind == "offset" and n >= 255:
            assert float(block[2]) == pytest.approx(1e-2, rel=0.2)


def test_statistics_binding_refusals_come_before_any_launch():
    ext = _ext()
    n = 300
    adv, ret = torch.randn(n, **F32), torch.randn(n, **F32)
    part = torch.full((4 * int(ext.adv_stats_nblk(n)),), 7.0, **F64)
    sums, block = torch.full((4,), 7.0, **F64), torch.full((4,), 7.0, **F32)
    idx = torch.arange(n, dtype=torch.int32, device=DEV)
    ei, none = torch.empty(0, dtype=torch.int32, device=DEV), torch.empty(0, **F32)
    bad = [
        (adv, ret, ei, 1, part, sums, 1.0, block),                       # n >= 2
        (adv, ret, ei, n, part, sums, 1.0, block),                       # n_total >= 2
        (adv, ret, ei, n + 1, part, sums, float(n), block),              # more rows than the buffer
        (adv, ret, idx[:-1], n, part, sums, float(n), block),            # idx shorter than n
        (adv, ret, idx.to(torch.int64), n, part, sums, float(n), block),
        (adv, ret[:-1], ei, n, part, sums, float(n), block),             # ret of another length
        (adv, ret, ei, n, part[:3], sums, float(n), block),              # scratch too small
        (adv, ret, ei, n, part.float(), sums, float(n), block),
        (adv, ret, ei, n, part, sums[:3], float(n), block),
        (adv, ret, ei, n, part, sums.float(), float(n), block),
        (adv, ret, ei, n, part, sums, float(n), block[:3]),              # block of 4 floats
        (adv.double(), ret, ei, n, part, sums, float(n), block),
        (adv.cpu(), ret, ei, n, part, sums, float(n), block),
    ]
    for args in bad:
        with pytest.raises(RuntimeError):
            ext.adv_stats(*args)
    for args in ((sums[:3], float(n), block), (sums, float(n), block[:3]), (sums, 1.0, block), (sums, float(n), none),
                 (sums.float(), float(n), block)):
        with pytest.raises(RuntimeError):
            ext.adv_block(*args)
    with pytest.raises(RuntimeError):
        ext.adv_stats_nblk(0)
    torch.cuda.synchronize()
    assert bool((part == 7.0).all()) and bool((sums == 7.0).all()) and bool((block == 7.0).all())
    ext.adv_stats(adv, ret, idx, n, part, sums, float(n), block)         # ... and the legal call runs
    torch.cuda.synchronize()
    assert not bool((block == 7.0).any())


# ---- the operand in each update kernel -------------------------------------------------------------------------------
def engine_with_block(**kw):
    """a ``global`` engine after rollout / values / GAE whose block is set (raw advantages in the buffer)"""
    w = gpu_worker(**dict(ON, **kw))
    prep(w)
    w.engine.adv_sums(finish=True)
    torch.cuda.synchronize()
    return w


def one_grad(eng, idx, block_on):
    """one first-step gradient from a fixed engine state; ``block_on`` False: the launch without the operand"""
    keep = (eng._xT_valid, eng._q8_next, list(eng._q8_cal), eng.q8_amax.clone(), eng.adv_scope)
    eng.adv_scope = keep[4] if block_on else ""
    if not block_on:
        eng._adv_arg = eng.no_q
    eng.begin_update()
    eng.grad_flat.zero_()
    eng.loss_sums.zero_()
    eng.grad(idx)
    torch.cuda.synchronize()
    out = eng.grad_flat.clone(), eng.loss_sums.clone()
    eng._xT_valid, eng._q8_next, eng._q8_cal, eng.adv_scope = keep[0], keep[1], keep[2], keep[4]
    eng.q8_amax.copy_(keep[3])
    return out


OPERAND = [
    ("phead-bf16x3", dict(SMALL, dtype="bf16x3", update_kernels="heads"), "phead"),
    ("phead-bf16", dict(SMALL, dtype="bf16", update_kernels="heads"), "phead"),
    ("phead-ref-loss", dict(SMALL, dtype="bf16x3", update_kernels="heads", loss="dppo_ref"), "phead"),
    ("head0-bf16x3", dict(SMALL, dtype="bf16x3", update_kernels="heads", phead_kernel=False), "head"),
    ("head0-bf16-ref-loss", dict(SMALL, dtype="bf16", update_kernels="heads", phead_kernel=False, loss="dppo_ref"), "head"),
    ("head0-fp8", dict(SMALL, dtype="fp8", update_kernels="heads"), "head"),
    ("tile-fp32", dict(SMALL, dtype="fp32", update_kernels="tile"), "tile"),
    ("tile-bf16x3", dict(SMALL, dtype="bf16x3", update_kernels="tile"), "tile"),
    ("tile-bf16-ref-loss", dict(SMALL, dtype="bf16", update_kernels="tile", loss="dppo_ref"), "tile"),
    ("tile-fp8", dict(SMALL, dtype="fp8", update_kernels="tile"), "tile"),
    ("mb-head0-bf16x3", dict(PENDULUM_MB, dtype="bf16x3", update_kernels="heads"), "head"),
    ("mb-tile-fp32", dict(PENDULUM_MB, dtype="fp32", update_kernels="tile"), "tile"),
    ("mb-phead-bf16x3", dict(HUMANOID, batch_size=512, dtype="bf16x3", update_kernels="heads"), "phead"),
]


@pytest.mark.parametrize("name,kw,kernel", OPERAND, ids=[c[0] for c in OPERAND])
def test_update_kernels_apply_the_block_at_the_advantage_load(name, kw, kernel):
    w = engine_with_block(**kw)
    eng = w.engine
    assert {"phead": eng.phead, "head": eng.heads and not eng.phead, "tile": not eng.heads}[kernel]
    idx = None
    if eng.mb < eng.N:
        g = torch.Generator().manual_seed(2)
        idx = torch.randperm(eng.N, generator=g)[:eng.mb]
        idx[-3:] = idx[:3]                                 # duplicates, as the worker's wrap-around makes
    raw = eng.adv.clone()
    g_on, s_on = one_grad(eng, idx, True)
    assert torch.equal(eng.adv, raw)                       # the buffer stays raw
    b = eng.adv_block
    eng.adv.copy_((raw - b[0]) * b[1])                     # torch's two fp32 operations
    g_pre, s_pre = one_grad(eng, idx, False)
    assert torch.equal(bits(g_on), bits(g_pre)) and torch.equal(bits(s_on), bits(s_pre))
    assert bool(torch.isfinite(g_on).all()) and float(g_on.abs().max()) > 0
    # ... and it is not the launch without the operand on the raw buffer (the policy range; the value range is)
    eng.adv.copy_(raw)
    g_raw, _ = one_grad(eng, idx, False)
    (plo, phi), (vlo, vhi) = eng.head_range
    assert not torch.equal(g_raw[plo:phi], g_on[plo:phi])
    assert torch.equal(bits(g_raw[vlo:vhi]), bits(g_on[vlo:vhi]))      # the value head never reads adv or the block


def test_value_head_launch_ignores_the_block():
    eng = engine_with_block(**dict(SMALL, dtype="bf16x3", update_kernels="heads")).engine
    out = []
    for arg in (eng.adv_block, eng.no_q):
        eng.begin_update()
        mbt = eng._minibatch(None)
        eng._adv_arg = arg
        eng.part_h[1].fill_(float("nan"))
        eng._head_chain(1, *mbt)
        torch.cuda.synchronize()
        vlo, vhi = eng.head_range[1]
        out.append((eng.part_h[1].clone(), eng.grad_flat[vlo:vhi].clone()))
    assert torch.equal(bits(out[0][0]), bits(out[1][0])) and torch.equal(bits(out[0][1]), bits(out[1][1]))
    assert bool(torch.isfinite(out[0][1]).all())


# ---- engine end to end: a twin fed the pre-normalised buffer ---------------------------------------------------------
def twin_worker(scope, **kw):
    """a worker without normalize_adv that the test feeds: ``global``: after GAE its buffer is overwritten by torch's
    (adv - m) * s with the statistics kernels' block of the whole buffer; ``minibatch``: before every step, with the
    block of that step's rows.  ``raw`` keeps the advantages GAE left."""
    w = gpu_worker(**dict(kw, normalize_adv=False))
    eng, ext = w.engine, _ext()
    part = torch.zeros(4 * int(ext.adv_stats_nblk(eng.N)), **F64)
    sums, block = torch.zeros(4, **F64), torch.zeros(4, **F32)
    raw = {}
    gae, minibatch = eng.gae, eng._minibatch

    def gae_then_normalise():
        gae()
        raw["adv"] = eng.adv.clone()
        ext.adv_stats(eng.adv, eng.ret, eng.empty, eng.N, part, sums, float(eng.N), block)
        if scope == "global":
            eng.adv.copy_((raw["adv"] - block[0]) * block[1])

    def minibatch_on_step_rows(idx):
        if scope == "minibatch" and idx is not None:
            i32 = idx.reshape(-1).to(DEV, torch.int32)
            ext.adv_stats(raw["adv"], eng.no_q, i32, i32.numel(), part, sums, float(i32.numel()), block)
            eng.adv.copy_((raw["adv"] - block[0]) * block[1])
        elif scope == "minibatch":
            ext.adv_stats(raw["adv"], eng.ret, eng.empty, eng.N, part, sums, float(eng.N), block)
            eng.adv.copy_((raw["adv"] - block[0]) * block[1])
        return minibatch(idx)
    eng.gae, eng._minibatch = gae_then_normalise, minibatch_on_step_rows
    return w, raw


E2E = [(p, dict(SMALL, dtype="bf16x3", num_epoch=3, **PATHS[p])) for p in ("joint", "unfused", "tile", "clip")] + \
      [("tile_fp32", dict(SMALL, dtype="fp32", num_epoch=3, **PATHS["tile"])),
       ("joint_fp8", dict(SMALL, dtype="fp8", num_epoch=3, **PATHS["joint"]))]


@pytest.mark.parametrize("path,kw", E2E, ids=[c[0] for c in E2E])
def test_global_iteration_is_the_twins_on_the_prenormalised_buffer(path, kw):
    w = gpu_worker(**dict(ON, **kw))
    t, raw = twin_worker("global", **kw)
    for _ in range(2):
        m, mt = w.iteration_step(), t.iteration_step()
        assert_same(moved(w.engine), moved(t.engine))
        assert torch.equal(w.engine.adv, raw["adv"])                  # unchanged by the update
        assert m["loss"] == mt["loss"] and m["approx_kl"] == mt["approx_kl"]
    assert w.engine.adam_step == 6 and float(w.engine.adv.std()) > 0


MB_E2E = [("heads", dict(PENDULUM_MB, dtype="bf16x3", update_kernels="heads", num_epoch=2)),
          ("tile_fp32", dict(PENDULUM_MB, dtype="fp32", update_kernels="tile", num_epoch=2)),
          ("phead", dict(HUMANOID, batch_size=512, dtype="bf16x3", update_kernels="heads", num_epoch=1)),
          ("heads_gated_clip", dict(PENDULUM_MB, dtype="bf16x3", update_kernels="heads", num_epoch=2, target_kl=1e9,
                                    max_grad_norm=0.5)),
          ("full_batch", dict(SMALL, dtype="bf16x3", num_epoch=2))]


@pytest.mark.parametrize("name,kw", MB_E2E, ids=[c[0] for c in MB_E2E])
def test_minibatch_iteration_is_the_twins_step_by_step(name, kw):
    on = dict(normalize_adv=True, adv_norm_scope="minibatch")
    # step by step, by hand: every step's parameters
    w = gpu_worker(**dict(on, **kw))
    t, raw = twin_worker("minibatch", **kw)
    for x in (w, t):
        prep(x)
    w.engine.adv_sums(finish=True)
    w.engine.begin_update()
    t.engine.begin_update()
    steps = minibatch_indices(w)
    assert [None if i is None else i.tolist() for i in steps] == [None if i is None else i.tolist()
                                                                   for i in minibatch_indices(t)]
    for idx in steps:
        w.engine.step(idx)
        t.engine.step(idx)
        assert_same(moved(w.engine), moved(t.engine))
    assert torch.equal(w.engine.adv, raw["adv"]) and len(steps) == w.p.num_epoch * w.p.num_minibatches()
    # ... and through the worker
    w = gpu_worker(**dict(on, **kw))
    t, raw = twin_worker("minibatch", **kw)
    m, mt = w.iteration_step(), t.iteration_step()
    assert_same(moved(w.engine), moved(t.engine))
    assert torch.equal(w.engine.adv, raw["adv"]) and m["loss"] == mt["loss"]
    if w.engine.mb < w.engine.N:
        assert not torch.equal(w.engine.adv_blocks[0], w.engine.adv_blocks[1])    # the last step's block is its own


# ---- against the CPU worker ----------------------------------------------------------------------------------------
VS_CPU = [("fp32", dict(CHEETAH, update_kernels="tile"), "global"), ("bf16x3", dict(HUMANOID, update_kernels="heads"), "global"),
          ("fp32", dict(CHEETAH, update_kernels="tile", batch_size=96), "minibatch"),
          ("bf16x3", dict(HUMANOID, update_kernels="heads", batch_size=512), "minibatch")]


@pytest.mark.parametrize("dtype,shape,scope", VS_CPU)
def test_gpu_worker_follows_the_cpu_worker(dtype, shape, scope):
    kw = dict(shape, normalize_adv=True, adv_norm_scope=scope, num_epoch=1 if scope == "minibatch" else 3)
    cpu_kw = {k: v for k, v in kw.items() if k != "update_kernels"}
    wc, wg = cpu_worker(**cpu_kw), gpu_worker(dtype=dtype, **kw)
    assert torch.equal(wg.model.flat.data.cpu(), wc.model.flat.data)
    mc, mg = wc.iteration_step(), wg.iteration_step()
    steps = wg.p.num_epoch * wg.p.num_minibatches()
    assert steps in (3, 4) and mg["updates"] == mc["updates"] == steps
    # test_gpu_worker_trips_where_the_cpu_worker_does' bounds
    d = (wg.model.flat.data.cpu() - wc.model.flat.data).abs()
    print(dtype, scope, "max |dp|", d.max().item(), "frac > 1e-5", (d > 1e-5).float().mean().item(),
          "loss_value", mg["loss_value"], mc["loss_value"], "block", wg.engine.adv_block.tolist(), wc.engine.adv_block.tolist())
    assert d.max().item() <= 2 * wg.p.lr * steps + 1e-6
    assert (d > 1e-5).float().mean().item() < 0.01
    assert abs(mg["loss_value"] - mc["loss_value"]) < 1e-3 * (1 + abs(mc["loss_value"]))
    for k in ("adv_mean", "adv_std", "explained_variance"):
        assert mg[k] == pytest.approx(mc[k], rel=1e-3, abs=1e-4), k


# ---- plumbing --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scope,kw", [("global", dict(HUMANOID, num_epoch=2)),
                                      ("minibatch", dict(HUMANOID, batch_size=512, num_epoch=1, update_kernels="heads")),
                                      ("minibatch", dict(PENDULUM_MB, num_epoch=1, update_kernels="tile"))])
def test_deferred_iteration_does_not_sync(scope, kw):
    w = gpu_worker(**dict(kw, dtype="bf16x3", phase_timing=0, normalize_adv=True, adv_norm_scope=scope))
    w.iteration_step(defer=True)                 # (first call: allocations, kernel loads)
    torch.cuda.synchronize()
    if not _sync_mode_raises():
        pytest.skip("torch.cuda.set_sync_debug_mode('error') does not raise on .item() in this build")
    ptrs = (w.engine.adv_blocks.data_ptr(), w.engine.adv_part.data_ptr(), w.engine.metrics_buf.data_ptr())
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        m = w.iteration_step(defer=True)
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    torch.cuda.synchronize()
    assert m["adv_std"] > 0 and math.isfinite(m["adv_mean"])
    assert ptrs == (w.engine.adv_blocks.data_ptr(), w.engine.adv_part.data_ptr(), w.engine.metrics_buf.data_ptr())
    m2 = w.finish_metrics()
    assert m2["iteration"] == m["iteration"] + 1 and m2["adv_std"] == float(w.engine.adv_block[2])


def test_flag_off_holds_nothing_and_passes_an_empty_operand():
    for kw in (dict(), dict(normalize_adv=True), dict(normalize_adv=True, adv_norm_scope="rank")):
        w = gpu_worker(**dict(SMALL, dtype="bf16x3", **kw))
        eng = w.engine
        m = w.iteration_step()
        assert eng.adv_block is None and not hasattr(eng, "adv_blocks") and not hasattr(eng, "adv_part")
        assert eng.metrics_buf.numel() == 11 and not any(k in m for k in ("adv_mean", "adv_std", "explained_variance"))
        a = eng._update_args(eng.empty, True, False, eng.part_joint)
        loss = [0.0, 1.0, float(eng.std_var), 1.0, float(w.p.clip), float(w.p.ent_coeff)]
        want = (eng.dt, eng.A, eng.tbufs, eng.layout, eng.x_buf, eng.empty, 0, eng.mb, eng.wimg, eng.scales,
                eng.model.flat.data, eng.log_std_old, eng.actions, eng.logp, eng.adv, eng.ret, eng.values_buf,
                eng.mu_prev, eng.v_prev, loss, eng.ldT, eng.part_joint, eng.part_joint.shape[1], False)
        assert len(a) == 25 and a[24].numel() == 0 and a[24] is eng.no_q
        for x, y in zip(a[:24], want):
            assert (x.data_ptr() == y.data_ptr() and x.shape == y.shape) if torch.is_tensor(y) else (x == y)
    on = gpu_worker(**dict(SMALL, dtype="bf16x3", **ON))
    m = on.iteration_step()
    assert on.engine.metrics_buf.numel() == 14 and on.engine._update_args(on.engine.empty, True, False,
                                                                        on.engine.part_joint)[24] is on.engine.adv_block
    a = on.engine.adv.double().cpu().numpy()
    assert m["adv_std"] == pytest.approx(a.std(ddof=1), rel=1e-6) and m["adv_mean"] == pytest.approx(a.mean(), rel=1e-5)
    # scope rank normalised the buffer in place, as ever
    assert abs(float(w.engine.adv.mean())) < 1e-5 and float(w.engine.adv.std()) == pytest.approx(1.0, rel=1e-4)


@pytest.mark.parametrize("scope", ["global", "minibatch"])
def test_resume_is_bit_identical(tmp_path, scope):
    from pytorch_dppo_amd.runtime.launcher import run_worker
    base = dict(PENDULUM_MB, device="gpu", num_processes=1, dtype="bf16x3", num_epoch=2, normalize_adv=True,
                adv_norm_scope=scope)
    ctx = DistContext(device=DEV)
    w_full, _ = run_worker(dppo_preset(max_iters=3, **base), ctx, evaluator=False, quiet=True)
    ck = str(tmp_path / "ck")
    run_worker(dppo_preset(max_iters=2, checkpoint_dir=ck, **base), ctx, evaluator=False, quiet=True)
    w_res, _ = run_worker(dppo_preset(max_iters=3, resume=ck, **base), ctx, evaluator=False, quiet=True)
    assert w_res.iteration == 3
    assert_same(moved(w_full.engine), moved(w_res.engine))
    assert torch.equal(bits(w_full.engine.adv_blocks), bits(w_res.engine.adv_blocks))
    assert w_res.last_metrics["adv_std"] == w_full.last_metrics["adv_std"]


def test_train_py_logs_the_three_fields(tmp_path):
    path = tmp_path / "train.jsonl"
    cmd = [sys.executable, "train.py", "--device", "gpu", "--env-name", "Pendulum-v0", "--max-iters", "2",
           "--num-processes", "1", "--num-envs", "64", "--exploration-size", "1024", "--batch-size", "256", "--seed", "3",
           "--dtype", "bf16x3", "--reward-clip", "0", "--normalize-adv", "true", "--adv-norm-scope", "minibatch",
           "--log-jsonl", str(path)]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=170)
    assert r.returncode == 0, r.stderr[-3000:]
    recs = [json.loads(l) for l in path.read_text().splitlines()]
    assert len(recs) == 2
    for x in recs:
        assert x["adv_std"] > 0 and math.isfinite(x["adv_mean"]) and x["explained_variance"] < 1.0
        assert all(math.isfinite(x[k]) for k in ("loss", "grad_norm", "approx_kl"))


# ---- two ranks -------------------------------------------------------------------------------------------------------
def _two_rank_child(rank, world, port, out_dir):
    """one of 2 ranks sharing cuda:0 over gloo (per-rank seeds): per gradient comm, two ``global`` iterations"""
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.set_num_threads(2)
    from pytorch_dppo_amd.parallel.dist import init_distributed
    base = init_distributed("gpu", rank=rank, world_size=world, backend="gloo", timeout_s=120)
    common = dict(SMALL, dtype="bf16x3", num_epoch=2, num_processes=world, dist_backend="gloo", verify_sync_every=1,
                  update_kernels="heads", **ON)
    out = {}
    for gc in ("auto", "process_group"):
        c = DistContext(rank=rank, world_size=world, local_rank=0, backend="gloo", device=base.device, timeout_s=120,
                        grad_comm=gc)
        w = gpu_worker(c, grad_comm=gc, **common)
        its = []
        for _ in range(2):
            m = w.iteration_step()
            torch.cuda.synchronize()
            eng = w.engine
            its.append({"block": eng.adv_block.cpu(), "adv": eng.adv.cpu(), "ret": eng.ret.cpu(),
                        "sums": eng.adv_sums_buf[0].cpu(), "in_sync": bool(m["replicas_in_sync"]),
                        "adv_std": m["adv_std"], "flat": w.model.flat.data.cpu()})
        out[gc] = {"its": its, "native": c.native is not None}
    torch.save(out, os.path.join(out_dir, f"adv{rank}.pt"))
    base.destroy()


def test_two_ranks_hold_one_global_block(tmp_path):
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
    r0 = torch.load(tmp_path / "adv0.pt", weights_only=True)
    r1 = torch.load(tmp_path / "adv1.pt", weights_only=True)
    for gc in ("auto", "process_group"):
        assert r0[gc]["native"] == (gc == "auto")
        for a, b in zip(r0[gc]["its"], r1[gc]["its"]):
            assert not torch.equal(a["adv"], b["adv"])                         # per-rank data
            assert same_bits(a["block"].numpy(), b["block"].numpy()) and torch.equal(a["sums"], b["sums"])
            assert a["in_sync"] and b["in_sync"] and torch.equal(a["flat"], b["flat"])
            # the block is the oracle's of the summed sums (bit for bit) and of both ranks' saved advantages
            n = a["adv"].numel() + b["adv"].numel()
            assert same_bits(a["block"].numpy(), oracle.adv_block(a["sums"], n).numpy())
            cat = oracle.adv_block(oracle.adv_sums(torch.cat([a["adv"], b["adv"]]), torch.cat([a["ret"], b["ret"]])), n)
            np.testing.assert_allclose(a["block"].numpy(), cat.numpy(), rtol=1e-6)
            rank_a = oracle.adv_block(oracle.adv_sums(a["adv"], a["ret"]), a["adv"].numel())
            rank_b = oracle.adv_block(oracle.adv_sums(b["adv"], b["ret"]), b["adv"].numel())
            assert not torch.equal(rank_a, rank_b) and a["adv_std"] == float(a["block"][2])
    # the two comm paths agree bit for bit
    assert torch.equal(r0["auto"]["its"][1]["flat"], r0["process_group"]["its"][1]["flat"])
