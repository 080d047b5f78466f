"""The gathers' streaming form (csrc/common.h slab_sum4 / slab_quad, kernels.h SlabTiles;
docs/ARCHITECTURE.md §26): the slab elements summed by quads — 16-byte chunk loads, two batches in flight,
indices from the tile table — beside the reduce items (item_reduce).  Every sum keeps the per-element form's
order, so everything here is compared with ``torch.equal`` against a reference that adds in that order in
fp32.

A Humanoid-dims engine at 2,176 rows (136 envs x 16 steps): the layer widths shape the tiles, the row count
only sets how many chunks exist (34 blocks of 64 rows: a tile has ceil(34 / k) chunks).  Joint plans for
6 / 36 / 100 / 256 tasks give tiles of 1, 5, 6, 7, 12, 17 and 34 chunks: one chunk, fewer than a batch, exactly
one batch (``ext.slab_sum_batch`` = 6), one batch + 1, and more than two batches.

grad_norm: the fused launch leaves per-block fp32 sums of squares in norm_part; a thread adds the 4 lanes of each
of its q quads with one rounding each (fmaf), the block tree adds 8 more levels, all terms >= 0: the fp64 sum of
the entries is within (1 + 2^-24)^(4 q + 8) - 1, relative, of the fp64 sum of squares of the gradient written.
"""
import functools
import math
import os
import re
import shutil
import subprocess

import pytest
import torch

from pytorch_dppo_amd.config import dppo_preset
from pytorch_dppo_amd.ops import _build

DEV = torch.device("cuda", 0) if torch.cuda.is_available() else None
ENVS, ROWS = 136, 2176
PLANS = (6, 36, 100, 256)
SCALE = 1.0 / ROWS


@functools.lru_cache(maxsize=None)
def _engine(dtype):
    from pytorch_dppo_amd.envs import get_spec, make_vec_env
    from pytorch_dppo_amd.models.actor_critic import ActorCritic
    from pytorch_dppo_amd.runtime.engine_hip import HipEngine
    from pytorch_dppo_amd.utils.obs_stats import RunningObsStats
    p = dppo_preset(device="gpu", env_name="Humanoid-v2", num_envs=ENVS, exploration_size=ROWS, batch_size=ROWS,
                    dtype=dtype, update_kernels="heads")
    spec = get_spec(p.env_name)
    torch.manual_seed(0)
    model = ActorCritic(spec.obs_dim, spec.act_dim, p.hidden).to(DEV)
    env = make_vec_env(spec, p.num_envs, seed=p.seed, device=DEV)
    eng = HipEngine(p, model, env, RunningObsStats(spec.obs_dim, DEV), DEV, 0)
    assert eng.ldT == ROWS and eng.heads
    return eng


@functools.lru_cache(maxsize=None)
def _plan(dtype, n_tasks):
    """the joint plan of ``n_tasks`` tasks: (bucket, src_off, src_meta); the engine keeps its own plan"""
    eng = _engine(dtype)
    saved = eng.buckets, eng.src_off, eng.src_meta
    eng._build_wgrad_plan(eng.model, target_wgs=n_tasks, joint=True)
    out = eng.buckets[0], eng.src_off, eng.src_meta
    eng.buckets, eng.src_off, eng.src_meta = saved
    return out


@functools.lru_cache(maxsize=None)
def _slab(dtype, n_tasks, seed=0):
    """the plan's slab filled with seeded fp32 normals, and the order-exact reference of every slab element:
    element i = (((x_0 + x_1) + x_2) + ...) over its tile's chunks x_c = slab[src_off[i] + c * stride], then
    * scale — from src_off / src_meta alone (the per-element definition), not from the tile table.  NaN elsewhere."""
    b, so, sm = _plan(dtype, n_tasks)
    gen = torch.Generator(device=DEV).manual_seed(1000 * n_tasks + seed)
    slab = torch.randn(b["slab"].numel(), generator=gen, device=DEV, dtype=torch.float32)
    ref = torch.full((so.numel(),), float("nan"), device=DEV)
    scale = torch.tensor(SCALE, dtype=torch.float32, device=DEV)
    for mv in sm.unique().tolist():
        if mv == 0:
            continue
        i = (sm == mv).nonzero().flatten()
        off, nch, st = so[i].long(), mv >> 5, (mv & 31) << 12
        s = slab[off]
        for c in range(1, nch):
            s = s + slab[off + c * st]
        ref[i] = s * scale
    return slab, ref


def _items(eng):
    return eng.items["joint"]


def _gather(eng, plan, slab, part, npblk, items, tiles=True):
    """grad_gather over the whole flat vector into a NaN-filled gradient; (grad, loss_out)"""
    b, so, sm = plan
    grad = torch.full((so.numel(),), float("nan"), device=DEV)
    loss = torch.full((8,), float("nan"), device=DEV)
    eng.ext.grad_gather(slab, so, sm, part, npblk, part.shape[1], *items, SCALE, grad, loss, b["runs"],
                        *(eng._tiles(b) if tiles else ()))
    torch.cuda.synchronize()
    return grad, loss


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["bf16x3", "bf16"])
def test_slab_sums_equal_the_order_exact_reference(dtype):
    eng = _engine(dtype)
    B = eng.ext.slab_sum_batch
    names = (("p_fc1",) if eng.phead_p2 else ("p_fc1", "p_fc2")) + ("v_fc1", "v_fc2")
    want = torch.zeros(eng.model.num_params, dtype=torch.bool, device=DEV)
    for nm in names:
        for kind in ("weight", "bias"):
            o, n = eng.model.offsets[f"{nm}.{kind}"]
            want[o:o + n] = True
    seen = set()
    empty = torch.empty(0, dtype=torch.int32, device=DEV)
    for n_tasks in PLANS:
        plan = _plan(dtype, n_tasks)
        b, so, sm = plan
        assert len(eng._tiles(b)) == 2, "the plan must come with a tile table"
        seen |= {r[1] for r in b["tile_rows"]}
        assert torch.equal(sm > 0, want)            # every element of the wgrad layers, the bias columns included
        slab, ref = _slab(dtype, n_tasks)
        for tiles in (True, False):                 # the streaming form, and the per-element form it must equal
            grad, _ = _gather(eng, plan, slab, eng.part_joint, eng.nhead_blk, (empty, empty), tiles)
            assert torch.equal(grad[want], ref[want]), (n_tasks, tiles)
            assert bool(grad[~want].isnan().all())  # ... and nothing else is written
    assert 1 in seen and any(1 < c < B for c in seen) and B in seen and B + 1 in seen and any(c > 2 * B for c in seen), \
        (B, sorted(seen))


def _item_reference(part, cols, scale):
    """item_reduce's order in torch fp32: row group g sums rows g, g + 8, ... in order, then groups 0..7 in order"""
    groups = []
    for g in range(8):
        s = torch.zeros(cols.numel(), device=DEV)
        for r in range(g, part.shape[0], 8):
            s = s + part[r, cols]
        groups.append(s)
    tot = groups[0]
    for g in range(1, 8):
        tot = tot + groups[g]
    return tot, tot * scale


@pytest.mark.gpu
@pytest.mark.parametrize("npblk", [1, 17, 128, 130, 512])
def test_item_sums_equal_the_order_exact_reference(npblk):
    eng = _engine("bf16x3")
    plan = _plan("bf16x3", 36)
    slab, _ = _slab("bf16x3", 36)
    rc, rd = _items(eng)
    gen = torch.Generator(device=DEV).manual_seed(npblk)
    part = torch.randn(npblk, eng.part_joint.shape[1], generator=gen, device=DEV, dtype=torch.float32)
    tot, scaled = _item_reference(part, rc.long(), torch.tensor(SCALE, dtype=torch.float32, device=DEV))
    to_grad = rd >= 0
    assert int((~to_grad).sum()) == 8               # the 8 loss sums
    for tiles in (True, False):
        grad, loss = _gather(eng, plan, slab, part, npblk, (rc, rd), tiles)
        assert torch.equal(grad[rd[to_grad].long()], scaled[to_grad]), tiles
        assert torch.equal(loss[(-1 - rd[~to_grad]).long()], tot[~to_grad]), tiles


def _state(eng, seed):
    """a seeded optimizer state over the whole flat vector: p, m, v, the weight image and (fp8) the e4m3 shadow"""
    gen = torch.Generator(device=DEV).manual_seed(seed)
    n = eng.model.num_params
    st = {"p": eng.model.flat.data.clone(), "m": 1e-3 * torch.randn(n, generator=gen, device=DEV),
          "v": 1e-6 * torch.rand(n, generator=gen, device=DEV), "g": torch.zeros(n, device=DEV),
          "wimg": eng.wimg.clone(), "state": torch.zeros(4, device=DEV), "loss": torch.zeros(8, device=DEV)}
    f8 = eng._f8()
    st["f8"] = (f8[0].clone(), f8[1], f8[2])
    return st


ADAM = (3e-4, 0.9, 0.999, 1e-5)
STEP = 3


def _fused(eng, plan, slab, part, st, norm_part, gate=None, tiles=True):
    b, so, sm = plan
    eng.ext.gather_adam(slab, so, sm, part, part.shape[0], part.shape[1], *_items(eng), b["runs"], SCALE, st["loss"],
                        st["g"], st["p"], st["m"], st["v"], *ADAM, 0 if gate is not None else STEP, st["state"],
                        norm_part, st["wimg"], eng.w_map, eng.wt_map, eng.dt, eng.no_q, *st["f8"],
                        eng.no_q if gate is None else gate, eng.no_q, *(eng._tiles(b) if tiles else ()))
    torch.cuda.synchronize()


def _pair(eng, plan, slab, part, st, norm_part):
    b, so, sm = plan
    eng.ext.grad_gather(slab, so, sm, part, part.shape[0], part.shape[1], *_items(eng), SCALE, st["g"], st["loss"],
                        b["runs"], *eng._tiles(b))
    eng.ext.adam(st["p"], st["g"], st["m"], st["v"], *ADAM, 0.0, st["state"], norm_part, st["wimg"], eng.w_map,
                 eng.wt_map, eng.dt, eng.no_q, STEP, *st["f8"], eng.no_q)
    torch.cuda.synchronize()


def _same(a, b, keys=("p", "m", "v", "g", "loss")):
    for k in keys:
        assert torch.equal(a[k], b[k]), k
    assert torch.equal(a["wimg"].view(torch.uint8), b["wimg"].view(torch.uint8))
    assert torch.equal(a["f8"][0], b["f8"][0])


def _part(eng, seed):
    gen = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randn(eng.nhead_blk, eng.part_joint.shape[1], generator=gen, device=DEV, dtype=torch.float32)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["bf16x3", "bf16", "fp8"])
def test_fused_launch_equals_the_gather_then_adam_pair(dtype):
    eng = _engine(dtype)
    part = _part(eng, 7)
    for n_tasks in PLANS:
        plan = _plan(dtype, n_tasks)
        slab, _ = _slab(dtype, n_tasks)
        a, b = _state(eng, n_tasks), _state(eng, n_tasks)
        _fused(eng, plan, slab, part, a, torch.zeros(eng.norm_n_whole, device=DEV))
        _pair(eng, plan, slab, part, b, torch.zeros(eng.norm_n_elem, device=DEV))
        _same(a, b)
        assert not torch.equal(a["p"], eng.model.flat.data)      # (the step moved the parameters)


@pytest.mark.gpu
def test_fused_launch_gated_and_stopped_moves_the_gradient_alone():
    eng = _engine("bf16x3")
    plan, (slab, _), part = _plan("bf16x3", 36), _slab("bf16x3", 36), _part(eng, 8)
    open_, stopped, start = _state(eng, 1), _state(eng, 1), _state(eng, 1)
    _fused(eng, plan, slab, part, open_, torch.zeros(eng.norm_n_whole, device=DEV))
    np_ = torch.full((eng.norm_n_whole,), float("nan"), device=DEV)
    _fused(eng, plan, slab, part, stopped, np_, gate=torch.tensor([1.0, 0.0, 0.0, 0.0], device=DEV))
    _same(stopped, start, keys=("p", "m", "v"))                  # p, m, v and the images stay
    assert torch.equal(stopped["g"], open_["g"]) and torch.equal(stopped["loss"], open_["loss"])
    assert bool(np_.isfinite().all()) and torch.equal(stopped["state"], start["state"])


@pytest.mark.gpu
def test_fused_launch_without_the_tile_table_is_the_per_element_form():
    eng = _engine("bf16x3")
    plan, (slab, _), part = _plan("bf16x3", 100), _slab("bf16x3", 100), _part(eng, 9)
    a, b = _state(eng, 2), _state(eng, 2)
    _fused(eng, plan, slab, part, a, torch.zeros(eng.norm_n_whole, device=DEV))
    _fused(eng, plan, slab, part, b, torch.zeros(eng.norm_n_elem, device=DEV), tiles=False)
    _same(a, b)


@pytest.mark.gpu
def test_norm_part_sums_the_gradient_written_and_nothing_stale():
    eng = _engine("bf16x3")
    plan, part = _plan("bf16x3", 256), _part(eng, 10)
    b = plan[0]
    nblk = eng.norm_n_whole
    slab_blocks = nblk - -(-_items(eng)[0].numel() // 32)
    assert slab_blocks >= 1
    depth = 4 * -(-b["nquads"] // (256 * slab_blocks)) + 8
    bound = (1.0 + 2.0 ** -24) ** depth - 1.0
    seen = []
    for seed in (0, 1):
        slab, _ = _slab("bf16x3", 256, seed)
        st = _state(eng, 3)
        norm_part = torch.full((nblk,), float("nan"), device=DEV)   # (an entry no block writes would poison the sum)
        _fused(eng, plan, slab, part, st, norm_part)
        got = norm_part.double().sum().item()
        ref = st["g"].double().square().sum().item()
        print(f"norm_part sum {got!r}  sum g^2 {ref!r}  rel {abs(got - ref) / ref:.3e}  bound {bound:.3e}")
        assert math.isfinite(got) and abs(got - ref) <= bound * ref, (got, ref, bound)
        seen.append(ref)
    assert seen[0] != seen[1]


@pytest.mark.skipif(shutil.which(_build.HIPCC) is None, reason="needs hipcc")
def test_isa_slab_loop_loads_16_bytes_and_keeps_a_batch_in_flight(tmp_path):
    """csrc/optim.hip with the build's flags: the split-bf16 streaming kernel's chunk loop — the basic blocks
    that issue a whole batch of chunk loads — loads 16 bytes per lane and never drains (no vmcnt(0))"""
    out = tmp_path / "optim.s"
    subprocess.run([_build.HIPCC] + _build.device_flags() + ["-S", "--cuda-device-only", "-o", str(out),
                                                            os.path.join(_build.CSRC, "optim.hip")], check=True)
    text = out.read_text()
    m = re.search(r"^(_ZN\S*gather_adam_kernelILi3ELb0ELb1E\S*):\s.*?s_endpgm", text, re.S | re.M)
    assert m, "the streaming gather + Adam kernel is missing"
    batch = 6
    src = open(os.path.join(_build.CSRC, "kernels.h")).read()
    assert re.search(rf"SLAB_SUM_BATCH = {batch};", src)
    blocks = [blk for blk in re.split(r"^\.LBB\S+:", m.group(0), flags=re.M)
              if len(re.findall(r"global_load_dwordx4", blk)) >= batch]
    assert blocks, "no block issues a batch of 16-byte loads"
    for blk in blocks:
        assert not re.search(r"s_waitcnt vmcnt\(0\)", blk), "the chunk loop drains between batches"
        assert not re.search(r"global_load_dword v\d+,", blk)
