"""The wgrad's k-loop (csrc/wgrad.hip): operand layouts as template parameters, inline-asm fragment
reads with one settle per read group, and the ring of half-stage units of the split-bf16 wide
tiles.

GPU cases: ``ext.wgrad`` on hand-written task records over EXACT data.  Operand values are h + l
with h in {+-1, +-2} and l in {-1, 0, 1} * 2^-10, so bf16(h + l) == h and the split-bf16 lo part is
l exactly; every partial product is a multiple of 2^-10 and a sum over <= 512 rows needs <= 21
bits: any fp32 summation order is exact, and each slab must EQUAL the fp64 reference
Gh^T Xh + Gh^T Xl + Gl^T Xh over its chunk's rows (the lo * lo term is the one the kernel drops; at
bf16 only h survives the encoding).  The values are independent per element, so a swapped row,
feature, half or unit cannot cancel.

CPU case: the ISA of the split-bf16 / bf16 kernels carries no s_waitcnt vmcnt(0) inside a k-loop
(the compiler used to drain the DMA ring in front of every row-major fragment read) and reads each
group of fragments as one batch.
"""
import functools
import os
import re
import shutil
import subprocess

import pytest
import torch

from pytorch_dppo_amd.config import dppo_preset
from pytorch_dppo_amd.models.actor_critic import fm_index
from pytorch_dppo_amd.ops import _build, storage

DEV = torch.device("cuda", 0) if torch.cuda.is_available() else None
ROWS = 384        # 24 envs x 16 steps: chunks of 64, 128 and 192 rows
FEATS = 512       # the widest Humanoid operand (v_fc1's 500 outputs, v_fc2's 500 inputs)
CHUNKS = [(0, 64), (64, 192), (192, 384)]


@functools.lru_cache(maxsize=None)
def _engine(dtype):
    """an engine of Humanoid dims at 384 rows: the extension, the dt code and the operand heights"""
    from pytorch_dppo_amd.envs import get_spec, make_vec_env
    from pytorch_dppo_amd.models.actor_critic import ActorCritic
    from pytorch_dppo_amd.runtime.engine_hip import HipEngine
    from pytorch_dppo_amd.utils.obs_stats import RunningObsStats
    p = dppo_preset(device="gpu", env_name="Humanoid-v2", num_envs=24, exploration_size=ROWS, batch_size=ROWS,
                    dtype=dtype, update_kernels="heads")
    spec = get_spec(p.env_name)
    torch.manual_seed(0)
    model = ActorCritic(spec.obs_dim, spec.act_dim, p.hidden).to(DEV)
    env = make_vec_env(spec, p.num_envs, seed=p.seed, device=DEV)
    eng = HipEngine(p, model, env, RunningObsStats(spec.obs_dim, DEV), DEV, 0)
    assert eng.ldT == ROWS and max(eng.g_rows) == FEATS and max(eng.x_rows) == FEATS
    return eng


@functools.lru_cache(maxsize=None)
def _values(dtype):
    """(hi, lo) fp64 parts [ROWS][FEATS] of the dY and the X master operand, as the kernel sees them"""
    eng = _engine(dtype)
    gen = torch.Generator().manual_seed(1234)
    out = []
    for _ in range(2):
        h = (torch.randint(0, 2, (ROWS, FEATS), generator=gen) + 1) * (torch.randint(0, 2, (ROWS, FEATS), generator=gen) * 2 - 1)
        lo = (torch.randint(0, 3, (ROWS, FEATS), generator=gen) - 1) * 2.0 ** -10
        x = (h.double() + lo.double()).float()
        assert torch.equal(x.double(), h.double() + lo.double())
        assert torch.equal(x.to(torch.bfloat16).double(), h.double())           # bf16(h + l) == h
        dec = storage.decode(storage.encode(x, eng.dt), eng.dt)
        if dtype == "bf16x3":
            assert torch.equal(dec, x)                                           # decode(encode(x)) == x
            assert (lo != 0).float().mean().item() > 0.6
        else:
            assert torch.equal(dec.double(), h.double())
            lo = torch.zeros_like(lo)
        out.append((h.double().to(DEV), lo.double().to(DEV), x.to(DEV)))
    return out


@functools.lru_cache(maxsize=None)
def _operand(dtype, side, width, rm):
    """the first `width` features of a master operand in storage precision: row-major
    [ROWS][width], or fragment-major [width][ROWS]"""
    eng = _engine(dtype)
    x = _values(dtype)[side][2][:, :width].contiguous()
    if rm:
        return storage.encode(x, eng.dt).view(-1)
    f = torch.arange(width, device=DEV).repeat_interleave(ROWS)
    c = torch.arange(ROWS, device=DEV).repeat(width)
    flat = torch.zeros(width * ROWS, device=DEV)
    flat[fm_index(f, c, ROWS)] = x.t().reshape(-1)
    return storage.encode(flat, eng.dt)


def _run(dtype, layer, tiles, g_rm, x_rm):
    """one launch: every (nq, kq, n0, k0) of `tiles` over the three chunks; each slab vs fp64"""
    eng = _engine(dtype)
    gw, xw = eng.g_rows[layer], eng.x_rows[layer]
    recs, off = [], 0
    for nq, kq, n0, k0 in tiles:
        assert eng.ext.wgrad_task_ok(eng.dt, nq, kq) and n0 + 64 * nq <= gw and k0 + 64 * kq <= xw
        for m0, m1 in CHUNKS:
            recs.append([layer, n0, k0, m0, m1, off, nq, kq])
            off += 64 * nq * 64 * kq
    th = torch.tensor(recs, dtype=torch.int32).view(-1)
    slab = torch.full((off,), float("nan"), device=DEV)
    empty = storage.encode(torch.zeros(8, device=DEV), eng.dt)
    gT = [_operand(dtype, 0, gw, g_rm) if i == layer else empty for i in range(6)]
    xT = [_operand(dtype, 1, xw, x_rm) if i == layer else empty for i in range(6)]
    g_rows = [gw if i == layer else 0 for i in range(6)]
    x_rows = [xw if i == layer else 0 for i in range(6)]
    rm = [0] * 12
    rm[layer], rm[6 + layer] = int(g_rm), int(x_rm)
    eng.ext.wgrad(eng.dt, gT, xT, g_rows, x_rows, ROWS, th.to(DEV), th, slab, *eng._q8_args(), rm)
    torch.cuda.synchronize()
    (gh, gl, _), (xh, xl, _) = _values(dtype)
    for layer_, n0, k0, m0, m1, o, nq, kq in recs:
        G = [t[m0:m1, n0:n0 + 64 * nq] for t in (gh, gl)]
        X = [t[m0:m1, k0:k0 + 64 * kq] for t in (xh, xl)]
        ref = G[0].t() @ X[0] + G[0].t() @ X[1] + G[1].t() @ X[0]
        got = slab[o:o + ref.numel()].view_as(ref).double()
        assert torch.equal(got, ref), ((nq, kq, n0, k0, m0, m1), (got - ref).abs().max().item(),
                                       (got != ref).float().mean().item())


LAYOUTS = [(False, False), (False, True), (True, False), (True, True)]   # (dY, X) row-major
# (layer, [(nq, kq, n0, k0)]): Humanoid p_fc1 0 = 128 x 384, p_fc2 1 = 128 x 128, v_fc1 3 = 512 x 384,
# v_fc2 4 = 128 x 512
TILES = {
    "1x1": (1, [(1, 1, 0, 0), (1, 1, 64, 64)]),
    "2x2": (1, [(2, 2, 0, 0)]),
    "1x5": (0, [(1, 5, 64, 64)]),
    "5x1": (3, [(5, 1, 128, 320)]),
    "4x3": (3, [(4, 3, 0, 0), (4, 3, 256, 192)]),      # half-stage ring (28 of 32 slots)
    "2x6": (0, [(2, 6, 0, 0)]),                        # half-stage ring (32 slots)
    "2x5": (0, [(2, 5, 0, 64)]),                       # half-stage ring (28 of 32 slots, 8 of dY)
    "2x8": (4, [(2, 8, 0, 0)]),                        # full-stage wide ring (40 slots)
    "4x2+2x4": (3, [(4, 2, 256, 64), (2, 4, 128, 128)]),
}


@pytest.mark.gpu
@pytest.mark.parametrize("g_rm,x_rm", LAYOUTS, ids=lambda v: "rm" if v else "fm")
@pytest.mark.parametrize("tile", list(TILES))
@pytest.mark.parametrize("dtype", ["bf16x3", "bf16"])
def test_wgrad_slabs_equal_fp64_reference(dtype, tile, g_rm, x_rm):
    layer, tiles = TILES[tile]
    _run(dtype, layer, tiles, g_rm, x_rm)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["bf16x3", "bf16"])
def test_wgrad_mixed_bodies_in_one_launch(dtype):
    """one launch whose workgroups take different loop bodies (one quadrant per wave, half-stage
    and full-stage wide) over one layer's operands — v_fc1 as the update runs it: dY
    fragment-major, X the observation rows"""
    _run(dtype, 3, [(4, 3, 256, 0), (2, 2, 64, 256), (1, 1, 448, 320), (2, 6, 384, 0), (5, 1, 0, 64), (4, 4, 0, 128)],
         False, True)


# ---- the ISA (no GPU) -------------------------------------------------------------------------

def _loops(body):
    """the loops of a function — the strongly connected components of its control-flow graph —
    each as the instructions of its basic blocks in layout order.  (The layout is rotated, the
    header sits in the middle, so the span from a branch target to a backward branch is not the
    loop; and a branch to a block laid out earlier need not close a cycle at all.)"""
    blocks, names = [[]], {}
    for ln in body:
        ln = ln.strip()
        m = re.match(r"^(\.LBB\d+_\d+):", ln)
        if m:
            if blocks[-1]:
                blocks.append([])
            names[m.group(1)] = len(blocks) - 1
        elif ln and not ln.startswith(";") and not ln.startswith("."):
            blocks[-1].append(ln)
            if re.match(r"s_c?branch|s_endpgm|s_setpc", ln):
                blocks.append([])
    succ = []
    for i, b in enumerate(blocks):
        last = b[-1] if b else ""
        s = [] if re.match(r"s_branch|s_endpgm|s_setpc", last) or i + 1 == len(blocks) else [i + 1]
        m = re.match(r"s_c?branch\S*\s+(\.LBB\d+_\d+)", last)
        if m:
            s.append(names[m.group(1)])
        succ.append(s)
    # Tarjan, iterative
    index, low, on, stack, comps, n = {}, {}, set(), [], [], 0
    for root in range(len(blocks)):
        if root in index:
            continue
        work = [(root, 0)]
        while work:
            v, pi = work.pop()
            if pi == 0:
                index[v] = low[v] = n
                n += 1
                stack.append(v)
                on.add(v)
            descended = False
            for k in range(pi, len(succ[v])):
                w = succ[v][k]
                if w not in index:
                    work.append((v, k + 1))
                    work.append((w, 0))
                    descended = True
                    break
                if w in on:
                    low[v] = min(low[v], index[w])
            if descended:
                continue
            if low[v] == index[v]:
                comp = []
                while True:
                    w = stack.pop()
                    on.discard(w)
                    comp.append(w)
                    if w == v:
                        break
                if len(comp) > 1 or v in succ[v]:
                    comps.append(sorted(comp))
            if work:
                u = work[-1][0]
                low[u] = min(low[u], low[v])
    return [[ln for b in comp for ln in blocks[b]] for comp in comps]


@pytest.mark.skipif(not (os.path.exists(_build.HIPCC) or shutil.which(_build.HIPCC)), reason="no hipcc")
def test_wgrad_k_loops_keep_the_dma_ring_in_flight(tmp_path):
    """Between every k-loop's header and back edge of wgrad_kernel<split-bf16 | bf16, *>: no
    s_waitcnt on vmcnt but the source's own counted wait in front of the barrier — counted > 0 in
    every body but the full-stage wide one at split-bf16, whose 2-stage ring waits to 0 — and the
    fragment reads of a step come in batches: >= 8 before the first lgkmcnt(0), at most one more
    lgkmcnt(0) per step (the second quadrant's 4 dY fragments).  s_waitcnt vmcnt(0) per kernel,
    before -> after this test's change: <3,true> 46 -> 21, <3,false> 18 -> 8, <1,true> 44 -> 16,
    <1,false> 18 -> 8 (what is left drains the ring after the loop)."""
    out = tmp_path / "wgrad.s"
    cmd = [_build.HIPCC] + _build.device_flags() + ["--offload-device-only", "-S",
                                                    os.path.join(_build.CSRC, "wgrad.hip"), "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    funcs, cur = {}, None
    for ln in out.read_text().split("\n"):
        m = re.match(r"^(_Z\w*wgrad_kernelILi(\d)ELb(\d)E\w*):", ln)
        if m:
            cur = (int(m.group(2)), bool(int(m.group(3))))
            funcs[cur] = []
        elif ln.startswith(".Lfunc_end"):
            cur = None
        elif cur is not None:
            funcs[cur].append(ln)
    # bodies per kernel: 4 layouts x (2 one-quadrant slot counts [+ 2 wide])
    for key, nbodies in {(3, True): 16, (3, False): 8, (1, True): 16, (1, False): 8}.items():
        kloops = [lp for lp in _loops(funcs[key]) if any(i.startswith("s_barrier") for i in lp)
                  and any(i.startswith("v_mfma") for i in lp)]
        assert len(kloops) == nbodies, (key, len(kloops))
        drained = 0
        for lp in kloops:
            nm = sum(i.startswith("v_mfma") for i in lp)
            for j, i in enumerate(lp):
                if i.startswith("s_waitcnt") and "vmcnt" in i:
                    assert lp[j + 1].startswith("s_barrier"), (key, i, lp[j + 1])     # the source's wait
                    if "vmcnt(0)" in i:
                        drained += 1
                        # split-bf16, two quadrants per wave, the 5-slot-per-wave ring of 2 full stages
                        ndma = sum(x.startswith("global_load_lds") for x in lp)
                        assert key == (3, True) and nm == 96 and ndma == 20, (key, nm, ndma)
            rd = [j for j, i in enumerate(lp) if i.startswith("ds_read")]
            waits = [j for j, i in enumerate(lp) if i.startswith("s_waitcnt") and "lgkmcnt(0)" in i and rd[0] < j]
            assert len(rd) >= 8 and 1 <= len(waits) <= 2, (key, len(rd), len(waits))
            assert sum(j < waits[0] for j in rd) >= 8, (key, "first read group split by a wait")
            assert all(j < waits[-1] for j in rd)
            if len(waits) == 2:
                assert sum(waits[0] < j < waits[1] for j in rd) >= 4
        assert drained == (4 if key == (3, True) else 0), (key, drained)
