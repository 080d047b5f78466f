"""Every form of the optimizer step against the float64 Adam and the exact image bits of
``tests/test_optimizer_reference.py`` (the references, the bounds, the edge sets and their CPU tests live there).

a  the launch forms through the bindings (``ext.adam`` / ``ext.gather_adam``): the one-launch no-clip kernel, the
   sumsq + adam pair reached by ``host_step = 0`` and by ``set_adam_fused(0)``, the pair with the limit above the norm
   (whose bits must be the no-clip form's), below it, and on an all-zero gradient, ``gather_adam`` per element over a
   synthetic gather (1 - 5 chunks per element, two slab runs around a hole, 41 reduce items over 19 partial rows,
   destinations >= 0 and -1 - q), and the gated twin of each; storage types 0, 1, 3 (and 2, the e4m3 image, on the
   no-clip form).  The set-up is ``test_gpu_lr_schedule.flat_case`` plus a block with ``w_map = -1`` (some of whose
   ``wt_map`` points at a slot nobody may write), permuted maps, a block of ``p == 0`` (put back before every step),
   the edge gradients (+-1e15 in a twin of every form's case: they swamp the norm), and a sentinel in every image
   unit.  Steps t = 1, 2, 3, 10, 1000, 100000 are chained; before each the device's (p, m, v) are read back and the
   reference starts from them, so every step is judged alone.  One clip case has gradients of norm ~1e-3, where the
   coefficient's 1e-6 shows.
   Sizes: n = 1, 255, 256, 257 with one block, 1000 with 3 (a ragged second pass), 300 with 8 (idle blocks).
   One case per storage type with a ``qmul`` operand, one with the e4m3 shadow operands.
b  ``ext.pack`` over ``EDGE_VALUES`` (permuted ``w_map``, partial ``wt_map``, a sentinel image; 262 152 elements once:
   the launch caps its grid at 1024 blocks and strides; once more with ``qmul``).
c  three optimizer steps of a ``HipEngine`` (64 envs x 8 steps, Pendulum and HalfCheetah) per storage type, update
   kernels and apply form; the heads cases without the fused launch are the ones that run Adam over the slices
   ``flat[lo:hi]`` against one shared image.

Every case prints ``OPT`` lines; after the module's last case the ``error_table`` fixture prints the table below from
the cases that ran (``pytest -s``).

Worst measured figures over (a) and (c) on the MI355X, by step number (every storage type runs the same fp32 step:
the columns differ by the cases that ran, not by arithmetic).  ``D``: the worst ``|D_dev - D| / Dabs`` in units of
u = 2^-24 over the parameters that start at exactly 0.0, next to the CPU emulation's figure and the budget
``tau(t) = max(16 u, 4 x emulated)``; ``m``, ``v``, ``p``, ``norm``: the worst error as a fraction of its bound.

    storage  step    D (u)  emulated  budget     m      v      p    norm
    fp32         1     3.8      4.3    17.4   0.95   0.98   1.00   0.15
    fp32         2    59.6     60.5   241.9   0.98   0.99   0.99   0.15
    fp32         3    57.6     54.4   217.8   0.95   1.00   0.99   0.10
    fp32        10     5.9      7.0    27.9   0.96   0.98   1.00   0.10
    fp32      1000     3.5      4.5    17.8   0.95   0.95   1.00   0.15
    fp32    100000     3.0      3.9    16.0   0.95   0.97   1.00   0.10
    bf16         1     4.6      4.3    17.4   0.95   0.97   1.00   0.15
    bf16         2    59.6     60.5   241.9   0.98   0.98   0.99   0.15
    bf16         3    57.6     54.4   217.8   0.99   0.99   0.99   0.10
    bf16        10     5.9      7.0    27.9   0.95   0.97   1.00   0.10
    bf16      1000     3.5      4.5    17.8   0.95   0.95   1.00   0.15
    bf16    100000     3.0      3.9    16.0   0.95   0.97   1.00   0.10
    e4m3         1     3.3      4.3    17.4   0.88   0.96   0.99   0.10
    e4m3         2    58.5     60.5   241.9   0.87   0.93   0.98   0.10
    e4m3         3    56.9     54.4   217.8   0.84   0.95   0.95   0.10
    e4m3        10     5.7      7.0    27.9   0.87   0.94   0.99   0.10
    e4m3      1000     3.1      4.5    17.8   0.95   0.90   0.98   0.10
    e4m3    100000     2.5      3.9    16.0   0.95   0.85   0.98   0.10
    bf16x3       1     4.1      4.3    17.4   0.95   0.97   1.00   0.15
    bf16x3       2    59.6     60.5   241.9   0.96   0.98   0.99   0.15
    bf16x3       3    57.6     54.4   217.8   0.98   0.99   0.99   0.10
    bf16x3      10     5.9      7.0    27.9   0.95   0.97   1.00   0.10
    bf16x3    1000     3.5      4.5    17.8   0.95   0.95   1.00   0.15
    bf16x3  100000     3.0      3.9    16.0   0.95   0.97   1.00   0.10

The device sits at the emulation's figure at every step, the 50 - 60 u of t = 2 and 3 included: that is the
documented fp32 contract (``1 - powf(b2, t)`` cancels; module docstring of the reference), not an error of the
kernels, which stay as they are.  ``m``, ``v`` and ``p`` reach their bounds (0.95 - 1.00: the bounds are the roundings
themselves, without slack) and never pass them.  ``norm`` is the worst of: every partial against the float64 sum of
squares of its own block's elements (k = chain + 8), the square root of their sum, ``state[2]`` on the pair, and the
engine's norms with k from the grid that ran (k = 4.5 - 6); the sums of a few hundred random squares use 0.05 - 0.15 of
the worst-case bound.  The cases tagged ``1e15`` carry the two gradients whose squares are the whole norm; there only
the per-block check says anything about the other blocks, and the plain cases are the ones the norm is judged on.
Every image unit was bit-exact, and so was every byte of the e4m3 shadow -- 0 tolerated midpoint ties in 132 614
entries per engine step, where ``test_fp8_update_per_layer_error_and_shadow_image`` allows 1 in 10 000.  Nothing
failed: no kernel was changed.
"""
import math

import numpy as np
import pytest
import torch

from pytorch_dppo_amd.config import dppo_preset
from test_gpu_kernels import _engine, _fill_buffer
from test_optimizer_reference import (DT_BF16, DT_E4M3, DT_F32, DT_S3, EDGE_GRADS, EDGE_VALUES, EDGE_ZERO_STATE, F32,
                                      F64, HYPER, STEPS, SUB, U, adam_reference, assert_bounds, assert_units, block_k,
                                      bound_fractions, clip_slack, device_coef, emulated_worst, expected_units,
                                      image_units, norm_k, s3_index, sentinel_image, shadow_mismatches, tau)

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0) if torch.cuda.is_available() else None
DT_NAME = {DT_F32: "fp32", DT_BF16: "bf16", DT_E4M3: "e4m3", DT_S3: "bf16x3"}
WORST = {}                      # (storage type, step) -> the worst figures of the cases that ran
SCALE = 1.0 / 200.0             # the synthetic gather's scale (the engine's is 1 / minibatch rows)
NPBLK, NPART = 19, 45           # its partial rows and columns
STRIDE = 4096                   # its chunk stride (src_meta's shift 1 << 12)
ST_SENT = (-5.0, -7.0, -9.0)    # state[1..3] before a launch


def _ext():
    from pytorch_dppo_amd.ops import native
    return native.load()


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(DEV)


def host(t):
    return t.detach().cpu().numpy().copy()


def gamma(k):
    return k * U / (1.0 - k * U)


def record(dt, t, fr, norm_frac=0.0):
    w = WORST.setdefault((dt, t), dict(delta_u=0.0, m=0.0, v=0.0, p=0.0, norm=0.0))
    for k in ("delta_u", "m", "v", "p"):
        w[k] = max(w[k], fr[k])
    w["norm"] = max(w["norm"], norm_frac)


# ---- (a) the set-up ------------------------------------------------------------------------------------------------
def make_case(n, dt, seed=11, zero_grad=False, big=False, gscale=1.0):
    """the flat vectors, the maps and the sentinel image (module docstring); host arrays under "h", tensors beside.
    ``big``: with the edge gradients +-1e15, whose squares ARE the norm (2e30 against ~90 of everything else), so the
    norm checks mean something only without them; every other edge gradient is in every case.  ``gscale``: the
    random gradients' scale (1e-4 brings the norm next to the clip's 1e-6)"""
    rng = np.random.default_rng(seed + 1000 * n)
    p = rng.standard_normal(n).astype(F32)
    g = (0.3 * gscale * rng.standard_normal(n)).astype(F32)
    m = (1e-2 * rng.standard_normal(n)).astype(F32)
    v = (1e-4 * rng.random(n)).astype(F32)
    unmapped, zero = np.zeros(n, bool), np.zeros(n, bool)
    if n >= 64:
        k = n // 8
        unmapped[k:2 * k] = True
        unmapped[n - 2 * k:n - 2 * k + 5] = True          # (in the half with transposed entries too)
        zero[2 * k:3 * k] = True
        zero[n - k:n - k + 9] = True
        e = EDGE_GRADS.size
        small = np.abs(EDGE_GRADS) < 1.0
        g[n - e:] = np.where(small | big, EDGE_GRADS, g[n - e:])
        m[n - e:n - e + EDGE_ZERO_STATE] = 0
        v[n - e:n - e + EDGE_ZERO_STATE] = 0
        zero[n - e:n - e + 2] = True
    if zero_grad:
        g[:] = 0
    p[zero] = 0
    total = (3 * n + 16 + 7) // 8 * 8
    perm = rng.permutation(total).astype(np.int32)
    w_map = np.where(unmapped, -1, perm[:n]).astype(np.int32)
    wt_map = np.full(n, -1, np.int32)
    wt_map[n // 2:] = perm[n + n // 2:2 * n]              # (an unmapped element keeps its: nothing may land there)
    h = dict(g=g, zero=zero, mapped=~unmapped, w_map=w_map, wt_map=wt_map, total=total)
    c = dict(h=h, n=n, dt=dt, p=dev(p), g=dev(g), m=dev(m), v=dev(v), w_map=dev(w_map), wt_map=dev(wt_map),
             wimg=sentinel_image(total, dt, DEV), zero_idx=dev(np.nonzero(zero)[0]))
    return c


def make_gather(c, seed=3):
    """a synthetic gather producing (about) the case's gradient: element i of the slab runs is the sum of 1 + i % 5
    chunks STRIDE apart at a permuted offset (one chunk for the edge gradients), the reduce items are column sums of
    NPBLK partial rows; with its float64 fixed-order reference and the sum's rounding bound"""
    n, g = c["n"], c["h"]["g"]
    rng = np.random.default_rng(seed)
    s64 = float(F32(SCALE))
    slab = (60.0 / math.sqrt(3.0) * rng.standard_normal(5 * STRIDE)).astype(F32)
    part = (60.0 / math.sqrt(NPBLK) * rng.standard_normal((NPBLK, NPART))).astype(F32)
    off = rng.permutation(STRIDE)[:n].astype(np.int32)
    nch = (1 + np.arange(n) % 5).astype(np.int32)
    if n >= 64:
        hole = n // 2
        dst = list(range(37)) + [hole, -1 - 0, -1 - 3, -1 - 7]
        runs = [37, hole, hole + 1, n]
        e = EDGE_GRADS.size
        nch[n - e:] = 1
        slab[off[n - e:]] = g[n - e:] * F32(200.0)
    else:
        dst, runs = [-1 - 2], [0, n]
    dst = np.array(dst, np.int32)
    col = rng.permutation(NPART)[:dst.size].astype(np.int32)
    in_run = np.zeros(n, bool)
    for lo, hi in zip(runs[::2], runs[1::2]):
        in_run[lo:hi] = True
    meta = np.where(in_run, (nch << 5) | 1, 0).astype(np.int32)
    ref, bound = np.zeros(n), np.zeros(n)
    for i in np.nonzero(in_run)[0]:
        x = slab[off[i] + STRIDE * np.arange(nch[i])].astype(F64)
        s = 0.0
        for xc in x:
            s += xc
        ref[i], bound[i] = s * s64, gamma(int(nch[i])) * np.abs(x).sum() * s64 + SUB
    depth = -(-NPBLK // 8) - 1 + 7 + 1                    # a row group's chain, the 7 group adds, the scale
    loss_ref, loss_bound = {}, {}
    for j, d in enumerate(dst):
        x = part[:, col[j]].astype(F64)
        s = sum(sum(x[r] for r in range(rg, NPBLK, 8)) for rg in range(8))
        if d >= 0:
            ref[d], bound[d] = s * s64, gamma(depth) * np.abs(x).sum() * s64
        else:
            loss_ref[-1 - d], loss_bound[-1 - d] = s, gamma(depth) * np.abs(x).sum()
    assert (in_run.sum() + (dst >= 0).sum()) == n and not in_run[dst[dst >= 0]].any()
    assert int((off + STRIDE * (nch - 1)).max()) < slab.size and int(col.max()) < NPART
    order = np.concatenate([np.arange(lo, hi) for lo, hi in zip(runs[::2], runs[1::2])])    # the kernel's runs.flat(j)
    return dict(order=order, dst_h=dst, slab=dev(slab), off=dev(off), meta=dev(meta), part=dev(part.reshape(-1)),
                col=dev(col), dst=dev(dst), runs=runs, nrb=-(-dst.size // 32), ref=ref, bound=bound, loss_ref=loss_ref, loss_bound=loss_bound,
                nrun=int(in_run.sum()))


FORMS = ("noclip", "pair_dev", "pair_unfused", "clip_above", "clip_below", "zero_grad", "gather_adam")


def run_step(form, gated, c, t, nblk, ga=None, qmul=None, f8=None):
    """ONE launch of the form at step number t on the case's device tensors; returns (state, norm_part, loss_out,
    the limit given, whether the sumsq + adam pair ran)"""
    ext = _ext()
    f32, i32 = dict(dtype=torch.float32, device=DEV), dict(dtype=torch.int32, device=DEV)
    no_q, no_i, no_u8 = torch.empty(0, **f32), torch.empty(0, **i32), torch.empty(0, dtype=torch.uint8, device=DEV)
    state = torch.tensor([float(t - 1), *ST_SENT], **f32)
    gate = torch.zeros(4, **f32) if gated else no_q
    q = no_q if qmul is None else qmul
    f8a = (no_u8, no_i, no_q) if f8 is None else f8
    loss_out = torch.full((8,), 123.0, **f32)
    norm_ref = math.sqrt(float((c["h"]["g"].astype(F64) ** 2).sum()))
    max_norm = {"clip_above": 2.0 * norm_ref, "clip_below": 0.5 * norm_ref, "zero_grad": 0.5}.get(form, 0.0)
    if form == "gather_adam":
        part = torch.full((ga["nrb"] + nblk,), 777.0, **f32)
        ext.gather_adam(ga["slab"], ga["off"], ga["meta"], ga["part"], NPBLK, NPART, ga["col"], ga["dst"], ga["runs"],
                        SCALE, loss_out, c["g"], c["p"], c["m"], c["v"], HYPER["lr"], HYPER["b1"], HYPER["b2"],
                        HYPER["eps"], t, state, part, c["wimg"], c["w_map"], c["wt_map"], c["dt"], q, *f8a, gate, None)
        pair = False
    else:
        part = torch.full((nblk,), 777.0, **f32)
        host_step = 0 if form == "pair_dev" else t
        if form == "pair_unfused":
            ext.set_adam_fused(0)
        try:
            ext.adam(c["p"], c["g"], c["m"], c["v"], HYPER["lr"], HYPER["b1"], HYPER["b2"], HYPER["eps"], max_norm,
                     state, part, c["wimg"], c["w_map"], c["wt_map"], c["dt"], q, host_step, *f8a, gate, None)
        finally:
            if form == "pair_unfused":
                ext.set_adam_fused(1)
        pair = max_norm > 0 or form == "pair_unfused" or (form == "pair_dev" and not gated)
    torch.cuda.synchronize()
    return state, part, loss_out, max_norm, pair


def check_step(tag, form, gated, c, t, nblk, before, out, ga=None, qmul=None):
    """the assertions after one step (module docstring); returns the device's (p, m, v) after it"""
    state, part, loss_out, max_norm, pair = out
    h, n, dt = c["h"], c["n"], c["dt"]
    p1, m1, v1, g1 = host(c["p"]), host(c["m"]), host(c["v"]), host(c["g"])
    assert all(np.isfinite(a).all() for a in (p1, m1, v1, g1)), tag
    nrb = 0
    if form == "gather_adam":
        nrb = ga["nrb"]
        err = np.abs(g1.astype(F64) - ga["ref"])
        assert (err <= ga["bound"]).all(), (tag, "gather", int(np.argmax(err - ga["bound"])))
        lo = host(loss_out)
        for q_ in range(8):
            if q_ in ga["loss_ref"]:
                assert abs(float(lo[q_]) - ga["loss_ref"][q_]) <= ga["loss_bound"][q_], (tag, "loss_out", q_)
            else:
                assert lo[q_] == 123.0, (tag, "loss_out", q_)
        g_in = g1
    else:
        assert np.array_equal(g1.view(np.uint32), before["g"].view(np.uint32)), (tag, "g was written")
        g_in = before["g"]
    st = host(state).tolist()
    # the clip's coefficient is formed from the norm the device wrote (state[2], held to the norm bound below)
    coef = device_coef(max_norm, st[2]) if max_norm > 0 else None
    ref = adam_reference(before["p"], g_in, before["m"], before["v"], t, **HYPER, max_norm=max_norm or None, coef=coef)
    assert (ref["own_coef"] < 1.0) == (ref["coef"] < 1.0) == (form == "clip_below"), (tag, ref["coef"], ref["own_coef"])
    fr = bound_fractions(ref, m1, v1, p1, t, h["zero"], before["p"], clip_slack(ref))
    # the norm: EVERY partial against the float64 sum of squares of its own block's elements (an idle block's is 0,
    # exactly), then their sum, and state[2] of the pair
    pt = host(part).astype(F64)
    nelem = ga["nrun"] if form == "gather_adam" else n
    sq = g_in.astype(F64) ** 2
    chain_len = -(-nelem // (256 * nblk))
    nfrac = 0.0
    for b in range(pt.size):
        if b < nrb:               # a reduce block: one square per item thread, a 6-level tree
            d = ga["dst_h"][32 * b:32 * b + 32]
            own, kb = sq[d[d >= 0]].sum(), block_k(1)
        else:                     # thread tid of block b takes elements (b - nrb) 256 + tid + k 256 nblk of the order
            j = np.arange(nelem).reshape(-1)
            mine = ((j // 256) % nblk) == (b - nrb)
            idx = ga["order"][mine] if form == "gather_adam" else j[mine]
            own, kb = sq[idx].sum(), block_k(chain_len)
        if own == 0.0:
            assert pt[b] == 0.0, (tag, "block without a gradient", b, pt[b])
        else:
            nfrac = max(nfrac, abs(pt[b] - own) / (kb * U * own))
    kn = norm_k(nelem, nblk)
    if ref["norm"] > 0:
        nfrac = max(nfrac, abs(math.sqrt(pt.sum()) - ref["norm"]) / (kn * U * ref["norm"]))
    want_state = [float(t - 1), ST_SENT[0]] if gated else [float(t), float(t)]
    assert st[:2] == want_state and st[3] == ST_SENT[2], (tag, "state", st)
    if pair:
        k2 = norm_k(n, nblk, state2=True)
        f2 = abs(st[2] - ref["norm"]) / (k2 * U * ref["norm"]) if ref["norm"] > 0 else float(st[2] != 0.0)
        nfrac = max(nfrac, f2)
    else:
        assert st[2] == ST_SENT[1], (tag, "state[2]", st)
    print(f"OPT {tag} t={t} D {fr['delta_u']:.1f}u (emulated {emulated_worst(t):.1f}u, budget {fr['tau_u']:.1f}u) "
          f"m {fr['m']:.2f} v {fr['v']:.2f} p {fr['p']:.2f} norm {nfrac:.2f}")
    record(dt, t, fr, nfrac)
    assert_bounds(fr, tag)
    assert nfrac <= 1.0, (tag, "norm", nfrac)
    # the image: every mapped slot mirrors the device's own parameter, every other unit keeps the sentinel
    val = p1 if qmul is None else (p1 * host(qmul)).astype(F32)
    mp = h["mapped"]
    mt = mp & (h["wt_map"] >= 0)
    want = expected_units(h["total"], dt, [(h["w_map"][mp], val[mp]), (h["wt_map"][mt], val[mt])])
    assert_units(image_units(c["wimg"], dt), want, tag)
    return dict(p=p1, m=m1, v=v1, g=g1)


def chain(form, gated, dt, n, nblk, steps=STEPS, qmul=False, twin=None, big=False, gscale=1.0):
    tag0 = (f"{form}{'-gated' if gated else ''} {DT_NAME[dt]} n={n} nblk={nblk}{' qmul' if qmul else ''}"
            f"{' 1e15' if big else ''}{f' g*{gscale:g}' if gscale != 1.0 else ''}")
    c = make_case(n, dt, zero_grad=form == "zero_grad", big=big, gscale=gscale)
    ga = make_gather(c) if form == "gather_adam" else None
    if ga is not None:
        c["g"].fill_(7.0)
    q = dev(np.random.default_rng(9).uniform(0.5, 2.0, n).astype(F32)) if qmul else None
    ct = make_case(n, dt, big=big, gscale=gscale) if twin else None
    for t in steps:
        c["p"][c["zero_idx"]] = 0.0
        before = {k: host(c[k]) for k in ("p", "m", "v", "g")}
        out = run_step(form, gated, c, t, nblk, ga, q)
        check_step(tag0, form, gated, c, t, nblk, before, out, ga, q)
        if ct is not None:          # the coefficient is exactly 1: the bits of the twin form
            ct["p"][ct["zero_idx"]] = 0.0
            run_step(twin, gated, ct, t, nblk)
            for k in ("p", "m", "v"):
                assert torch.equal(c[k].view(torch.int32), ct[k].view(torch.int32)), (tag0, t, k, "differs from", twin)
            assert np.array_equal(image_units(c["wimg"], dt), image_units(ct["wimg"], dt)), (tag0, t, "image", twin)


@pytest.mark.parametrize("big", [False, True], ids=["plain", "1e15"])
@pytest.mark.parametrize("dt", [DT_F32, DT_BF16, DT_S3])
@pytest.mark.parametrize("gated", [False, True], ids=["ungated", "gated"])
@pytest.mark.parametrize("form", FORMS)
def test_launch_form_against_fp64(form, gated, dt, big):
    """every form, type and edge gradient; ``1e15``: once more with the two gradients that swamp the norm"""
    chain(form, gated, dt, 1000, 3, twin="noclip" if form == "clip_above" else None, big=big)


@pytest.mark.parametrize("gated", [False, True], ids=["ungated", "gated"])
def test_clip_epsilon_is_part_of_the_coefficient(gated):
    """gradients of norm ~1e-3: the 1e-6 of ``max_norm / (norm + 1e-6)`` is a part in a thousand of the coefficient
    (at the other cases' norm of ~9.5 it is 1e-7, inside the clip's slack)"""
    chain("clip_below", gated, DT_F32, 1000, 3, steps=(1, 10), gscale=1e-4)


def test_e4m3_image_of_the_noclip_form():
    chain("noclip", False, DT_E4M3, 1000, 3)


@pytest.mark.parametrize("dt", [DT_F32, DT_BF16, DT_S3])
@pytest.mark.parametrize("n,nblk", [(1, 1), (255, 1), (256, 1), (257, 1), (300, 8)])
@pytest.mark.parametrize("form", ["noclip", "clip_below", "gather_adam"])
def test_launch_form_sizes(form, n, nblk, dt):
    chain(form, False, dt, n, nblk, steps=(1, 2, 1000))


@pytest.mark.parametrize("dt", [DT_F32, DT_BF16, DT_E4M3, DT_S3])
@pytest.mark.parametrize("form", ["noclip", "clip_below", "gather_adam"])
def test_qmul_operand_scales_the_image_only(form, dt):
    chain(form, False, dt, 300, 2, steps=(1, 10), qmul=True)


@pytest.mark.parametrize("form", ["noclip", "clip_below", "gather_adam"])
def test_e4m3_shadow_operands(form):
    """the shadow e4m3 image (fp8 mode runs it beside a bf16 image): three layers with different scales, one
    parameter beyond 448 x its scale; bytes = e4m3(fl32(p_after / qs[lid])) saturated, by the shadow rule"""
    n, nblk, dt = 300, 2, DT_BF16
    c = make_case(n, dt)
    h = c["h"]
    ga = make_gather(c) if form == "gather_adam" else None
    qs = np.array([1e30, 0.01, 1e30, 0.37, 1e30, 3.0], F32)        # (the layers in use: 1, 3, 5)
    lid = (1 + 2 * (np.arange(n) % 3)).astype(np.int32)
    big = int(np.nonzero(h["mapped"] & (lid == 1) & ~h["zero"])[0][5])
    c["p"][big] = 5.0                                                # 5 / 0.01 = 500 > 448
    shadow = torch.full((h["total"],), 0xA5, dtype=torch.uint8, device=DEV)
    f8 = (shadow, dev(lid), dev(qs))
    for t in (1, 10):
        c["p"][c["zero_idx"]] = 0.0
        before = {k: host(c[k]) for k in ("p", "m", "v", "g")}
        out = run_step(form, False, c, t, nblk, ga, None, f8)
        after = check_step(f"shadow {form}", form, False, c, t, nblk, before, out, ga)
        quot = (after["p"] / qs[lid]).astype(F32)
        mp = h["mapped"]
        mt = mp & (h["wt_map"] >= 0)
        got = host(shadow)
        slots = np.concatenate([h["w_map"][mp], h["wt_map"][mt]])
        qq = np.concatenate([quot[mp], quot[mt]])
        bad, ties = shadow_mismatches(got[slots], qq)
        print(f"OPT shadow {form} t={t}: {len(ties)} tolerated ties {ties[:4]}")
        assert not bad, ("shadow", form, t, bad[:8])
        assert np.array_equal(got[h["w_map"][mt]], got[h["wt_map"][mt]])
        assert abs(quot[big]) > 448.0 and got[h["w_map"][big]] == 0x7E
        rest = np.ones(h["total"], bool)
        rest[slots] = False
        assert (got[rest] == 0xA5).all(), "the shadow was written outside the mapped slots"


# ---- (b) pack ------------------------------------------------------------------------------------------------------
def pack_case(n, dt, qmul=False, seed=4):
    rng = np.random.default_rng(seed)
    vals = np.resize(EDGE_VALUES, n).astype(F32)
    vals = vals[rng.permutation(n)] if n > EDGE_VALUES.size else vals
    total = (3 * n + 16 + 7) // 8 * 8
    perm = rng.permutation(total).astype(np.int32)
    w_map = perm[:n].copy()
    w_map[::7] = -1
    wt_map = np.where(np.arange(n) % 3 == 1, perm[n:2 * n], -1).astype(np.int32)     # partial, some on unmapped
    q = rng.uniform(0.5, 2.0, n).astype(F32) if qmul else None
    img = sentinel_image(total, dt, DEV)
    _ext().pack(dev(vals), img, dev(w_map), dev(wt_map), dt, dev(q) if qmul else torch.empty(0, device=DEV))
    torch.cuda.synchronize()
    with np.errstate(under="ignore"):
        val = vals if q is None else (vals * q).astype(F32)
    mp = w_map >= 0
    mt = mp & (wt_map >= 0)
    assert mt.any() and (~mp & (wt_map >= 0)).any()
    want = expected_units(total, dt, [(w_map[mp], val[mp]), (wt_map[mt], val[mt])])
    assert_units(image_units(img, dt), want, f"pack {DT_NAME[dt]} n={n}")


@pytest.mark.parametrize("qmul", [False, True], ids=["plain", "qmul"])
@pytest.mark.parametrize("dt", [DT_F32, DT_BF16, DT_S3])
def test_pack_on_the_edge_values(dt, qmul):
    pack_case(EDGE_VALUES.size, dt, qmul)


def test_pack_strides_past_its_grid_cap():
    pack_case(1024 * 256 + 8, DT_S3)


# ---- (c) the engine's own step ---------------------------------------------------------------------------------
ENGINE_PATHS = [("fp32", "tile"), ("bf16", "tile"), ("bf16", "heads"), ("bf16x3", "tile"), ("bf16x3", "heads"),
                ("fp8", "heads")]
APPLY_FORMS = {"fused-stream": {}, "fused-elem": {}, "gather-then-adam": dict(fused_apply=False),
               "clip": dict(max_grad_norm=0.01), "gated": dict(target_kl=1e9)}     # (0.01: under every gradient's norm)


def engine_norm_grid(eng, apply_form, n):
    """(partials the step must have left, the terms one thread chained into a partial) of the launch that ran,
    from the engine's own grid sizes (runtime/engine_hip.py): the fused launch takes one reduce block per 32 items and
    then one QUAD per thread (4 fused squares) of the tile table, or with the streaming form off one element per
    thread of the slab runs, over the same grid; the whole-vector Adam strides n elements over norm_n_elem blocks;
    the per-head pair strides each head's slice over its own region"""
    up = lambda a, b: -(-a // b)   # noqa: E731
    if apply_form in ("fused-stream", "fused-elem", "gated"):
        fb = eng.joint_bucket if eng.heads else eng.buckets[0]
        nrb = up(len(eng.items["joint" if eng.heads else "legacy"][0]), 32)
        nb = eng.norm_n_whole - nrb
        assert nb >= 1
        if apply_form == "fused-elem":
            return eng.norm_n_whole, up(sum(fb["runs"][1::2]) - sum(fb["runs"][0::2]), 256 * nb)
        return eng.norm_n_whole, 4 * up(fb["nquads"], 256 * nb)
    if eng.heads and apply_form == "gather-then-adam":
        return eng.norm_regions[1][1], max(up(hi - lo, 256 * (r1 - r0))
                                           for (lo, hi), (r0, r1) in zip(eng.head_range, eng.norm_regions))
    return eng.norm_n_elem, up(n, 256 * eng.norm_n_elem)


@pytest.mark.parametrize("apply_form", list(APPLY_FORMS))
@pytest.mark.parametrize("dtype,kernels", ENGINE_PATHS, ids=[f"{d}-{k}" for d, k in ENGINE_PATHS])
@pytest.mark.parametrize("env_name", ["Pendulum-v0", "HalfCheetah-v2"])
def test_engine_step_against_fp64(env_name, dtype, kernels, apply_form):
    over = APPLY_FORMS[apply_form]
    p = dppo_preset(device="gpu", env_name=env_name, num_envs=64, exploration_size=512, batch_size=512, dtype=dtype,
                    update_kernels=kernels, **over)
    eng, model, _, _ = _engine(p)
    ext = _ext()
    tag = f"engine {env_name} {dtype}-{kernels} {apply_form}"
    assert eng.heads == (kernels == "heads"), tag
    fused = apply_form in ("fused-stream", "fused-elem", "gated")
    assert eng.can_fuse_apply() == fused and (eng.gate is not None) == (apply_form == "gated"), tag
    if fused:                   # the streaming form needs the fused bucket's tile table (the switch is on by default)
        assert eng._tiles(eng.joint_bucket if eng.heads else eng.buckets[0]), tag
    hyper = dict(lr=p.lr, b1=p.adam_betas[0], b2=p.adam_betas[1], eps=p.adam_eps)
    assert hyper == HYPER                                  # (tau is sized for these)
    L = model.packed_layout()
    w_map, wt_map = L.flat_to_w.numpy().astype(np.int64), L.flat_to_wt.numpy().astype(np.int64)
    mp = w_map >= 0
    mt = mp & (wt_map >= 0)
    n = model.num_params
    dt = eng.dt
    if eng.fp8:
        eng.refresh_fwd_image()
    _fill_buffer(eng, model)
    if apply_form == "fused-elem":
        ext.set_gather_stream(0)
    try:
        eng.begin_update()
        for t in (1, 2, 3):
            torch.cuda.synchronize()
            before = dict(p=host(model.flat.data), m=host(eng.adam_m), v=host(eng.adam_v))
            eng.step(None)
            eng.finish_steps()
            torch.cuda.synchronize()
            p1, m1, v1, g1 = host(model.flat.data), host(eng.adam_m), host(eng.adam_v), host(eng.grad_flat)
            assert all(np.isfinite(a).all() for a in (p1, m1, v1, g1)), tag
            st = host(eng.adam_state).tolist()
            assert st[:2] == [float(t), float(t)], (tag, st)
            coef = device_coef(eng.max_norm, st[2]) if eng.max_norm else None       # (from the norm the device wrote)
            ref = adam_reference(before["p"], g1, before["m"], before["v"], t, **hyper, max_norm=eng.max_norm or None,
                                 coef=coef)
            assert (ref["own_coef"] < 1.0) == (ref["coef"] < 1.0) == (apply_form == "clip"), (tag, ref["norm"], ref["coef"])
            fr = bound_fractions(ref, m1, v1, p1, t, before["p"] == 0, before["p"], clip_slack(ref))
            # the norm, with k derived from the grid that ran
            nparts, terms = engine_norm_grid(eng, apply_form, n)
            assert eng._norm_n == nparts and 1 <= terms <= 4, (tag, eng._norm_n, nparts, terms)
            pt = host(eng.norm_part[:nparts]).astype(F64)
            nfrac = abs(math.sqrt(pt.sum()) - ref["norm"]) / (norm_k(n, nparts, chain=terms) * U * ref["norm"])
            if eng.max_norm:
                k2 = norm_k(n, nparts, state2=True, chain=terms)
                nfrac = max(nfrac, abs(st[2] - ref["norm"]) / (k2 * U * ref["norm"]))
            print(f"OPT {tag} t={t} D {fr['delta_u']:.1f}u (emulated {emulated_worst(t):.1f}u, budget {fr['tau_u']:.1f}u)"
                  f" m {fr['m']:.2f} v {fr['v']:.2f} p {fr['p']:.2f} norm {nfrac:.2f} coef {ref['coef']:.3f}")
            record(dt, t, fr, nfrac)
            assert_bounds(fr, tag)
            assert nfrac <= 1.0, (tag, "norm", nfrac)
            # the image of the packed parameters at every mapped slot, forward and transposed
            packed = host(L.pack(model.flat.data.detach().cpu()))
            slots = np.unique(np.concatenate([w_map[mp], wt_map[mt]]))
            assert np.array_equal(packed[w_map[mp]], p1[mp]) and np.array_equal(packed[wt_map[mt]], p1[mt])
            want = expected_units(L.total, dt, [(slots, packed[slots])])
            got = image_units(eng.wimg, dt)
            units = slots if dt != DT_S3 else np.concatenate([s3_index(slots), s3_index(slots) + 8])
            assert_units(got[units], want[units], tag)
            if eng.fp8:
                lid = host(eng.layer_id).astype(np.int64)
                assert np.array_equal(lid >= 0, mp)
                quot = np.zeros(n, F32)
                quot[mp] = (p1[mp] / host(eng.qscale)[lid[mp]]).astype(F32)
                sh = host(eng.wimg_fwd)
                bad, ties = shadow_mismatches(np.concatenate([sh[w_map[mp]], sh[wt_map[mt]]]),
                                              np.concatenate([quot[mp], quot[mt]]))
                print(f"OPT {tag} t={t} shadow: {len(ties)} tolerated ties of {mp.sum() + mt.sum()} {ties[:3]}")
                assert not bad, (tag, "shadow", bad[:8])
    finally:
        if apply_form == "fused-elem":
            ext.set_gather_stream(1)


# ---- the record ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", autouse=True)
def error_table():
    """after the module's last case: the module docstring's table, from whichever cases ran in this process"""
    yield
    print("\n    storage  step    D (u)  emulated  budget     m      v      p    norm")
    for (dt, t) in sorted(WORST):
        w = WORST[(dt, t)]
        print(f"    {DT_NAME[dt]:7s} {t:6d} {w['delta_u']:7.1f} {emulated_worst(t):8.1f} {tau(t) / U:7.1f} "
              f"{w['m']:6.2f} {w['v']:6.2f} {w['p']:6.2f} {w['norm']:6.2f}")
