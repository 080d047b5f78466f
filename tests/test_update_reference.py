"""One fp64 reference, one comparison and the fixtures of the update kernels' conformance matrix.

This module is a helper (``tests/test_gpu_update_conformance.py`` imports it) and the CPU tests of the
helper itself, as ``tests/test_rollout_replay.py`` is for the rollout.

``reference``   the update's gradient, loss terms and per-row forward in float64 on the CPU: a float64
                ``ActorCritic`` holding the engine's parameters, ``oracle.ppo_loss`` / ``oracle.dppo_ref_loss`` and
                autograd.  No vendor BLAS at working precision is involved, so its own error (~1e-15) is no part of
                any tolerance.
``compare``     the relative error ``|g_k[b] - g_ref[b]| / |g_ref[b]|`` of each of the 13 parameter blocks and of the
                whole vector, each asserted against a budget; a block without a budget fails.
fixtures        seeded, pure CPU (``build_fixture``), one set per class of path.  The observation rows are values the
                class's storage types hold exactly, so that one reference serves every path of the class: 16-bit
                ``hi + lo`` rows (``storage.decode(storage.encode(x))``, both halves of bf16x3's operand non-zero, the
                low mantissa bits of fp32's too) for fp32 / bf16x3, bf16 rows for bf16 and fp8 mode's bf16 buffer.
                The GPU module asserts ``eng.decode(eng.x_buf)`` equals them bit for bit.

Fixture design.  A block whose gradient is a cancelling sum over the rows has a relative error that says nothing
(the rounding of each row's term is measured against a sum much smaller than the terms), so ``base``:

* ``ret = v + 0.3 + 0.5 randn`` and ``adv = 0.6 + randn`` (neither has zero mean; with ``adv = 0.3 + randn`` the
  policy blocks' share |sum| / sum|.| is at most E adv / E|adv| = 0.36 before clipping and fell below 1/4 on
  three of the five shapes);
* the action noise is ``z = t + 0.3 randn`` with a fixed per-dim ``t = +-0.75``, where ``_fill_buffer`` of
  ``test_gpu_kernels.py`` draws ``0.6 randn``: with zero-mean noise ``dL/dmu = -adv ratio z / sigma`` and
  ``dL/dlog_std ~ adv (z^2 - 1)`` cancel over the rows whatever the advantages' mean is;
* the observations are ``1 + randn`` (clamped to +-5), where ``_fill_buffer`` draws ``randn``: a weight gradient of
  a first layer is ``sum_i g_i x_i^T``, which cancels for zero-mean ``x`` however coherent ``g`` is;
* the biases are ``0.1 randn`` (the model's init zeroes them, so a forward that dropped the bias column would pass).

``test_no_block_is_a_cancelling_sum`` asserts ``|sum_i g_i[b]| >= 1/4 |sum_i |g_i[b]||`` for every block.

Branch bands.  A row whose fp64 ``ln ratio`` (or ``v``) lies within rounding of a branch point takes a different,
equally legitimate branch in a kernel.  The builders re-draw such a row's ``logp_old`` (``values_buf``) entry and
then assert that NO row lies within the band of ``ln(1 +- clip)``, of ``|v - v_old| = clip`` or of the tie of the
two value terms.  The band is 4 x the largest ``|logp - logp_fp64|`` (``|v - v_fp64|``) over the fixture's 512
rows of the same forward emulated on the CPU (``emulate``), by class of path:

* ``f32`` (the fp32 and bf16x3 paths): the forward in fp32, and with weights and layer outputs as bf16x3 holds them
  (hi + lo, 16 bits); the larger of the two;
* ``bf16``: weights and layer outputs rounded to bf16;
* ``fp8``: bf16, and the value head's fc1 with e4m3 weights and inputs (fp8 mode's e4m3 forward GEMM in every
  configuration).  Its ``ln ratio`` width is bf16's: the band does NOT model the e4m3 policy GEMMs of
  ``fp8_policy_gemms`` (emulated as ``fp8pg`` for the record: their width, 0.2 - 0.46, holds the whole clip range
  and would leave no unclipped row), so on that path alone the clip count may differ from the reference's, by at
  most ``clip_flip_allowance``: the rows whose OWN emulated error, times 4, reaches a clip bound (27 - 80 of 200).

Widths, the largest over the five shapes (``test_band_widths`` prints them), default-init fixtures | `saturated`:

    class    band(ln ratio)       band(v)
    f32      4.7e-05 | 2.4e-04    1.6e-05 | 4.9e-05
    bf16     3.6e-02 | 1.7e-01    8.9e-03 | 3.5e-02
    fp8      3.6e-02 | 1.7e-01    1.4e-01 | 7.2e-01     (v: `saturated` runs with the mse value term only)
    fp8pg    4.6e-01 | 2.4e+00    1.4e-01 | 7.2e-01     (no fixture is built with it)

(At `saturated` the bf16 band leaves only ln ratio in (-0.06, 0.02) between the two branch points ln 0.8 and ln 1.2:
the re-drawn rows land there or, the noise of the re-draws growing, well beyond the clip range.)

Budgets (``budgets``).  Floors: fp32 and bf16x3 6e-4 per block, 2e-4 whole; bf16 1e-1 per block, 6e-2 whole (the
project's figures of ``test_phead_update_matches_16x16_head_update`` and the bench-geometry tests).  Error model,
emulated on the CPU against the fp64 reference (``emulate``): the same loss and backward in fp32 (``f32``); weights,
layer outputs and the wgrad operands ``h`` / ``g`` rounded to bf16, fp32 sums (``bf16``).  Where 4 x the model exceeds
the floor, the budget is 4 x the model (4: the summation orders of the emulation and of a kernel differ).  fp8 has
measurements: the limits of ``test_fp8_update_per_layer_error_and_shadow_image`` per head (policy 0.06, 0.22 with
``fp8_policy_gemms``; value 0.12), for the weight blocks and, a bias gradient being a row sum of the same ``g``
operand, for the bias blocks and ``log_std``; the whole vector takes the larger of the two heads' limits (a vector's
relative error is at most its blocks' largest).  Its emulation (e4m3 forward GEMMs, bf16 backward) is a lower bound
of the path's error and raises a head's budget, to limit + model, only where it exceeds the limit by itself:
``budgets``.

Emulated error table: the largest over the matrix's ppo-loss cases at 200 rows, default-init fixtures and, ``/sat``,
`saturated` (``test_emulated_error_table`` prints it; ``s3``: bf16x3's 16-bit operands, ``fp8pg``: fp8_policy_gemms):

    block                f32        s3      bf16       fp8     fp8pg   f32/sat    s3/sat  bf16/sat   fp8/sat fp8pg/sat
    log_std          6.6e-07   9.5e-06   2.7e-03   2.7e-03   3.6e-02   4.6e-07   8.6e-06   6.3e-03   6.3e-03   1.7e-01
    p_fc1.weight     3.7e-07   4.2e-06   3.0e-03   3.0e-03   2.6e-02   8.7e-07   1.1e-05   7.9e-03   7.9e-03   2.5e-01
    p_fc1.bias       2.6e-07   4.1e-06   2.9e-03   2.9e-03   2.1e-02   6.2e-07   8.9e-06   6.5e-03   6.5e-03   2.3e-01
    p_fc2.weight     3.8e-07   4.1e-06   2.7e-03   2.7e-03   4.1e-02   6.0e-07   8.6e-06   5.7e-03   5.7e-03   2.1e-01
    p_fc2.bias       2.7e-07   3.5e-06   2.1e-03   2.1e-03   1.9e-02   3.2e-07   6.0e-06   4.2e-03   4.2e-03   1.9e-01
    mu.weight        3.8e-07   4.1e-06   2.6e-03   2.6e-03   5.0e-02   3.6e-07   6.7e-06   4.6e-03   4.6e-03   1.6e-01
    mu.bias          2.8e-07   2.4e-06   1.0e-03   1.0e-03   1.6e-02   1.2e-07   4.5e-06   3.2e-03   3.2e-03   1.5e-01
    v_fc1.weight     2.3e-07   7.1e-06   3.5e-03   5.2e-02   5.2e-02   6.3e-07   1.0e-05   5.9e-03   8.6e-02   8.6e-02
    v_fc1.bias       8.8e-08   7.3e-06   3.5e-03   5.3e-02   5.3e-02   4.6e-07   9.1e-06   4.7e-03   6.5e-02   6.5e-02
    v_fc2.weight     2.3e-07   7.0e-06   3.4e-03   6.1e-02   6.1e-02   4.6e-07   8.8e-06   4.1e-03   6.2e-02   6.2e-02
    v_fc2.bias       8.8e-08   7.0e-06   3.0e-03   5.3e-02   5.3e-02   2.9e-07   7.7e-06   2.8e-03   3.9e-02   3.9e-02
    v.weight         2.2e-07   6.5e-06   2.9e-03   6.0e-02   6.0e-02   2.6e-07   7.2e-06   3.3e-03   3.8e-02   3.8e-02
    v.bias           7.8e-08   6.1e-06   2.1e-03   5.3e-02   5.3e-02   3.1e-08   5.9e-06   6.8e-04   1.2e-02   1.2e-02
    whole            3.6e-07   5.1e-06   2.9e-03   3.9e-02   4.5e-02   5.3e-07   8.1e-06   5.5e-03   1.8e-02   1.8e-01

Every fp32 / bf16x3 / bf16 figure is far below its floor, so those budgets are the floors.
"""
from __future__ import annotations

import functools
import math
from typing import Dict, Optional

import pytest
import torch

from pytorch_dppo_amd.config import Params, dppo_preset, ppo_preset
from pytorch_dppo_amd.envs import get_spec
from pytorch_dppo_amd.models.actor_critic import ActorCritic
from pytorch_dppo_amd.ops import oracle, storage

F64 = torch.float64
POLICY_LAYERS = ("p_fc1", "p_fc2", "mu")
VALUE_LAYERS = ("v_fc1", "v_fc2", "v")
BLOCKS = ["log_std"] + [f"{n}.{s}" for n in POLICY_LAYERS + VALUE_LAYERS for s in ("weight", "bias")]
POLICY_BLOCKS = [f"{n}.{s}" for n in POLICY_LAYERS for s in ("weight", "bias")]
LOSS_TERMS = ("loss_clip", "loss_value", "loss_ent", "approx_kl", "clipfrac")

SHAPES = ("Humanoid-v2", "Ant-v2", "Synthetic-64x8", "HalfCheetah-v2", "Pendulum-v0")
ENVS, STEPS = 64, 8
ROWS = ENVS * STEPS                      # 512: no case uses more
MINIBATCHES = (None, 200, 129)
KINDS = ("base", "saturated", "all_clipped", "none_clipped", "value_clip")
CLASSES = ("f32", "bf16", "fp8")
STORAGE_CLASS = {"fp32": "f32", "bf16x3": "f32", "bf16": "bf16", "fp8": "fp8"}
FLOORS = {"f32": (6e-4, 2e-4), "bf16": (1e-1, 6e-2)}       # (per block, whole vector)
FP8_LIMITS = {False: (0.06, 0.12), True: (0.22, 0.12)}     # fp8_policy_gemms -> (policy head, value head)
MARGIN = 4.0


def make_params(shape: str, dtype: str = "fp32", mb: Optional[int] = None, loss: str = "ppo",
                value_loss: str = "mse", conv: str = "std", device: str = "cpu", **over) -> Params:
    """the Params of one case: a 64 x 8 buffer of ``shape``, minibatch ``mb`` (None: the full batch)"""
    kw = dict(device=device, env_name=shape, num_envs=ENVS, exploration_size=ROWS, batch_size=mb or ROWS,
              dtype=dtype, ent_coeff=0.01, loss=loss)
    if loss == "dppo_ref":       # (its value term is the clipped one, its convention var: the preset's)
        return dppo_preset(**kw, **over)
    return ppo_preset(value_loss=value_loss, std_convention=conv, **kw, **over)


def minibatch_index(mb: Optional[int]) -> Optional[torch.Tensor]:
    return None if mb is None else torch.randperm(ROWS, generator=torch.Generator().manual_seed(11))[:mb]


def _f64(t: torch.Tensor) -> torch.Tensor:
    return t.detach().to("cpu", F64)


def _model_like(model: ActorCritic, flat: torch.Tensor, dtype) -> ActorCritic:
    m = ActorCritic(model.num_inputs, model.num_outputs, model.hidden, model.value_mult).to(dtype)
    with torch.no_grad():
        m.flat.copy_(flat.detach().to("cpu", dtype))
    return m


def _ln_ratio_ref(actions, mu, log_std, mu_old, log_std_old):
    """ln of the reference loss's per-dim ratio p / (1e-10 + p_old)"""
    p = oracle.normal_pdf_var(actions, mu, torch.exp(log_std))
    po = oracle.normal_pdf_var(actions, mu_old, torch.exp(log_std_old))
    return torch.log(p / (1e-10 + po))


def _loss(p: Params, mu, log_std, v, batch: Dict[str, torch.Tensor], old=None):
    if p.loss == "ppo":
        return oracle.ppo_loss(mu, log_std, v, batch["actions"], batch["logp_old"], batch["adv"], batch["ret"],
                               batch["v_old"], clip=p.clip, ent_coeff=p.ent_coeff, value_loss=p.value_loss,
                               convention=p.std_convention)
    mu_o, ls_o, v_o = (mu.detach(), log_std.detach(), v.detach()) if old is None else old
    return oracle.dppo_ref_loss(mu, log_std, v, mu_o, ls_o, v_o, batch["actions"], batch["adv"], batch["ret"],
                                clip=p.clip, ent_coeff=p.ent_coeff)


def _batch(dtype, idx, actions, logp_old, adv, ret, v_old, old):
    c = lambda t: t.detach().to("cpu", dtype)[idx]      # noqa: E731
    b = {"actions": c(actions), "logp_old": c(logp_old), "adv": c(adv), "ret": c(ret), "v_old": c(v_old)}
    o = None
    if old is not None:
        mu_o, ls_o, v_o = old
        o = (c(mu_o), ls_o.detach().to("cpu", dtype).reshape(1, -1), c(v_o).reshape(-1, 1))
    return b, o


def reference(model: ActorCritic, params: Params, rows, actions, logp_old, adv, ret, v_old, idx, old=None) -> Dict:
    """The update of ``params`` (a Params: loss, value_loss, std_convention, clip, ent_coeff) on the minibatch
    ``idx`` (None: every row) of the buffer in float64 on the CPU, with ``model``'s parameters.

    ``rows`` [N, O] are the observation rows as the engine stored them (``eng.decode(eng.x_buf)[:N, :O]``); ``actions``
    [N, A], ``logp_old`` / ``adv`` / ``ret`` / ``v_old`` [N] the buffer's fp32 arrays.  ``old`` = ``(mu_old [N, A],
    log_std_old [A], v_old [N])`` is the reference loss's previous step (None: old = current, its first step).

    Returns ``grad`` (flat), ``losses`` (the five terms), per row ``ln_ratio`` ([mb]; the reference loss: [mb, A]),
    ``v`` [mb], ``mu`` [mb, A], ``clip_count`` (rows -- the reference loss: row-dims -- with |ratio - 1| > clip),
    ``mb`` and ``blocks`` = {name: (offset, size)} of the 13 blocks."""
    m = _model_like(model, model.flat, F64)
    n = rows.shape[0]
    ii = torch.arange(n) if idx is None else idx.detach().cpu().long().reshape(-1)
    x = _f64(rows)[ii]
    batch, old64 = _batch(F64, ii, actions, logp_old, adv, ret, v_old, old)
    mu, ls, v = m(x)
    out = _loss(params, mu, ls, v, batch, old64)
    out["loss"].backward()
    with torch.no_grad():
        if params.loss == "ppo":
            lnr = (oracle.gaussian_logp(batch["actions"], mu, ls, params.std_convention)
                   - batch["logp_old"].reshape(-1, 1)).reshape(-1)
        else:
            mu_o, ls_o = (mu, ls) if old64 is None else old64[:2]
            lnr = _ln_ratio_ref(batch["actions"], mu, ls, mu_o, ls_o)
        count = int(((torch.exp(lnr) - 1.0).abs() > params.clip).sum())
    return {"grad": m.flat.grad.detach().clone(), "losses": {k: float(out[k].detach()) for k in LOSS_TERMS},
            "ln_ratio": lnr, "v": v.detach().reshape(-1), "mu": mu.detach(), "clip_count": count,
            "mb": int(ii.numel()), "blocks": {b: m.offsets[b] for b in BLOCKS}}


def error_table(g_kernel: torch.Tensor, ref: Dict) -> Dict[str, float]:
    """relative error of each block and of the ``whole`` vector.  A block whose reference is exactly zero has
    error 0 when the kernel's is exactly zero too, else inf."""
    g, gr = _f64(g_kernel).reshape(-1), ref["grad"]
    assert g.shape == gr.shape, (g.shape, gr.shape)

    def rel(a, b):
        nb = b.norm().item()
        if nb == 0.0:
            return 0.0 if not bool((a != 0).any()) else math.inf
        e = (a - b).norm().item() / nb
        return e if math.isfinite(e) else math.inf
    table = {b: rel(g[o:o + n], gr[o:o + n]) for b, (o, n) in ref["blocks"].items()}
    table["whole"] = rel(g, gr)
    return table


def format_table(table: Dict[str, float], budget: Optional[Dict[str, float]] = None) -> str:
    rows = []
    for b in BLOCKS + ["whole"]:
        lim = "" if budget is None else f"   budget {budget.get(b, float('nan')):.3e}"
        rows.append(f"  {b:14s} {table[b]:.3e}{lim}")
    return "\n".join(rows)


def compare(g_kernel: torch.Tensor, ref: Dict, budget: Dict[str, float]) -> Dict[str, float]:
    """the per-block error table of ``g_kernel`` against ``ref``; every one of the 13 blocks and ``whole`` is
    asserted against ``budget`` -- a block without an entry fails, nothing is skipped"""
    table = error_table(g_kernel, ref)
    bad = []
    for b in BLOCKS + ["whole"]:
        if b not in budget:
            bad.append(f"block {b}: no budget")
        elif not table[b] <= budget[b]:
            bad.append(f"block {b}: relative error {table[b]:.3e} over budget {budget[b]:.3e}")
    assert not bad, "; ".join(bad) + "\n" + format_table(table, budget)
    return table


# ---------------------------------------------------------------------------------------------------------------
# CPU emulation of the kernels' roundings: the band widths (forward) and the budgets' error model (backward)
# ---------------------------------------------------------------------------------------------------------------
def _bf16(t: torch.Tensor) -> torch.Tensor:
    return t.to(torch.bfloat16).to(t.dtype)


def _split16(t: torch.Tensor) -> torch.Tensor:
    """bf16x3's operand: hi + lo, two bf16 (ops/storage.py)"""
    hi = _bf16(t)
    return hi + _bf16(t - hi)


def _e4m3(t: torch.Tensor, scale: float) -> torch.Tensor:
    return (t * scale).clamp(-448.0, 448.0).to(torch.float8_e4m3fn).to(t.dtype) / scale


# fp8 mode's e4m3 forward GEMM in every configuration: the value head's fc1.  ("fp8pg", the policy's fc1 and fc2 of
# fp8_policy_gemms too, is emulated for the record only: test_band_widths prints it, no fixture is built with it.)
_F8_LAYERS = {"fp8": ("v_fc1",), "fp8pg": ("v_fc1", "p_fc1", "p_fc2")}
_LOWP = ("bf16", "fp8", "fp8pg")
_F8_INPUT = {"p_fc1": 64.0, "v_fc1": 64.0, "p_fc2": 256.0}     # the fixed power-of-two scales of their inputs


def emulate(cls: str, model: ActorCritic, x: torch.Tensor, loss_fn=None):
    """``model``'s forward -- and with ``loss_fn(mu, log_std, v) -> {"loss"}`` the flat gradient -- with the roundings
    of class ``cls``: ``f64`` / ``f32`` none (the arithmetic alone); ``s3`` weights and layer outputs as bf16x3 holds
    them (hi + lo); ``bf16`` weights, layer outputs and the wgrad operands rounded to bf16 with fp32 sums; ``fp8`` /
    ``fp8pg`` the e4m3 forward GEMMs of fp8 mode on top of bf16 (weights by the layer's amax / 416, inputs by their
    fixed power-of-two scale; the backward stays bf16's: a lower bound of that path's error).
    Returns ``(mu, v)`` or ``(mu, v, grad)``.  The backward is written out (dtanh on the rounded activation, as the
    kernels compute it); in ``f64`` it is autograd's, which ``test_emulation_in_fp64_is_autograd`` checks."""
    dt = F64 if cls == "f64" else torch.float32
    flat = model.flat.detach().to("cpu", dt)
    W = {k: t for k, t in model.views(flat).items()}
    rt = _bf16 if cls in _LOWP else _split16 if cls == "s3" else (lambda t: t)
    f8 = _F8_LAYERS.get(cls, ())

    def wq(name, fwd=True):
        w, b = W[f"{name}.weight"], W[f"{name}.bias"]
        # (the dgrad reads the bf16 image)  per-layer scale amax / 416: HipEngine.refresh_fwd_image
        if name in f8 and fwd:
            s = 416.0 / max(w.abs().max().item(), b.abs().max().item())
            return _e4m3(w, s), _e4m3(b, s)
        return rt(w), rt(b)

    def head(names):
        h, ins = x.detach().to("cpu", dt), []
        for i, name in enumerate(names):
            w, b = wq(name)
            ins.append(h)
            hin = _e4m3(h, _F8_INPUT[name]) if name in f8 else h
            z = hin @ w.t() + b
            h = rt(torch.tanh(z)) if i < 2 else z
        return h, ins
    mu, pin = head(POLICY_LAYERS)
    v, vin = head(VALUE_LAYERS)
    if loss_fn is None:
        return mu, v
    mu_l, v_l = mu.detach().requires_grad_(), v.detach().requires_grad_()
    ls_l = W["log_std"].detach().clone().requires_grad_()
    loss_fn(mu_l, ls_l, v_l)["loss"].backward()
    g = torch.zeros_like(flat)
    model.view("log_std", g).copy_(ls_l.grad)
    for names, ins, gout in ((POLICY_LAYERS, pin, mu_l.grad), (VALUE_LAYERS, vin, v_l.grad)):
        gk = rt(gout)
        for i in (2, 1, 0):
            model.view(f"{names[i]}.weight", g).copy_(gk.t() @ ins[i])
            model.view(f"{names[i]}.bias", g).copy_(gk.sum(0))
            if i:
                gk = rt((gk @ wq(names[i], fwd=False)[0]) * (1.0 - ins[i] * ins[i]))
    return mu, v, g


# ---------------------------------------------------------------------------------------------------------------
# fixtures
# ---------------------------------------------------------------------------------------------------------------
class Fixture:
    """one seeded buffer: ``flat`` the fp32 parameters, ``x`` [512, O] bf16-valued rows, ``actions``, ``logp_old``,
    ``adv``, ``ret``, ``v_old`` (values_buf) as fp32; ``band`` = (ln-ratio width, v width) it was built with"""

    def __init__(self, shape, kind, cls, conv, **t):
        self.shape, self.kind, self.cls, self.conv = shape, kind, cls, conv
        self.__dict__.update(t)

    def model(self, dtype=torch.float32) -> ActorCritic:
        spec = get_spec(self.shape)
        return _model_like(ActorCritic(spec.obs_dim, spec.act_dim), self.flat, dtype)

    def reference(self, params: Params, idx, model: Optional[ActorCritic] = None, old=None, v_old=None) -> Dict:
        return reference(model or self.model(), params, self.x, self.actions, self.logp_old, self.adv, self.ret,
                         self.v_old if v_old is None else v_old, idx, old)

    def loss_fn(self, params: Params, idx, dtype, old=None, v_old=None):
        ii = torch.arange(ROWS) if idx is None else idx.long()
        batch, o = _batch(dtype, ii, self.actions, self.logp_old, self.adv, self.ret,
                          self.v_old if v_old is None else v_old, old)
        return lambda mu, ls, v: _loss(params, mu, ls, v, batch, o)


def ratio_band_clear(lnr: torch.Tensor, clip: float, band: float) -> torch.Tensor:
    """rows whose ln ratio keeps ``band`` away from both ln(1 +- clip)"""
    return ((lnr - math.log1p(clip)).abs() > band) & ((lnr - math.log1p(-clip)).abs() > band)


def value_branch(v: torch.Tensor, v_old: torch.Tensor, ret: torch.Tensor, clip: float):
    """per row: group (0 clamp inactive, 1 clamp active and (v - R)^2 the larger term, 2 clamp active and
    (vc - R)^2 the larger) and the distance to the nearest branch point a change of ``v`` can cross:
    ``||v - v_old| - clip|`` and, clamp active, ``|(v + vc) / 2 - R|`` (the tie of the two terms)"""
    dd = v - v_old
    active = dd.abs() > clip
    vc = v_old + dd.clamp(-clip, clip)
    f1, f2 = (v - ret) ** 2, (vc - ret) ** 2
    group = torch.where(active, torch.where(f1 > f2, 1, 2), 0)
    dist = (dd.abs() - clip).abs()
    tie = (0.5 * (v + vc) - ret).abs()
    dist = torch.where(active, torch.minimum(dist, tie), dist)
    return group, dist


def place_value_clip(v: torch.Tensor, ret: torch.Tensor, clip: float, band: float, seed: int) -> torch.Tensor:
    """``values_buf`` for ``value_clip``: a third of the rows in each group of ``value_branch`` (a row whose
    ``|v - R|`` is too small for group 1 at this band goes to group 2), every row at least ``band`` away from the
    branch points after the rounding of the entry to fp32.  Asserts each group holds at least 20 % of the rows."""
    assert band < clip, (band, clip)
    g = torch.Generator().manual_seed(seed)
    n = v.numel()
    e = v - ret
    pad = 1.1 * band + 0.01
    ok1 = e.abs() > 1.5 * pad + 0.02                     # group 1 needs pad < d < 2 |e| - 2 pad
    order = torch.randperm(n, generator=g)
    first = order[ok1[order]][: n // 3]                  # a third of the rows, among those group 1 can hold
    want = torch.zeros(n, dtype=torch.long)
    want[first] = 1
    rest = order[want[order] == 0]
    want[rest[: rest.numel() // 2]] = 2
    s1 = torch.where(e >= 0, 1.0, -1.0).to(F64)
    for _ in range(100):
        u = torch.rand(n, generator=g, dtype=F64)
        lo1, hi1 = pad, 2.0 * e.abs() - 2.0 * pad
        d1 = lo1 + (hi1 - lo1) * u                       # group 1: on the side of e, the tie at d = 2 |e|
        d2 = 2.0 * pad + 0.4 * u                         # group 2: the other side, any d
        vo = torch.where(want == 0, v + (clip - band) * (u - 0.5),
                         torch.where(want == 1, v - s1 * (clip + d1), v + s1 * (clip + d2)))
        vo = vo.float().to(F64)
        group, dist = value_branch(v, vo, ret, clip)
        if bool(((dist > band) & (group == want)).all()):
            break
    else:
        raise AssertionError("value_clip: rows left inside the branch band")
    shares = [float((group == k).double().mean()) for k in range(3)]
    assert min(shares) >= 0.2, shares
    return vo.float()


_SEED = {s: 100 * (i + 1) for i, s in enumerate(SHAPES)}
SAT_TARGET_STD = 3.2        # pre-activation std of `saturated`: P(|tanh| > 0.99) ~ 0.4, P(|tanh| < 0.9) ~ 0.35


def _init_flat(shape: str, kind: str, x: torch.Tensor) -> torch.Tensor:
    spec = get_spec(shape)
    with torch.random.fork_rng():
        torch.manual_seed(_SEED[shape])
        m = ActorCritic(spec.obs_dim, spec.act_dim)
        with torch.no_grad():
            m.view("log_std").copy_(torch.linspace(-0.5, 0.3, spec.act_dim).reshape(1, -1))
            for name in POLICY_LAYERS + VALUE_LAYERS:
                m.view(f"{name}.bias").copy_(0.1 * torch.randn(m.view(f"{name}.bias").shape))
            if kind == "saturated":
                # fc1 then fc2 of each head scaled so that its pre-activations have std SAT_TARGET_STD over the rows
                for fc1, fc2 in (("p_fc1", "p_fc2"), ("v_fc1", "v_fc2")):
                    h = x.double()
                    for name in (fc1, fc2):
                        w, b = m.view(f"{name}.weight"), m.view(f"{name}.bias")
                        z = h @ w.double().t() + b.double()
                        w.mul_(SAT_TARGET_STD / z.std().item())
                        h = torch.tanh(h @ w.double().t() + b.double())
    return m.flat.detach().clone()


def hidden_activations(model64: ActorCritic, x: torch.Tensor):
    p = model64.views()
    out = []
    for fc1, fc2 in (("p_fc1", "p_fc2"), ("v_fc1", "v_fc2")):
        h = x.to(F64)
        for name in (fc1, fc2):
            h = torch.tanh(torch.nn.functional.linear(h, p[f"{name}.weight"], p[f"{name}.bias"]))
            out.append(h.detach())
    return out


def forward_errors(model32: ActorCritic, x, actions, conv: str) -> Dict[str, tuple]:
    """per class: max (|logp - logp_fp64|, |v - v_fp64|, |mu - mu_fp64|) of the emulated forward over the rows"""
    mu64, v64 = emulate("f64", model32, x)
    ls = model32.view("log_std").detach()
    lp64 = oracle.gaussian_logp(actions.double(), mu64, ls.double(), conv)
    out = {}
    for cls in CLASSES + ("s3", "fp8pg"):
        mu, v = emulate(cls, model32, x)
        lp = oracle.gaussian_logp(actions.float(), mu, ls.float(), conv)
        out[cls] = ((lp.double() - lp64).abs().max().item(), (v.double() - v64).abs().max().item(),
                    (mu.double() - mu64).abs().max().item())
    # class f32 serves the fp32 and the bf16x3 paths: the larger of the fp32 forward's and the 16-bit operands' error
    out["f32"] = tuple(max(a, b) for a, b in zip(out["f32"], out.pop("s3")))
    return out


@functools.lru_cache(maxsize=None)
def build_fixture(shape: str, kind: str = "base", cls: str = "f32", conv: str = "std", value_loss: str = "mse",
                  clip: float = 0.2) -> Fixture:
    """the fixture ``kind`` of ``shape`` for the paths of class ``cls`` (its bands), the loss reading log_std under
    ``conv`` and the value term ``value_loss``.  Pure CPU, seeded; the conditions of each kind are asserted here."""
    assert kind in KINDS and cls in CLASSES
    spec = get_spec(shape)
    O, A = spec.obs_dim, spec.act_dim
    g = torch.Generator().manual_seed(_SEED[shape] + 7)
    randn = lambda *s: torch.randn(*s, generator=g, dtype=F64)       # noqa: E731
    x = (1.0 + randn(ROWS, O)).clamp(-5, 5).float()
    if cls == "f32":    # 16-bit rows, hi + lo as bf16x3 stores them: exact in fp32 and bf16x3, both halves non-zero
        x = storage.decode(storage.encode(x, storage.DT_S3), storage.DT_S3)
    else:               # bf16 rows: what the bf16 paths and fp8 mode's bf16 buffer hold
        x = x.to(torch.bfloat16).float()
    flat = _init_flat(shape, kind, x)
    m64 = _model_like(ActorCritic(O, A), flat, F64)
    with torch.no_grad():
        mu, ls, v = m64(x.double())
    v = v.reshape(-1)
    if kind == "saturated":
        hs = torch.cat([h.reshape(-1) for h in hidden_activations(m64, x)]).abs()
        hi, lo = float((hs > 0.99).double().mean()), float((hs < 0.9).double().mean())
        assert hi >= 0.25 and lo >= 0.25, (shape, hi, lo)
    sigma = oracle.sigma_from_log_std(ls, conv)
    t = 0.75 * (1.0 - 2.0 * (torch.arange(A) % 2)).to(F64)
    actions = (mu + sigma * (t + 0.3 * randn(ROWS, A))).float()
    adv = (0.6 + randn(ROWS)).float()
    ret = (v + 0.3 + 0.5 * randn(ROWS)).float()
    logp = oracle.gaussian_logp(actions.double(), mu, ls, conv).reshape(-1)
    errs = forward_errors(_model_like(m64, flat, torch.float32), x, actions, conv)
    band = (MARGIN * errs[cls][0], MARGIN * errs[cls][1])

    # ---- logp_old: the ratio's branch ----
    if kind == "all_clipped":
        # |ln ratio| in [0.5, 1.0] on the side its advantage sign clips (adv > 0: ratio > 1 + clip)
        # (a band that reaches past 0.5 narrows the range from below)
        up = adv.double() > 0
        lo = torch.where(up, math.log1p(clip), -math.log1p(-clip)) + 1.01 * band[0]
        lo = lo.clamp(min=0.5)
        assert bool((lo < 0.99).all()), (shape, kind, cls, band)
        lr = (lo + (0.995 - lo) * torch.rand(ROWS, generator=g, dtype=F64)) * torch.where(up, 1.0, -1.0)
        logp_old = (logp - lr).float()
    elif kind == "none_clipped":
        logp_old = (logp + 0.01 * randn(ROWS)).float()
    else:
        # the old policy: mu moved by noise of a size that clips about a tenth of the rows; rows inside the
        # band are re-drawn
        logp_old = torch.zeros(ROWS)
        todo, scale = torch.ones(ROWS, dtype=torch.bool), 0.12
        for _ in range(60):
            k = int(todo.sum())
            pert = scale / math.sqrt(A) * randn(k, A)
            scale *= 1.1            # (a band wider than the clip range leaves only rows well beyond it)
            logp_old[todo] = oracle.gaussian_logp(actions.double()[todo], mu[todo] + pert, ls, conv).reshape(-1).float()
            todo = ~ratio_band_clear(logp - logp_old.double(), clip, band[0])
            if not bool(todo.any()):
                break
    lnr = logp - logp_old.double()
    assert bool(ratio_band_clear(lnr, clip, band[0]).all()), (shape, kind, cls, band)
    clipped = (torch.exp(lnr) - 1.0).abs() > clip
    if kind == "all_clipped":
        assert bool(clipped.all()) and bool((lnr.abs() >= 0.5).all()) and bool((lnr.abs() <= 1.0).all())
        assert bool((torch.sign(lnr) == torch.sign(adv.double())).all())
    if kind == "none_clipped":
        assert not bool(clipped.any())

    # ---- values_buf: the value term's branches ----
    if kind == "value_clip":
        v_old = place_value_clip(v, ret.double(), clip, band[1], _SEED[shape] + 13)
    else:
        v_old = (v + 0.3 * randn(ROWS)).float()
        if value_loss != "mse":
            for _ in range(100):
                bad = value_branch(v, v_old.double(), ret.double(), clip)[1] <= band[1]
                if not bool(bad.any()):
                    break
                v_old[bad] = (v[bad] + 0.3 * randn(int(bad.sum()))).float()
    if value_loss != "mse" or kind == "value_clip":
        assert bool((value_branch(v, v_old.double(), ret.double(), clip)[1] > band[1]).all()), (shape, kind, cls)
    return Fixture(shape, kind, cls, conv, flat=flat, x=x, actions=actions, logp_old=logp_old, adv=adv, ret=ret,
                   v_old=v_old, band=band, forward_errors=errs)


def clip_flip_allowance(model: ActorCritic, params: Params, rows, actions, idx, ref: Dict,
                        old_model: Optional[ActorCritic] = None, first: bool = False) -> int:
    """fp8_policy_gemms: how many entries of ``ref["ln_ratio"]`` a kernel whose policy forward runs on e4m3 GEMMs may
    count on the other side of a clip bound.  No fixture band models that forward (4 x its largest error exceeds
    the clip range), so the entry's own error decides: the ``fp8pg`` forward is emulated for the minibatch's rows
    with ``model``'s parameters, and an entry counts when its distance to the nearer of ln(1 +- clip) is within
    4 x ITS emulated |ln ratio - ln ratio_fp64|.  The reference loss's ratio carries the old forward's error too
    (``old_model``: the previous step's parameters; ``first``: old = current, the ratio is 1 whatever the error)."""
    n = rows.shape[0]
    ii = torch.arange(n) if idx is None else idx.detach().cpu().long().reshape(-1)
    x, a = rows.detach().cpu().float()[ii], _f64(actions)[ii]

    def ln_p(m):        # per entry: the emulated and the fp64 log-density
        ls = m.view("log_std").detach().cpu().double()
        out = []
        for cls in ("fp8pg", "f64"):
            mu = emulate(cls, m, x)[0].double()
            if params.loss == "ppo":
                out.append(oracle.gaussian_logp(a, mu, ls, params.std_convention).reshape(-1))
            else:
                out.append(torch.log(oracle.normal_pdf_var(a, mu, torch.exp(ls))))
        return out
    if first:
        return 0
    emu, exact = ln_p(model)
    err = (emu - exact).abs()
    if old_model is not None:
        emu_o, exact_o = ln_p(old_model)
        err = err + (emu_o - exact_o).abs()
    lnr = ref["ln_ratio"]
    dist = torch.minimum((lnr - math.log1p(params.clip)).abs(), (lnr - math.log1p(-params.clip)).abs())
    return int((dist <= MARGIN * err).sum())


def budgets(storage: str, model_table: Dict[str, float], policy_gemms: bool = False) -> Dict[str, float]:
    """the budget of every block and of ``whole`` for a storage type (``model_table``: ``emulated_table`` of the case).

    fp32 / bf16x3 / bf16: max(floor, 4 x the emulated error model), the floor being the project's per-block figure.
    fp8: the measured per-head limit.  Its model holds the e4m3 forward GEMMs and a bf16 backward, not the e4m3
    wgrad operands, so it is a LOWER bound of that path's error: where the model of a block alone exceeds its head's
    measured limit no kernel can meet that limit, and the blocks of that head (one limit, one chain of ``g``
    operands) and the whole vector take limit + model.  (The model is this fixture's e4m3 forward error; the limit,
    measured at the default init, covers every source of the path's error there, the unmodelled e4m3 wgrad operands
    among them: errors add at most linearly.  The factor 4 of the other storage types covers summation orders
    around a model of 1e-6 .. 1e-2; it says nothing about a model that is e4m3 rounding of 0.2.)  That happens on
    `saturated` with fp8_policy_gemms only (pre-activations five times the default init's through two e4m3 GEMMs:
    model 0.15 - 0.25 on the policy blocks against the limit 0.22), whose budgets are 0.37 - 0.48: a zeroed block
    (error 1.0) or one wrong by half fails, which ``test_emulated_error_table`` asserts."""
    if storage == "fp8":
        pol, val = FP8_LIMITS[bool(policy_gemms)]
        limit = {b: (pol if (b in POLICY_BLOCKS or b == "log_std") else val) for b in BLOCKS}
        limit["whole"] = max(pol, val)
        heads = (["log_std"] + POLICY_BLOCKS, [b for b in BLOCKS if b not in POLICY_BLOCKS and b != "log_std"])
        out = dict(limit)
        for head in heads:
            if any(model_table[b] > limit[b] for b in head):
                for b in head + ["whole"]:
                    out[b] = limit[b] + model_table[b]
        return out
    blk, whole = FLOORS[STORAGE_CLASS[storage]]
    out = {b: max(blk, MARGIN * model_table[b]) for b in BLOCKS}
    out["whole"] = max(whole, MARGIN * model_table["whole"])
    return out


def loss_tolerance(storage: str, policy_gemms: bool = False) -> float:
    """the whole-vector tolerance of the storage type (the four loss sums are held to it times 1 + |ref|)"""
    return max(FP8_LIMITS[bool(policy_gemms)]) if storage == "fp8" else FLOORS[STORAGE_CLASS[storage]][1]


@functools.lru_cache(maxsize=None)
def emulated_table(shape, kind, cls, conv, value_loss, loss, mb, emu=None) -> Dict[str, float]:
    """``error_table`` of the emulated gradient (``emu``: the emulation, by default the fixture's class; "fp8pg" on
    the "fp8" fixtures) against the fp64 reference, for one case (the reference loss: its first step)"""
    fx = build_fixture(shape, kind, cls, conv, value_loss)
    p = make_params(shape, mb=mb, loss=loss, value_loss=value_loss, conv=conv)
    idx = minibatch_index(mb)
    ref = fx.reference(p, idx)
    rows = fx.x if idx is None else fx.x[idx]
    *_, g = emulate(emu or cls, fx.model(), rows, fx.loss_fn(p, idx, torch.float32))
    return error_table(g, ref)


# ---------------------------------------------------------------------------------------------------------------
# CPU tests of the harness
# ---------------------------------------------------------------------------------------------------------------
def test_blocks_partition_the_flat_vector():
    for shape in SHAPES:
        m = build_fixture(shape).model()
        spans = sorted(m.offsets[b] for b in BLOCKS)
        assert len(BLOCKS) == 13 and set(BLOCKS) == set(m.offsets)
        assert spans[0][0] == 0 and all(a[0] + a[1] == b[0] for a, b in zip(spans, spans[1:]))
        assert spans[-1][0] + spans[-1][1] == m.num_params


@pytest.mark.parametrize("loss,value_loss,conv", [("ppo", "mse", "std"), ("ppo", "clipped_half", "var"),
                                                  ("dppo_ref", "clipped_half", "var")])
def test_emulation_in_fp64_is_autograd(loss, value_loss, conv):
    """the written-out backward of ``emulate`` without roundings is the reference's autograd gradient"""
    fx = build_fixture("HalfCheetah-v2", "value_clip", "f32", conv, value_loss)
    p = make_params("HalfCheetah-v2", mb=200, loss=loss, value_loss=value_loss, conv=conv)
    idx = minibatch_index(200)
    ref = fx.reference(p, idx)
    mu, v, g = emulate("f64", fx.model(), fx.x[idx], fx.loss_fn(p, idx, F64))
    assert max(error_table(g, ref).values()) < 1e-12
    assert (mu - ref["mu"]).abs().max() < 1e-13 and (v.reshape(-1) - ref["v"]).abs().max() < 1e-13


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("cls", CLASSES)
def test_fixture_conditions(shape, cls):
    """every fixture of the matrix builds: saturation shares, branch-group shares and empty bands are asserted by
    the builders; here the consequences the GPU module relies on, from the fp64 reference"""
    idx = minibatch_index(200)
    p = make_params(shape, mb=200)
    for kind in ("base", "saturated"):
        fx = build_fixture(shape, kind, cls)
        ref = fx.reference(p, idx)
        assert all(ref["grad"][o:o + n].norm() > 0 for o, n in ref["blocks"].values())
    ref = build_fixture(shape, "all_clipped", cls).reference(p, idx)
    for b in POLICY_BLOCKS:
        o, n = ref["blocks"][b]
        assert bool((ref["grad"][o:o + n] == 0).all()), b
    o, n = ref["blocks"]["log_std"]                       # the entropy term alone: d(-c H)/dlog_std_j = -c
    assert torch.allclose(ref["grad"][o:o + n], torch.full((n,), -p.ent_coeff, dtype=F64), rtol=0, atol=1e-15)
    assert ref["clip_count"] == 200 and ref["losses"]["clipfrac"] == 1.0
    ref = build_fixture(shape, "none_clipped", cls).reference(p, idx)
    assert ref["clip_count"] == 0 and ref["losses"]["clipfrac"] == 0.0
    pv = make_params(shape, mb=200, value_loss="clipped_half", conv="var")
    fx = build_fixture(shape, "value_clip", cls, "var", "clipped_half")
    ref = fx.reference(pv, idx)
    group, dist = value_branch(ref["v"], fx.v_old.double()[idx], fx.ret.double()[idx], pv.clip)
    assert bool((dist > fx.band[1]).all()) and len(set(group.tolist())) == 3


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("kind", ["base", "saturated"])
@pytest.mark.parametrize("cls", CLASSES)
def test_no_block_is_a_cancelling_sum(shape, kind, cls):
    """per-row fp64 gradients of the 200-row minibatch: |sum_i g_i[b]| >= 1/4 |sum_i |g_i[b]|| for every block, so no
    block's relative error is the rounding of its terms measured against a much smaller sum"""
    fx = build_fixture(shape, kind, cls)
    p = make_params(shape, mb=200)
    idx = minibatch_index(200)
    m = fx.model(F64)
    tot, tot_abs = torch.zeros(m.num_params, dtype=F64), torch.zeros(m.num_params, dtype=F64)
    for i in idx.tolist():
        m.flat.grad = None
        one = torch.tensor([i])
        mu, ls, v = m(fx.x.double()[one])
        batch = _batch(F64, one, fx.actions, fx.logp_old, fx.adv, fx.ret, fx.v_old, None)[0]
        _loss(p, mu, ls, v, batch)["loss"].backward()
        tot += m.flat.grad
        tot_abs += m.flat.grad.abs()
    ref = fx.reference(p, idx)
    assert (tot / 200 - ref["grad"]).norm() <= 1e-12 * ref["grad"].norm()      # the rows' mean is the minibatch's
    share = {b: (tot[o:o + n].norm() / tot_abs[o:o + n].norm()).item() for b, (o, n) in ref["blocks"].items()}
    print(shape, kind, cls, {b: round(s, 3) for b, s in share.items()})
    assert all(s >= 0.25 for s in share.values()), share


def _plant(fault: str, ref: Dict, fx: Fixture, p: Params, idx: torch.Tensor) -> torch.Tensor:
    g = ref["grad"].clone()
    blk = lambda b: slice(ref["blocks"][b][0], sum(ref["blocks"][b]))      # noqa: E731
    if fault == "log_std halved":
        g[blk("log_std")] *= 0.5
    elif fault == "v.bias zeroed":
        g[blk("v.bias")] = 0.0
    elif fault == "mu.bias x 1.05":
        g[blk("mu.bias")] *= 1.05
    elif fault == "p_fc2.weight x 1.01":
        g[blk("p_fc2.weight")] *= 1.01
    else:       # one row's contribution removed from v_fc2.bias (the minibatch's last row, as a tail mask would)
        assert fault == "v_fc2.bias less one row"
        rest = fx.reference(p, idx[:-1])["grad"] * (idx.numel() - 1) / idx.numel()
        g[blk("v_fc2.bias")] = rest[blk("v_fc2.bias")]
    return g


# fault -> (the block compare must name, whether the whole-vector figure stays under the fp32 paths' 2e-4 too,
# whether the block's error is beyond bf16's per-block budget as well as beyond the fp32 paths')
FAULTS = {"log_std halved": ("log_std", False, True), "v.bias zeroed": ("v.bias", False, True),
          "mu.bias x 1.05": ("mu.bias", False, False), "v_fc2.bias less one row": ("v_fc2.bias", True, False),
          "p_fc2.weight x 1.01": ("p_fc2.weight", False, False)}


@pytest.mark.parametrize("fault", list(FAULTS))
def test_planted_fault_is_caught_by_block(fault):
    """each fault planted into a copy of the fp64 gradient (Humanoid, `base`, 200 rows; the bf16x3 paths' fixture
    and the bf16 paths') passes the whole-vector check at bf16's 6e-2 -- whether it passes the fp32 paths' 2e-4 too
    is stated in FAULTS -- and fails ``compare`` by block name at the fp32-class budgets; at bf16's per-block
    budget where FAULTS says so"""
    shape = "Humanoid-v2"
    p = make_params(shape, mb=200)
    idx = minibatch_index(200)
    block, under_2e4, at_bf16 = FAULTS[fault]
    for storage in ("bf16x3", "bf16"):
        cls = STORAGE_CLASS[storage]
        fx = build_fixture(shape, "base", cls)
        ref = fx.reference(p, idx)
        g = _plant(fault, ref, fx, p, idx)
        table = error_table(g, ref)
        print(fault, storage, "whole", table["whole"], block, table[block])
        assert table["whole"] < 6e-2
        assert (table["whole"] < 2e-4) == under_2e4, table["whole"]
        budget = budgets(storage, emulated_table(shape, "base", cls, "std", "mse", "ppo", 200))
        compare(ref["grad"], ref, budget)                   # the unfaulted gradient passes
        if storage == "bf16x3":
            with pytest.raises(AssertionError) as exc:
                compare(g, ref, budget)
            named = [ln.split(":")[0] for ln in str(exc.value).split("\n")[0].split("; ")]
            assert named == [f"block {block}"] + (["block whole"] if not under_2e4 else []), named
            continue
        assert (table[block] > budget[block]) == at_bf16, (table[block], budget[block])
        if at_bf16:
            with pytest.raises(AssertionError, match=f"block {block}:"):
                compare(g, ref, budget)


@pytest.mark.parametrize("shape", SHAPES)
def test_clip_flip_allowance_can_fail(shape):
    """fp8_policy_gemms' clip-count allowance on `base`: it covers the emulated e4m3 forward's own miscounts, and it is
    a minority of the rows, so a wrong count fails"""
    fx = build_fixture(shape, "base", "fp8")
    p = make_params(shape, mb=200)
    idx = minibatch_index(200)
    ref = fx.reference(p, idx)
    allow = clip_flip_allowance(fx.model(), p, fx.x, fx.actions, idx, ref)
    mu = emulate("fp8pg", fx.model(), fx.x[idx])[0].double()
    ls = fx.model().view("log_std").detach().double()
    lnr = oracle.gaussian_logp(fx.actions.double()[idx], mu, ls, "std").reshape(-1) - fx.logp_old.double()[idx]
    count = int(((torch.exp(lnr) - 1.0).abs() > p.clip).sum())
    print(shape, "allowance", allow, "of 200; emulated count", count, "reference", ref["clip_count"])
    assert abs(count - ref["clip_count"]) <= allow < 100


def test_compare_refuses_a_block_without_budget():
    fx = build_fixture("Pendulum-v0")
    ref = fx.reference(make_params("Pendulum-v0"), None)
    budget = {b: 1.0 for b in BLOCKS + ["whole"]}
    compare(ref["grad"], ref, budget)
    del budget["v_fc1.bias"]
    with pytest.raises(AssertionError, match="block v_fc1.bias: no budget"):
        compare(ref["grad"], ref, budget)
    bad = ref["grad"].clone()
    bad[ref["blocks"]["mu.bias"][0]] = float("nan")
    with pytest.raises(AssertionError, match="block mu.bias:"):
        compare(bad, ref, {b: 1.0 for b in BLOCKS + ["whole"]})


def test_band_widths():
    """the band widths of the docstring: per class the largest over the shapes, for the default-init fixtures and
    for `saturated`; and the emulated e4m3 policy GEMMs (fp8pg), which no band covers"""
    for kind in ("base", "saturated"):
        worst = {cls: [0.0, 0.0] for cls in CLASSES + ("fp8pg",)}
        for shape in SHAPES:
            for cls in worst:       # (each class on its own fixtures' rows; fp8pg on fp8's)
                errs = build_fixture(shape, kind, "fp8" if cls == "fp8pg" else cls).forward_errors[cls]
                worst[cls] = [max(w, MARGIN * e) for w, e in zip(worst[cls], errs)]
        print(f"band widths, {kind} (ln ratio, v):", {c: (f"{a:.2e}", f"{b:.2e}") for c, (a, b) in worst.items()})
        assert worst["f32"][0] < 1e-2 * worst["bf16"][0] and worst["fp8"][0] == worst["bf16"][0]
        assert worst["f32"][1] < 1e-2 * worst["bf16"][1] and worst["bf16"][1] < worst["fp8"][1]
        if kind == "base":     # (the value term's branches are driven on the default-init weights only)
            assert worst["fp8"][1] < 0.2 and worst["bf16"][0] < 0.5 * math.log1p(0.2)


EMULATIONS = (("f32", "f32", None), ("s3", "f32", "s3"), ("bf16", "bf16", None), ("fp8", "fp8", None),
              ("fp8pg", "fp8", "fp8pg"))       # (column, the fixtures' class, the emulation)


def test_emulated_error_table():
    """the error model of the budgets over the matrix's ppo-loss cases (printed for the docstring): far below the
    floors for fp32 / bf16x3 / bf16, whose budgets are therefore the floors; fp8's model (a lower bound) passes the
    measured limits only on `saturated` with fp8_policy_gemms"""
    cases = [(s, "base", "std", "mse", 200) for s in SHAPES]
    cases += [("Humanoid-v2", k, "std", "mse", 200) for k in ("saturated", "all_clipped", "none_clipped")]
    cases += [("Humanoid-v2", "value_clip", "var", "clipped_half", 200)]
    worst = {}
    for col, cls, emu in EMULATIONS:
        for sat in (False, True):
            w = worst[col, sat] = {b: 0.0 for b in BLOCKS + ["whole"]}
            for shape, kind, conv, vl, mb in cases:
                if (kind == "saturated") != sat:
                    continue
                for b, e in emulated_table(shape, kind, cls, conv, vl, "ppo", mb, emu).items():
                    assert math.isfinite(e), (col, shape, kind, b)
                    w[b] = max(w[b], e)
    cols = [(c, sat) for sat in (False, True) for c, _, _ in EMULATIONS]
    print("\n    " + "block".ljust(14) + "".join((c + ("/sat" if sat else "")).rjust(10) for c, sat in cols))
    for b in BLOCKS + ["whole"]:
        print("    " + b.ljust(14) + "".join(f"{worst[k][b]:10.1e}" for k in cols))
    for sat in (False, True):
        for col, storage in (("f32", "fp32"), ("s3", "bf16x3"), ("bf16", "bf16")):
            budget = budgets(storage, worst[col, sat])
            blk, whole = FLOORS[STORAGE_CLASS[storage]]
            assert all(budget[b] == (whole if b == "whole" else blk) for b in budget), (col, sat)
        for col, pg in (("fp8", False), ("fp8pg", True)):
            limits = budgets("fp8", {b: 0.0 for b in BLOCKS + ["whole"]}, pg)
            over = [b for b, lim in limits.items() if worst[col, sat][b] > lim]
            assert bool(over) == (sat and pg), (col, sat, over)
            # a raised budget can still fail: every one stays under 0.5
            assert max(budgets("fp8", worst[col, sat], pg).values()) < 0.5, (col, sat)
