"""Categorical policies on the GPU engine (docs/ARCHITECTURE.md §27): the act kernel's categorical step (csrc/act.hip,
csrc/policy_step.h categorical_row) against ``oracle.policy_act(dist="categorical")``, the tile kernel's loss_kind 2
(csrc/mlp.hip) per parameter block against an fp64 gradient, and the engine on ``CartPole-v1``.
tests/test_categorical.py holds the oracle itself to scalar float64 arithmetic on the CPU.

Decisions.  A sampled action is an arg-max of ``z + g``; a kernel's logits differ from the twin's by rounding, so a row
whose two largest ``z_k + g_k`` are closer than that rounding may legitimately choose the other action.  The rule
(``decision_gap`` / ``decision_band``): the gap is taken from the fp64 forward on the CPU plus the fp32 noise, the band
is ``max(1e-5, 4 x max |z_emulated - z_fp64|)`` with ``test_update_reference.emulate`` of the dtype's class (the larger
of ``f32`` and ``s3`` for fp32 / bf16x3, as that module's class f32; ``bf16`` on the rows as bf16 stores them), and
rows whose gap exceeds the band must carry exactly the oracle's one-hot row.  At most 1/8 of the rows may fall inside
the band, asserted on the CPU before any launch.

Gradient fixtures follow test_update_reference's design (``cat_fixture``): observations ``1 + randn`` held exactly by
the storage class, ``adv = 0.6 + randn``, biases ``0.1 randn``, rows within the band of ``ln(1 +- clip)`` re-drawn and
then asserted clear.  A categorical ``dL/dz = dlogp (o - p)`` cancels over rows whose actions were drawn from the
policy itself (``E[o] = p``), whatever the advantages' mean, so the fixture's actions are action 0 with probability
0.75 and a draw from the policy otherwise: ``check_no_policy_block_is_a_cancelling_sum`` (run by tests/test_categorical.py)
holds the share to 1/4."""
import functools
import json
import math
import os
import subprocess
import sys
import types

import pytest
import torch

from pytorch_dppo_amd.config import Params, dppo_preset
from pytorch_dppo_amd.envs import VecEnv, get_spec, make_vec_env, register_tensor_env
from pytorch_dppo_amd.models.actor_critic import ActorCritic
from pytorch_dppo_amd.ops import oracle, storage
from pytorch_dppo_amd.parallel.dist import DistContext
from pytorch_dppo_amd.runtime.evaluator import EVAL_ENV_SEED_OFFSET, evaluate_batch
from pytorch_dppo_amd.utils import rng
from pytorch_dppo_amd.utils.obs_stats import RunningObsStats
from test_update_reference import (BLOCKS, F64, MARGIN, POLICY_BLOCKS, ROWS, STORAGE_CLASS, budgets, compare, emulate,
                                   error_table, format_table, loss_tolerance, make_params, minibatch_index,
                                   ratio_band_clear)

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0) if torch.cuda.is_available() else None
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CARTPOLE = "CartPole-v1"
DTYPES = ["fp32", "bf16x3", "bf16"]
HIDDEN = (64, 64)
STEP_KEY = 4321


class BanditEnv(VecEnv):
    """a discrete test env of any (obs, actions): s' = 0.9 s + 0.1 (a + 1) / K, reward 1 for action 0"""
    @property
    def state_dim(self):
        return self.O

    def _reset_state(self, step_key):
        d = torch.arange(self.O, device=self.device, dtype=torch.int64)
        return rng.gauss(self.key_reset, self.env_idx[:, None], step_key, d[None, :])

    def observe(self):
        return self.state.clone()

    def _dynamics(self, a, step_key):
        assert a.dtype == torch.int64 and a.shape == (self.E,)
        new = 0.9 * self.state + 0.1 * ((a.to(torch.float32) + 1.0) / self.A)[:, None]
        return new, (a == 0).to(torch.float32), torch.zeros(self.E, dtype=torch.bool, device=self.device)


def bandit(O, K):
    name = f"Bandit-{O}x{K}"
    register_tensor_env(name, BanditEnv, obs_dim=O, act_dim=K, time_limit=50, discrete=True)
    return name


def _engine(env_name, dtype, E=16, T=4, seed=0, model_seed=0, **kw):
    from pytorch_dppo_amd.runtime.engine_hip import HipEngine
    kw.setdefault("hidden", HIDDEN)
    kw.setdefault("exploration_size", E * T)
    kw.setdefault("batch_size", E * T)
    p = dppo_preset(device="gpu", env_name=env_name, num_envs=E, dtype=dtype, seed=seed, **kw)
    spec = get_spec(env_name)
    torch.manual_seed(model_seed)
    model = ActorCritic(spec.obs_dim, spec.act_dim, p.hidden).to(DEV)
    env = make_vec_env(spec, E, seed=p.seed, device=DEV, max_episode_length=p.max_episode_length)
    stats = RunningObsStats(spec.obs_dim, DEV)
    eng = HipEngine(p, model, env, stats, DEV, 0)
    eng.params_changed()
    return eng, model, env, stats


# ---- the decision rule ---------------------------------------------------------------------------------------------
def _emulated_logit_error(model, x, dtype):
    """max |z_emulated - z_fp64| over the rows ``x`` (normalised, fp32, CPU) for the dtype's class"""
    x = x.detach().cpu().float()
    z64 = emulate("f64", model, x)[0]
    if STORAGE_CLASS[dtype] == "f32":
        errs = [(emulate(c, model, x)[0].double() - z64).abs().max().item() for c in ("f32", "s3")]
        return max(errs), z64
    xb = x.to(torch.bfloat16).float()                    # the tile holds the rows in bf16
    return (emulate("bf16", model, xb)[0].double() - z64).abs().max().item(), z64


def decision_band(model, x, dtype):
    err, z64 = _emulated_logit_error(model, x, dtype)
    return max(1e-5, MARGIN * err), z64


def decision_gap(z64, key_action, env_idx, step_key, deterministic):
    """per row: the gap between the largest and the second largest z_k + g_k (fp64 logits, the fp32 keyed noise)"""
    s = z64.clone()
    if not deterministic:
        K = z64.shape[1]
        s = s + rng.gumbel(key_action, env_idx.cpu()[:, None], step_key, torch.arange(K)[None, :]).double()
    top = s.topk(2, dim=1).values
    return top[:, 0] - top[:, 1]


def _assert_close(got, want, dtype, what):
    """tests/test_gpu_act.py's per-dtype tolerance"""
    d = (got - want).abs()
    print(f"{what} {dtype}: max {d.max().item():.3e} mean {d.mean().item():.3e}")
    if dtype in ("fp32", "bf16x3"):
        assert torch.allclose(got, want, atol=2e-4, rtol=1e-4), what
    else:
        assert d.max().item() < 5e-2 and d.mean().item() < 5e-3, (what, d.max().item(), d.mean().item())


def _obs(E, O, seed_only=False):
    g = torch.Generator().manual_seed(1000 * E + O)
    scale = 0.5 + 3.0 * torch.rand(O, generator=g)
    offs = torch.randn(O, generator=g)
    if seed_only:
        return (torch.randn(256, O, generator=g) * scale + offs).to(DEV)
    obs = torch.randn(E, O, generator=g) * scale + offs
    obs[0, 0] = offs[0] + 9.0 * scale[0]                 # beyond the +-5 clamp
    return obs.to(DEV)


# ---- 1. the act kernel against oracle.policy_act --------------------------------------------------------------------
# Two logit patterns.  "lead": the default-init weights and per-action biases 0.5 randn, the largest 0.3 clear of the
# next -- the arg-max of K near-equal logits would otherwise sit inside the bf16 band on more than 1/8 of the rows.  Its
# deterministic rows mostly choose that one action, so "spread" (fp32 / bf16x3, whose bands are ~1e-5): the mu weights
# times 8 and the biases without the lead, where the deterministic rows choose several actions (asserted) and a wrong
# lane-to-index mapping of the shuffled arg-max cannot hide.  In both the sampled rows choose many.
ACT_CASES = [(d, K, O, pat) for d in DTYPES for K in (2, 3, 18, 40) for O in (4, 11)
             for pat in (("lead", "spread") if d != "bf16" else ("lead",))]


@pytest.mark.parametrize("dtype,K,O,pattern", ACT_CASES, ids=lambda v: str(v))
def test_act_matches_oracle(dtype, K, O, pattern):
    """E = 1, 17 (a partial tile), 256; K = 2, 3 leave lanes of a row idle, K = 40 exceeds the 32 lanes of a row at
    the 8-wave forms and K = 18 the 16 lanes of fp32's 4-wave form (the strided loop)"""
    eng, model, env, stats = _engine(bandit(O, K), dtype)
    assert eng.discrete and eng.stepped_env
    stats.observes(_obs(256, O, seed_only=True))
    with torch.no_grad():
        b = 0.5 * torch.randn(K, generator=torch.Generator().manual_seed(K))
        if pattern == "lead":
            b[b.argmax()] += 0.3
        else:
            model.view("mu.weight").mul_(8.0)
        model.view("mu.bias").copy_(b.to(DEV))
        model.flat.data[:K] = 0.7                         # (a log_std it must ignore)
    eng.params_changed()
    for E in (1, 17, 256):
        obs = _obs(E, O)
        eidx = torch.arange(E, device=DEV)
        for det in (False, True):
            o_t, logp_t, z_t, x_t = oracle.policy_act(model, stats, obs, eng.key_action, eidx, STEP_KEY, "std", det,
                                                      dist="categorical")
            # on the CPU, from the oracle alone, before any launch: which rows are clear of the band
            band, z64 = decision_band(model, x_t, dtype)
            gap = decision_gap(z64, eng.key_action, eidx, STEP_KEY, det)
            clear = gap > band
            inside = int((~clear).sum())
            print(f"E {E} K {K} O {O} det {det}: band {band:.3e}, {inside} of {E} rows inside")
            assert inside <= E // 8, (band, inside)
            # (the oracle's own decision is the fp64 one on the clear rows)
            s64 = z64 if det else z64 + rng.gumbel(eng.key_action, eidx.cpu()[:, None], STEP_KEY,
                                                   torch.arange(K)[None, :]).double()
            assert torch.equal(o_t.cpu().argmax(1)[clear], s64.argmax(1)[clear])
            a, logp, z = (t.clone() for t in eng.act(obs, STEP_KEY, det))
            torch.cuda.synchronize()
            assert a.shape == (E, K) and logp.shape == (E,) and z.shape == (E, K)
            assert bool(((a == 0) | (a == 1)).all()) and bool((a.sum(1) == 1).all())        # one-hot rows
            assert torch.equal(a.cpu()[clear], o_t.cpu()[clear])
            _assert_close(z, z_t, dtype, "logits")
            # logp: the twin's log-softmax at the action the launch chose (the oracle's logp on the clear rows)
            want = torch.log_softmax(z_t.double(), 1).gather(1, a.argmax(1, keepdim=True)).squeeze(1).float()
            assert torch.allclose(want.cpu()[clear], logp_t.cpu()[clear], atol=1e-5)
            _assert_close(logp, want, dtype, "logp")
            # ... and exactly this launch's own logits' (fp32 arithmetic on K terms)
            own = torch.log_softmax(z.double(), 1).gather(1, a.argmax(1, keepdim=True)).squeeze(1)
            assert (logp.double() - own).abs().max().item() <= 1e-5 * (1.0 + float(z.abs().max()))
            if det:
                tie_free = a.argmax(1) == z.argmax(1)      # the launch's own arg-max
                assert bool(tie_free.all())
            if E == 256:
                distinct = int(a.argmax(1).unique().numel())
                print(f"distinct actions chosen: {distinct}")
                if not det:
                    assert distinct >= min(K, 6), distinct
                elif pattern == "spread":
                    assert distinct >= min(K, 3), distinct


def test_ties_go_to_the_lowest_index():
    """equal logits, deterministic: every lane and shuffle step must prefer the lower index"""
    for dtype, K in (("fp32", 18), ("bf16x3", 40), ("bf16", 3)):
        eng, model, env, stats = _engine(bandit(4, K), dtype)
        with torch.no_grad():
            model.view("mu.weight").zero_()
            model.view("mu.bias").zero_()
        eng.params_changed()
        a, logp, z = eng.act(_obs(17, 4), STEP_KEY, True)
        assert bool((z == 0).all()) and bool((a.argmax(1) == 0).all()) and bool((a.sum(1) == 1).all())
        assert torch.allclose(logp, torch.full_like(logp, -math.log(K)), atol=1e-6)
        with torch.no_grad():
            model.view("mu.bias")[K - 2:] = 1.0                 # the last two tie above the rest
        eng.params_changed()
        a, _, _ = eng.act(_obs(17, 4), STEP_KEY, True)
        assert bool((a.argmax(1) == K - 2).all()) and bool((a.sum(1) == 1).all())


@pytest.mark.parametrize("dtype", DTYPES)
def test_act_outputs_are_optional_and_nothing_else_moves(dtype):
    E, O, K = 45, 11, 18
    eng, model, env, stats = _engine(bandit(O, K), dtype)
    stats.observes(_obs(256, O, seed_only=True))
    obs = _obs(E, O)
    nblk, TILE = (E + 15) // 16, 16
    f32 = dict(dtype=torch.float32, device=DEV)

    def fresh():
        outs = {"actions": torch.zeros(E + TILE, K, **f32), "logp": torch.zeros(E + TILE, **f32),
                "mu": torch.zeros(E + TILE, K, **f32), "x_out": torch.zeros(E + TILE, eng.d0, dtype=eng.sdtype, device=DEV),
                "mom": torch.zeros(nblk + 1, 2, O, **f32)}
        for t in outs.values():
            t.view(torch.uint8).fill_(0x5A)
        return outs

    def launch(outs, want):
        none = eng.no_q
        g = lambda k: outs[k] if k in want else (eng.empty_x if k == "x_out" else none)     # noqa: E731
        eng._launch_act(obs, STEP_KEY, False, 0, eng.key_action, stats, stats.shift(), g("actions"), g("logp"), g("mu"),
                        g("x_out"), g("mom"), True)
        torch.cuda.synchronize()
    full = fresh()
    launch(full, set(full))
    for name, t in full.items():
        n = nblk if name == "mom" else E
        assert bool((t[n:].view(torch.uint8) == 0x5A).all()), name
        assert not bool((t[:n].reshape(n, -1).view(torch.uint8) == 0x5A).all(1).any()), name
    for want in ({"actions"}, {"logp"}, {"mu"}, {"actions", "x_out"}, {"logp", "mom"}):
        outs = fresh()
        launch(outs, want)
        for name, t in outs.items():
            if name in want:
                assert torch.equal(t.view(torch.uint8), full[name].view(torch.uint8)), (want, name)
            else:
                assert bool((t.view(torch.uint8) == 0x5A).all()), (want, name)
    a, logp, z = eng.act(obs, STEP_KEY)
    assert torch.equal(a, full["actions"][:E]) and torch.equal(logp, full["logp"][:E]) and torch.equal(z, full["mu"][:E])


@pytest.mark.parametrize("dtype", DTYPES)
def test_gaussian_launch_is_unchanged(dtype):
    """dist 0: the launch without the argument and with it give the same bits, and both are the Gaussian twin at
    tests/test_gpu_act.py's tolerances"""
    E, O, A = 45, 17, 6
    eng, model, env, stats = _engine(f"Synthetic-{O}x{A}", dtype)
    assert not eng.discrete
    stats.observes(_obs(256, O, seed_only=True))
    obs = _obs(E, O)
    a7, lp7, mu7 = (t.clone() for t in eng.act(obs, STEP_KEY))
    f32 = dict(dtype=torch.float32, device=DEV)
    a6, lp6, mu6 = torch.zeros(E, A, **f32), torch.zeros(E, **f32), torch.zeros(E, A, **f32)
    none = eng.no_q
    eng.ext.policy_act(eng.dt_fwd, eng.wimg_fwd, eng.layout, eng.scales, model.flat.data, stats.mean_f32,
                       stats.inv_std_f32, stats.shift(), obs, a6, lp6, mu6, eng.empty_x, none,
                       [E, O, A, 0, 0, 0], [eng.key_action, 0, STEP_KEY], eng.qscale)
    torch.cuda.synchronize()
    assert torch.equal(a6, a7) and torch.equal(lp6, lp7) and torch.equal(mu6, mu7)
    a_t, lp_t, mu_t, _ = oracle.policy_act(model, stats, obs, eng.key_action, torch.arange(E, device=DEV), STEP_KEY)
    _assert_close(a7, a_t, dtype, "actions")
    _assert_close(mu7, mu_t, dtype, "mu")
    assert torch.allclose(lp7, lp_t, atol=1e-4, rtol=1e-5)
    with pytest.raises(RuntimeError, match="dist"):
        eng.ext.policy_act(eng.dt_fwd, eng.wimg_fwd, eng.layout, eng.scales, model.flat.data, stats.mean_f32,
                           stats.inv_std_f32, stats.shift(), obs, a6, lp6, mu6, eng.empty_x, none,
                           [E, O, A, 0, 0, 0, 2], [eng.key_action, 0, STEP_KEY], eng.qscale)


# ---- 2. the tile kernel's gradient against fp64, per parameter block -------------------------------------------------
GRAD_O = 11
KS = (2, 3, 18)
PATHS = {"fp32-16": ("fp32", 16), "bf16x3-32": ("bf16x3", 32), "bf16-32": ("bf16", 32), "bf16-64": ("bf16", 64)}
CLIP = 0.2
SAT_ACTION = 1
TILT = 0.75          # the share of rows whose action is action 0 whatever the policy (see the module docstring)


def _cat_logp(onehot, z):
    return oracle.categorical_logp(onehot, z).reshape(-1)


@functools.lru_cache(maxsize=None)
def cat_fixture(K, kind="base", cls="f32"):
    """512 rows of a (GRAD_O, K) categorical policy, hidden 64,64; kinds base | saturated | all_clipped"""
    O = GRAD_O
    g = torch.Generator().manual_seed(500 + 10 * K + len(kind))
    randn = lambda *s: torch.randn(*s, generator=g, dtype=F64)       # noqa: E731
    x = (1.0 + randn(ROWS, O)).clamp(-5, 5).float()
    x = storage.decode(storage.encode(x, storage.DT_S3), storage.DT_S3) if cls == "f32" else x.to(torch.bfloat16).float()
    with torch.random.fork_rng():
        torch.manual_seed(40 + K)
        m = ActorCritic(O, K, HIDDEN)
        with torch.no_grad():
            m.view("log_std").copy_(torch.linspace(-0.5, 0.3, K).reshape(1, -1))     # (unread: its gradient is 0)
            for name in ("p_fc1", "p_fc2", "mu", "v_fc1", "v_fc2", "v"):
                m.view(f"{name}.bias").copy_(0.1 * torch.randn(m.view(f"{name}.bias").shape))
            m.view("mu.weight").mul_(8.0)                # logits of spread ~0.3 (the init leaves them ~0.04)
    m64 = ActorCritic(O, K, HIDDEN).double()
    with torch.no_grad():
        m64.flat.copy_(m.flat.double())
        if kind == "saturated":
            # ONE action's logit (SAT_ACTION's row of the mu layer) scaled until it stands 30 above the rest on 30 % of
            # the rows; the other logits keep their size, so no storage class has to hold a logit of 100 whose
            # probability matters (where the scaled logit is far below, its action has probability 0)
            J = SAT_ACTION
            z = m64(x.double())[0]
            rest = torch.cat([z[:, :J], z[:, J + 1:]], 1).max(1).values
            lo_s, hi_s = 1.0, 1e5
            for _ in range(60):
                mid = math.sqrt(lo_s * hi_s)
                if torch.quantile(mid * z[:, J] - rest, 0.70).item() < 30.0:
                    lo_s = mid
                else:
                    hi_s = mid
            m64.view("mu.weight")[J].mul_(hi_s)
            m64.view("mu.bias")[J].mul_(hi_s)
        flat = m64.flat.detach().float().clone()
        m64.flat.copy_(flat.double())
        z, _, v = m64(x.double())
    v = v.reshape(-1)
    if kind == "saturated":
        top = z.topk(2, dim=1).values
        assert float(((top[:, 0] - top[:, 1]) >= 30.0).double().mean()) >= 0.25
    p = torch.softmax(z, 1)
    drawn = torch.multinomial(p, 1, generator=g).reshape(-1)
    a = torch.where(torch.rand(ROWS, generator=g) < TILT, torch.zeros_like(drawn), drawn)
    if kind == "saturated":          # an action of probability e^-30 has no ratio worth testing: where one logit leads
        lead = (z.topk(2, dim=1).values[:, 0] - z.topk(2, dim=1).values[:, 1]) >= 3.0       # by 3, the policy's own draw
        a = torch.where(lead, drawn, a)
    onehot = torch.zeros(ROWS, K).scatter_(1, a[:, None], 1.0)
    adv = (0.6 + randn(ROWS)).float()
    ret = (v + 0.3 + 0.5 * randn(ROWS)).float()
    v_old = (v + 0.3 * randn(ROWS)).float()
    logp = _cat_logp(onehot.double(), z)
    m32 = ActorCritic(O, K, HIDDEN)
    with torch.no_grad():
        m32.flat.copy_(flat)
    err = 0.0
    for c in (("f32", "s3") if cls == "f32" else ("bf16",)):
        ze = emulate(c, m32, x)[0]
        err = max(err, (_cat_logp(onehot, ze.float()).double() - logp).abs().max().item())
    band = MARGIN * err
    if kind == "all_clipped":
        up = adv.double() > 0
        lo = (torch.where(up, math.log1p(CLIP), -math.log1p(-CLIP)) + 1.01 * band).clamp(min=0.5)
        assert bool((lo < 0.99).all()), band
        lr = (lo + (0.995 - lo) * torch.rand(ROWS, generator=g, dtype=F64)) * torch.where(up, 1.0, -1.0)
        logp_old = (logp - lr).float()
    else:
        logp_old = torch.zeros(ROWS)
        todo, scale = torch.ones(ROWS, dtype=torch.bool), 0.25
        for _ in range(12 if kind == "saturated" else 60):       # (saturated: no perturbations of the scaled logit's size)
            k = int(todo.sum())
            logp_old[todo] = _cat_logp(onehot.double()[todo], z[todo] + scale * randn(k, K)).float()
            scale *= 1.1
            todo = ~ratio_band_clear(logp - logp_old.double(), CLIP, band)
            if not bool(todo.any()):
                break
        if kind == "saturated" and bool(todo.any()):
            # A logit that rises by 30 across the rows is a steep function of the hidden layer: rounded to bf16 it
            # moves by ~1 on every row, so bf16's band (1.2) is wider than the clip range, and no perturbation of a
            # saturated row's logits moves its ratio (logp ~ 0 before and after).  The rows left are placed beyond the
            # band directly, on either side whatever their advantage's sign: ratios of e^+-(band + 0.2 .. 0.5), half of
            # them on the side where the clip does not bind and the surrogate's gradient -adv ratio (o - p) is live
            n = int(todo.sum())
            side = torch.where(torch.rand(n, generator=g) < 0.5, 1.0, -1.0).double()
            lr = side * (math.log1p(CLIP) - math.log1p(-CLIP) + 1.01 * band + 0.3 * torch.rand(n, generator=g, dtype=F64))
            logp_old[todo] = (logp[todo] - lr).float()
            print(f"saturated {cls}: band {band:.3e}, {n} of {ROWS} rows placed beyond it")
    lnr = logp - logp_old.double()
    assert bool(ratio_band_clear(lnr, CLIP, band).all()), (K, kind, cls, band)
    clipped = (torch.exp(lnr) - 1.0).abs() > CLIP
    if kind == "all_clipped":
        assert bool(clipped.all()) and bool((torch.sign(lnr) == torch.sign(adv.double())).all())
    elif kind == "base":
        # both branches of the clip are driven (a wide band leaves few rows between ln 0.8 and ln 1.2)
        assert 0.02 <= float(clipped.double().mean()) <= 0.9, (float(clipped.double().mean()), band)
    if kind == "saturated":
        # the saturated rows themselves stay in the surrogate: on at least a third of them the clip does not bind
        sat = (z.topk(2, dim=1).values[:, 0] - z.topk(2, dim=1).values[:, 1]) >= 30.0
        ratio = torch.exp(lnr)
        live = ratio * adv.double() <= ratio.clamp(1.0 - CLIP, 1.0 + CLIP) * adv.double()
        assert float(live[sat].double().mean()) >= 1.0 / 3.0, float(live[sat].double().mean())
    return types.SimpleNamespace(K=K, kind=kind, cls=cls, flat=flat, x=x, actions=onehot, logp_old=logp_old, adv=adv,
                                 ret=ret, v_old=v_old, band=band)


def _cat_loss(p, fx, ii, dtype, ent_only=False):
    c = lambda t: t.to(dtype)[ii]      # noqa: E731

    def fn(mu, ls, v):
        out = oracle.ppo_loss(mu, ls, v, c(fx.actions), c(fx.logp_old), c(fx.adv), c(fx.ret), c(fx.v_old), clip=p.clip,
                              ent_coeff=p.ent_coeff, value_loss=p.value_loss, dist="categorical")
        # (a zero log_std gradient; the entropy term alone: a zero value gradient too)
        out["loss"] = (out["loss_ent"] + 0.0 * v.sum() if ent_only else out["loss"]) + 0.0 * ls.sum()
        return out
    return fn


def _model(fx, dtype):
    m = ActorCritic(GRAD_O, fx.K, HIDDEN).to(dtype)
    with torch.no_grad():
        m.flat.copy_(fx.flat.to(dtype))
    return m


@functools.lru_cache(maxsize=None)
def cat_reference(K, kind, cls, mb, ent_only=False):
    """the fp64 update on the CPU: ActorCritic in float64 with oracle.ppo_loss(dist="categorical"), and the emulated
    gradient's error table against it (the budgets' model)"""
    fx = cat_fixture(K, kind, cls)
    p = make_params(bandit(GRAD_O, K), mb=mb, hidden=HIDDEN)
    idx = minibatch_index(mb)
    ii = torch.arange(ROWS) if idx is None else idx.long()
    m = _model(fx, F64)
    mu, ls, v = m(fx.x.double()[ii])
    out = _cat_loss(p, fx, ii, F64, ent_only)(mu, ls, v)
    out["loss"].backward()
    lnr = (_cat_logp(fx.actions.double()[ii], mu.detach()) - fx.logp_old.double()[ii])
    ref = {"grad": m.flat.grad.detach().clone(), "losses": {k: float(out[k].detach()) for k in
                                                             ("loss_clip", "loss_value", "loss_ent", "approx_kl", "clipfrac")},
           "ln_ratio": lnr, "clip_count": int(((torch.exp(lnr) - 1.0).abs() > p.clip).sum()), "mb": int(ii.numel()),
           "blocks": {b: m.offsets[b] for b in BLOCKS}}
    *_, g_emu = emulate(cls, _model(fx, torch.float32), fx.x[ii], _cat_loss(p, fx, ii, torch.float32, ent_only))
    table = error_table(g_emu, ref)
    return ref, table


def _grad_engine(K, storage_name, rows, mb, fx, **over):
    from pytorch_dppo_amd.runtime.engine_hip import HipEngine
    p = make_params(bandit(GRAD_O, K), dtype=storage_name, mb=mb, device="gpu", hidden=HIDDEN, update_kernels="tile",
                    mlp_rows=rows, **over)
    spec = get_spec(p.env_name)
    model = ActorCritic(spec.obs_dim, spec.act_dim, p.hidden).to(DEV)
    with torch.no_grad():
        model.flat.copy_(fx.flat.to(DEV))
    env = make_vec_env(spec, p.num_envs, seed=p.seed, device=DEV)
    eng = HipEngine(p, model, env, RunningObsStats(spec.obs_dim, DEV), DEV, 0)
    eng.params_changed()
    O = spec.obs_dim
    xb = torch.zeros(ROWS + p.num_envs, eng.d0)
    xb[:ROWS, :O] = fx.x
    xb[:, O] = 1.0
    eng.x_buf.copy_(eng.encode(xb.to(DEV)))
    assert torch.equal(eng.decode(eng.x_buf)[:ROWS, :O].cpu(), fx.x)
    eng.actions.copy_(fx.actions)
    eng.logp.copy_(fx.logp_old)
    eng.adv.copy_(fx.adv)
    eng.ret.copy_(fx.ret)
    eng.values_buf[:ROWS].copy_(fx.v_old)
    assert eng.discrete and not eng.heads and not eng.phead and eng.train_rows == rows
    return eng, model, p


def _check_grad(tag, eng, ref, model_table, storage_name):
    budget = budgets(storage_name, model_table)
    g = eng.grad_flat.detach().cpu()
    table = error_table(g, ref)
    print(f"\n{tag}\n" + format_table(table, budget))
    assert bool(torch.isfinite(g).all()), tag
    compare(g, ref, budget)
    o, n = ref["blocks"]["log_std"]
    assert bool((g[o:o + n].view(torch.int32) == 0).all()), tag          # bit-zero
    ll = eng.last_losses()
    tol = loss_tolerance(storage_name)
    for k in ("loss_clip", "loss_value", "loss_ent", "approx_kl"):
        r = ref["losses"][k]
        assert abs(ll[k] - r) <= tol * (1.0 + abs(r)), (tag, k, ll[k], r)
    # every row is a band away from ln(1 +- clip): the kernel counts the reference's rows
    assert abs(ll["clipfrac"] - ref["clip_count"] / ref["mb"]) <= 2.0 ** -23, (tag, ll["clipfrac"], ref["clip_count"])
    return g, budget


GRAD_CASES = [(path, K, mb, "base") for path in PATHS for K in KS for mb in (None, 200, 129)]
GRAD_CASES += [(path, 18, 200, kind) for path in PATHS for kind in ("saturated", "all_clipped")]
# 40 logits: more than the 32 outputs the head kernels' dW_mu block holds (such an engine has no per-head reduce items
# and takes the tile kernel) and more than the JMAX * TPR = 32 action entries bf16's loss lanes keep in registers
GRAD_CASES += [(path, 40, 200, "base") for path in PATHS]


@pytest.mark.parametrize("path,K,mb,kind", GRAD_CASES, ids=lambda v: str(v))
def test_tile_kernel_gradient_matches_fp64_per_block(path, K, mb, kind):
    storage_name, rows = PATHS[path]
    cls = STORAGE_CLASS[storage_name]
    fx = cat_fixture(K, kind, cls)
    ref, model_table = cat_reference(K, kind, cls, mb)
    tag = f"{path} K{K} mb{mb or ROWS} {kind}"
    try:
        eng, model, p = _grad_engine(K, storage_name, rows, mb, fx)
        eng.begin_update()
        eng.grad(minibatch_index(mb))
        torch.cuda.synchronize()
        g, budget = _check_grad(tag, eng, ref, model_table, storage_name)
        if kind == "all_clipped":
            # the policy blocks are the entropy term's gradient alone
            ent_ref, _ = cat_reference(K, kind, cls, mb, True)
            assert ref["clip_count"] == ref["mb"] and eng.last_losses()["clipfrac"] == 1.0
            for b in POLICY_BLOCKS:
                o, n = ref["blocks"][b]
                want = ent_ref["grad"][o:o + n]
                assert float(want.norm()) > 0
                assert (g[o:o + n].double() - want).norm() <= budget[b] * want.norm(), (tag, b)
    finally:
        from pytorch_dppo_amd.ops import native
        native.load().set_mlp_rows(0)


CANCEL_CASES = [(K, "base") for K in KS + (40,)] + [(18, "saturated")]


def check_no_policy_block_is_a_cancelling_sum(K, kind):
    """per-row fp64 gradients of the 200-row minibatch: |sum_i g_i[b]| >= 1/4 sum_i |g_i[b]| for every policy block.
    Pure CPU: tests/test_categorical.py runs it over CANCEL_CASES."""
    fx = cat_fixture(K, kind, "f32")
    p = make_params(bandit(GRAD_O, K), mb=200, hidden=HIDDEN)
    idx = minibatch_index(200)
    m = _model(fx, F64)
    tot, tot_abs = torch.zeros(m.num_params, dtype=F64), torch.zeros(m.num_params, dtype=F64)
    for i in idx.tolist():
        m.flat.grad = None
        one = torch.tensor([i])
        mu, ls, v = m(fx.x.double()[one])
        _cat_loss(p, fx, one, F64)(mu, ls, v)["loss"].backward()
        tot += m.flat.grad
        tot_abs += m.flat.grad.abs()
    ref, _ = cat_reference(K, kind, "f32", 200)
    assert (tot / 200 - ref["grad"]).norm() <= 1e-12 * ref["grad"].norm()
    share = {b: (tot[o:o + n].norm() / tot_abs[o:o + n].norm()).item() for b, (o, n) in ref["blocks"].items()
             if b in POLICY_BLOCKS}
    print(K, kind, {b: round(s, 3) for b, s in share.items()})
    assert all(s >= 0.25 for s in share.values()), share


def test_head_kernels_refuse_the_categorical_loss():
    """loss_kind 2 reaches the per-head and 32x32 policy kernels' bindings only by hand: both name the tile kernel"""
    for phead in (True, False):
        eng, model, env, stats = _engine("Ant-v2", "bf16x3", E=32, T=16, hidden=(100, 100),
                                         update_kernels="heads", phead_kernel=phead)
        assert eng.heads and eng.phead == phead
        eng.discrete = True                        # (_update_args then passes loss_kind 2)
        eng.begin_update()
        with pytest.raises(RuntimeError, match="tile kernel"):
            eng.grad(None)
        torch.cuda.synchronize()


# ---- 3. adv_norm -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["fp32-16", "bf16x3-32", "bf16-64"])
def test_adv_norm_block_is_the_prenormalised_buffer(path):
    storage_name, rows = PATHS[path]
    fx = cat_fixture(3, "base", STORAGE_CLASS[storage_name])
    try:
        eng, model, p = _grad_engine(3, storage_name, rows, 200, fx, normalize_adv=True, adv_norm_scope="global")
        idx = minibatch_index(200)
        eng.adv_sums(finish=True)
        raw = eng.adv.clone()

        def one(block_on):
            scope = eng.adv_scope
            if not block_on:
                eng.adv_scope, eng._adv_arg = "", eng.no_q
            eng.begin_update()
            eng.grad_flat.zero_()
            eng.loss_sums.zero_()
            eng.grad(idx)
            torch.cuda.synchronize()
            eng.adv_scope = scope
            return eng.grad_flat.clone(), eng.loss_sums.clone()
        g_on, s_on = one(True)
        assert torch.equal(eng.adv, raw)
        b = eng.adv_block
        eng.adv.copy_((raw - b[0]) * b[1])
        g_pre, s_pre = one(False)
        assert torch.equal(g_on.view(torch.int32), g_pre.view(torch.int32))
        assert torch.equal(s_on.view(torch.int32), s_pre.view(torch.int32))
        eng.adv.copy_(raw)
        g_raw, _ = one(False)
        assert not torch.equal(g_raw, g_on) and bool(torch.isfinite(g_on).all())
    finally:
        from pytorch_dppo_amd.ops import native
        native.load().set_mlp_rows(0)


# ---- 4. the engine on CartPole-v1 ------------------------------------------------------------------------------------
ROLLOUT_SEED = 11


def _cartpole_pair(dtype, E=64, T=8, seed=ROLLOUT_SEED):
    """the GPU engine and, on the CPU, the torch engine with the same parameters and statistics"""
    from pytorch_dppo_amd.runtime.engine_torch import TorchEngine
    eng, model, env, stats = _engine(CARTPOLE, dtype, E=E, T=T, seed=seed, model_seed=seed, max_episode_length=10000)
    stats.observes(env.observe())
    with torch.no_grad():
        model.view("mu.weight").mul_(8.0)
    eng.params_changed()
    spec = get_spec(CARTPOLE)
    p_cpu = Params.from_dict({**eng.p.to_dict(), "device": "cpu"})
    m_cpu = ActorCritic(spec.obs_dim, spec.act_dim, eng.p.hidden)
    with torch.no_grad():
        m_cpu.flat.copy_(model.flat.detach().cpu())
    env_cpu = make_vec_env(spec, E, seed=seed, max_episode_length=10000)
    st_cpu = RunningObsStats(spec.obs_dim)
    st_cpu.load_state_dict({k: (v.cpu() if torch.is_tensor(v) else v) for k, v in stats.state_dict().items()})
    ref = TorchEngine(p_cpu, m_cpu, env_cpu, st_cpu, torch.device("cpu"), 0)
    return eng, model, env, stats, ref


def test_engine_takes_the_tile_kernel():
    eng, *_ = _engine(CARTPOLE, "bf16x3", E=64, T=8, hidden=(100, 100))
    assert eng.discrete and eng.heads is False and eng.phead is False and eng.stepped_env
    from pytorch_dppo_amd.runtime.engine_hip import HipEngine
    for kw, match in ((dict(update_kernels="heads"), "update_kernels=heads"), (dict(dtype="fp8"), "dtype=fp8"),
                      (dict(loss="dppo_ref"), "dppo_ref"), (dict(env_fused=True), "env_fused|in-kernel")):
        p = dppo_preset(**{**dict(device="gpu", env_name=CARTPOLE, num_envs=16, exploration_size=64, batch_size=64,
                                  dtype="bf16x3"), **kw})
        spec = get_spec(CARTPOLE)
        with pytest.raises(ValueError, match=match):
            HipEngine(p, ActorCritic(4, 2, p.hidden).to(DEV), make_vec_env(spec, 16, device=DEV),
                      RunningObsStats(4, DEV), DEV, 0)


@pytest.mark.parametrize("dtype", ["fp32", "bf16x3"])
def test_rollout_matches_torch_engine(dtype):
    eng, model, env, stats, ref = _cartpole_pair(dtype)
    T, E = eng.T, eng.E
    seen = []
    step = ref.env.step

    def recording(a):
        seen.append((ref.stats.normalize(ref.env.observe()).clone(), ref.env.t))
        return step(a)
    ref.env.step = recording
    ro_t = ref.rollout()
    # on the CPU, before the launch: every one of the torch engine's T * E decisions clears the band
    worst = math.inf
    for x, k in seen:
        band, z64 = decision_band(ref.model, x, dtype)
        gap = decision_gap(z64, ref.key_action, ref.env.env_idx, k, False)
        assert bool((gap > band).all()), (k, band, float(gap.min()))
        worst = min(worst, float(gap.min()) / band)
    print("smallest gap / band", worst)
    assert len({tuple(r) for r in ref.actions.reshape(T * E, 2).tolist()}) == 2 and int(ref.dones.sum()) > 0
    ro_h = eng.rollout()
    torch.cuda.synchronize()
    close = lambda a, b: torch.allclose(a.cpu().float(), b.float(), atol=2e-4, rtol=1e-4)      # noqa: E731
    assert torch.equal(eng.actions.view(T, E, 2).cpu(), ref.actions)
    assert torch.equal(eng.dones.view(T, E).cpu(), ref.dones) and torch.equal(eng.rewards.view(T, E).cpu(), ref.rewards)
    assert close(eng.logp.view(T, E), ref.logp)
    assert close(eng.decode(eng.x_buf).view(T + 1, E, -1)[..., :4], ref.x)
    assert close(env.state, ref.env.state) and torch.equal(env.ep_len.cpu(), ref.env.ep_len)
    assert close(env.ep_ret, ref.env.ep_ret) and env.t == ref.env.t == T
    assert float(ro_h["ep_count"]) == float(ro_t["ep_count"]) == float(ref.dones.sum())


def test_bf16_rollout_is_self_consistent():
    eng, model, env, stats, ref = _cartpole_pair("bf16")
    T, E = eng.T, eng.E
    state0, len0, ret0 = (t.cpu().clone() for t in (env.state, env.ep_len, env.ep_ret))
    eng.rollout()
    torch.cuda.synchronize()
    rows = eng.actions.cpu()
    assert bool(((rows == 0) | (rows == 1)).all()) and bool((rows.sum(1) == 1).all())
    # the stored logp against the twin's log-softmax on the stored rows, within the bf16 band of the logits
    x = eng.decode(eng.x_buf)[:T * E, :4].cpu()
    err, z64 = _emulated_logit_error(ref.model, x, "bf16")
    want = torch.log_softmax(z64, 1).gather(1, rows.argmax(1, keepdim=True)).squeeze(1)
    gap = (eng.logp.cpu().double() - want).abs().max().item()
    print("logp gap", gap, "band", MARGIN * err)
    assert gap <= 2.0 * max(1e-5, MARGIN * err)         # (z_a - lse: both terms move by at most the band)
    # bookkeeping: VecEnv.step replayed under the recorded indices
    renv = ref.env
    renv.state, renv.ep_len, renv.ep_ret = state0.clone(), len0.clone(), ret0.clone()
    idx = rows.argmax(1).view(T, E)
    for t in range(T):
        _, r, done, _ = renv.step(idx[t])
        assert torch.equal(eng.rewards.view(T, E)[t].cpu(), r) and torch.equal(eng.dones.view(T, E)[t].cpu(), done.float())
    assert torch.allclose(env.state.cpu(), renv.state, atol=2e-4, rtol=1e-4) and torch.equal(env.ep_len.cpu(), renv.ep_len)


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


def test_stepped_rollout_and_deferred_iteration_do_not_sync():
    from pytorch_dppo_amd.runtime.worker import DPPOWorker
    p = dppo_preset(device="gpu", env_name=CARTPOLE, num_envs=32, exploration_size=128, batch_size=64, num_epoch=2,
                    dtype="bf16x3", hidden=HIDDEN, max_episode_length=6)
    w = DPPOWorker(p, DistContext(device=DEV))
    w.iteration_step(defer=True)               # (first iteration: allocations, kernel loads)
    w.engine.evaluate(20, False)
    torch.cuda.synchronize()
    if not _sync_mode_raises():
        pytest.skip("torch.cuda.set_sync_debug_mode('error') does not raise on .item() in this build")
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        ro = w.engine.rollout_stepped()
        w.iteration_step(defer=True)
        ret, ln = w.engine.evaluate(20, False)
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    torch.cuda.synchronize()
    assert float(ro["ep_count"]) > 0 and int(ln.min()) >= 1 and int(ln.max()) <= 6


def test_log_std_and_its_moments_stay_bit_identical():
    from pytorch_dppo_amd.runtime.worker import DPPOWorker
    p = dppo_preset(device="gpu", env_name=CARTPOLE, num_envs=32, exploration_size=256, batch_size=64, num_epoch=2,
                    dtype="bf16x3", hidden=HIDDEN)
    w = DPPOWorker(p, DistContext(device=DEV))
    eng, A = w.engine, 2
    with torch.no_grad():
        w.model.flat.data[:A] = torch.tensor([0.37, -0.21], device=DEV)
    eng.params_changed()
    before = w.model.flat.data.clone()
    w.iteration_step()
    torch.cuda.synchronize()
    assert eng.adam_step > 0 and not torch.equal(w.model.flat.data[A:], before[A:])
    assert torch.equal(w.model.flat.data[:A].view(torch.int32), before[:A].view(torch.int32))
    assert bool((eng.adam_m[:A].view(torch.int32) == 0).all()) and bool((eng.adam_v[:A].view(torch.int32) == 0).all())
    assert bool((eng.grad_flat[:A].view(torch.int32) == 0).all())


@pytest.mark.parametrize("deterministic", [False, True])
def test_evaluate_agrees_with_evaluate_batch(deterministic):
    E, limit, seed = 64, 40, 5
    eng, model, env, stats = _engine(CARTPOLE, "bf16x3", E=32, T=8, seed=seed, model_seed=seed, max_episode_length=limit)
    stats.observes(env.observe())
    with torch.no_grad():
        model.view("mu.weight").mul_(8.0)
    eng.params_changed()
    # the twin on the CPU, its decisions' gaps recorded: the gap rule, before the launch
    m_cpu = ActorCritic(4, 2, eng.p.hidden)
    with torch.no_grad():
        m_cpu.flat.copy_(model.flat.detach().cpu())
    st_cpu = RunningObsStats(4)
    st_cpu.load_state_dict({k: (v.cpu() if torch.is_tensor(v) else v) for k, v in stats.state_dict().items()})
    twin_env = make_vec_env(get_spec(CARTPOLE), E, seed=seed + EVAL_ENV_SEED_OFFSET, rank=0, max_episode_length=limit)
    key = rng.base_key(seed, rng.STREAM_EVAL, 0)
    step, clear = twin_env.step, torch.ones(E, dtype=torch.bool)

    def recording(a):
        band, z64 = decision_band(m_cpu, st_cpu.normalize(twin_env.observe()), "bf16x3")
        clear.logical_and_(decision_gap(z64, key, twin_env.env_idx, twin_env.t, deterministic) > band)
        return step(a)
    twin_env.step = recording
    ret_t, ln_t = evaluate_batch(m_cpu, st_cpu, twin_env, E, seed, limit, "std", deterministic)
    # an env one of whose decisions lay inside the band may take another path from there on: the envs all of whose
    # decisions were clear (at least 7/8 of them, asserted here, before the launch) must agree exactly
    print("envs with every decision clear:", int(clear.sum()), "of", E)
    assert int(clear.sum()) >= E - E // 8
    assert deterministic or int(ln_t.min()) < limit            # (the arg-max policy holds the pole for all 40 steps)
    ret, ln = eng.evaluate(E, deterministic)
    torch.cuda.synchronize()
    assert ret.dtype == torch.float32 and ln.dtype == torch.int32 and ret.shape == (E,) and ln.shape == (E,)
    assert torch.equal(ln.cpu()[clear], ln_t[clear]) and torch.equal(ret.cpu()[clear], ret_t[clear])
    assert torch.equal(ret, ln.to(torch.float32)) and int(ln.min()) >= 1 and int(ln.max()) <= limit


def test_resume_is_bit_identical(tmp_path):
    from pytorch_dppo_amd.runtime.launcher import run_worker
    base = dict(device="gpu", env_name=CARTPOLE, num_processes=1, num_envs=32, exploration_size=32 * 8,
                batch_size=32 * 8, num_epoch=2, dtype="bf16x3", seed=4, hidden=HIDDEN)
    ctx = DistContext(device=DEV)
    w_full, _ = run_worker(dppo_preset(max_iters=3, **base), ctx, evaluator=False, quiet=True)
    ck = str(tmp_path / "ck")
    run_worker(dppo_preset(max_iters=2, checkpoint_dir=ck, **base), ctx, evaluator=False, quiet=True)
    w_res, _ = run_worker(dppo_preset(max_iters=3, resume=ck, **base), ctx, evaluator=False, quiet=True)
    torch.cuda.synchronize()
    assert w_full.engine.discrete and w_res.iteration == 3 and w_res.engine.adam_step == w_full.engine.adam_step
    assert torch.equal(w_full.model.flat.data, w_res.model.flat.data)
    assert torch.equal(w_full.engine.adam_m, w_res.engine.adam_m) and torch.equal(w_full.engine.adam_v, w_res.engine.adam_v)
    assert torch.equal(w_full.env.state, w_res.env.state) and w_full.env.t == w_res.env.t == 24
    assert torch.equal(w_full.stats.mean, w_res.stats.mean)


def test_train_py_end_to_end(tmp_path):
    path = tmp_path / "train.jsonl"
    cmd = [sys.executable, "train.py", "--device", "gpu", "--env-name", CARTPOLE, "--eval-every", "1", "--eval-mode",
           "inline", "--max-iters", "2", "--num-processes", "1", "--num-envs", "32", "--exploration-size", "1024",
           "--batch-size", "256", "--num-epoch", "2", "--dtype", "bf16x3", "--eval-envs", "32",
           "--max-episode-length", "50", "--target-kl", "0.01", "--normalize-adv", "true", "--adv-norm-scope",
           "minibatch", "--log-jsonl", str(path)]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=170)
    assert r.returncode == 0, r.stderr[-3000:]
    recs = [json.loads(l) for l in path.read_text().splitlines()]
    its = [x for x in recs if "eval_iteration" not in x]
    evs = [x for x in recs if "eval_iteration" in x]
    assert len(its) == 2 and len(evs) >= 1
    for m in its:
        assert all(math.isfinite(m[k]) for k in ("loss", "loss_clip", "loss_value", "loss_ent", "grad_norm")), m
        assert m["ep_count"] > 0 and 1.0 <= m["mean_ep_return"] <= 50.0
        assert 0.0 < -m["loss_ent"] <= 0.01 * math.log(2.0) * 1.001 or m["loss_ent"] == 0.0     # -c H, H <= ln 2
    for e in evs:
        assert e["eval_episodes"] == 32 and 1.0 <= e["eval_length_mean"] <= 50.0
        assert e["eval_return_mean"] == pytest.approx(e["eval_length_mean"])


def test_dppo_learns_discrete_cartpole_on_the_gpu_engine():
    """tests/test_categorical.py's criterion (the continuous cart-pole test's configuration: 12 iterations at least
    triple the mean episode length) on the GPU engine at bf16x3"""
    from pytorch_dppo_amd.runtime.worker import DPPOWorker
    p = dppo_preset(device="gpu", dtype="bf16x3", env_name=CARTPOLE, num_envs=32, exploration_size=2048,
                    batch_size=512, num_epoch=4, hidden=(32, 32), lr=3e-3, seed=1)
    w = DPPOWorker(p, DistContext(device=DEV))
    assert w.engine.discrete and not w.engine.heads
    steps_per_episode = []
    for _ in range(12):
        w.iteration_step()
        steps_per_episode.append(p.buffer_rows / float(w.engine.dones.sum()))
    print("steps per episode:", [round(s, 1) for s in steps_per_episode])
    assert steps_per_episode[-1] >= 3.0 * steps_per_episode[0], steps_per_episode
