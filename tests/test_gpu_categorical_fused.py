"""The categorical head INSIDE the rollout and evaluation kernels (``RolloutArgs`` / ``EvalArgs`` ``dist`` 1 on the
cart-pole's physics, docs/ARCHITECTURE.md §29): ``CartPole-v0`` with ``env_fused=True`` against the torch engine and
against the device-stepped path, chained launches, placed states, the partial tile, evaluation, ``bootstrap_time_limit``,
the refusals, and the engine through resume, learning, ``train.py`` and ``play.py``.

Shapes are tests/test_gpu_cartpole_fused.py's: 45 envs (two whole 16-env tiles and a 13-row one), 24 steps, a step limit
of 6 where ends by the limit are wanted and 10000 where they are not.

Decisions follow tests/test_gpu_categorical.py's band rule (``decision_band`` / ``decision_gap``), here without an
allowance: before a launch is compared with the torch engine, EVERY one of the torch engine's decisions is asserted, on
the CPU, to clear the band, and every pre-reset state to lie more than 1e-3 from a termination threshold (as the
continuous cart-pole's tests do).  The seeds were picked on the CPU, by running the torch engine alone.  Tolerances
are those two files' for the same quantities (``CLOSE``: atol 2e-4, rtol 1e-4; the moments: ``_compare_rollouts``')."""
import json
import math
import subprocess
import sys
import types

import pytest
import torch

from pytorch_dppo_amd.config import dppo_preset
from pytorch_dppo_amd.envs import get_spec, make_vec_env
from pytorch_dppo_amd.models.actor_critic import ActorCritic
from pytorch_dppo_amd.parallel.dist import DistContext
from pytorch_dppo_amd.runtime.evaluator import EVAL_ENV_SEED_OFFSET, evaluate_batch
from pytorch_dppo_amd.utils import rng
from pytorch_dppo_amd.utils.obs_stats import RunningObsStats
from test_gpu_categorical import DEV, HIDDEN, ROOT, _engine, _sync_mode_raises, decision_band, decision_gap
from test_gpu_tensor_env import _record_new_states, _threshold_margin, _training_state

pytestmark = pytest.mark.gpu

V0, V1 = "CartPole-v0", "CartPole-v1"
E, T = 45, 24
CLOSE = dict(atol=2e-4, rtol=1e-4)
# Seeds at which the torch engine alone meets the preconditions below, scanned on the CPU; each test asserts them.
# Rollout, seeds 1..139: ten had >= 5 state-decided ends and a threshold margin above 1e-3 with every decision clear
# of its band; 126 has 28 ends, margin 1.31e-3, smallest gap 31.6 bands (11, tests/test_gpu_categorical.py's seed at
# 64 x 8, comes within 1.96e-4 of a threshold at 45 x 24).  Evaluation at the natural limit, seeds 1..59: 16 clears
# EVAL_MARGIN both ways (stochastic 6.85e-4, lengths 9..34, 18.4 bands; arg-max 4.36e-4, lengths 8..24, 148 bands).
ROLLOUT_SEED = 126
EVAL_SEEDS = {(6, False): 5, (6, True): 5, (200, False): 16, (200, True): 16}
BAD_BIAS = 1.0      # evaluation at the natural limit: a lead of action 0's logit under which the poles fall


def _fused(dtype, limit, seed=ROLLOUT_SEED, fused=True, **kw):
    """the GPU engine on CartPole-v0, statistics seeded from the reset observations, logits of spread ~0.3 (the last
    layer times 8, as tests/test_gpu_categorical.py's rollout test)"""
    eng, model, env, stats = _engine(V0, dtype, E=kw.pop("E", E), T=kw.pop("T", T), seed=seed, model_seed=seed,
                                     max_episode_length=limit, env_fused=fused, **kw)
    stats.observes(env.observe())
    with torch.no_grad():
        model.view("mu.weight").mul_(8.0)
    eng.params_changed()
    return eng, model, env, stats


def _cpu_twin(model, stats):
    """the model and the statistics as CPU copies (the torch references run there)"""
    m = ActorCritic(4, 2, HIDDEN)
    with torch.no_grad():
        m.flat.copy_(model.flat.detach().cpu())
    st = RunningObsStats(4)
    st.load_state_dict({k: (v.cpu() if torch.is_tensor(v) else v) for k, v in stats.state_dict().items()})
    return m, st


_REFS = {}


def torch_reference(seed, limit, m_cpu, st_cpu, dtype="bf16x3", start=None, E=E, T=T):
    """One rollout of the torch engine on the CPU, with what the preconditions need: the smallest decision gap over
    its band (fp32 and bf16x3 share a band: the storage class f32) and the threshold margin of its pre-reset states.
    Computed once per (seed, limit, placed start) and shared; never modified."""
    from pytorch_dppo_amd.runtime.engine_torch import TorchEngine
    key = (seed, limit, E, T, None if start is None else id(start))
    if key in _REFS:
        R = _REFS[key]
        assert torch.equal(R.flat, m_cpu.flat.detach()) and torch.equal(R.mean_f32, st_cpu.mean_f32)
        return R
    p = dppo_preset(env_name=V0, num_envs=E, exploration_size=E * T, batch_size=E * T, hidden=HIDDEN, seed=seed,
                    max_episode_length=limit)
    env = make_vec_env(get_spec(V0), E, seed=seed, max_episode_length=limit)
    ref = TorchEngine(p, m_cpu, env, st_cpu, torch.device("cpu"), 0)
    if start is not None:
        ref.load_env_state({k: (v.clone() if torch.is_tensor(v) else v) for k, v in start.items()})
    new_states, seen = [], []
    _record_new_states(env, new_states)
    step = env.step

    def recording(a):
        seen.append((st_cpu.normalize(env.observe()).clone(), env.t))
        return step(a)
    env.step = recording
    ro = ref.rollout()
    worst = math.inf
    for x, k in seen:
        band, z64 = decision_band(m_cpu, x, dtype)
        worst = min(worst, float(decision_gap(z64, ref.key_action, env.env_idx, k, False).min()) / band)
    R = types.SimpleNamespace(
        actions=ref.actions.clone(), logp=ref.logp.clone(), rewards=ref.rewards.clone(), dones=ref.dones.clone(),
        x=ref.x.clone(), state=env.state.clone(), ep_len=env.ep_len.clone(), ep_ret=env.ep_ret.clone(), t=env.t,
        s1=ro["s1"].clone(), s2=ro["s2"].clone(), ep_count=float(ro["ep_count"]), ep_return_sum=float(ro["ep_return_sum"]),
        gap_over_band=worst, margin=_threshold_margin(new_states), decisions=len(seen) * E,
        flat=m_cpu.flat.detach().clone(), mean_f32=st_cpu.mean_f32.clone())
    _REFS[key] = R
    return R


def assert_preconditions(R, ends_by_state):
    print(f"reference: {R.decisions} decisions, smallest gap / band {R.gap_over_band:.2f}, threshold margin "
          f"{R.margin:.3e}, episode ends {int(R.dones.sum())}")
    assert R.decisions == T * E and R.gap_over_band > 1.0          # every decision clears the band
    assert R.margin > 1e-3                                         # no done flag can flip inside the tolerance
    assert len({tuple(r) for r in R.actions.reshape(-1, 2).tolist()}) == 2      # both actions taken
    if ends_by_state:
        assert int(R.dones.sum()) >= 5
    assert torch.equal(R.rewards, torch.ones_like(R.rewards))


def engine_result(eng, env, ro):
    """a launch's outputs in the reference's shapes, on the CPU"""
    torch.cuda.synchronize()
    Tn, En = eng.T, eng.E
    xk = eng.decode(eng.x_buf).view(Tn + 1, En, -1).cpu().float()
    return types.SimpleNamespace(
        actions=eng.actions.view(Tn, En, 2).cpu().clone(), logp=eng.logp.view(Tn, En).cpu().clone(),
        rewards=eng.rewards.view(Tn, En).cpu().clone(), dones=eng.dones.view(Tn, En).cpu().clone(), x=xk[..., :4], xk=xk,
        state=env.state.cpu().clone(), ep_len=env.ep_len.cpu().clone(), ep_ret=env.ep_ret.cpu().clone(), t=env.t,
        s1=ro["s1"].cpu().clone(), s2=ro["s2"].cpu().clone(), ep_count=float(ro["ep_count"]),
        ep_return_sum=float(ro["ep_return_sum"]))


def one_hot_rows(a):
    rows = a.reshape(-1, 2)
    return bool(((rows == 0) | (rows == 1)).all()) and bool((rows.sum(1) == 1).all())


def compare(G, R):
    """G: the fused launch (engine_result); R: the torch engine's rollout or another engine_result"""
    close = lambda a, b: torch.allclose(a.float(), b.float(), **CLOSE)      # noqa: E731
    assert one_hot_rows(G.actions) and torch.equal(G.actions, R.actions)
    assert torch.equal(G.dones, R.dones) and torch.equal(G.rewards, R.rewards)
    for name in ("logp", "x", "state", "ep_ret"):
        gap = (getattr(G, name).float() - getattr(R, name).float()).abs().max().item()
        print(f"{name}: max gap {gap:.3e}")
        assert close(getattr(G, name), getattr(R, name)), name
    assert bool((G.logp <= 0).all())
    assert bool((G.xk[..., 4] == 1.0).all()) and bool((G.xk[..., 5:] == 0.0).all())       # bias column, padding
    assert torch.equal(G.ep_len, R.ep_len) and G.t == R.t
    # the moments (tests/test_gpu_tensor_env.py _compare_rollouts) and the episode statistics
    assert torch.allclose(G.s1, R.s1, rtol=1e-4, atol=1e-2)
    assert torch.allclose(G.s2, R.s2, rtol=1e-4, atol=1e-4 * (float(R.s2.abs().max()) + 1.0))
    assert G.ep_count == R.ep_count == float(G.dones.sum())
    assert G.ep_return_sum == pytest.approx(R.ep_return_sum, rel=1e-6)


# ---- 1. rollout against the torch engine ------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["fp32", "bf16x3"])
def test_fused_rollout_matches_torch_engine(dtype):
    eng, model, env, stats = _fused(dtype, 10000)
    assert eng.discrete and not eng.stepped_env and eng.kernel_kind == 2 and eng.kernel_dist == 1
    assert not eng.heads and not eng.phead                     # the update stays on the tile kernel
    R = torch_reference(ROLLOUT_SEED, 10000, *_cpu_twin(model, stats), dtype)
    assert_preconditions(R, ends_by_state=True)                # on the CPU, before the launch
    ptrs = (env.state.data_ptr(), env.ep_len.data_ptr(), env.ep_ret.data_ptr())
    G = engine_result(eng, env, eng.rollout())
    compare(G, R)
    assert ptrs == (env.state.data_ptr(), env.ep_len.data_ptr(), env.ep_ret.data_ptr())


def test_fused_rollout_bf16_bookkeeping():
    """low precision: no reference shares its decisions; the bookkeeping must still be consistent (limit 6)"""
    limit = 6
    eng, model, env, stats = _fused("bf16", limit)
    assert not eng.stepped_env and eng.kernel_dist == 1
    G = engine_result(eng, env, eng.rollout())
    assert one_hot_rows(G.actions) and len({tuple(r) for r in G.actions.reshape(-1, 2).tolist()}) == 2
    assert bool(torch.isfinite(G.logp).all()) and bool((G.logp <= 0).all())
    assert bool(torch.isfinite(G.xk).all()) and bool(torch.isfinite(G.state).all())
    assert torch.equal(G.rewards, torch.ones_like(G.rewards)) and bool(((G.dones == 0) | (G.dones == 1)).all())
    for e in range(E):
        ends = [t for t in range(T) if G.dones[t, e] > 0]
        assert ends, e                                           # limit 6 < 24 steps: every column ends
        assert int(G.ep_len[e]) == T - 1 - ends[-1] and float(G.ep_ret[e]) == float(G.ep_len[e]), e
        gaps = [b - a for a, b in zip([-1] + ends, ends)]
        assert max(gaps) <= limit and T - 1 - ends[-1] < limit, e
    assert G.ep_count == float(G.dones.sum()) > 0 and G.t == T


# ---- 2. fused against the device-stepped path ---------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["fp32", "bf16x3"])
def test_fused_rollout_matches_stepped_path(dtype):
    eng_f, model, env_f, stats = _fused(dtype, 10000)
    eng_s, model2, env_s, stats2 = _fused(dtype, 10000)
    assert torch.equal(model.flat.data, model2.flat.data) and torch.equal(stats.mean_f32, stats2.mean_f32)
    R = torch_reference(ROLLOUT_SEED, 10000, *_cpu_twin(model, stats), dtype)
    assert_preconditions(R, ends_by_state=True)
    S = engine_result(eng_s, env_s, eng_s.rollout_stepped())   # works on this env whatever the flag says
    # no host synchronisation in the fused rollout (the probe of tests/test_gpu_categorical.py)
    probe = _sync_mode_raises()
    prev = torch.cuda.get_sync_debug_mode()
    if probe:
        torch.cuda.set_sync_debug_mode("error")
    try:
        ro = eng_f.rollout()
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    print("sync probe armed:", probe)
    G = engine_result(eng_f, env_f, ro)
    compare(G, S)
    compare(G, R)


# ---- 3. two chained launches ----------------------------------------------------------------------------------------------
def test_chained_launches_equal_the_single_launch():
    """10 + 14 steps through t_base: the env state, the episode trackers and the step key carry over"""
    limit = 6
    runs = []
    for parts in ((T,), (10, 14)):
        eng, model, env, stats = _fused("bf16x3", limit)
        moms, eps, t_base = [], [], 0
        for n in parts:
            mom, ep = torch.zeros_like(eng.mom), torch.zeros_like(eng.epstat)
            eng._launch_rollout(n, t_base, env.t, stats, stats.shift(), mom=mom, epstat=ep)
            env.t += n
            t_base += n
            moms.append(mom)
            eps.append(ep)
        torch.cuda.synchronize()
        runs.append((eng, env, moms, eps))
    (e1, v1, m1, p1), (e2, v2, m2, p2) = runs
    for name in ("x_buf", "actions", "logp", "rewards", "dones"):
        assert torch.equal(getattr(e1, name).view(torch.uint8), getattr(e2, name).view(torch.uint8)), name
    assert torch.equal(v1.state, v2.state) and torch.equal(v1.ep_len, v2.ep_len) and torch.equal(v1.ep_ret, v2.ep_ret)
    assert v1.t == v2.t == T
    dones = e1.dones.view(T, E)
    want = torch.zeros(T, E, device=DEV)
    want[limit - 1::limit] = 1.0                                 # a pole cannot fall in 6 steps from its reset
    assert torch.equal(dones, want) and one_hot_rows(e1.actions.cpu())
    # per-tile episode sums (return sum, count: small integers, exact in any order) and moments
    assert torch.equal(p1[0], p2[0] + p2[1]) and float(p1[0][:, 1].sum()) == float(dones.sum())
    assert torch.allclose(m1[0], m2[0] + m2[1], rtol=1e-5, atol=1e-5)


# ---- 4. placed states ------------------------------------------------------------------------------------------------------
def test_placed_states_and_the_push_mapping():
    """x' = x + dt x_dot and th' = th + dt th_dot do not depend on the action, so which rows terminate at the first
    step is fixed by the placed states; from rest at the origin, x_dot' has the sign of the push."""
    limit = 50
    eng, model, env, stats = _fused("fp32", limit, T=1)
    placed = torch.zeros(E, 4)
    placed[0] = torch.tensor([2.39, 1.0, 0.0, 0.0])         # x' =  2.41: terminal
    placed[1] = torch.tensor([-2.39, -1.0, 0.0, 0.0])       # x' = -2.41: terminal
    placed[2] = torch.tensor([0.0, 0.0, 0.205, 0.5])        # th' =  0.215 > 0.20944: terminal
    placed[3] = torch.tensor([0.0, 0.0, -0.205, -0.5])      # th' = -0.215: terminal
    placed[4] = torch.tensor([2.39, -1.0, 0.0, 0.0])        # x' = 2.37: goes on (the old |x| is the larger one)
    placed[5] = torch.tensor([0.0, 0.0, 0.205, -0.5])       # th' = 0.195: goes on
    ep_len0 = torch.zeros(E, dtype=torch.int32)
    ep_len0[6] = limit - 1                                  # at the origin, ends by the step limit
    want = torch.zeros(E)
    want[[0, 1, 2, 3, 6]] = 1.0
    # on the CPU, before the launch: the outcome under EITHER action, and its margins to the thresholds
    twin = make_vec_env(get_spec(V0), E, seed=ROLLOUT_SEED, max_episode_length=limit)
    new = {}
    for idx in (0, 1):
        twin.state = placed.clone()
        new[idx], _, term = twin._dynamics(torch.full((E,), idx, dtype=torch.int64), 0)
        assert torch.equal(term.float() + (ep_len0 + 1 >= limit).float(), want)
        assert _threshold_margin([new[idx]]) > 1e-3
    assert bool((new[1][7:, 1] > 0).all()) and bool((new[0][7:, 1] < 0).all())       # +10 for index 1, -10 for index 0
    eng.load_env_state({"state": placed.clone(), "ep_len": ep_len0.clone(), "ep_ret": ep_len0.float(), "t": 0})
    reset0 = twin._reset_state(0)
    eng.rollout()
    torch.cuda.synchronize()
    assert torch.equal(eng.dones.cpu(), want) and torch.equal(eng.rewards.cpu(), torch.ones(E))
    a = eng.actions.cpu()
    assert one_hot_rows(a)
    idx = a.argmax(1)
    rest = torch.arange(7, E)
    assert 0 < int(idx[rest].sum()) < len(rest)             # both actions among the rows at rest
    st = env.state.cpu()
    assert bool((st[rest, 1] > 0).eq(idx[rest] == 1).all()) and bool((st[rest, 1] < 0).eq(idx[rest] == 0).all())
    assert bool((st[rest, 1] != 0).all())
    going = torch.tensor([4, 5] + rest.tolist())
    expect = torch.where((idx == 1)[:, None], new[1], new[0])
    assert torch.allclose(st[going], expect[going], **CLOSE)
    ended = torch.tensor([0, 1, 2, 3, 6])
    assert torch.allclose(st[ended], reset0[ended], atol=1e-6, rtol=1e-5) and float(st[ended].abs().max()) <= 0.05 + 1e-6
    assert env.ep_len.cpu().tolist() == [0, 0, 0, 0, 1, 1, 0] + [1] * (E - 7)


# ---- 5. the partial tile ------------------------------------------------------------------------------------------------------
GUARD = 0x5A


def _raw_args(eng, model, env, stats, ints, bufs=None, dt=None, rows=16):
    """the positional arguments of ext.rollout (tests/test_gpu_cartpole_fused.py's binding test)"""
    b = bufs or {}
    g = lambda k, d: b.get(k, d)       # noqa: E731
    kp = env.kernel_params()
    keys = [kp["key_env"], kp["key_term"], kp["key_reset"], eng.key_action]
    return (eng.dt_fwd if dt is None else dt, rows, g("state", env.state), g("ep_len", env.ep_len), g("ep_ret", env.ep_ret),
            eng.wimg_fwd, eng.layout, eng.scales, model.flat.data, stats.mean_f32, stats.inv_std_f32, stats.shift(),
            g("x_buf", eng.x_buf), g("actions", eng.actions), g("logp", eng.logp), g("rewards", eng.rewards),
            g("dones", eng.dones), g("mom", eng.mom), g("epstat", eng.epstat), ints, keys, float(eng.p.reward_clip),
            eng.qscale, eng.empty_x, eng.x_rows[0])


def _ints(eng, env, kind=2, O=4, A=2, S=4, dist=1, T_=None):
    kp = env.kernel_params()
    ints = [kind, eng.E, O, A, S, eng.T if T_ is None else T_, 0, eng.E, 0, kp["limit"], eng.std_var]
    return ints if dist is None else ints + [dist]


@pytest.mark.parametrize("fin", [False, True])
def test_partial_tile_stores_nothing_past_its_rows(fin):
    """45 envs: the last tile has 13 valid rows.  Every output gets 16 rows of guard bytes behind its last valid row —
    where rows 45-47 of the last step (and of the bootstrap row) would land — and they must come back untouched."""
    limit = 6
    eng, model, env, stats = _fused("bf16x3", limit, bootstrap_time_limit=fin)
    nblk, d0, K = (E + 15) // 16, eng.d0, -(-T // limit)
    f32 = dict(dtype=torch.float32, device=DEV)
    valid = {"state": (E, (4,), torch.float32), "ep_len": (E, (), torch.int32), "ep_ret": (E, (), torch.float32),
             "x_buf": ((T + 1) * E, (d0,), eng.sdtype), "actions": (T * E, (2,), torch.float32),
             "logp": (T * E, (), torch.float32), "rewards": (T * E, (), torch.float32), "dones": (T * E, (), torch.float32),
             "mom": (nblk, (2, 4), torch.float32), "epstat": (nblk, (2,), torch.float32)}
    if fin:
        valid.update({"trunc": (T * E, (), torch.float32), "x_fin": (K * E, (d0,), eng.sdtype)})
    bufs = {}
    for k, (n, tail, dtype) in valid.items():
        bufs[k] = torch.zeros(n + 16, *tail, dtype=dtype, device=DEV)
        bufs[k].view(torch.uint8).fill_(GUARD)
    bufs["state"][:E], bufs["ep_len"][:E], bufs["ep_ret"][:E] = env.state, env.ep_len, env.ep_ret
    if fin:
        bufs["x_fin"][:K * E] = 0                            # (allocated zeroed by the caller)
    args = _raw_args(eng, model, env, stats, _ints(eng, env), bufs)
    if fin:
        eng.ext.rollout_fin(*args, bufs["trunc"], bufs["x_fin"], K)
    else:
        eng.ext.rollout(*args)
    torch.cuda.synchronize()
    for k, (n, tail, dtype) in valid.items():
        assert bool((bufs[k][n:].view(torch.uint8) == GUARD).all()), k
        if k != "x_fin":                                         # every valid row was written
            assert not bool((bufs[k][:n].reshape(n, -1).view(torch.uint8) == GUARD).all(1).any()), k
    # ... and the valid rows are the engine's own rollout from the same start
    ro = eng.rollout()
    torch.cuda.synchronize()
    mine = {"state": env.state, "ep_len": env.ep_len, "ep_ret": env.ep_ret, "x_buf": eng.x_buf, "actions": eng.actions,
            "logp": eng.logp, "rewards": eng.rewards, "dones": eng.dones, "mom": eng.mom, "epstat": eng.epstat}
    if fin:
        mine.update({"trunc": eng.trunc, "x_fin": eng.x_fin})
        assert float(eng.trunc.sum()) == float(eng.dones.sum()) == E * (T // limit)
    for k, (n, tail, dtype) in valid.items():
        assert torch.equal(bufs[k][:n].reshape(-1).view(torch.uint8), mine[k].reshape(-1).view(torch.uint8)), k
    assert float(ro["ep_count"]) == E * (T // limit)


# ---- 6. evaluation ------------------------------------------------------------------------------------------------------------
# At the natural limit every one of the 64 poles falls, and a falling pole crosses its threshold at ~0.017 rad per
# step: no seed keeps 64 crossings 1e-3 away.  The actions here are exact (+-1), so the kernel's states differ from the
# torch env's by the rounding of sinf / cosf and a division alone; the rollout tests above hold them to CLOSE's atol of
# 2e-4, and a done flag can flip only for a state closer to a threshold than the states are to each other.  So the
# evaluation asks for that tolerance as the margin, over the states an env's first episode goes through.
EVAL_MARGIN = 2e-4


def eval_twin(m_cpu, st_cpu, seed, limit, deterministic, En):
    """evaluate_batch on the CPU -> (ret, len, the smallest decision gap over its band, the threshold margin), both
    over the steps of each env's first episode (what ret / len depend on)"""
    twin_env = make_vec_env(get_spec(V0), En, seed=seed + EVAL_ENV_SEED_OFFSET, rank=0, max_episode_length=limit)
    key = rng.base_key(seed, rng.STREAM_EVAL, 0)
    new_states = []
    _record_new_states(twin_env, new_states)
    step, worst, margin, active = twin_env.step, [math.inf], [math.inf], torch.ones(En, dtype=torch.bool)

    def recording(a):
        if bool(active.any()):
            band, z64 = decision_band(m_cpu, st_cpu.normalize(twin_env.observe()), "bf16x3")
            gap = decision_gap(z64, key, twin_env.env_idx, twin_env.t, deterministic)       # deterministic: g = 0
            worst[0] = min(worst[0], float(gap[active].min()) / band)
        out = step(a)
        if bool(active.any()):
            margin[0] = min(margin[0], _threshold_margin([new_states[-1][active]]))
        active.logical_and_(~out[2].bool())      # (an env past its first episode end no longer counts)
        return out
    twin_env.step = recording
    ret_t, ln_t = evaluate_batch(m_cpu, st_cpu, twin_env, En, seed, limit, "std", deterministic)
    return ret_t, ln_t, worst[0], margin[0]


@pytest.mark.parametrize("deterministic", [False, True])
@pytest.mark.parametrize("limit", [6, 200])
def test_evaluate_matches_evaluate_batch(limit, deterministic):
    En, seed = 64, EVAL_SEEDS[(limit, deterministic)]
    eng, model, env, stats = _fused("bf16x3", limit, seed=seed, E=32, T=8)
    assert not eng.stepped_env and eng.kernel_dist == 1 and env.limit == limit
    if limit == 200:
        with torch.no_grad():
            model.view("mu.bias")[0] += BAD_BIAS
        eng.params_changed()
    eng.rollout()                                # non-trivial env state, trackers, step counter, buffers
    torch.cuda.synchronize()
    before = {k: v.clone() for k, v in _training_state(eng, model, env, stats).items()}
    # the twin on the CPU with every decision's gap recorded: the band rule, before the launch
    ret_t, ln_t, worst, margin = eval_twin(*_cpu_twin(model, stats), seed, limit, deterministic, En)
    print(f"twin lengths {sorted(set(ln_t.tolist()))}, smallest gap / band {worst:.2f}, threshold margin {margin:.3e}")
    assert worst > 1.0 and margin > EVAL_MARGIN
    if limit == 6:
        assert bool((ln_t == 6).all())                           # a pole cannot fall in 6 steps
    else:
        assert int(ln_t.max()) < 200 and int(ln_t.min()) >= 5    # every pole falls
    ret, ln = eng.evaluate(En, deterministic)    # the evaluation kernel
    torch.cuda.synchronize()
    assert ret.dtype == torch.float32 and ln.dtype == torch.int32 and ret.shape == (En,) and ln.shape == (En,)
    assert torch.equal(ln.cpu(), ln_t) and torch.equal(ret.cpu(), ret_t) and torch.equal(ret, ln.to(torch.float32))
    for k, v in _training_state(eng, model, env, stats).items():
        assert torch.equal(v, before[k]), k
    ptrs = {v.data_ptr() for v in _training_state(eng, model, env, stats).values() if v.is_cuda}
    assert ret.data_ptr() not in ptrs and ln.data_ptr() not in ptrs


# ---- 7. bootstrap_time_limit ----------------------------------------------------------------------------------------------------
def _boot_start():
    """rows 0 / 1 terminate at step 0 whatever the action; row 2 terminates ON its limit step (terminal wins); row 3
    ends by the limit at step 0; the rest are fresh"""
    state = torch.zeros(E, 4)
    state[0] = torch.tensor([2.39, 1.0, 0.0, 0.0])
    state[1] = torch.tensor([0.0, 0.0, -0.205, -0.5])
    state[2] = torch.tensor([-2.39, -1.0, 0.0, 0.0])
    ep_len = torch.zeros(E, dtype=torch.int32)
    ep_len[2], ep_len[3] = 5, 5
    return {"state": state, "ep_len": ep_len, "ep_ret": ep_len.float(), "t": 0}


def test_bootstrap_time_limit_outputs():
    limit, K = 6, 4
    snaps = {}
    for name, lim, flag in (("on", limit, True), ("off", limit, False), ("free", 10000, False)):
        eng, model, env, stats = _fused("bf16x3", lim, bootstrap_time_limit=flag)
        assert not eng.stepped_env and eng.boot == flag and eng.kernel_dist == 1
        start = _boot_start()
        start["state"][4:] = env.state.cpu()[4:]             # (the fresh rows keep their reset state)
        eng.load_env_state(start)
        ro = eng.rollout()
        torch.cuda.synchronize()
        s = {"x_buf": eng.x_buf, "actions": eng.actions, "logp": eng.logp, "rewards": eng.rewards, "dones": eng.dones,
             "state": env.state, "ep_len": env.ep_len, "ep_ret": env.ep_ret, "mom": eng.mom, "epstat": eng.epstat,
             "s1": ro["s1"], "s2": ro["s2"]}
        if flag:
            s.update({"trunc": eng.trunc, "x_fin": eng.x_fin})
        snaps[name] = {k: v.detach().clone() for k, v in s.items()}
    on, off, free = snaps["on"], snaps["off"], snaps["free"]
    for k, v in off.items():                                 # the flag leaves every rollout output bit-identical
        assert torch.equal(on[k].view(torch.uint8), v.view(torch.uint8)), k
    # the ends, by construction: a fresh pole cannot fall within 6 steps
    dones, trunc = torch.zeros(T, E), torch.zeros(T, E)
    for e in range(E):
        first = 0 if e in (0, 1, 2, 3) else limit - 1
        for t in range(first, T, limit):
            dones[t, e] = 1.0
            trunc[t, e] = 0.0 if (t == 0 and e in (0, 1, 2)) else 1.0
    assert torch.equal(on["dones"].view(T, E).cpu(), dones)
    assert torch.equal(on["trunc"].view(T, E).cpu(), trunc)   # exactly the limit-only ends
    # the final rows: under a limit no env reaches, every state up to an env's first limit end is the same, so that
    # run's next buffer row is the final row, bit for bit
    d0 = on["x_fin"].shape[-1]
    xf, xb = on["x_fin"].view(K, E, d0), free["x_buf"].view(T + 1, E, d0)
    for e in range(E):
        t = int(trunc[:, e].argmax())
        assert trunc[t, e] == 1.0 and t == (0 if e == 3 else limit if e in (0, 1, 2) else limit - 1)
        assert torch.equal(xf[t // limit, e].view(torch.uint8), xb[t + 1, e].view(torch.uint8)), (t, e)
        assert bool(xf[t // limit, e].view(torch.uint8).any())


# ---- 8. refusals -----------------------------------------------------------------------------------------------------------------
def test_binding_refusals():
    eng, model, env, stats = _fused("bf16x3", 6, T=4)
    ret = torch.zeros(E, dtype=torch.float32, device=DEV)
    ln = torch.zeros(E, dtype=torch.int32, device=DEV)

    def rollout(dt=None, rows=16, **kw):
        eng.ext.rollout(*_raw_args(eng, model, env, stats, _ints(eng, env, **kw), dt=dt, rows=rows))

    def rollout_fin(dt=None, rows=16, **kw):
        K = 1
        eng.ext.rollout_fin(*_raw_args(eng, model, env, stats, _ints(eng, env, **kw), dt=dt, rows=rows),
                            torch.zeros(eng.N, device=DEV), torch.zeros(K * E, eng.d0, dtype=eng.sdtype, device=DEV), K)

    def evaluate(dt=None, rows=16, kind=2, O=4, A=2, S=4, dist=1):
        kp = env.kernel_params()
        ints = [kind, E, O, A, S, kp["limit"], eng.std_var, 0] + ([] if dist is None else [dist])
        keys = [kp["key_env"], kp["key_term"], kp["key_reset"], eng.key_action]
        eng.ext.eval_rollout(eng.dt_fwd if dt is None else dt, eng.wimg_fwd, eng.layout, eng.scales, model.flat.data,
                             stats.mean_f32, stats.inv_std_f32, ret, ln, ints, keys, eng.qscale)

    watched = (env.state, env.ep_len, eng.dones, eng.actions, eng.logp, ret, ln)
    before = [t.clone() for t in watched]
    for call in (rollout, rollout_fin, evaluate):
        for bad in (2, -1, 3):
            with pytest.raises(RuntimeError, match="dist"):
                call(dist=bad)
        for kw in (dict(kind=0), dict(kind=1, O=3, S=2)):                       # every kind but the cart-pole
            with pytest.raises(RuntimeError, match="cart-pole"):
                call(**kw)
        for A in (1, 3):
            with pytest.raises(RuntimeError, match="state dims"):
                call(A=A)
        for dist in (0, None):                                                   # the Gaussian cart-pole still has A == 1
            with pytest.raises(RuntimeError, match="state dims"):
                call(A=2, dist=dist)
        with pytest.raises(RuntimeError, match="fp8"):
            call(dt=2)
    for call in (rollout, rollout_fin):
        with pytest.raises(RuntimeError, match="16-row"):
            call(rows=32)
    # the per-step filter's operands
    ls = RunningObsStats(4, DEV)
    ls.copy_from(stats)
    shift = stats.shift().clone()
    head, tail = eng._rollout_args(eng.T, 0, env.t, shift)
    assert tail[8][-1] == 1                                                      # (the engine's ints carry dist 1)
    nroll = eng.mom.shape[0]
    g1 = torch.zeros(2 * (-(-4 // 4)) * (-(-nroll // 4)) * 16, dtype=torch.int64, device=DEV)
    g2 = torch.zeros(8, dtype=torch.int64, device=DEV)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError, match="per-step"):
        eng.ext.rollout_stepnorm(*head, *tail, [ls.mean, ls.mean_diff, ls.mean_f32, ls.inv_std_f32], g1, g2, err,
                                 float(ls.n), 1, 1e-2)
    torch.cuda.synchronize()
    for x, y in zip(before, watched):
        assert torch.equal(x, y)                     # every refusal came before a launch
    assert int(err[0]) == 0 and not bool(g2.any())
    rollout()                                        # and the well-formed calls are taken
    evaluate()
    torch.cuda.synchronize()
    assert int(ln.min()) >= 1 and int(ln.max()) <= 6 and one_hot_rows(eng.actions.cpu())
    assert torch.equal(eng.rewards, torch.ones_like(eng.rewards))


def test_engine_refusals():
    from pytorch_dppo_amd.runtime.engine_hip import HipEngine

    def build(name, **kw):
        p = dppo_preset(**{**dict(device="gpu", env_name=name, num_envs=16, exploration_size=64, batch_size=64,
                                  dtype="bf16x3"), **kw})
        spec = get_spec(name)
        return HipEngine(p, ActorCritic(4, 2, p.hidden).to(DEV), make_vec_env(spec, 16, device=DEV),
                         RunningObsStats(4, DEV), DEV, 0)
    with pytest.raises(ValueError, match="per-step") as ei:
        build(V0, env_fused=True, obs_norm_update="step")
    assert V0 in str(ei.value)
    with pytest.raises(ValueError, match="env_fused|in-kernel"):
        build(V1, env_fused=True)                   # the v1 name stays unfused
    with pytest.raises(ValueError, match="dtype=fp8"):
        build(V0, env_fused=True, dtype="fp8")
    with pytest.raises(ValueError, match="update_kernels=heads"):
        build(V0, env_fused=True, update_kernels="heads")
    stepped = build(V0)                             # without the flag: device-stepped, like CartPole-v1
    assert stepped.stepped_env and stepped.kernel_kind is None and stepped.kernel_dist == 0
    assert build(V0, obs_norm_update="step").stepped_env
    fused = build(V0, env_fused=True)
    assert not fused.stepped_env and fused.kernel_kind == 2 and fused.kernel_dist == 1 and not fused.heads


# ---- 9. the engine ---------------------------------------------------------------------------------------------------------------
def test_resume_continues_bit_identically(tmp_path):
    """3 iterations straight == 2 iterations, checkpoint, a fresh worker resumed from it, 1 more"""
    from pytorch_dppo_amd.runtime.launcher import run_worker
    base = dict(device="gpu", env_name=V0, num_processes=1, num_envs=32, exploration_size=32 * 8,
                batch_size=32 * 8, num_epoch=2, dtype="bf16x3", seed=4, env_fused=True)
    ctx = DistContext(device=DEV)
    w_full, _ = run_worker(dppo_preset(max_iters=3, **base), ctx, evaluator=False, quiet=True)
    ck = str(tmp_path / "ck")
    w_two, _ = run_worker(dppo_preset(max_iters=2, checkpoint_dir=ck, **base), ctx, evaluator=False, quiet=True)
    w_res, _ = run_worker(dppo_preset(max_iters=3, resume=ck, **base), ctx, evaluator=False, quiet=True)
    torch.cuda.synchronize()
    assert w_full.engine.kernel_dist == 1 and not w_res.engine.stepped_env and w_res.iteration == 3
    assert w_res.engine.adam_step == w_full.engine.adam_step
    assert not torch.equal(w_two.env.state, w_full.env.state)       # the third iteration moved the envs
    assert torch.equal(w_full.model.flat.data, w_res.model.flat.data)
    assert torch.equal(w_full.engine.adam_m, w_res.engine.adam_m)
    assert torch.equal(w_full.engine.adam_v, w_res.engine.adam_v)
    assert torch.equal(w_full.env.state, w_res.env.state)
    assert torch.equal(w_full.env.ep_len, w_res.env.ep_len) and torch.equal(w_full.env.ep_ret, w_res.env.ep_ret)
    assert w_full.env.t == w_res.env.t == 24
    assert torch.equal(w_full.stats.mean, w_res.stats.mean)


def test_fused_cartpole_v0_learns():
    """tests/test_categorical_fused_cpu.py's criterion on the GPU engine at bf16x3 with the env in the kernel: 12
    iterations at least triple the mean episode length"""
    from pytorch_dppo_amd.runtime.worker import DPPOWorker
    p = dppo_preset(device="gpu", dtype="bf16x3", env_name=V0, num_envs=32, exploration_size=2048, batch_size=512,
                    num_epoch=4, hidden=(32, 32), lr=3e-3, seed=1, env_fused=True)
    w = DPPOWorker(p, DistContext(device=DEV))
    assert w.engine.discrete and w.engine.kernel_dist == 1 and not w.engine.stepped_env and not w.engine.heads
    steps_per_episode = []
    for _ in range(12):
        w.iteration_step()
        steps_per_episode.append(p.buffer_rows / float(w.engine.dones.sum()))
    print("steps per episode:", [round(s, 1) for s in steps_per_episode])
    assert steps_per_episode[-1] >= 3.0 * steps_per_episode[0], steps_per_episode


def test_train_py_and_play_py_end_to_end(tmp_path):
    path, ck = tmp_path / "train.jsonl", str(tmp_path / "ck")
    cmd = [sys.executable, "train.py", "--device", "gpu", "--env-name", V0, "--env-fused", "true", "--eval-every", "1",
           "--eval-mode", "inline", "--max-iters", "2", "--num-processes", "1", "--num-envs", "32", "--exploration-size",
           "1024", "--batch-size", "256", "--num-epoch", "2", "--dtype", "bf16x3", "--eval-envs", "32",
           "--max-episode-length", "50", "--bootstrap-time-limit", "true", "--log-jsonl", str(path),
           "--checkpoint-dir", ck]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=170)
    assert r.returncode == 0, r.stderr[-3000:]
    recs = [json.loads(l) for l in path.read_text().splitlines()]
    its = [x for x in recs if "eval_iteration" not in x]
    evs = [x for x in recs if "eval_iteration" in x]
    assert len(its) == 2 and len(evs) >= 1
    for m in its:
        assert all(math.isfinite(m[k]) for k in ("loss", "loss_clip", "loss_value", "loss_ent", "grad_norm")), m
        assert m["ep_count"] > 0 and 1.0 <= m["mean_ep_return"] <= 50.0
    for e in evs:
        assert e["eval_episodes"] == 32 and 1.0 <= e["eval_length_mean"] <= 50.0
        assert e["eval_return_mean"] == pytest.approx(e["eval_length_mean"])      # reward 1 per step
    # play.py on its checkpoint: the registry entry is all it needs
    r = subprocess.run([sys.executable, "play.py", "--checkpoint", ck, "--device", "gpu", "--episodes", "2"], cwd=ROOT,
                       capture_output=True, text=True, timeout=170)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if "episode length" in l]
    assert len(lines) == 2
    for l in lines:
        length = int(l.rsplit(" ", 1)[1])
        assert 1 <= length <= 50 and f"episode reward {float(length)}" in l
