"""An fp64 action-replay oracle for the in-kernel env kinds 0 (synthetic) and 1 (pendulum), and the CPU tests
that hold it to ``TorchEngine``.

For these two kinds ``done`` is a keyed draw OR the step limit and never depends on a state threshold, so given
the actions an engine recorded everything on the env side (states, rewards, done flags, reset states, episode
returns, moments) is a pure function of them.  ``replay`` recomputes it in float64 from the integer hashes of
``utils/rng.py``; it calls neither ``VecEnv.step`` nor ``_dynamics``.  The policy side (noise, log-prob,
normalised rows, the mean given the rows) has small fp64 helpers beside it.  Unlike the fp32 torch engine, which
mirrors the kernels operation for operation and therefore only serves where the actions agree, this reference
works at every storage precision: tests/test_gpu_rollout_episodes.py imports it.

Tolerances (``compare``): fp32 / bf16x3 are those of test_gpu_kernels.py test_rollout_matches_torch_engine;
the low-precision ones bind only what depends on the precision (the stored rows: one bf16 rounding; the mean
given those rows: tests/test_gpu_tensor_env.py ``_close`` for bf16, test_fp8_rollout_tracks_fp32_and_engine_trains's
mean gap for fp8)."""
import math

import pytest
import torch

from pytorch_dppo_amd.config import dppo_preset
from pytorch_dppo_amd.envs import get_spec, make_vec_env
from pytorch_dppo_amd.envs.registry import KIND_PENDULUM, KIND_SYNTHETIC
from pytorch_dppo_amd.models.actor_critic import ActorCritic
from pytorch_dppo_amd.utils import rng
from pytorch_dppo_amd.utils.obs_stats import CLIP, RunningObsStats

F64 = torch.float64
SYN_DECAY, SYN_DRIVE, SYN_NOISE, SYN_RESET, SYN_TERM_P = 0.9, 0.1, 0.05, 0.1, 0.002
PEND_DT, PEND_MAX_SPEED, PEND_MAX_TORQUE = 0.05, 8.0, 2.0


# ---- keyed draws in fp64 (the hashes and the 24-bit uniforms are utils/rng.py's) -----------------------------
def uniform64(base, env, step, dim):
    return rng.uniform01(rng.keyed(base, env, step, dim)).to(F64)


def gauss64(base, env_idx, step, ndim):
    """[E, ndim] standard normals: rng.gauss's Box-Muller (dims 2p, 2p+1 share the uniform pair keyed 2p, 2p+1
    and take its cosine / sine branch), the log, sqrt, cos and sin in float64"""
    d = torch.arange(ndim, dtype=torch.int64)
    p2 = (d >> 1) * 2
    u1 = uniform64(base, env_idx[:, None], step, p2[None, :])
    u2 = uniform64(base, env_idx[:, None], step, p2[None, :] + 1)
    r = torch.sqrt(-2.0 * torch.log(u1))
    ang = (2.0 * math.pi) * u2
    return r * torch.where(((d & 1) == 0)[None, :], torch.cos(ang), torch.sin(ang))


def _observe(kind, state):
    if kind == KIND_PENDULUM:
        return torch.stack([torch.cos(state[:, 0]), torch.sin(state[:, 0]), state[:, 1]], 1)
    return state.clone()


def pend_wrap(th):
    """the angle the pendulum's cost sees, in [-pi, pi)"""
    return torch.remainder(th + math.pi, 2.0 * math.pi) - math.pi


def pend_unclamped_speed(state, a):
    """the new angular speed before the +-8 clamp"""
    u = a[:, 0].to(F64).clamp(-PEND_MAX_TORQUE, PEND_MAX_TORQUE)
    th, thd = state[:, 0].to(F64), state[:, 1].to(F64)
    return thd + (-3.0 * 10.0 / 2.0 * torch.sin(th + math.pi) + 3.0 * u) * PEND_DT


def replay(env, state0, ep_len0, ep_ret0, t0, actions, limit):
    """Re-run a kind-0 / kind-1 env in float64 from (state0, ep_len0, ep_ret0) at step counter ``t0`` under the
    recorded ``actions`` [T, E, A].  ``env`` only names the kind, the dims and the three key prefixes.
    Per step: observe; reward and terminal; ep_len += 1, ep_ret += reward (unclipped); done = terminal |
    (ep_len >= limit); done envs add ep_ret to ep_return_sum and 1 to ep_count, reset in place from the reset
    stream and zero ep_len / ep_ret."""
    kind, O, A = env.kind, env.O, env.A
    assert kind in (KIND_SYNTHETIC, KIND_PENDULUM)
    actions = actions.detach().to("cpu", F64)
    T, E = actions.shape[0], actions.shape[1]
    assert actions.shape == (T, E, A)
    eidx = torch.arange(E, dtype=torch.int64)
    state = state0.detach().to("cpu", F64).clone()
    ep_len = ep_len0.detach().to("cpu", torch.int64).clone()
    ep_ret = ep_ret0.detach().to("cpu", F64).clone()
    obs = torch.zeros(T + 1, E, O, dtype=F64)
    rewards = torch.zeros(T, E, dtype=F64)
    dones = torch.zeros(T, E, dtype=torch.bool)
    terminals = torch.zeros(T, E, dtype=torch.bool)
    ep_return_sum, ep_count = 0.0, 0
    zero = torch.zeros(E, dtype=torch.int64)
    for t in range(T):
        k = (int(t0) + t) & rng.MASK32
        a = actions[t]
        obs[t] = _observe(kind, state)
        if kind == KIND_SYNTHETIC:
            ac = a.clamp(-1.0, 1.0)
            na = min(A, O)
            err = ac[:, :na] - torch.tanh(state[:, :na])
            reward = 1.0 - (err * err).sum(1) / na
            d = torch.arange(O, dtype=torch.int64)
            w = 0.5 + (d % 7).to(F64) / 7.0
            new = (SYN_DECAY * state + SYN_DRIVE * torch.tanh(w[None, :] * ac[:, d % A])
                   + SYN_NOISE * gauss64(env.key_env, eidx, k, O))
            terminal = uniform64(env.key_term, eidx, k, zero) < SYN_TERM_P
            reset = SYN_RESET * gauss64(env.key_reset, eidx, k, O)
        else:
            th, thd = state[:, 0], state[:, 1]
            u = a[:, 0].clamp(-PEND_MAX_TORQUE, PEND_MAX_TORQUE)
            thn = pend_wrap(th)
            reward = -(thn * thn + 0.1 * thd * thd + 0.001 * u * u)
            nthd = pend_unclamped_speed(state, a)
            nth = th + nthd * PEND_DT
            new = torch.stack([nth, nthd.clamp(-PEND_MAX_SPEED, PEND_MAX_SPEED)], 1)
            terminal = torch.zeros(E, dtype=torch.bool)
            u0 = uniform64(env.key_reset, eidx, k, zero)
            u1 = uniform64(env.key_reset, eidx, k, zero + 1)
            reset = torch.stack([(2.0 * u0 - 1.0) * math.pi, 2.0 * u1 - 1.0], 1)
        ep_len += 1
        ep_ret += reward
        done = terminal | (ep_len >= int(limit))
        ep_return_sum += float(ep_ret[done].sum())
        ep_count += int(done.sum())
        state = torch.where(done[:, None], reset, new)
        ep_len[done] = 0
        ep_ret[done] = 0.0
        rewards[t], dones[t], terminals[t] = reward, done, terminal
    obs[T] = _observe(kind, state)
    return {"obs": obs, "rewards": rewards, "dones": dones, "terminals": terminals, "state": state,
            "ep_len": ep_len, "ep_ret": ep_ret, "ep_return_sum": ep_return_sum, "ep_count": ep_count}


# ---- the policy side ---------------------------------------------------------------------------------------
def action_eps(key_action, E, A, t0, T):
    """eps[t, e, j] of the action stream, keyed (key_action, e, (t0 + t) & 0xFFFFFFFF, j)"""
    eidx = torch.arange(E, dtype=torch.int64)
    return torch.stack([gauss64(key_action, eidx, (int(t0) + t) & rng.MASK32, A) for t in range(T)])


def log_sigma64(model, std_convention):
    ls = model.view("log_std").detach().to("cpu", F64).reshape(-1)
    return ls if std_convention == "std" else 0.5 * ls


def logp64(eps, log_sigma):
    return (-0.5 * eps * eps - 0.5 * math.log(2.0 * math.pi) - log_sigma).sum(-1)


def _normalize64(obs, stats):
    m, s = stats.mean_f32.detach().to("cpu", F64), stats.inv_std_f32.detach().to("cpu", F64)
    return torch.clamp((obs - m) * s, -CLIP, CLIP)


def normalized_rows(obs, stats, mode):
    """[T+1, E, O] rows clamp((obs - mean) inv_std, +-5) under the fp32 images of ``stats``.  rollout mode: the
    engine's stats as they are; step mode: a RunningObsStats copy that absorbs obs[t] before normalising it, as
    TorchEngine.rollout does (the bootstrap row is normalised, not absorbed).  Returns (rows, the stats used)."""
    if mode == "rollout":
        return _normalize64(obs, stats), stats
    local = RunningObsStats(obs.shape[-1], "cpu")
    local.copy_from(stats)
    rows = torch.zeros_like(obs)
    for t in range(obs.shape[0] - 1):
        local.observes(obs[t])
        rows[t] = _normalize64(obs[t], local)
    rows[-1] = _normalize64(obs[-1], local)
    return rows, local


def moments64(obs, shift):
    """(count, s1, s2) of obs[0..T-1] about ``shift``"""
    d = obs[:-1].reshape(-1, obs.shape[-1]) - shift.detach().to("cpu", F64)
    return float(d.shape[0]), d.sum(0), (d * d).sum(0)


def policy_mean64(model, x):
    """the policy mean of rows x [..., O] under a float64 copy of ``model``'s weights"""
    m64 = ActorCritic(model.num_inputs, model.num_outputs, model.hidden, model.value_mult)
    with torch.no_grad():
        m64.flat.data.copy_(model.flat.detach().to("cpu"))
    m64 = m64.double()
    with torch.no_grad():
        mu, _, _ = m64(x.detach().to("cpu", F64).reshape(-1, model.num_inputs))
    return mu.reshape(*x.shape[:-1], model.num_outputs)


def expected(env, model, stats, params, key_action, start, actions):
    """everything one rollout of T steps from ``start`` ({"state", "ep_len", "ep_ret", "t"}) must leave behind,
    given the [T, E, A] actions it recorded; ``stats`` the engine's observation statistics at the launch"""
    T, E, A = actions.shape
    out = replay(env, start["state"], start["ep_len"], start["ep_ret"], start["t"], actions, env.limit)
    clip = float(params.reward_clip)
    out["rewards_clipped"] = out["rewards"].clamp(-clip, clip) if clip > 0 else out["rewards"]
    out["rows"], local = normalized_rows(out["obs"], stats, params.obs_norm_update)
    out["stats_n"], out["stats_mean"] = local.n, local.mean.detach().to("cpu", F64).clone()
    out["count"], out["s1"], out["s2"] = moments64(out["obs"], stats.shift())
    out["eps"] = action_eps(key_action, E, A, start["t"], T)
    out["log_sigma"] = log_sigma64(model, params.std_convention)
    out["logp"] = logp64(out["eps"], out["log_sigma"])
    out["t"] = int(start["t"]) + T
    return out


# ---- an engine's rollout as plain CPU tensors, and the comparison ----------------------------------------------
def torch_engine_view(eng, ro):
    return {"actions": eng.actions.clone(), "logp": eng.logp.clone(), "rewards": eng.rewards.clone(),
            "dones": eng.dones.clone(), "x": eng.x.clone(), "state": eng.env.state.clone(),
            "ep_len": eng.env.ep_len.clone(), "ep_ret": eng.env.ep_ret.clone(), "t": eng.env.t,
            "ep_count": float(ro["ep_count"]), "ep_return_sum": float(ro["ep_return_sum"]),
            "count": float(ro["count"]), "s1": ro["s1"].clone(), "s2": ro["s2"].clone()}


def _gap(name, got, want, stats=None):
    g = (got.to("cpu", F64) - want.to("cpu", F64)).abs()
    mx, mean = (float(g.max()), float(g.mean())) if g.numel() else (0.0, 0.0)
    print(f"  {name}: max gap {mx:.3e} mean {mean:.3e}")
    if stats is not None:
        stats[name] = (mx, mean)
    return g


def _allclose(name, got, want, atol, rtol, stats=None):
    g = _gap(name, got, want, stats)
    want = want.to("cpu", F64)
    bad = g > atol + rtol * want.abs()
    assert not bool(bad.any()), f"{name}: {int(bad.sum())} of {bad.numel()} beyond atol {atol} rtol {rtol}, " \
                                f"max gap {float(g.max()):.3e}"


def compare(got, exp, model, dtype="fp32", stats=None, fp8_max=None):
    """``got`` (an engine's rollout: CPU or device tensors, [T, E] layouts) against ``exp`` (``expected``).
    ``stats``: a dict that receives every (max, mean) gap; ``fp8_max``: a bound on the fp8 mean's largest gap
    (the caller's, from a measurement: the project has none of its own)."""
    T, E, A = exp["eps"].shape
    O = exp["obs"].shape[-1]
    lowp = dtype in ("bf16", "fp8")
    cpu = lambda v: v.detach().to("cpu") if torch.is_tensor(v) else v   # noqa: E731
    got = {k: cpu(v) for k, v in got.items()}
    # the env side: exact flags and counters, fp32-accurate values at every dtype
    assert torch.equal(got["dones"].view(T, E) > 0.5, exp["dones"]), "dones"
    assert bool(((got["dones"] == 0) | (got["dones"] == 1)).all())
    assert torch.equal(got["ep_len"].to(torch.int64), exp["ep_len"]), "ep_len"
    assert got["t"] == exp["t"]
    assert got["ep_count"] == float(exp["ep_count"])
    assert got["count"] == float(T * E) == exp["count"]
    _allclose("rewards", got["rewards"].view(T, E), exp["rewards_clipped"], 2e-4, 1e-4, stats)
    _allclose("env.state", got["state"], exp["state"], 2e-4, 1e-4, stats)
    _allclose("env.ep_ret", got["ep_ret"], exp["ep_ret"], 2e-4, 1e-4, stats)
    gap = abs(got["ep_return_sum"] - exp["ep_return_sum"])
    print(f"  ep_return_sum: gap {gap:.3e} over {exp['ep_count']} episodes")
    if stats is not None:
        stats["ep_return_sum"] = (gap, exp["ep_count"])
    assert gap <= 1e-5 * abs(exp["ep_return_sum"]) + 2e-4 * exp["ep_count"], "ep_return_sum"
    _allclose("s1", got["s1"], exp["s1"], 1e-2, 1e-4, stats)
    _allclose("s2", got["s2"], exp["s2"], 1e-4 * (float(exp["s2"].abs().max()) + 1.0), 1e-4, stats)
    _allclose("logp", got["logp"].view(T, E), exp["logp"], 1e-4, 1e-5, stats)
    # the stored rows, the bias column and the padding
    x = got["x"].view(T + 1, E, -1).to(F64)
    if x.shape[-1] > O:
        assert bool((x[..., O] == 1.0).all()) and bool((x[..., O + 1:] == 0.0).all()), "bias column / padding"
    if lowp:
        g = _gap("rows", x[..., :O], exp["rows"], stats)
        bad = g > 2.0 ** -8 * exp["rows"].abs() + 1e-6
        assert not bool(bad.any()), f"rows: {int(bad.sum())} of {bad.numel()} beyond one bf16 rounding, " \
                                    f"worst excess {float((g - 2.0 ** -8 * exp['rows'].abs()).max()):.3e}"
    else:
        _allclose("rows", x[..., :O], exp["rows"], 2e-4, 1e-4, stats)
    # the mean the kernel computed from the rows it stored: a - sigma eps against the fp64 forward of those rows
    mu_got = got["actions"].view(T, E, A).to(F64) - torch.exp(exp["log_sigma"]) * exp["eps"]
    mu_ref = policy_mean64(model, x[:T, :, :O])
    if dtype == "bf16":
        g = _gap("mean", mu_got, mu_ref, stats)
        assert float(g.max()) < 5e-2 and float(g.mean()) < 5e-3, "mean"
    elif dtype == "fp8":
        g = _gap("mean", mu_got, mu_ref, stats)
        assert float(g.mean()) < 0.05, "mean"
        assert fp8_max is None or float(g.max()) < fp8_max, "mean (max gap)"
    else:
        _allclose("mean", mu_got, mu_ref, 2e-4, 1e-4, stats)
    if "stats_n" in got:
        assert got["stats_n"] == pytest.approx(exp["stats_n"])
        _allclose("running mean", got["stats_mean"], exp["stats_mean"], 1e-6, 1e-6, stats)


def placement(env, limit, gen_seed, t0, state=None):
    """a start for ``load_env_state``: the env's current state (or ``state``), ep_len0 drawn in [0, limit) from a
    seeded CPU generator (limit ends on different steps in different rows of a tile), ep_ret0 non-zero"""
    g = torch.Generator(device="cpu").manual_seed(gen_seed)
    E = env.E
    ep_len0 = torch.randint(0, limit, (E,), generator=g, dtype=torch.int32)
    ep_ret0 = (0.25 + torch.rand(E, generator=g)) * (1.0 if env.kind == KIND_SYNTHETIC else -1.0)
    st = env.state.detach().to("cpu").clone() if state is None else state.to(torch.float32).clone()
    return {"state": st, "ep_len": ep_len0, "ep_ret": ep_ret0.to(torch.float32), "t": int(t0)}


def copy_start(start):
    return {k: (v.clone() if torch.is_tensor(v) else v) for k, v in start.items()}


# ---- placed pendulum states (shared with the GPU test) -----------------------------------------------------
def pendulum_placed_states(E):
    """rows 0-7: angles at and beyond +-pi and several turns out, speeds at and next to the +-8 clamp; the rest:
    the origin.  15 sin(th) dt is +0.49 at th = 7, +0.41 at -10, -0.38 at 100, +0.38 at -100 and the torque moves
    the speed by at most 0.3, so rows 4 and 5 end above +8 and row 6 below -8 whatever the action"""
    st = torch.zeros(E, 2)
    th = [3.1, -3.1, 3.2, -3.2, 7.0, -10.0, 100.0, -100.0]
    thd = [7.9, -7.9, 8.0, -8.0, 7.9, 8.0, -7.9, -8.0]
    st[:8, 0] = torch.tensor(th)
    st[:8, 1] = torch.tensor(thd)
    return st


def assert_pendulum_placement(start, exp, actions):
    """on the oracle alone: the placed rows do what they were placed for"""
    s0 = start["state"].to(F64)
    a0 = actions.detach().to("cpu", F64)[0]
    wrapped = pend_wrap(s0[:, 0])
    moved = (wrapped - s0[:, 0]).abs() > 1.0
    assert moved.tolist()[:8] == [False, False, True, True, True, True, True, True]
    assert bool((s0[:, 0] + math.pi < 0).sum() >= 3)                  # the remainder's negative branch
    assert bool(((wrapped - s0[:, 0]).abs() > 4 * math.pi).sum() >= 2)  # several turns
    raw = pend_unclamped_speed(s0, a0)
    assert bool((raw[[4, 5]] > 8.0).all()) and bool(raw[6] < -8.0)    # the speed clamp binds from both sides
    assert bool((exp["state"][:, 1].abs() <= 8.0).all())
    a_all = actions.detach().to("cpu", F64)
    assert bool((a_all > 2.0).any()) and bool((a_all < -2.0).any())   # the torque clamp binds from both sides
    want = torch.zeros_like(exp["dones"])
    want[0, 12] = True                                                # ep_len0 = limit - 1: ends at step 0
    assert torch.equal(exp["dones"], want)
    assert exp["ep_len"].tolist() == [int(n) + 2 for n in start["ep_len"][:12]] + [1]


# ---- CPU tests: the oracle against TorchEngine ---------------------------------------------------------------
GEOMETRIES = [("Synthetic-17x6", 45), ("Synthetic-5x8", 21), ("Synthetic-1x1", 19), ("Synthetic-600x3", 19),
              ("Humanoid-v2", 21), ("Pendulum-v0", 45)]
# (the clips of tests/test_gpu_rollout_episodes.py: rewards fall on both sides of them)
CLIP_FOR = {KIND_SYNTHETIC: 0.5, KIND_PENDULUM: 2.0}


def _cpu_engine(env_name, E, T, limit, seed=1, mode="rollout", clip=0.0):
    from pytorch_dppo_amd.runtime.engine_torch import TorchEngine
    p = dppo_preset(device="cpu", env_name=env_name, num_envs=E, exploration_size=E * T, batch_size=E * T,
                    max_episode_length=limit, seed=seed, obs_norm_update=mode, reward_clip=clip)
    spec = get_spec(env_name)
    torch.manual_seed(0)
    model = ActorCritic(spec.obs_dim, spec.act_dim, p.hidden)
    env = make_vec_env(spec, E, seed=seed, device="cpu", max_episode_length=limit)
    stats = RunningObsStats(spec.obs_dim, "cpu")
    eng = TorchEngine(p, model, env, stats, torch.device("cpu"), 0)
    stats.observes(env.observe())
    with torch.no_grad():
        model.flat.data[:model.num_outputs] = -0.3
    return p, eng, model, env, stats


def _cpu_case(env_name, E, T, limit, t0, seed=1, mode="rollout", clip=0.0, gen_seed=0):
    p, eng, model, env, stats = _cpu_engine(env_name, E, T, limit, seed, mode, clip)
    start = placement(env, limit, gen_seed, t0)
    eng.load_env_state(copy_start(start))
    ro = eng.rollout()
    got = torch_engine_view(eng, ro)
    if mode == "step":
        got["stats_n"], got["stats_mean"] = eng.local_stats.n, eng.local_stats.mean.clone()
    exp = expected(env, model, stats, p, eng.key_action, start, got["actions"])
    return got, exp, model


@pytest.mark.parametrize("clipped", [False, True])
@pytest.mark.parametrize("mode", ["rollout", "step"])
@pytest.mark.parametrize("env_name,E", GEOMETRIES)
def test_replay_matches_torch_engine(env_name, E, mode, clipped):
    clip = CLIP_FOR[get_spec(env_name).kind] if clipped else 0.0
    got, exp, model = _cpu_case(env_name, E, T=12, limit=5, t0=1000, mode=mode, clip=clip)
    assert int(exp["dones"].sum()) >= 2 * E                  # every env ends at least twice (limit 5, 12 steps)
    assert bool((exp["ep_len"] > 0).any())                   # and carries a running episode out
    if clipped:
        share = float((exp["rewards"].abs() > clip).double().mean())
        print("clipped share", share)
        assert 0.1 <= share <= 0.9
        assert not torch.equal(exp["rewards"], exp["rewards_clipped"])
    compare(got, exp, model)


@pytest.mark.parametrize("mode", ["rollout", "step"])
@pytest.mark.parametrize("env_name", ["Synthetic-17x6", "Pendulum-v0"])
def test_replay_matches_torch_engine_across_the_counter_wrap(env_name, mode):
    t0 = 2 ** 32 - 5
    got, exp, model = _cpu_case(env_name, 45, T=8, limit=5, t0=t0, mode=mode)
    compare(got, exp, model)
    # the keys wrapped: steps 5.. draw what a counter starting at 0 draws
    key_action = rng.base_key(1, rng.STREAM_ACTION, 0)
    assert torch.equal(exp["eps"][5:], action_eps(key_action, 45, exp["eps"].shape[-1], 0, 3))
    assert got["t"] == 2 ** 32 + 3


def test_replay_keyed_synthetic_terminations_at_seed_30():
    """the synthetic env's keyed terminations in the window tests/test_gpu_rollout_episodes.py uses (seed 30, rank
    0, 45 envs, steps 0-23): six cells, one of them (env 40) in the partial tile; TorchEngine ends there too"""
    got, exp, model = _cpu_case("Synthetic-17x6", 45, T=24, limit=7, t0=0, seed=30, gen_seed=0)
    cells = sorted((int(t), int(e)) for t, e in exp["terminals"].nonzero().tolist())
    assert cells == [(5, 20), (7, 5), (9, 27), (10, 40), (17, 9), (23, 19)]
    compare(got, exp, model)
    for t, e in cells:
        assert got["dones"][t, e] == 1.0


def test_replay_pendulum_wrap_clamps_and_reset():
    """the pieces of the pendulum a reset angle never reaches in a few steps, on the oracle and on TorchEngine:
    the cost's angle wrap from below -pi and over several turns, the +-8 speed clamp from both sides, the +-2
    torque clamp, and the keyed reset as the next observation"""
    E, T, limit = 13, 2, 50
    p, eng, model, env, stats = _cpu_engine("Pendulum-v0", E, T, limit, seed=1)
    with torch.no_grad():
        model.flat.data[:model.num_outputs] = 0.7           # sigma ~ 2: torques beyond the clamp
    start = placement(env, limit, 0, 0, state=pendulum_placed_states(E))
    start["ep_len"][12] = limit - 1
    eng.load_env_state(copy_start(start))
    ro = eng.rollout()
    got = torch_engine_view(eng, ro)
    exp = expected(env, model, stats, p, eng.key_action, start, got["actions"])
    assert_pendulum_placement(start, exp, got["actions"])
    compare(got, exp, model)
