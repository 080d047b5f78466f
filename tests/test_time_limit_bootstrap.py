"""``bootstrap_time_limit`` on the CPU: ``oracle.gae`` with ``boot`` against a scalar float64 loop, ``VecEnv.step``'s
``truncated`` / ``final_obs``, ``TorchEngine`` with the flag against the fp64 action replay of
tests/test_rollout_replay.py, and the refused combinations.

The replay knows nothing of truncation, so the reference is built from it alone: the rollout is replayed one step at
a time, and every step once more under a limit no env reaches, whose next observation is the one the env reached
before its reset (``replay_final``).  tests/test_gpu_time_limit_bootstrap.py imports the helpers."""
import math

import pytest
import torch

from pytorch_dppo_amd.config import PRESETS, Params, dppo_preset, params_from_args, ppo_preset
from pytorch_dppo_amd.envs import get_spec, make_vec_env
from pytorch_dppo_amd.models.actor_critic import ActorCritic
from pytorch_dppo_amd.ops import oracle
from test_rollout_replay import (_allclose, _cpu_engine, _normalize64, copy_start, expected, placement, replay)

F64 = torch.float64
SYN, PEND, CARTPOLE = "Synthetic-17x6", "Pendulum-v0", "CartPoleContinuous-v1"
SYN_SEED = 30            # tests/test_rollout_replay.py: keyed terminations at (5, 20), (7, 5), (9, 27), (10, 40), ...
NO_LIMIT = 1 << 40


# ---- oracle.gae with boot --------------------------------------------------------------------------------------
def _gae_scalar(r, v, d, boot, gamma, lam, seg):
    """GAE of ops/oracle.gae's docstring as a float64 loop over python floats, one env at a time"""
    T, E = len(r), len(r[0])
    adv = [[0.0] * E for _ in range(T)]
    for e in range(E):
        cont, s = [1.0] * T, 0
        if seg > 0:
            for t in range(T):
                done = d[t][e] != 0
                if s + 1 == seg and not done:
                    cont[t] = 0.0
                s = 0 if (done or s + 1 == seg) else s + 1
        nxt = 0.0
        for t in range(T - 1, -1, -1):
            nonterm = 1.0 - d[t][e]
            delta = r[t][e] + gamma * (v[t + 1][e] * nonterm + boot[t][e]) - v[t][e]
            nxt = delta + gamma * lam * nonterm * cont[t] * nxt
            adv[t][e] = nxt
    return adv


def _gae_before(rewards, values, dones, gamma, lam):
    """ops/oracle.gae's recurrence as it stood before ``boot`` (segment 0)"""
    adv = torch.zeros_like(rewards)
    nxt = torch.zeros_like(rewards[0])
    for t in range(rewards.shape[0] - 1, -1, -1):
        nonterm = 1.0 - dones[t].to(rewards.dtype)
        delta = rewards[t] + gamma * values[t + 1] * nonterm - values[t]
        nxt = delta + gamma * lam * nonterm * nxt
        adv[t] = nxt
    return adv, adv + values[:-1]


HAND = dict(r=[[1.0, -0.5], [0.5, 2.0], [-1.0, 0.25], [2.0, 1.0], [0.75, -2.0]],
            v=[[0.3, -1.0], [1.5, 0.2], [-0.7, 0.9], [0.4, -0.3], [1.1, 0.6], [-0.2, 2.0]],
            d=[[0.0, 0.0], [1.0, 0.0], [0.0, 0.0], [0.0, 1.0], [0.0, 0.0]],        # env 0 ends at t=1, env 1 at t=3
            boot=[[0.0, 0.0], [1.7, 0.0], [0.0, 0.0], [0.0, 0.0], [0.0, 0.0]])     # t=1 truncated, t=3 terminal


@pytest.mark.parametrize("seg", [0, 2])
def test_gae_boot_matches_scalar_loop(seg):
    gamma, lam = 0.9, 0.8
    t = {k: torch.tensor(x, dtype=F64) for k, x in HAND.items()}
    adv, ret = oracle.gae(t["r"], t["v"], t["d"], gamma, lam, segment=seg, boot=t["boot"])
    want = torch.tensor(_gae_scalar(HAND["r"], HAND["v"], HAND["d"], HAND["boot"], gamma, lam, seg), dtype=F64)
    assert torch.allclose(adv, want, atol=1e-14, rtol=0)
    assert torch.allclose(ret, want + t["v"][:5], atol=1e-14, rtol=0)
    # by hand: the truncated step's delta holds gamma * boot and nothing of the post-reset value; the recursion is cut
    assert float(adv[1, 0]) == pytest.approx(0.5 + 0.9 * 1.7 - 1.5, abs=1e-14)
    assert float(adv[3, 1]) == pytest.approx(1.0 - (-0.3), abs=1e-14)
    no_boot, _ = oracle.gae(t["r"], t["v"], t["d"], gamma, lam, segment=seg)
    diff = (adv - no_boot).abs() > 1e-12
    # only env 0 moves, at the truncated step and the steps before it that the recursion still reaches
    assert not bool(diff[:, 1].any()) and bool(diff[1, 0]) and not bool(diff[2:, 0].any())
    # (seg 2: the segment that would end by length at t=1 ends by the done, so step 0 still reaches step 1)
    assert float(adv[0, 0] - no_boot[0, 0]) == pytest.approx(gamma * lam * 0.9 * 1.7, abs=1e-14)


def test_gae_boot_of_the_uncut_value_gives_the_uncut_advantages():
    """lam = 0: adv_t = delta_t, so a trajectory cut at step k and bootstrapped with the uncut run's V_{k+1} has the
    uncut run's advantages up to k, whatever value the post-reset state has"""
    g = torch.Generator().manual_seed(5)
    T, E, k, gamma = 9, 4, 5, 0.97
    r, v = torch.randn(T, E, generator=g, dtype=F64), torch.randn(T + 1, E, generator=g, dtype=F64)
    uncut, _ = oracle.gae(r, v, torch.zeros(T, E, dtype=F64), gamma, 0.0)
    d, boot, v_cut = torch.zeros(T, E, dtype=F64), torch.zeros(T, E, dtype=F64), v.clone()
    d[k], boot[k] = 1.0, v[k + 1]
    v_cut[k + 1] = torch.randn(E, generator=g, dtype=F64)               # V of the reset state
    cut, _ = oracle.gae(r, v_cut, d, gamma, 0.0, boot=boot)
    assert torch.allclose(cut[:k + 1], uncut[:k + 1], atol=1e-14, rtol=0)
    zeroed, _ = oracle.gae(r, v_cut, d, gamma, 0.0)
    assert float((zeroed[k] - uncut[k]).abs().min()) > 1e-3             # without boot the cut step is biased


@pytest.mark.parametrize("dtype", [torch.float32, F64])
@pytest.mark.parametrize("seg", [0, 3])
def test_gae_without_boot_is_unchanged(seg, dtype):
    g = torch.Generator().manual_seed(11)
    T, E = 17, 6
    r, v = torch.randn(T, E, generator=g).to(dtype), torch.randn(T + 1, E, generator=g).to(dtype)
    d = (torch.rand(T, E, generator=g) < 0.2).to(dtype)
    none = oracle.gae(r, v, d, 0.99, 0.95, segment=seg)
    zero = oracle.gae(r, v, d, 0.99, 0.95, segment=seg, boot=torch.zeros_like(r))
    explicit = oracle.gae(r, v, d, 0.99, 0.95, segment=seg, boot=None)
    for a, b, c in zip(none, zero, explicit):
        assert torch.equal(a, b) and torch.equal(a, c)
    if seg == 0:
        for a, b in zip(none, _gae_before(r, v, d, 0.99, 0.95)):
            assert torch.equal(a, b)


# ---- VecEnv.step: truncated / final_obs ----------------------------------------------------------------------------
def _env(name, E, limit, seed=1):
    env = make_vec_env(get_spec(name), E, seed=seed, device="cpu", max_episode_length=limit)
    env.reset()
    return env


def test_step_reports_nothing_unless_told():
    env = _env(PEND, 5, 3)
    _, _, _, info = env.step(torch.zeros(5, 1))
    assert "truncated" not in info and "final_obs" not in info


def test_pendulum_every_end_is_truncated_and_final_obs_is_the_stepped_state():
    E, limit = 7, 3
    env, plain = _env(PEND, E, limit), _env(PEND, E, limit)
    env.report_final = True
    g = torch.Generator().manual_seed(0)
    ends = 0
    for t in range(7):
        a = torch.randn(E, 1, generator=g)
        new_state, _, _ = env._dynamics(a, env.t & 0xFFFFFFFF)         # a pure function of the state
        want = torch.stack([torch.cos(new_state[:, 0]), torch.sin(new_state[:, 0]), new_state[:, 1]], 1)
        obs, r, done, info = env.step(a)
        obs_p, r_p, done_p, info_p = plain.step(a)
        # the flag changes nothing else
        assert torch.equal(obs, obs_p) and torch.equal(r, r_p) and torch.equal(done, done_p)
        assert torch.equal(env.state, plain.state) and torch.equal(env.ep_ret, plain.ep_ret)
        assert torch.equal(info["finished_ret"], info_p["finished_ret"])
        assert info["truncated"].dtype == torch.bool and torch.equal(info["truncated"], done)
        assert torch.equal(info["final_obs"], want)
        if bool(done.any()):
            ends += int(done.sum())
            assert bool(((info["final_obs"] - obs).abs().sum(1)[done] > 1e-3).all())   # not the reset's observation
            assert torch.equal(info["final_obs"][~done], obs[~done])
    assert ends == 2 * E


def test_cartpole_terminal_wins_over_the_limit():
    limit = 4
    env = _env(CARTPOLE, 3, limit)
    env.report_final = True
    # row 0: the pole crosses 12 degrees (0.2094 rad) on the very step its episode reaches the limit; row 1 only
    # reaches the limit; row 2 does neither
    env.state = torch.tensor([[0.0, 0.0, 0.2090, 1.0], [0.1, 0.0, 0.01, 0.0], [0.0, 0.0, 0.0, 0.0]])
    env.ep_len = torch.tensor([limit - 1, limit - 1, 0], dtype=torch.int32)
    new_state, _, terminal = env._dynamics(torch.zeros(3, 1), env.t)
    assert terminal.tolist() == [True, False, False] and float(new_state[0, 2]) > 12.0 * math.pi / 180.0
    obs, _, done, info = env.step(torch.zeros(3, 1))
    assert done.tolist() == [True, True, False]
    assert info["truncated"].tolist() == [False, True, False]
    assert torch.equal(info["final_obs"], new_state)
    assert not torch.equal(obs[1], new_state[1]) and torch.equal(obs[2], new_state[2])


def test_synthetic_keyed_end_on_the_limit_step_is_not_truncated():
    E, T, limit = 45, 24, 7
    env = _env(SYN, E, limit, seed=SYN_SEED)
    env.report_final = True
    start = placement(env, limit, 0, 0)
    start["ep_len"][20] = 1                                               # 1 + 6 steps: the limit falls on step 5,
    # where env 20 also draws its keyed termination (the draws do not depend on the episode length)
    env.load_state_dict(copy_start(start))
    trunc, dones = torch.zeros(T, E, dtype=torch.bool), torch.zeros(T, E, dtype=torch.bool)
    for t in range(T):
        _, _, dones[t], info = env.step(torch.zeros(E, env.A))
        trunc[t] = info["truncated"]
    pure = (start["ep_len"].to(torch.int64)[None, :] + torch.arange(T)[:, None] + 1) % limit == 0
    assert bool(pure[5, 20]) and bool(dones[5, 20]) and not bool(trunc[5, 20])
    keyed = sorted((int(t), int(e)) for t, e in (dones & ~trunc).nonzero().tolist())
    assert keyed == [(5, 20), (7, 5), (9, 27), (10, 40), (17, 9), (23, 19)]
    assert int(trunc.sum()) > 100 and not bool((trunc & ~dones).any())


# ---- the fp64 reference of a rollout with the flag (shared with the GPU tests) ----------------------------------------
def value64(model, x):
    """V of rows x [..., O] under a float64 copy of ``model``'s weights"""
    m64 = ActorCritic(model.num_inputs, model.num_outputs, model.hidden, model.value_mult)
    with torch.no_grad():
        m64.flat.data.copy_(model.flat.detach().to("cpu"))
    m64 = m64.double()
    with torch.no_grad():
        _, _, v = m64(x.detach().to("cpu", F64).reshape(-1, model.num_inputs))
    return v.reshape(x.shape[:-1])


def replay_final(env, start, actions, limit):
    """(trunc [T, E] bool, final [T, E, O] f64): the replay chained one step at a time, each step once more under a
    limit no env reaches: that run's next observation is the state the env reached, without the limit's reset (its
    keyed ends reset as ever: those rows are never truncated)"""
    actions = actions.detach().to("cpu", F64)
    T, E = actions.shape[0], actions.shape[1]
    whole = replay(env, start["state"], start["ep_len"], start["ep_ret"], start["t"], actions, limit)
    state, ep_len, ep_ret = start["state"], start["ep_len"], start["ep_ret"]
    trunc = torch.zeros(T, E, dtype=torch.bool)
    final = torch.zeros(T, E, env.O, dtype=F64)
    for t in range(T):
        one = replay(env, state, ep_len, ep_ret, int(start["t"]) + t, actions[t:t + 1], limit)
        free = replay(env, state, ep_len, ep_ret, int(start["t"]) + t, actions[t:t + 1], NO_LIMIT)
        assert torch.equal(free["dones"][0], one["terminals"][0])
        trunc[t] = one["dones"][0] & ~one["terminals"][0]
        final[t] = free["obs"][1]
        state, ep_len, ep_ret = one["state"], one["ep_len"], one["ep_ret"]
    assert torch.equal(state, whole["state"])                             # the chain is the replay
    assert torch.equal(trunc, whole["dones"] & ~whole["terminals"])
    return trunc, final


def expected_boot(env, model, stats, params, key_action, start, actions):
    """``expected`` plus what bootstrap_time_limit adds: trunc, x_fin [K, E, O] (zero where never written), v_fin,
    boot, and adv / ret from the fp64 value forward of the fp64 rows"""
    T, E, _ = actions.shape
    limit = env.limit
    exp = expected(env, model, stats, params, key_action, start, actions)
    trunc, final = replay_final(env, start, actions, limit)
    K = -(-T // limit)
    x_fin = torch.zeros(K, E, env.O, dtype=F64)
    written = torch.zeros(K, E, dtype=torch.bool)
    rows = _normalize64(final, stats)
    for t, e in trunc.nonzero().tolist():
        assert not bool(written[t // limit, e])                           # a slot is written once
        written[t // limit, e] = True
        x_fin[t // limit, e] = rows[t, e]
    slot = torch.arange(T) // limit
    v_fin = value64(model, x_fin)
    values = value64(model, exp["rows"])
    boot = trunc.to(F64) * v_fin[slot]
    adv, ret = oracle.gae(exp["rewards_clipped"], values, exp["dones"].to(F64), params.gamma, params.gae_param,
                          segment=params.gae_segment(), boot=boot)
    adv0, _ = oracle.gae(exp["rewards_clipped"], values, exp["dones"].to(F64), params.gamma, params.gae_param,
                         segment=params.gae_segment())
    exp.update(trunc=trunc, final=final, x_fin=x_fin, written=written, v_fin=v_fin, values=values, boot=boot,
               adv=adv, ret=ret, adv_no_boot=adv0, fin_K=K)
    return exp


def assert_truncation_preconditions(exp, kind_synthetic):
    """on the replay alone: the cases the comparison is there for are present"""
    trunc = exp["trunc"]
    T = trunc.shape[0]
    assert bool(trunc[0].any()), "no truncation at step 0"
    assert bool(trunc[T - 1].any()), "no truncation at the last step"
    assert bool((trunc.sum(0) >= 3).any()), "no env with three truncations"
    if kind_synthetic:
        assert bool((exp["terminals"] & ~trunc).any()), "no keyed terminal"
        assert bool((exp["dones"] & ~trunc).any())
    else:
        assert torch.equal(trunc, exp["dones"])
    # the bootstrap matters: the advantages move by far more than any tolerance below
    assert float((exp["adv"] - exp["adv_no_boot"]).abs().max()) > 1e-2


def compare_boot(got, exp, lowp=False):
    """``got``: trunc [T, E], x_fin [K, E, >= O] decoded, and (fp32-accurate dtypes) v_fin [K, E], adv / ret [T, E]"""
    T, E = exp["trunc"].shape
    K, O = exp["fin_K"], exp["x_fin"].shape[-1]
    cpu = lambda v: v.detach().to("cpu")   # noqa: E731
    trunc = cpu(got["trunc"]).view(T, E)
    assert bool(((trunc == 0) | (trunc == 1)).all()) and torch.equal(trunc > 0.5, exp["trunc"]), "trunc"
    x = cpu(got["x_fin"]).view(K, E, -1).to(F64)
    w = exp["written"]
    assert bool((x[~w] == 0).all()), "x_fin rows never written must stay zero"
    if x.shape[-1] > O:
        assert bool((x[w][:, O] == 1.0).all()) and bool((x[w][:, O + 1:] == 0.0).all()), "bias column / padding"
    if lowp:
        g = (x[w][:, :O] - exp["x_fin"][w]).abs()
        print(f"  x_fin: max gap {float(g.max()):.3e}")
        bad = g > 2.0 ** -8 * exp["x_fin"][w].abs() + 1e-6
        assert not bool(bad.any()), f"x_fin: {int(bad.sum())} of {bad.numel()} beyond one bf16 rounding"
    else:
        _allclose("x_fin", x[w][:, :O], exp["x_fin"][w], 2e-4, 1e-4)
    if "v_fin" in got:
        _allclose("v_fin", cpu(got["v_fin"]).view(K, E), exp["v_fin"], 2e-5, 2e-5)
        _allclose("adv", cpu(got["adv"]).view(T, E), exp["adv"], 2e-5, 2e-5)
        _allclose("ret", cpu(got["ret"]).view(T, E), exp["ret"], 2e-5, 2e-5)


def _cpu_engine_boot(env_name, E, T, limit, seed):
    """tests/test_rollout_replay.py _cpu_engine with the flag on"""
    from pytorch_dppo_amd.runtime.engine_torch import TorchEngine
    p, eng0, model, env, stats = _cpu_engine(env_name, E, T, limit, seed)
    pb = Params.from_dict({**p.to_dict(), "bootstrap_time_limit": True})
    env_b = make_vec_env(get_spec(env_name), E, seed=seed, device="cpu", max_episode_length=limit)
    eng = TorchEngine(pb, model, env_b, stats, torch.device("cpu"), 0)
    return pb, eng, eng0, model, env_b, stats


@pytest.mark.parametrize("env_name", [SYN, PEND])
def test_torch_engine_bootstrap_matches_replay(env_name):
    E, T, limit = 45, 24, 7
    seed = SYN_SEED if env_name == SYN else 1
    p, eng, eng0, model, env, stats = _cpu_engine_boot(env_name, E, T, limit, seed)
    assert eng.fin_K == 4 and eng.x_fin.shape == (4, E, env.O)
    start = placement(env, limit, 0, 0)
    eng.load_env_state(copy_start(start))
    eng0.load_env_state(copy_start(start))
    ro, ro0 = eng.rollout(), eng0.rollout()
    # the rollout itself does not move with the flag: buffers, env, episode statistics
    for name in ("x", "actions", "logp", "rewards", "dones"):
        assert torch.equal(getattr(eng, name), getattr(eng0, name)), name
    assert torch.equal(eng.env.state, eng0.env.state) and torch.equal(eng.env.ep_ret, eng0.env.ep_ret)
    assert ro["ep_return_sum"] == ro0["ep_return_sum"] and ro["ep_count"] == ro0["ep_count"]
    assert torch.equal(ro["s1"], ro0["s1"]) and torch.equal(ro["s2"], ro0["s2"]) and ro["count"] == ro0["count"]
    eng.values()
    eng.gae()
    exp = expected_boot(env, model, stats, p, eng.key_action, start, eng.actions)
    assert_truncation_preconditions(exp, env_name == SYN)
    compare_boot({"trunc": eng.trunc, "x_fin": eng.x_fin, "v_fin": eng.v_fin, "adv": eng.adv, "ret": eng.ret}, exp)
    eng0.values()
    eng0.gae()
    assert float((eng.adv - eng0.adv).abs().max()) > 1e-2                 # and the flag does move the advantages


# ---- refusals, and nothing changes with the flag off -------------------------------------------------------------------
@pytest.mark.parametrize("other,named", [(dict(obs_norm_update="step"), "obs_norm_update"), (dict(compat=True), "compat"),
                                         (dict(env_backend="gym"), "env_backend")])
def test_refused_combinations_name_both_options(other, named):
    with pytest.raises(ValueError) as ei:
        Params(bootstrap_time_limit=True, **other)
    assert "bootstrap_time_limit" in str(ei.value) and named in str(ei.value)
    Params(**other)                                                       # each is fine on its own
    with pytest.raises(ValueError):
        params_from_args(["--bootstrap-time-limit", "true"] + [f"--{k.replace('_', '-')}={v}" for k, v in other.items()])


def test_flag_defaults_off_everywhere():
    assert Params().bootstrap_time_limit is False
    assert dppo_preset().bootstrap_time_limit is False and ppo_preset().bootstrap_time_limit is False
    assert all(f().bootstrap_time_limit is False for f in PRESETS.values())
    assert params_from_args([]).bootstrap_time_limit is False
    assert params_from_args(["--bootstrap-time-limit", "true"]).bootstrap_time_limit is True
    assert params_from_args(["--bootstrap-time-limit", "false"]).bootstrap_time_limit is False
    on, off = params_from_args(["--bootstrap-time-limit", "true"]).to_dict(), params_from_args([]).to_dict()
    assert {k for k in on if on[k] != off[k]} == {"bootstrap_time_limit"}
    assert Params.from_dict(on).bootstrap_time_limit is True
    # a TorchEngine without the flag carries none of the feature's buffers
    _, eng, _, _, _ = _cpu_engine(PEND, 5, 4, 3)
    assert not eng.boot and not hasattr(eng, "x_fin") and eng.env.report_final is False
