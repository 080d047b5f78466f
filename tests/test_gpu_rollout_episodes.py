"""The fused rollout kernel's env kinds 0 (synthetic) and 1 (pendulum) against the fp64 action replay of
tests/test_rollout_replay.py: episode ends by the keyed draw and by the step limit, the in-place reset, the episode
trackers carried in and out of a launch, the reward clip, the step counter crossing 2^32, the per-step observation
filter (cooperative launch and per-step fallback), the 4- and 8-wave forms, every storage precision, and the
geometries of ``env_transition``'s two-items-per-turn loop (S = 1, A > O, more dim pairs than threads).

Every case places the env through ``load_env_state`` (episode lengths drawn in [0, limit) so that limit ends fall
on different steps in different rows of a tile, non-zero returns so far), runs ``rollout()`` (the fused kernel),
replays the recorded actions in float64 and compares everything the launch left behind (``compare``).  The done
flags are compared exactly at every precision: for these kinds they do not depend on the state.  Preconditions
(off-schedule ends present, clipped share, placed states doing what they were placed for) are asserted on the
oracle alone before the kernel's output is compared."""
import pytest
import torch

from test_gpu_tensor_env import _engine, _params
from test_rollout_replay import (CLIP_FOR, assert_pendulum_placement, compare, copy_start, expected,
                                 pendulum_placed_states, placement, replay)

pytestmark = pytest.mark.gpu

SYN, PEND = "Synthetic-17x6", "Pendulum-v0"
# seed 30: the synthetic env's keyed terminations fall on (step, env) = (5, 20), (7, 5), (9, 27), (10, 40),
# (17, 9), (23, 19) of the 45 x 24 window (tests/test_rollout_replay.py asserts the list); only 8 of the seeds
# 1-40 give three or more there
SYN_SEED = 30
FP8_MEAN_MAX = 0.09      # 2 x 4.45e-2, the largest fp8 gap measured against the fp64 forward (case a's docstring)


def _view(eng, env, ro):
    """what the launch left behind, as [T, E] tensors"""
    T, E = eng.T, eng.E
    torch.cuda.synchronize()
    got = {"actions": eng.actions.view(T, E, -1).clone(), "logp": eng.logp.view(T, E).clone(),
           "rewards": eng.rewards.view(T, E).clone(), "dones": eng.dones.view(T, E).clone(),
           "x": eng.decode(eng.x_buf).view(T + 1, E, -1), "state": env.state.clone(), "ep_len": env.ep_len.clone(),
           "ep_ret": env.ep_ret.clone(), "t": env.t, "ep_count": float(ro["ep_count"]),
           "ep_return_sum": float(ro["ep_return_sum"]), "count": float(ro["count"]), "s1": ro["s1"].clone(),
           "s2": ro["s2"].clone()}
    if eng.p.obs_norm_update == "step":
        got["stats_n"], got["stats_mean"] = eng.local_stats.n, eng.local_stats.mean.clone()
    return got


def _keyed_ends_present(start, dry, limit=7):
    """at least 4 episode ends by the keyed draw off the pure limit schedule (ep_len0 + t + 1) % limit == 0"""
    T = dry["dones"].shape[0]
    steps = torch.arange(T, dtype=torch.int64)[:, None]
    pure = (start["ep_len"].to(torch.int64)[None, :] + steps + 1) % limit == 0
    assert int((dry["terminals"] & ~pure).sum()) >= 4


def _run(env_name, dtype, E, T, limit, seed=1, t0=0, gen_seed=0, launches=1, state=None, last_step_row=None,
         log_std=-0.3, fallback=False, check_start=None, check_exp=None, fp8_max=None, **kw):
    p = _params(env_name, dtype, E=E, T=T, max_episode_length=limit, seed=seed, **kw)
    eng, model, env, stats = _engine(p, log_std=log_std)
    assert not eng.stepped_env                                  # rollout() is the fused kernel
    step_mode = p.obs_norm_update == "step"
    if step_mode:
        assert eng._stepnorm_fits()
        if fallback:
            eng._sn_cap = 0                                     # the existing hook: per step one observe + one launch
            assert not eng._stepnorm_fits()
    start = placement(env, limit, gen_seed, t0, state)
    if last_step_row is not None:
        start["ep_len"][last_step_row] = limit - 1
    assert bool((start["ep_ret"] != 0).all()) and int(start["ep_len"].max()) < limit
    # the done flags do not depend on the actions: what the schedule must hold is known before the launch
    dry = replay(env, start["state"], start["ep_len"], start["ep_ret"], t0, torch.zeros(T, E, env.A), limit)
    assert int(dry["dones"].sum()) > 0
    if check_start is not None:
        check_start(start, dry)
    eng.load_env_state(copy_start(start))
    gaps = []
    for launch in range(launches):
        ro = eng.rollout()
        if step_mode:
            eng.raise_if_failed(sync=True)
        torch.cuda.synchronize()
        # the recorded actions are the oracle's only input from the kernel; its preconditions come first
        actions = eng.actions.view(T, E, -1).clone()
        exp = expected(env, model, stats, p, eng.key_action, start, actions)
        if launch == 0:
            assert torch.equal(exp["dones"], dry["dones"])
        if check_exp is not None:
            check_exp(start, exp, actions)
        print(f"{env_name} {dtype} launch {launch}: {int(exp['dones'].sum())} episode ends")
        got = _view(eng, env, ro)
        assert torch.equal(got["actions"], actions)
        gaps.append({})
        compare(got, exp, model, dtype, stats=gaps[-1], fp8_max=fp8_max)
        # the next launch starts from what this one wrote
        start = {"state": got["state"].cpu(), "ep_len": got["ep_len"].cpu(), "ep_ret": got["ep_ret"].cpu(),
                 "t": got["t"]}
    assert env.t == t0 + launches * T
    return gaps


# ---- a. every dtype, both kinds -----------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["fp32", "bf16x3", "bf16", "fp8"])
@pytest.mark.parametrize("env_name", [SYN, PEND])
def test_rollout_episode_ends_match_replay(env_name, dtype):
    """45 envs = two full 16-env tiles + 13 rows, 24 steps, limit 7.

    Measured on an MI355X, largest gap to the replay (synthetic / pendulum), the env side at every dtype within:
    rewards 1.5e-7 / 5.4e-7, final state 6.5e-8 / 9.8e-7, ep_ret 4.2e-7 / 7.6e-6, ep_return_sum 4.5e-5 / 2.0e-4
    over ~155 episodes, s1 3.8e-6 / 3.7e-5, s2 3.1e-6 / 2.7e-4 (of max|s2| ~ 1e3), logp 1.8e-6 / 9.0e-7.  Rows:
    fp32 1.1e-6 / 2.1e-6, bf16x3 2.8e-5 / 3.1e-5, bf16 and fp8 1.5e-2 / 1.6e-2 at |x| up to 5 (inside one bf16
    rounding everywhere).  Mean against the fp64 forward of the stored rows: fp32 3.3e-7 / 3.1e-7, bf16x3
    3.9e-6 / 4.5e-6, bf16 max 2.2e-3 / 1.6e-3 and mean 4.5e-4 / 4.4e-4, fp8 max 4.45e-2 / 3.04e-2 and mean
    8.0e-3 / 7.4e-3.  The fp8 mean's largest gap has no bound of the project's: FP8_MEAN_MAX is twice the larger
    measured value."""
    _run(env_name, dtype, E=45, T=24, limit=7, seed=SYN_SEED if env_name == SYN else 1, t0=0,
         check_start=_keyed_ends_present if env_name == SYN else None, fp8_max=FP8_MEAN_MAX)


# ---- b. the episode trackers carried from one launch into the next ----------------------------------------
def test_rollout_carries_episodes_across_launches():
    _run(SYN, "bf16x3", E=45, T=24, limit=7, seed=SYN_SEED, t0=0, launches=2, check_start=_keyed_ends_present)


# ---- c. the reward clip: `rewards` clipped, the episode return not ---------------------------------------------
@pytest.mark.parametrize("env_name,clip", [(SYN, 0.5), (PEND, 2.0)])
def test_rollout_reward_clip_leaves_episode_returns_unclipped(env_name, clip):
    from pytorch_dppo_amd.envs import get_spec
    assert clip == CLIP_FOR[get_spec(env_name).kind]

    def check_exp(start, exp, actions):
        share = float((exp["rewards"].abs() > clip).double().mean())
        print("clipped share", share)
        assert 0.1 <= share <= 0.9
        assert exp["ep_count"] > 0

    _run(env_name, "fp32", E=45, T=24, limit=7, seed=SYN_SEED if env_name == SYN else 1, reward_clip=clip,
         check_exp=check_exp)


# ---- d. the step counter crossing 2^32 ------------------------------------------------------------------------
@pytest.mark.parametrize("env_name", [SYN, PEND])
def test_rollout_step_counter_wraps(env_name):
    _run(env_name, "bf16x3", E=45, T=8, limit=5, t0=2 ** 32 - 5)


# ---- e. placed pendulum states ---------------------------------------------------------------------------------
def test_rollout_pendulum_placed_states():
    """angles at and beyond +-pi and several turns out (the reward's wrap and its negative branch), speeds at the
    +-8 clamp from both sides, sigma ~ 2 so that torques pass the +-2 clamp, and one row one step from its limit:
    its step-1 observation is (cos, sin, thdot) of the keyed reset"""
    E = 13
    _run(PEND, "fp32", E=E, T=2, limit=50, state=pendulum_placed_states(E), last_step_row=12, log_std=0.7,
         check_exp=assert_pendulum_placement)


# ---- f. the per-step observation filter ------------------------------------------------------------------------
@pytest.mark.parametrize("fallback", [False, True])
@pytest.mark.parametrize("env_name", [SYN, PEND])
def test_rollout_step_obs_norm_episode_ends_match_replay(env_name, fallback):
    """once as the cooperative launch, once through the per-step fallback (one observe + a one-step launch per
    step: the trackers go through global memory between all 12 steps)"""
    _run(env_name, "fp32", E=45, T=12, limit=5, obs_norm_update="step", fallback=fallback)


# ---- g. launch forms and edge geometries -----------------------------------------------------------------------
@pytest.mark.parametrize("waves", [8, 4])
def test_rollout_humanoid_wave_forms(waves):
    """188 dim pairs per row against 512 / 256 threads: a thread's second item lies one to three rows on"""
    from pytorch_dppo_amd.ops import native
    ext = native.load()
    ext.set_rollout_waves(waves)
    try:
        _run("Humanoid-v2", "bf16x3", E=19, T=6, limit=3)
        torch.cuda.synchronize()
    finally:
        ext.set_rollout_waves(8)


@pytest.mark.parametrize("dtype", ["fp32", "bf16x3"])
@pytest.mark.parametrize("env_name", ["Synthetic-5x8", "Synthetic-1x1"])
def test_rollout_edge_geometries(env_name, dtype):
    """A > O (the reward's mean runs over min(A, O) dims, dim d is driven by action d mod A) and S = 1 (one
    item per row, no second dim anywhere)"""
    _run(env_name, dtype, E=19, T=8, limit=3)


def test_rollout_more_dim_pairs_than_threads():
    """O = 600 at fp32: 256 threads against 300 dim pairs, so a thread's second item lies in the same row"""
    _run("Synthetic-600x3", "fp32", E=19, T=6, limit=3)
