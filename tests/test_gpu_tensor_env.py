"""Device-stepped tensor envs on the GPU engine: the episode-bookkeeping kernel (csrc/envstep.hip,
``env_advance``) against the torch expression of ``VecEnv.step``, ``HipEngine.rollout_stepped`` against
the torch engine and against the fused rollout kernel, the continuous cart-pole through rollout,
evaluation, resume and ``train.py``, and that none of it synchronises with the host.

Geometry of the rollout comparisons: 37 envs = two full 16-env tiles + a 5-env tail, 5 steps,
``max_episode_length`` 3, so every env resets once inside the rollout (tests/test_tensor_env.py checks
the cart-pole and the registry themselves on the CPU)."""
import json
import math
import os
import subprocess
import sys

import pytest
import torch

from pytorch_dppo_amd.config import Params, dppo_preset
from pytorch_dppo_amd.envs import get_spec, make_vec_env
from pytorch_dppo_amd.models.actor_critic import ActorCritic
from pytorch_dppo_amd.parallel.dist import DistContext
from pytorch_dppo_amd.runtime.evaluator import EVAL_ENV_SEED_OFFSET, evaluate_batch
from pytorch_dppo_amd.utils.obs_stats import RunningObsStats

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0) if torch.cuda.is_available() else None
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CARTPOLE = "CartPoleContinuous-v1"
X_LIMIT, TH_LIMIT = 2.4, 12.0 * 2.0 * math.pi / 360.0
CANARY = -7.0


def _ext():
    from pytorch_dppo_amd.ops import native
    return native.load()


# ---- env_advance against the torch expression of VecEnv.step ---------------------------------------------
def _torch_advance(reward, terminal, new_state, reset_state, ep_len, ep_ret, limit, clip):
    """VecEnv.step's bookkeeping (envs/vec_env.py) + the engines' reward clip, on the same device"""
    ep_len = ep_len + 1
    ep_ret = ep_ret + reward
    done = terminal | (ep_len >= limit)
    finished_ret = torch.where(done, ep_ret, torch.zeros_like(ep_ret))
    state = torch.where(done[:, None], reset_state, new_state)
    ep_len = torch.where(done, torch.zeros_like(ep_len), ep_len)
    ep_ret = torch.where(done, torch.zeros_like(ep_ret), ep_ret)
    r = reward.clamp(-clip, clip) if clip > 0 else reward
    return state, ep_len, ep_ret, r, done.to(torch.float32), finished_ret, done


class _Bufs:
    """the kernel's in/out and output tensors as views of buffers one 16-env tile longer, the rest
    holding a canary"""

    def __init__(self, E, S):
        self.E, self.S, self.ntile = E, S, (E + 15) // 16
        f = lambda *shape: torch.full(shape, CANARY, dtype=torch.float32, device=DEV)   # noqa: E731
        self.raw = {"state": f(E + 16, S), "ep_ret": f(E + 16), "rewards_row": f(E + 16), "dones_row": f(E + 16),
                    "epstat": f(self.ntile + 1, 2),
                    "ep_len": torch.full((E + 16,), int(CANARY), dtype=torch.int32, device=DEV)}
        self.state, self.ep_ret, self.ep_len = self.raw["state"][:E], self.raw["ep_ret"][:E], self.raw["ep_len"][:E]
        self.rewards_row, self.dones_row = self.raw["rewards_row"][:E], self.raw["dones_row"][:E]
        self.epstat = self.raw["epstat"][:self.ntile]

    def canaries_intact(self):
        n = {"epstat": self.ntile}
        return all(bool((v[n.get(k, self.E):] == (int(CANARY) if k == "ep_len" else CANARY)).all())
                   for k, v in self.raw.items())

    def outputs(self):
        return [self.state, self.ep_len, self.ep_ret, self.rewards_row, self.dones_row, self.epstat]


def _reduce_epstat(ext, epstat):
    """the engine's obs_reduce call on an epstat buffer -> (return sum, count) fp64 on the host"""
    ntile = epstat.shape[0]
    mom = torch.zeros(ntile, 2, 1, dtype=torch.float32, device=DEV)
    s12 = torch.zeros(2, 1, dtype=torch.float64, device=DEV)
    ep = torch.zeros(2, dtype=torch.float64, device=DEV)
    ext.obs_reduce(mom, ntile, 1, s12, epstat.contiguous(), ep)
    return ep.tolist()


@pytest.mark.parametrize("clip", [0.0, 1.0])
@pytest.mark.parametrize("E", [1, 13, 37, 257])
def test_env_advance_matches_vec_env_step(E, clip):
    ext = _ext()
    limit = 3
    for S in (1, 2, 4, 17):
        g = torch.Generator(device="cpu").manual_seed(1000 * E + S)
        rnd = lambda *shape: torch.rand(*shape, generator=g)   # noqa: E731
        # rewards in +-3 (beyond the clip), returns so far in [5, 10]: every finished return is
        # positive, so the fixed-order fp32 tile sums (<= 15 roundings of 2^-24 each) stay within the
        # rtol of 1e-6 the reduced sum is held to
        steps = []
        # (the second step's rewards are in [1.5, 3]: the envs the first step reset finish positive too)
        for lo, hi in ((-3.0, 3.0), (1.5, 3.0)):
            steps.append(dict(reward=(lo + (hi - lo) * rnd(E)).to(DEV), terminal=(rnd(E) < 0.3).to(DEV),
                              new_state=torch.randn(E, S, generator=g).to(DEV),
                              reset_state=torch.randn(E, S, generator=g).to(DEV)))
        ep_len0 = (torch.arange(E, dtype=torch.int32) % 4).to(DEV)          # 0..3: the limit fires on some
        ep_ret0 = (5.0 + 5.0 * rnd(E)).to(DEV)

        def launch(b, st, init):
            ext.env_advance(st["reward"], st["terminal"].to(torch.uint8), st["new_state"], st["reset_state"],
                            b.state, b.ep_len, b.ep_ret, b.rewards_row, b.dones_row, b.epstat, limit, clip, init)

        b = _Bufs(E, S)
        b.ep_len.copy_(ep_len0)
        b.ep_ret.copy_(ep_ret0)
        launch(b, steps[0], True)
        ref = _torch_advance(ep_len=ep_len0, ep_ret=ep_ret0, limit=limit, clip=clip, **steps[0])
        state, ep_len, ep_ret, rew, dones, fin, done = ref
        assert 0 < int(done.sum()) or E == 1
        assert bool(((ep_len0 + 1 >= limit) & ~steps[0]["terminal"]).any()) or E == 1     # the limit alone fired
        for got, want, name in zip(b.outputs()[:5], (state, ep_len, ep_ret, rew, dones),
                                   ("state", "ep_len", "ep_ret", "rewards_row", "dones_row")):
            assert got.dtype == want.dtype and torch.equal(got, want), (name, S)
        if clip > 0:
            assert float(b.rewards_row.abs().max()) <= clip and (E == 1 or float(steps[0]["reward"].abs().max()) > clip)
        s, c = _reduce_epstat(ext, b.epstat)
        assert c == float(done.sum())
        assert s == pytest.approx(float(fin.double().sum()), rel=1e-6, abs=0.0)
        assert b.canaries_intact(), S
        first = [t.clone() for t in b.outputs()]
        # an identical launch gives identical bits
        b2 = _Bufs(E, S)
        b2.ep_len.copy_(ep_len0)
        b2.ep_ret.copy_(ep_ret0)
        launch(b2, steps[0], True)
        for x, y in zip(first, b2.outputs()):
            assert torch.equal(x, y)
        # a bool terminal is taken as the uint8 one
        b3 = _Bufs(E, S)
        b3.ep_len.copy_(ep_len0)
        b3.ep_ret.copy_(ep_ret0)
        st = steps[0]
        ext.env_advance(st["reward"], st["terminal"], st["new_state"], st["reset_state"], b3.state, b3.ep_len,
                        b3.ep_ret, b3.rewards_row, b3.dones_row, b3.epstat, limit, clip, True)
        for x, y in zip(first, b3.outputs()):
            assert torch.equal(x, y)
        # a second, accumulating launch: epstat is the sum of both launches' tile stats, everything
        # else is the second step's
        launch(b, steps[1], False)
        alone = _Bufs(E, S)
        alone.ep_len.copy_(ep_len)
        alone.ep_ret.copy_(ep_ret)
        launch(alone, steps[1], True)
        assert torch.equal(b.epstat, first[5] + alone.epstat)
        ref2 = _torch_advance(ep_len=ep_len, ep_ret=ep_ret, limit=limit, clip=clip, **steps[1])
        for got, want in zip(b.outputs()[:5], ref2[:5]):
            assert torch.equal(got, want), S
        s2, c2 = _reduce_epstat(ext, b.epstat)
        assert c2 == float(done.sum() + ref2[6].sum())
        assert s2 == pytest.approx(float(fin.double().sum() + ref2[5].double().sum()), rel=1e-6, abs=0.0)
        assert b.canaries_intact() and alone.canaries_intact(), S


def test_env_advance_binding_validation():
    ext = _ext()
    E, S = 37, 4
    b = _Bufs(E, S)
    b.ep_len.zero_()
    b.ep_ret.zero_()
    before = [t.clone() for t in b.outputs()]
    ok = dict(reward=torch.ones(E, device=DEV), terminal=torch.zeros(E, dtype=torch.uint8, device=DEV),
              new_state=torch.zeros(E, S, device=DEV), reset_state=torch.ones(E, S, device=DEV), state=b.state,
              ep_len=b.ep_len, ep_ret=b.ep_ret, rewards_row=b.rewards_row, dones_row=b.dones_row, epstat=b.epstat)
    order = list(ok)

    def call(limit=3, **kw):
        a = {**ok, **kw}
        ext.env_advance(*[a[k] for k in order], limit, 1.0, True)

    bad = [dict(reward=torch.ones(E + 1, device=DEV)), dict(reward=torch.ones(E, device=DEV).double()),
           dict(reward=torch.ones(E)), dict(terminal=torch.zeros(E, dtype=torch.int32, device=DEV)),
           dict(terminal=torch.zeros(E - 1, dtype=torch.uint8, device=DEV)),
           dict(new_state=torch.zeros(E, S + 1, device=DEV)), dict(reset_state=torch.zeros(E - 1, S, device=DEV)),
           dict(new_state=torch.zeros(S, E, device=DEV).t()),                 # not contiguous
           dict(state=b.raw["state"][:E].reshape(-1)),                          # not [E][S]
           dict(ep_len=b.raw["ep_len"][:E].long()), dict(ep_len=b.raw["ep_len"][:E + 1]),
           dict(ep_ret=b.raw["ep_ret"][:E - 1]), dict(rewards_row=b.raw["rewards_row"][:E + 1]),
           dict(dones_row=b.raw["dones_row"][:E].double()), dict(epstat=b.raw["epstat"][:b.ntile - 1]),
           dict(epstat=b.raw["epstat"][:b.ntile + 1]), dict(limit=0), dict(limit=1 << 31)]
    for kw in bad:
        with pytest.raises(RuntimeError):
            call(**kw)
    torch.cuda.synchronize()
    # every refusal came before a launch
    for x, y in zip(before, b.outputs()):
        assert torch.equal(x, y)
    call()
    assert bool((b.ep_len == 1).all()) and bool((b.state == 0).all()) and b.canaries_intact()


# ---- rollout_stepped against the torch engine and the fused kernel ---------------------------------------
def _params(env_name, dtype, E=37, T=5, **kw):
    kw.setdefault("max_episode_length", 3)
    return dppo_preset(device="gpu", env_name=env_name, num_envs=E, exploration_size=E * T, batch_size=E * T,
                       dtype=dtype, **kw)


def _engine(params, seed=0, log_std=-0.3):
    """engine with stats seeded from the reset observations and a non-trivial log_std (as
    test_gpu_kernels.py test_rollout_matches_torch_engine)"""
    from pytorch_dppo_amd.runtime.engine_hip import HipEngine
    spec = get_spec(params.env_name)
    torch.manual_seed(seed)
    model = ActorCritic(spec.obs_dim, spec.act_dim, params.hidden).to(DEV)
    env = make_vec_env(spec, params.num_envs, seed=params.seed, device=DEV,
                       max_episode_length=params.max_episode_length)
    stats = RunningObsStats(spec.obs_dim, DEV)
    eng = HipEngine(params, model, env, stats, DEV, 0)
    stats.observes(env.observe())
    with torch.no_grad():
        model.flat.data[:model.num_outputs] = log_std
    eng.params_changed()
    return eng, model, env, stats


def _torch_engine(params, model, stats_from, record=None):
    """the oracle: TorchEngine on the same device with its own env and a copy of the stats;
    ``record``: a list that receives every pre-reset new state of its env"""
    from pytorch_dppo_amd.runtime.engine_torch import TorchEngine
    p_cpu = Params.from_dict({**params.to_dict(), "device": "cpu"})
    spec = get_spec(params.env_name)
    env = make_vec_env(spec, params.num_envs, seed=params.seed, device=DEV,
                       max_episode_length=params.max_episode_length)
    if record is not None:
        _record_new_states(env, record)
    stats = RunningObsStats(spec.obs_dim, DEV)
    stats.copy_from(stats_from)
    return TorchEngine(p_cpu, model, env, stats, DEV, 0)


def _record_new_states(env, out):
    dyn = env._dynamics

    def recording(a, k):
        res = dyn(a, k)
        out.append(res[0].clone())
        return res
    env._dynamics = recording


def _threshold_margin(states):
    s = torch.stack(states).double()
    return float(torch.minimum(((s[..., 0].abs() - X_LIMIT).abs()).min(), ((s[..., 2].abs() - TH_LIMIT).abs()).min()))


def _close(a, b, dtype, name, scale=1.0):
    """fp32 / bf16x3: test_rollout_matches_torch_engine's atol 2e-4, rtol 1e-4; bf16: max < 5e-2 and
    mean < 5e-3 (x ``scale``, for the quantities that are sums of such terms)"""
    a, b = a.float(), b.float()
    gap = (a - b).abs()
    print(f"{name}: max gap {float(gap.max()):.3e} mean {float(gap.mean()):.3e}")
    if dtype == "bf16":
        assert float(gap.max()) < 5e-2 * scale and float(gap.mean()) < 5e-3 * scale, name
    else:
        assert torch.allclose(a, b, atol=2e-4, rtol=1e-4), name


def _compare_rollouts(eng, env, ro_h, ref, ro_t, dtype, ref_is_torch=True):
    """the stepped rollout of ``eng`` against a reference engine's (TorchEngine, or a HipEngine that ran
    the fused kernel)"""
    T, E, O, N = eng.T, eng.E, eng.O, eng.T * eng.E
    torch.cuda.synchronize()
    if ref_is_torch:
        r_act, r_logp, r_rew, r_done, r_x = ref.actions, ref.logp, ref.rewards, ref.dones, ref.x
    else:
        r_act, r_logp, r_rew = ref.actions.view(T, E, -1), ref.logp.view(T, E), ref.rewards.view(T, E)
        r_done, r_x = ref.dones.view(T, E), ref.decode(ref.x_buf).view(T + 1, E, -1)[..., :O]
    assert torch.equal(eng.dones.view(T, E), r_done)
    assert torch.allclose(eng.logp.view(T, E), r_logp, atol=1e-4, rtol=1e-5)
    _close(eng.actions.view(T, E, -1), r_act, dtype, "actions")
    xk = eng.decode(eng.x_buf).view(T + 1, E, -1)
    _close(xk[..., :O], r_x, dtype, "x (with the bootstrap rows)")
    assert bool((xk[..., O] == 1.0).all()) and bool((xk[..., O + 1:] == 0.0).all())   # bias column, padding
    # the env after the rollout: the live tensors of the env the engine was given
    assert torch.equal(env.ep_len, ref.env.ep_len) and env.t == ref.env.t == T
    _close(env.state, ref.env.state, dtype, "env.state")
    # per-step rewards: a bf16 action error of d moves the reward by at most 2 |a_c - tanh s| d <= 4 d
    # (synthetic) / the clip (pendulum): 4x the action bound; ep_ret sums up to `limit` = 3 of them
    _close(eng.rewards.view(T, E), r_rew, dtype, "rewards", scale=4.0)
    _close(env.ep_ret, ref.env.ep_ret, dtype, "ep_ret", scale=12.0)
    assert abs(float(ro_h["ep_count"]) - float(ro_t["ep_count"])) < 0.5
    assert float(ro_h["ep_count"]) == float(eng.dones.sum()) > 0
    if dtype == "bf16":
        # observations within d = 5e-2 of the reference's: |ds1| <= N d, |ds2| <= 2 d sqrt(N s2) + N d^2
        d = 5e-2
        assert bool(((ro_h["s1"] - ro_t["s1"]).abs() <= N * d).all())
        assert bool(((ro_h["s2"] - ro_t["s2"]).abs() <= 2 * d * (N * ro_t["s2"]).sqrt() + N * d * d).all())
    else:
        assert torch.allclose(ro_h["s1"], ro_t["s1"], rtol=1e-4, atol=1e-2)
        s2_scale = float(ro_t["s2"].abs().max()) + 1.0
        assert torch.allclose(ro_h["s2"], ro_t["s2"], rtol=1e-4, atol=1e-4 * s2_scale)
    assert float(ro_h["count"]) == float(ro_t["count"]) == N


@pytest.mark.parametrize("dtype", ["fp32", "bf16x3", "bf16"])
@pytest.mark.parametrize("env_name", ["Pendulum-v0", "Synthetic-17x6"])
def test_rollout_stepped_matches_torch_engine(env_name, dtype):
    p = _params(env_name, dtype)
    eng, model, env, stats = _engine(p)
    assert not eng.stepped_env                  # kinds 0 / 1: rollout() is the fused kernel, this is the public path
    ref = _torch_engine(p, model, stats)
    state_ptr = (env.state.data_ptr(), env.ep_len.data_ptr(), env.ep_ret.data_ptr())
    ro_h = eng.rollout_stepped()
    ro_t = ref.rollout()
    assert int(ref.dones.sum()) >= eng.E        # every env reset inside the rollout (limit 3, 5 steps)
    _compare_rollouts(eng, env, ro_h, ref, ro_t, dtype)
    # updated in place: the env's tensors are the ones a checkpoint reads
    assert state_ptr == (env.state.data_ptr(), env.ep_len.data_ptr(), env.ep_ret.data_ptr())
    assert not eng._xT_valid


@pytest.mark.parametrize("env_name", ["Pendulum-v0", "Synthetic-17x6"])
def test_rollout_stepped_step_obs_norm_matches_torch_engine(env_name):
    p = _params(env_name, "fp32", obs_norm_update="step")
    eng, model, env, stats = _engine(p)
    ref = _torch_engine(p, model, stats)
    ro_h = eng.rollout_stepped()
    ro_t = ref.rollout()
    _compare_rollouts(eng, env, ro_h, ref, ro_t, "fp32")
    # the per-rollout stats copy absorbed all T*E observations, like the torch engine's
    assert eng.local_stats.n == pytest.approx(ref.local_stats.n)
    assert torch.allclose(eng.local_stats.mean, ref.local_stats.mean, rtol=1e-6, atol=1e-6)
    assert torch.equal(stats.mean, ref.stats.mean)          # the shared stats are merged by the worker, not here


def test_rollout_stepped_matches_fused_rollout_kernel():
    p = _params("Pendulum-v0", "bf16x3")
    eng, model, env, stats = _engine(p)
    eng2, model2, env2, stats2 = _engine(p)
    assert torch.equal(model.flat.data, model2.flat.data) and torch.equal(stats.mean_f32, stats2.mean_f32)
    ro_s = eng.rollout_stepped()
    ro_f = eng2.rollout()
    ro_s, ro_f = ({k: (v.clone() if torch.is_tensor(v) else v) for k, v in ro.items()} for ro in (ro_s, ro_f))
    _compare_rollouts(eng, env, ro_s, eng2, ro_f, "bf16x3", ref_is_torch=False)
    assert float(ro_s["ep_return_sum"]) == pytest.approx(float(ro_f["ep_return_sum"]), rel=1e-4, abs=2e-4 * eng.N)


# ---- the cart-pole ------------------------------------------------------------------------------------------
# seeds for which the references below meet their preconditions (asserted in each test): terminations
# happen and no pre-reset state comes within 1e-3 of a termination threshold.  A falling pole crosses
# its threshold at ~0.017 rad per step, so one crossing in eight lands that close: the seeds are picked
ROLLOUT_SEED, EVAL_SEED = 200, 18


def _balancing_policy(model, log_std, eps=0.05):
    """a policy that mostly balances the pole: mu ~= g . x through one unit per layer in tanh's
    linear range (the evaluation then has both early terminations, from the action noise, and
    episodes that reach the time limit)"""
    with torch.no_grad():
        for k in ("p_fc1", "p_fc2", "mu"):
            model.view(k + ".weight").zero_()
            model.view(k + ".bias").zero_()
        model.view("p_fc1.weight")[0] = eps * torch.tensor([0.01, 0.03, 1.0, 0.15], device=DEV)
        model.view("p_fc2.weight")[0, 0] = 1.0
        model.view("mu.weight")[0, 0] = 1.0 / eps
        model.flat.data[:model.num_outputs] = log_std


@pytest.mark.parametrize("dtype", ["bf16x3", "fp32"])
def test_cartpole_rollout_matches_torch_engine(dtype):
    p = _params(CARTPOLE, dtype, E=45, T=24, max_episode_length=10000, seed=ROLLOUT_SEED)
    eng, model, env, stats = _engine(p)
    assert eng.stepped_env and env.kind == 3
    new_states = []
    ref = _torch_engine(p, model, stats, record=new_states)
    ro_h = eng.rollout()                        # dispatches to rollout_stepped
    ro_t = ref.rollout()
    # precondition, on the reference alone: terminations happened, none within 1e-3 of a threshold
    # (so no flag can flip inside the tolerance)
    margin = _threshold_margin(new_states)
    print("reference terminations", int(ref.dones.sum()), "threshold margin", margin)
    assert int(ref.dones.sum()) >= 5 and margin > 1e-3
    assert torch.equal(ref.rewards, torch.ones_like(ref.rewards))
    _compare_rollouts(eng, env, ro_h, ref, ro_t, dtype)


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


@pytest.mark.parametrize("obs_norm_update", ["rollout", "step"])
def test_stepped_rollout_and_evaluate_do_not_sync(obs_norm_update):
    p = _params(CARTPOLE, "bf16x3", E=45, T=4, max_episode_length=6, obs_norm_update=obs_norm_update)
    eng, model, env, stats = _engine(p)
    eng.rollout_stepped()                       # (first call: allocations, kernel loads)
    eng.evaluate(20, False)
    torch.cuda.synchronize()
    if not _sync_mode_raises():
        pytest.skip("torch.cuda.set_sync_debug_mode('error') does not raise on .item() in this build")
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        ro = eng.rollout_stepped()
        ret, ln = eng.evaluate(20, False)
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    torch.cuda.synchronize()
    assert float(ro["ep_count"]) > 0 and int(ln.min()) >= 1 and int(ln.max()) <= 6


_TRAINING_STATE = ("env.state", "ep_len", "ep_ret", "env.t", "x_buf", "actions", "logp", "rewards", "dones", "mom",
                   "epstat", "stats.mean", "stats.mean_diff", "stats.mean_f32", "stats.inv_std_f32", "model.flat",
                   "wimg", "adam_m", "adam_v", "adam_state")


def _training_state(eng, model, env, stats):
    """the set tests/test_gpu_eval.py checks"""
    d = {"env.state": env.state, "ep_len": env.ep_len, "ep_ret": env.ep_ret,
         "env.t": torch.tensor(env.t), "x_buf": eng.x_buf, "actions": eng.actions, "logp": eng.logp,
         "rewards": eng.rewards, "dones": eng.dones, "mom": eng.mom, "epstat": eng.epstat,
         "stats.mean": stats.mean, "stats.mean_diff": stats.mean_diff, "stats.mean_f32": stats.mean_f32,
         "stats.inv_std_f32": stats.inv_std_f32, "model.flat": model.flat.data, "wimg": eng.wimg,
         "adam_m": eng.adam_m, "adam_v": eng.adam_v, "adam_state": eng.adam_state}
    assert tuple(d) == _TRAINING_STATE
    return d


@pytest.mark.parametrize("deterministic", [False, True])
def test_cartpole_evaluate_matches_twin(deterministic):
    E, limit = 64, 40
    p = _params(CARTPOLE, "bf16x3", E=32, T=8, max_episode_length=limit, seed=EVAL_SEED)
    eng, model, env, stats = _engine(p)
    _balancing_policy(model, log_std=0.5)
    eng.params_changed()
    eng.rollout()                               # non-trivial env state, episode trackers, step counter, buffers
    before = {k: v.clone() for k, v in _training_state(eng, model, env, stats).items()}
    ret, ln = eng.evaluate(E, deterministic)
    torch.cuda.synchronize()
    # the twin, on the same device, on an env whose pre-reset states are recorded
    twin_env = make_vec_env(get_spec(CARTPOLE), E, seed=p.seed + EVAL_ENV_SEED_OFFSET, rank=0, device=DEV,
                            max_episode_length=limit)
    new_states = []
    _record_new_states(twin_env, new_states)
    ret_t, ln_t = evaluate_batch(model, stats, twin_env, E, p.seed, limit, p.std_convention, deterministic)
    margin = _threshold_margin(new_states)
    print("twin lengths", sorted(set(ln_t.tolist())), "threshold margin", margin)
    assert margin > 1e-3
    if not deterministic:
        assert int((ln_t < limit).sum()) >= 5 and int((ln_t == limit).sum()) >= 1     # both kinds of episode end
    assert ret.dtype == torch.float32 and ln.dtype == torch.int32 and ret.shape == (E,) and ln.shape == (E,)
    assert torch.equal(ln, ln_t)
    assert torch.equal(ret, ret_t) and torch.equal(ret, ln.to(torch.float32))         # reward 1 per step
    for k, v in _training_state(eng, model, env, stats).items():
        assert torch.equal(v, before[k]), k
    ptrs = {v.data_ptr() for v in _training_state(eng, model, env, stats).values() if v.is_cuda}
    assert ret.data_ptr() not in ptrs and ln.data_ptr() not in ptrs


def test_cartpole_resume_continues_bit_identically(tmp_path):
    """3 iterations straight == 2 iterations, checkpoint, a fresh worker resumed from it, 1 more"""
    from pytorch_dppo_amd.runtime.launcher import run_worker
    base = dict(device="gpu", env_name=CARTPOLE, num_processes=1, num_envs=32, exploration_size=32 * 8,
                batch_size=32 * 8, num_epoch=2, dtype="bf16x3", seed=4)
    ctx = DistContext(device=DEV)
    w_full, _ = run_worker(dppo_preset(max_iters=3, **base), ctx, evaluator=False, quiet=True)
    ck = str(tmp_path / "ck")
    w_two, _ = run_worker(dppo_preset(max_iters=2, checkpoint_dir=ck, **base), ctx, evaluator=False, quiet=True)
    w_res, _ = run_worker(dppo_preset(max_iters=3, resume=ck, **base), ctx, evaluator=False, quiet=True)
    torch.cuda.synchronize()
    assert w_full.engine.stepped_env and w_res.iteration == 3
    assert w_res.engine.adam_step == w_full.engine.adam_step
    assert not torch.equal(w_two.env.state, w_full.env.state)       # the third iteration moved the envs
    assert torch.equal(w_full.model.flat.data, w_res.model.flat.data)
    assert torch.equal(w_full.engine.adam_m, w_res.engine.adam_m)
    assert torch.equal(w_full.engine.adam_v, w_res.engine.adam_v)
    assert torch.equal(w_full.env.state, w_res.env.state)
    assert torch.equal(w_full.env.ep_len, w_res.env.ep_len) and torch.equal(w_full.env.ep_ret, w_res.env.ep_ret)
    assert w_full.env.t == w_res.env.t == 24
    assert torch.equal(w_full.stats.mean, w_res.stats.mean)


def test_train_py_cartpole_end_to_end(tmp_path):
    path = tmp_path / "train.jsonl"
    cmd = [sys.executable, "train.py", "--device", "gpu", "--env-name", CARTPOLE, "--eval-every", "1", "--eval-mode",
           "inline", "--max-iters", "2", "--num-processes", "1", "--num-envs", "32", "--exploration-size", "1024",
           "--batch-size", "1024", "--num-epoch", "2", "--dtype", "bf16x3", "--eval-envs", "32",
           "--max-episode-length", "50", "--log-jsonl", str(path)]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=170)
    assert r.returncode == 0, r.stderr[-3000:]
    recs = [json.loads(l) for l in path.read_text().splitlines()]
    its = [x for x in recs if "eval_iteration" not in x]
    evs = [x for x in recs if "eval_iteration" in x]
    assert len(its) == 2 and len(evs) >= 1
    for m in its:
        assert all(math.isfinite(m[k]) for k in ("loss", "loss_clip", "loss_value", "grad_norm")), m
        assert m["ep_count"] > 0 and 1.0 <= m["mean_ep_return"] <= 50.0
    for e in evs:
        assert e["eval_episodes"] == 32 and 1.0 <= e["eval_length_mean"] <= 50.0
        assert e["eval_return_mean"] == pytest.approx(e["eval_length_mean"])      # reward 1 per step
