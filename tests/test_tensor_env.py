"""Registered tensor envs (envs.register_tensor_env, Params.env_module) and the continuous cart-pole
(envs/vec_env.py CartPoleContinuousEnv), on the CPU: registration, the physics against an
independent float64 transcription, episode accounting, that training on it learns, and the two
optional arguments of evaluator.evaluate_batch.  tests/test_gpu_tensor_env.py holds the GPU engine's
device-stepped path to the same oracles."""
import math
import queue
import sys
import textwrap

import numpy as np
import pytest
import torch

from pytorch_dppo_amd.config import Params, dppo_preset, params_from_args
from pytorch_dppo_amd.envs import (KIND_TENSOR, CartPoleContinuousEnv, PendulumEnv, VecEnv, get_spec, known_envs,
                                   make_vec_env, register_tensor_env)
from pytorch_dppo_amd.envs.registry import KIND_PENDULUM, KIND_SYNTHETIC
from pytorch_dppo_amd.models.actor_critic import ActorCritic
from pytorch_dppo_amd.parallel.dist import DistContext
from pytorch_dppo_amd.runtime.evaluator import evaluate_batch, evaluator_main
from pytorch_dppo_amd.utils import rng
from pytorch_dppo_amd.utils.obs_stats import RunningObsStats

ENV_MODULE_SRC = """
    import torch
    from pytorch_dppo_amd.envs import VecEnv, register_tensor_env


    class DriftEnv(VecEnv):
        '''s' = 0.5 s + a, reward -s^2, never terminal'''
        @property
        def state_dim(self):
            return 2

        def _reset_state(self, step_key):
            return torch.zeros(self.E, 2, device=self.device)

        def observe(self):
            return self.state.clone()

        def _dynamics(self, a, step_key):
            new = 0.5 * self.state + a
            return new, -(new * new).sum(1), torch.zeros(self.E, dtype=torch.bool, device=self.device)


    register_tensor_env("{name}", DriftEnv, obs_dim=2, act_dim=2, time_limit=9)
"""


# ---- registration -----------------------------------------------------------------------------------
def test_register_tensor_env_and_make_vec_env():
    class Twin(PendulumEnv):
        pass

    spec = register_tensor_env("TwinPendulum-v0", Twin, obs_dim=3, act_dim=1, time_limit=11)
    assert spec.kind == KIND_TENSOR == 3 and get_spec("TwinPendulum-v0") is spec
    assert "TwinPendulum-v0" in known_envs()
    env = make_vec_env(spec, 5, seed=3)
    assert type(env) is Twin and isinstance(env, VecEnv) and (env.E, env.O, env.A, env.limit) == (5, 3, 1, 11)
    # the shipped cart-pole is such an entry; the built-in table is as it was
    cp = get_spec("CartPoleContinuous-v1")
    assert (cp.obs_dim, cp.act_dim, cp.kind, cp.time_limit) == (4, 1, KIND_TENSOR, 500)
    assert type(make_vec_env(cp, 2)) is CartPoleContinuousEnv
    assert get_spec("InvertedPendulum-v1").kind == KIND_SYNTHETIC and get_spec("Pendulum-v0").kind == KIND_PENDULUM
    assert type(make_vec_env(get_spec("Pendulum-v0"), 2)) is PendulumEnv
    with pytest.raises(ValueError):
        register_tensor_env("Pendulum-v0", Twin, 3, 1, 200)       # a built-in entry is never re-kinded
    with pytest.raises(KeyError):
        get_spec("NoSuchEnv-v0")


def test_env_module_is_imported_by_worker_and_evaluator(tmp_path, monkeypatch):
    from pytorch_dppo_amd.runtime.worker import DPPOWorker
    monkeypatch.syspath_prepend(str(tmp_path))
    (tmp_path / "user_env_a.py").write_text(textwrap.dedent(ENV_MODULE_SRC.format(name="DriftA-v0")))
    (tmp_path / "user_env_b.py").write_text(textwrap.dedent(ENV_MODULE_SRC.format(name="DriftB-v0")))
    assert Params().env_module == ""
    with pytest.raises(KeyError):
        get_spec("DriftA-v0")
    # in-process: the CLI flag reaches Params, the worker imports the module and trains on the env
    p = params_from_args(["--env-module", "user_env_a", "--env-name", "DriftA-v0", "--num-envs", "4",
                          "--exploration-size", "32", "--batch-size", "32", "--num-epoch", "1", "--hidden", "8,8"])
    assert p.env_module == "user_env_a"
    w = DPPOWorker(p, DistContext())
    assert "user_env_a" in sys.modules and get_spec("DriftA-v0").kind == KIND_TENSOR
    assert type(w.env).__name__ == "DriftEnv" and w.env.limit == 9
    m = w.iteration_step()
    assert math.isfinite(m["loss"]) and bool(torch.isfinite(w.model.flat.data).all())
    # the evaluator's entry point imports it itself (it runs in a spawned process): module b is
    # known only through it
    with pytest.raises(KeyError):
        get_spec("DriftB-v0")
    q = queue.Queue()
    q.put(None)                                  # stop at the first poll
    pb = dppo_preset(env_module="user_env_b", env_name="DriftB-v0", hidden=(8, 8))
    evaluator_main(pb.to_dict(), q)
    assert "user_env_b" in sys.modules and get_spec("DriftB-v0").time_limit == 9
    # without the module the same call does not know the env
    q.put(None)
    with pytest.raises(KeyError):
        evaluator_main(dppo_preset(env_name="DriftC-v0", hidden=(8, 8)).to_dict(), q)


# ---- cart-pole physics --------------------------------------------------------------------------------
X_LIMIT, TH_LIMIT = 2.4, 12.0 * 2.0 * math.pi / 360.0


def cartpole_step_f64(s, a):
    """gym CartPole-v1's published equations in float64 numpy: s [E,4] (x, x_dot, theta, theta_dot),
    a [E] -> the new state"""
    g, mc, mp, l, dt = 9.8, 1.0, 0.1, 0.5, 0.02
    x, xd, th, thd = s[:, 0], s[:, 1], s[:, 2], s[:, 3]
    f = 10.0 * np.clip(a, -1.0, 1.0)
    mt = mc + mp
    ct, st = np.cos(th), np.sin(th)
    tmp = (f + mp * l * thd ** 2 * st) / mt
    tha = (g * st - ct * tmp) / (l * (4.0 / 3.0 - mp * ct ** 2 / mt))
    xa = tmp - mp * l * tha * ct / mt
    return np.stack([x + dt * xd, xd + dt * xa, th + dt * thd, thd + dt * tha], 1)


def threshold_margin(s):
    """smallest distance of |x| / |theta| of the states s [..., 4] to their termination thresholds"""
    s = np.asarray(s, dtype=np.float64)
    return float(min(np.abs(np.abs(s[..., 0]) - X_LIMIT).min(), np.abs(np.abs(s[..., 2]) - TH_LIMIT).min()))


def test_cartpole_matches_float64_transcription():
    E, T, seed = 64, 50, 17     # (seed: the reference's threshold margin is 5e-4 for it, asserted below)
    env = make_vec_env(get_spec("CartPoleContinuous-v1"), E, seed=seed)
    obs = env.reset()
    assert obs.shape == (E, 4) and float(obs.abs().max()) <= 0.05 and torch.equal(obs, env.state)
    gen = torch.Generator().manual_seed(seed)
    ref = env.state.double().numpy().copy()
    margin, n_term = float("inf"), 0
    for t in range(T):
        a = (torch.rand(E, 1, generator=gen) * 4.0 - 2.0)
        # the reset draw is the keyed RNG's (not physics): the reference takes the same uniforms
        d = torch.arange(4, dtype=torch.int64)
        u = rng.uniform01(rng.keyed(env.key_reset, env.env_idx[:, None], env.t, d[None, :])).double().numpy()
        reset = (2.0 * u - 1.0) * 0.05
        new = cartpole_step_f64(ref, a[:, 0].double().numpy())
        margin = min(margin, threshold_margin(new))
        term = (np.abs(new[:, 0]) > X_LIMIT) | (np.abs(new[:, 2]) > TH_LIMIT)
        ref = np.where(term[:, None], reset, new)
        n_term += int(term.sum())
        obs, r, done, info = env.step(a)
        assert torch.equal(r, torch.ones(E))
        assert np.array_equal(done.numpy(), term), t            # limit 500: done == terminal here
        err = float(np.abs(env.state.double().numpy() - ref).max())
        assert err <= 1e-5, (t, err)
        assert torch.equal(obs, env.state)
    # precondition, on the reference alone: no state came within 1e-4 of a threshold (no flag could
    # flip inside the tolerance), and the run did terminate (and reset in place) many times
    assert margin > 1e-4, margin
    assert n_term >= 20, n_term


def test_cartpole_episode_accounting_under_time_limit():
    E = 6
    env = make_vec_env(get_spec("CartPoleContinuous-v1"), E, seed=2, max_episode_length=7)
    assert env.limit == 7
    env.reset()
    zero = torch.zeros(E, 1)
    for t in range(1, 15):
        _, r, done, info = env.step(zero)          # an unforced pole from +-0.05 stays up for 7 steps
        fired = t % 7 == 0
        assert bool(done.all()) == fired and bool(done.any()) == fired
        if fired:
            assert torch.equal(info["finished_len"], torch.full((E,), 7, dtype=torch.int32))
            assert torch.equal(info["finished_ret"], torch.full((E,), 7.0))
            assert float(info["ep_count"]) == E and float(info["ep_return_sum"]) == 7.0 * E
            assert int(env.ep_len.abs().sum()) == 0 and float(env.ep_ret.abs().sum()) == 0.0
            assert float(env.state.abs().max()) <= 0.05          # reset in place
        else:
            assert float(info["ep_count"]) == 0 and int(info["finished_len"].sum()) == 0
            assert torch.equal(env.ep_len, torch.full((E,), t % 7, dtype=torch.int32))
            assert torch.equal(env.ep_ret, torch.full((E,), float(t % 7)))


# ---- learning -------------------------------------------------------------------------------------------
def test_dppo_learns_cartpole():
    """12 CPU iterations at least triple the mean episode length (steps per episode end)."""
    from pytorch_dppo_amd.runtime.worker import DPPOWorker
    torch.set_num_threads(2)
    p = dppo_preset(env_name="CartPoleContinuous-v1", num_envs=32, exploration_size=2048, batch_size=512,
                    num_epoch=4, hidden=(32, 32), lr=3e-3, seed=1)
    w = DPPOWorker(p, DistContext())
    steps_per_episode = []
    for _ in range(12):
        w.iteration_step()
        steps_per_episode.append(p.buffer_rows / float(w.engine.dones.sum()))
    print("steps per episode:", [round(s, 1) for s in steps_per_episode])
    assert steps_per_episode[-1] >= 3.0 * steps_per_episode[0], steps_per_episode


# ---- evaluate_batch(act_fn, early_exit) -----------------------------------------------------------------
@pytest.mark.parametrize("deterministic", [False, True])
def test_evaluate_batch_act_fn_and_no_early_exit(deterministic):
    E, seed, limit = 16, 4, 40
    spec = get_spec("CartPoleContinuous-v1")
    torch.manual_seed(0)
    model = ActorCritic(spec.obs_dim, spec.act_dim, (16, 16))
    stats = RunningObsStats(spec.obs_dim)
    stats.observes(0.05 * torch.randn(64, spec.obs_dim))
    ret0, len0 = evaluate_batch(model, stats, spec, E, seed, limit, "std", deterministic)
    assert int(len0.min()) < limit          # every default run may stop early; some episodes end early
    key = rng.base_key(seed, rng.STREAM_EVAL, 0)
    calls = []

    def act_fn(obs, step_key):
        calls.append(int(step_key))
        mu, log_std, _ = model(stats.normalize(obs))
        if deterministic:
            return mu
        eidx = torch.arange(E, dtype=torch.int64)
        eps = rng.gauss(key, eidx[:, None], step_key, torch.arange(spec.act_dim, dtype=torch.int64)[None, :])
        return mu + torch.exp(log_std) * eps

    ret1, len1 = evaluate_batch(model, stats, spec, E, seed, limit, "std", deterministic, act_fn=act_fn,
                                early_exit=False)
    assert calls == list(range(limit))      # all `limit` steps ran, keyed by the shared step counter
    assert torch.equal(ret1, ret0) and torch.equal(len1, len0)
    assert ret1.dtype == torch.float32 and len1.dtype == torch.int32
    # each argument alone changes nothing either
    ret2, len2 = evaluate_batch(model, stats, spec, E, seed, limit, "std", deterministic, early_exit=False)
    assert torch.equal(ret2, ret0) and torch.equal(len2, len0)
