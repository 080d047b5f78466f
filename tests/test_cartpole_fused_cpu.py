"""The fused cart-pole's host side, without a GPU: the ``env_fused`` parameter and its command-line flag,
the in-kernel kind of every env class (``VecEnv.kernel_kind``) and the helper that refuses an env that
has none (tests/test_gpu_cartpole_fused.py holds the kernels themselves to the torch env)."""
import pytest
import torch

from pytorch_dppo_amd.config import Params, dppo_preset, params_from_args
from pytorch_dppo_amd.envs import (KIND_CARTPOLE, KIND_PENDULUM, KIND_SYNTHETIC, KIND_TENSOR, VecEnv, get_spec,
                                   kernel_kind_of, make_vec_env, register_tensor_env)

CARTPOLE = "CartPoleContinuous-v1"


class _DriftEnv(VecEnv):
    """a user's tensor env: the state drifts by the action, never terminates"""

    @property
    def state_dim(self):
        return 3

    def _reset_state(self, step_key):
        return torch.zeros(self.E, 3, device=self.device)

    def observe(self):
        return self.state.clone()

    def _dynamics(self, a, step_key):
        return (self.state + a[:, :1], torch.ones(self.E, device=self.device),
                torch.zeros(self.E, dtype=torch.bool, device=self.device))


USER_ENV = "FusedTestDrift-v0"
register_tensor_env(USER_ENV, _DriftEnv, obs_dim=3, act_dim=1, time_limit=20)


def test_env_fused_defaults_to_false_and_parses():
    assert Params().env_fused is False and dppo_preset().env_fused is False
    assert params_from_args([]).env_fused is False
    assert params_from_args(["--env-fused", "true"]).env_fused is True
    assert params_from_args(["--env-fused", "false"]).env_fused is False
    assert params_from_args(["--env-fused"]).env_fused is True           # as --fused-apply: a bare flag is true
    p = params_from_args(["--env-name", CARTPOLE, "--env-fused", "true", "--device", "gpu"])
    assert Params.from_dict(p.to_dict()).env_fused is True                # survives a checkpoint's params


def test_env_fused_refuses_the_gym_backend():
    with pytest.raises(ValueError, match="env_fused"):
        dppo_preset(env_backend="gym", env_fused=True)
    assert dppo_preset(env_backend="gym").env_fused is False


def test_kernel_kind_of_every_env_class():
    assert (KIND_SYNTHETIC, KIND_PENDULUM, KIND_CARTPOLE) == (0, 1, 2)
    assert VecEnv.kernel_kind is None
    want = {"Synthetic-17x6": KIND_SYNTHETIC, "HalfCheetah-v1": KIND_SYNTHETIC, "Pendulum-v0": KIND_PENDULUM,
            CARTPOLE: KIND_CARTPOLE}
    for name, kind in want.items():
        env = make_vec_env(get_spec(name), 3)
        assert env.kernel_kind == kind and kernel_kind_of(env) == kind, name
        assert type(kernel_kind_of(env)) is int
    # the cart-pole's spec kind is what it was: a registered tensor env
    assert get_spec(CARTPOLE).kind == KIND_TENSOR and make_vec_env(get_spec(CARTPOLE), 3).kind == KIND_TENSOR


def test_user_env_has_no_kernel_kind_and_is_refused_by_name():
    env = make_vec_env(get_spec(USER_ENV), 5)
    assert env.kind == KIND_TENSOR and env.kernel_kind is None
    with pytest.raises(ValueError) as ei:
        kernel_kind_of(env)
    assert USER_ENV in str(ei.value) and "_DriftEnv" in str(ei.value)


def test_cpu_engine_ignores_env_fused():
    """the torch env is the twin either way: the same rollout with the flag on and off"""
    from pytorch_dppo_amd.models.actor_critic import ActorCritic
    from pytorch_dppo_amd.runtime.engine_torch import TorchEngine
    from pytorch_dppo_amd.utils.obs_stats import RunningObsStats
    outs = []
    for fused in (False, True):
        p = dppo_preset(env_name=CARTPOLE, num_envs=5, exploration_size=40, batch_size=40, seed=3, env_fused=fused)
        spec = get_spec(CARTPOLE)
        torch.manual_seed(0)
        model = ActorCritic(spec.obs_dim, spec.act_dim, p.hidden)
        env = make_vec_env(spec, p.num_envs, seed=p.seed)
        eng = TorchEngine(p, model, env, RunningObsStats(spec.obs_dim, torch.device("cpu")), torch.device("cpu"), 0)
        eng.rollout()
        outs.append((eng.actions.clone(), eng.dones.clone(), env.state.clone()))
    for a, b in zip(*outs):
        assert torch.equal(a, b)
