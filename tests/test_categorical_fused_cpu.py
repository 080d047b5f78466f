"""``CartPole-v0``, the discrete cart-pole that owns an in-kernel twin (docs/ARCHITECTURE.md §29), without a GPU: its
spec and kernel kind, that it is ``CartPole-v1`` but for the step limit, that the CPU engine ignores ``env_fused``, the
command line, and learning.  tests/test_gpu_categorical_fused.py holds the kernels to the torch env."""
import pytest
import torch

from pytorch_dppo_amd.config import Params, dppo_preset, params_from_args
from pytorch_dppo_amd.envs import KIND_CARTPOLE, KIND_TENSOR, get_spec, kernel_kind_of, make_vec_env
from pytorch_dppo_amd.envs.vec_env import CartPoleEnv, CartPoleV0Env
from pytorch_dppo_amd.parallel.dist import DistContext

V0, V1 = "CartPole-v0", "CartPole-v1"


def test_spec_and_kernel_kind():
    spec = get_spec(V0)
    assert (spec.obs_dim, spec.act_dim, spec.kind, spec.time_limit, spec.discrete) == (4, 2, KIND_TENSOR, 200, True)
    env = make_vec_env(spec, 3)
    assert type(env) is CartPoleV0Env and isinstance(env, CartPoleEnv) and env.kind == KIND_TENSOR
    assert CartPoleV0Env.kernel_kind == KIND_CARTPOLE == 2
    assert kernel_kind_of(env) == 2 and type(kernel_kind_of(env)) is int
    assert CartPoleV0Env._dynamics is CartPoleEnv._dynamics           # no physics of its own
    assert env.limit == 200 and make_vec_env(spec, 3, max_episode_length=50).limit == 50
    # CartPole-v1 is as before: no twin, refused by name
    v1 = make_vec_env(get_spec(V1), 3)
    assert type(v1) is CartPoleEnv and v1.kernel_kind is None and get_spec(V1).time_limit == 500
    with pytest.raises(ValueError, match="no in-kernel twin") as ei:
        kernel_kind_of(v1)
    assert V1 in str(ei.value)


def test_v0_is_v1_under_the_same_limit():
    E, limit = 33, 30
    a0 = make_vec_env(get_spec(V0), E, seed=7, max_episode_length=limit)
    a1 = make_vec_env(get_spec(V1), E, seed=7, max_episode_length=limit)
    assert torch.equal(a0.reset(), a1.reset())
    g = torch.Generator().manual_seed(0)
    by_limit = by_state = 0
    for _ in range(40):
        a = torch.randint(0, 2, (E,), generator=g)
        len_before = a0.ep_len.clone()
        o0, r0, d0, i0 = a0.step(a)
        o1, r1, d1, i1 = a1.step(a)
        assert torch.equal(o0, o1) and torch.equal(r0, r1) and torch.equal(d0, d1)
        assert torch.equal(a0.state, a1.state) and torch.equal(a0.ep_len, a1.ep_len) and torch.equal(a0.ep_ret, a1.ep_ret)
        assert float(i0["ep_return_sum"]) == float(i1["ep_return_sum"]) and float(i0["ep_count"]) == float(i1["ep_count"])
        ended = d0.bool()
        by_limit += int((ended & (len_before + 1 >= limit)).sum())
        by_state += int((ended & (len_before + 1 < limit)).sum())
    assert by_limit > 0 and by_state > 0                               # both kinds of episode end occurred
    assert a0.t == a1.t == 40


def test_cpu_engine_ignores_env_fused():
    from pytorch_dppo_amd.models.actor_critic import ActorCritic
    from pytorch_dppo_amd.runtime.engine_torch import TorchEngine
    from pytorch_dppo_amd.utils.obs_stats import RunningObsStats
    outs = []
    for fused in (False, True):
        p = dppo_preset(env_name=V0, num_envs=5, exploration_size=40, batch_size=40, seed=3, env_fused=fused)
        spec = get_spec(V0)
        torch.manual_seed(0)
        model = ActorCritic(spec.obs_dim, spec.act_dim, p.hidden)
        env = make_vec_env(spec, p.num_envs, seed=p.seed)
        eng = TorchEngine(p, model, env, RunningObsStats(spec.obs_dim, torch.device("cpu")), torch.device("cpu"), 0)
        assert eng.discrete
        eng.rollout()
        outs.append((eng.actions.clone(), eng.logp.clone(), eng.dones.clone(), env.state.clone()))
    rows = outs[0][0].reshape(-1, 2)
    assert bool(((rows == 0) | (rows == 1)).all()) and bool((rows.sum(1) == 1).all())
    for a, b in zip(*outs):
        assert torch.equal(a, b)


def test_command_line_round_trip():
    p = params_from_args(["--env-name", V0, "--env-fused", "true", "--device", "gpu", "--dtype", "bf16x3"])
    assert p.env_name == V0 and p.env_fused is True
    q = Params.from_dict(p.to_dict())                                  # (a checkpoint's params)
    assert q.env_name == V0 and q.env_fused is True and q.to_dict() == p.to_dict()
    assert params_from_args(["--env-name", V0]).env_fused is False
    # the per-step filter's refusal belongs to the GPU engine (the CPU engine ignores the flag): the parameters parse
    assert params_from_args(["--env-name", V0, "--env-fused", "true", "--obs-norm-update", "step"]).env_fused is True


def test_dppo_learns_cartpole_v0():
    """tests/test_categorical.py test_dppo_learns_discrete_cartpole's configuration and criterion on CartPole-v0 (the
    200-step cap is the one difference): 12 CPU iterations at least triple the mean episode length.  Measured ratios at
    seeds 1-3: profiles/categorical_fused/README.md."""
    from pytorch_dppo_amd.runtime.worker import DPPOWorker
    torch.set_num_threads(2)
    p = dppo_preset(env_name=V0, num_envs=32, exploration_size=2048, batch_size=512,
                    num_epoch=4, hidden=(32, 32), lr=3e-3, seed=1)
    w = DPPOWorker(p, DistContext())
    steps_per_episode = []
    for _ in range(12):
        w.iteration_step()
        steps_per_episode.append(p.buffer_rows / float(w.engine.dones.sum()))
    print("steps per episode:", [round(s, 1) for s in steps_per_episode])
    assert steps_per_episode[-1] >= 3.0 * steps_per_episode[0], steps_per_episode
