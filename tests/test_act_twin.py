"""Policy inference, CPU side: the torch twin ``oracle.policy_act`` (the oracle of the GPU tests in
test_gpu_act.py) pinned to ``TorchEngine.rollout`` / ``run_episode``, the ``host_policy`` config
field, ``PolicyRunner`` on the CPU and the ``play.py`` CLI."""
import os
import sys

import pytest
import torch

from pytorch_dppo_amd.config import Params, dppo_preset, params_from_args
from pytorch_dppo_amd.envs import get_spec, make_vec_env
from pytorch_dppo_amd.models.actor_critic import ActorCritic
from pytorch_dppo_amd.ops import oracle
from pytorch_dppo_amd.parallel.dist import DistContext
from pytorch_dppo_amd.runtime.engine_torch import TorchEngine
from pytorch_dppo_amd.runtime.evaluator import run_episode
from pytorch_dppo_amd.utils import rng
from pytorch_dppo_amd.utils.obs_stats import RunningObsStats

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


@pytest.mark.parametrize("env_name", ["Pendulum-v0", "HalfCheetah-v2"])
@pytest.mark.parametrize("convention", ["std", "var"])
def test_twin_is_the_torch_engines_rollout_step(env_name, convention):
    """the first step of a TorchEngine rollout, bit for bit; deterministic: a = mu, closed-form logp"""
    spec = get_spec(env_name)
    O, A = spec.obs_dim, spec.act_dim
    p = dppo_preset(env_name=env_name, num_envs=5, exploration_size=5 * 4, batch_size=20, seed=3,
                    std_convention=convention)
    torch.manual_seed(0)
    model = ActorCritic(O, A)
    with torch.no_grad():
        model.flat.data[:A] = torch.linspace(-0.5, 0.3, A)
    env = make_vec_env(spec, 5, seed=p.seed, rank=0, max_episode_length=50)
    stats = RunningObsStats(O)
    eng = TorchEngine(p, model, env, stats, torch.device("cpu"), 0)
    stats.observes(eng.obs * 3.0 + 0.5)
    obs0, t0 = eng.obs.clone(), env.t
    eng.rollout()
    a, logp, mu, x = oracle.policy_act(model, stats, obs0, eng.key_action, env.env_idx, t0, convention)
    assert torch.equal(a, eng.actions[0]) and torch.equal(logp, eng.logp[0]) and torch.equal(x, eng.x[0])
    assert not torch.equal(a, mu)
    ad, logpd, mud, xd = oracle.policy_act(model, stats, obs0, eng.key_action, env.env_idx, t0, convention, True)
    assert torch.equal(ad, mud) and torch.equal(mud, mu) and torch.equal(xd, x)
    log_std = model.view("log_std")
    log_sigma = log_std if convention == "std" else 0.5 * log_std
    want = -log_sigma.sum() - 0.5 * A * oracle.LOG_2PI
    assert logpd.shape == (5,) and bool((logpd == want).all())


def test_host_policy_param():
    assert Params().host_policy == "torch"
    with pytest.raises(ValueError, match="host_policy"):
        Params(host_policy="x")
    assert params_from_args(["--host-policy", "kernel"]).host_policy == "kernel"
    assert Params.from_dict({**Params().to_dict(), "host_policy": "kernel"}).host_policy == "kernel"


@pytest.fixture(scope="module")
def trained(tmp_path_factory):
    """two CPU iterations on the synthetic env, small network, checkpointed"""
    from pytorch_dppo_amd.runtime.launcher import run_worker
    d = tmp_path_factory.mktemp("ckpt")
    p = dppo_preset(env_name="Synthetic-3x1", num_envs=4, exploration_size=32, batch_size=32, num_epoch=2,
                    hidden=(16, 12), value_mult=2, seed=5, checkpoint_dir=str(d), log_every=0)
    w, _ = run_worker(p, DistContext(), max_iters=2, quiet=True)
    return str(d), w


def test_policy_runner_cpu(trained):
    from pytorch_dppo_amd.runtime.policy import PolicyRunner
    d, w = trained
    r = PolicyRunner.from_checkpoint(d, device="cpu")
    assert (r.O, r.A, r.seed, r.step) == (3, 1, 5, 0)
    key = rng.base_key(5, rng.STREAM_EVAL, 0)
    torch.manual_seed(1)
    for call in range(3):
        obs = torch.randn(7, 3) * 2.0
        a, logp = r.act(obs)
        wa, wl, _, _ = oracle.policy_act(w.model, w.stats, obs, key, torch.arange(7), call, "std")
        assert torch.equal(a, wa) and torch.equal(logp, wl)
        assert r.step == call + 1
    a, logp = r.act(obs, deterministic=True, step_key=99)
    wa, wl, _, _ = oracle.policy_act(w.model, w.stats, obs, key, torch.arange(7), 99, "std", True)
    assert torch.equal(a, wa) and torch.equal(logp, wl) and r.step == 4
    one, _ = r.act(obs[0])                       # a single observation is one row
    assert one.shape == (1, 1)
    with pytest.raises(ValueError, match="fp8"):
        PolicyRunner.from_checkpoint(d, device="cpu", dtype="fp8")
    with pytest.raises(ValueError, match="hidden"):
        PolicyRunner(w.model.state_dict(), w.stats.state_dict(), hidden=(100, 100), device="cpu")


def test_play_cli_is_run_episode(trained, capsys):
    """play.py's loop is the evaluator's run_episode (same loop order: exact)"""
    import play
    d, w = trained
    out = play.main(["--checkpoint", d, "--device", "cpu", "--episodes", "2", "--env-name", "Pendulum-v0"])
    assert len(out) == 2 and all(length == 200 for _, length in out)
    env = make_vec_env(get_spec("Pendulum-v0"), 1, seed=5 + 7777, rank=0, device="cpu", max_episode_length=10000)
    key = rng.base_key(5, rng.STREAM_EVAL, 0)
    want = [run_episode(w.model, w.stats, env, key, "std") for _ in range(2)]
    assert out == want
    lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith("Time ")]
    assert len(lines) == 2 and all(", episode reward " in l and ", episode length 200" in l for l in lines)
