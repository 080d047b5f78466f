"""Batched evaluation, CPU side: the torch twin ``evaluate_batch`` (the oracle of the GPU tests in
test_gpu_eval.py), the inline evaluation of ``run_worker`` on the CPU engine and the new config
fields."""
import json
import math

import pytest
import torch

from pytorch_dppo_amd.config import Params, dppo_preset
from pytorch_dppo_amd.envs import get_spec, make_vec_env
from pytorch_dppo_amd.models.actor_critic import ActorCritic
from pytorch_dppo_amd.parallel.dist import DistContext
from pytorch_dppo_amd.runtime.evaluator import evaluate_batch, run_episode
from pytorch_dppo_amd.utils import rng
from pytorch_dppo_amd.utils.obs_stats import RunningObsStats

SEED = 1


def _snapshot(env_name, hidden=(100, 100)):
    """a policy with a non-trivial log_std and stats seeded from evaluation reset observations"""
    spec = get_spec(env_name)
    torch.manual_seed(0)
    model = ActorCritic(spec.obs_dim, spec.act_dim, hidden)
    with torch.no_grad():
        model.flat.data[:spec.act_dim] = torch.linspace(-0.5, 0.3, spec.act_dim)
    stats = RunningObsStats(spec.obs_dim)
    seed_env = make_vec_env(spec, 64, seed=SEED + 7777, rank=0, max_episode_length=50)
    stats.observes(seed_env.reset())
    return spec, model, stats


class _Recording:
    """an env that records the rewards ``run_episode`` saw (everything else is the env's own)"""

    def __init__(self, env):
        self._env = env
        self.rewards = []

    def __getattr__(self, name):
        return getattr(self._env, name)

    def step(self, a):
        out = self._env.step(a)
        self.rewards.append(out[1][0].clone())
        return out


@pytest.mark.parametrize("env_name", ["Pendulum-v0", "HalfCheetah-v2"])
@pytest.mark.parametrize("deterministic", [False, True])
def test_single_env_twin_is_run_episode(env_name, deterministic):
    """num_envs = 1: the twin is the existing evaluator's ``run_episode`` on a fresh evaluator env.
    The length is equal; the fp32 return is bit-equal to the step-order fp32 sum of the very
    rewards run_episode received (run_episode itself adds them as Python floats, i.e. in fp64, so
    its total is the same sum up to fp32 accumulation rounding: <= len * 2^-24 * sum |r|)."""
    spec, model, stats = _snapshot(env_name)
    env = _Recording(make_vec_env(spec, 1, seed=SEED + 7777, rank=0, max_episode_length=50))
    key = rng.base_key(SEED, rng.STREAM_EVAL, 0)
    total, length = run_episode(model, stats, env, key, "std", deterministic=deterministic)
    ret, ln = evaluate_batch(model, stats, spec, 1, SEED, 50, "std", deterministic)
    assert ret.dtype == torch.float32 and ln.dtype == torch.int32 and ret.shape == (1,) and ln.shape == (1,)
    assert int(ln[0]) == length and length == len(env.rewards) and 1 <= length <= 50
    acc = torch.zeros((), dtype=torch.float32)
    for r in env.rewards:
        acc = acc + r
    assert float(ret[0]) == float(acc)
    assert total == sum(float(r) for r in env.rewards)
    assert abs(float(ret[0]) - total) <= length * 2.0 ** -24 * sum(abs(float(r)) for r in env.rewards)
    # a given env (here: a fresh evaluator env) is accepted in place of the spec
    env2 = make_vec_env(spec, 1, seed=SEED + 7777, rank=0, max_episode_length=50)
    ret2, ln2 = evaluate_batch(model, stats, env2, 1, SEED, 50, "std", deterministic)
    assert torch.equal(ret2, ret) and torch.equal(ln2, ln)


def test_twin_spans_early_and_time_limit_ends():
    """the GPU tests' geometry (HalfCheetah-v2, 45 envs, seed 1, limit 96): the twin's own output
    covers early terminations and time-limit ends before it serves as an oracle.  Termination is a
    keyed uniform, so the lengths do not depend on the policy."""
    spec, model, stats = _snapshot("HalfCheetah-v2")
    ret, ln = evaluate_batch(model, stats, spec, 45, SEED, 96, "std", False)
    assert ret.shape == (45,) and ln.shape == (45,)
    assert int((ln < 96).sum()) >= 1
    assert int((ln == 96).sum()) >= 1
    assert len(set(ln.tolist())) >= 3
    assert int(ln.min()) >= 1 and int(ln.max()) == 96
    assert bool(torch.isfinite(ret).all())
    ret_d, ln_d = evaluate_batch(model, stats, spec, 45, SEED, 96, "std", True)
    assert torch.equal(ln_d, ln)                 # policy-independent lengths
    assert not torch.equal(ret_d, ret)           # ... but the returns follow the action rule
    # envs are independent (keys are per env): a smaller batch is a prefix of a larger one
    ret_s, ln_s = evaluate_batch(model, stats, spec, 17, SEED, 96, "std", False)
    assert torch.equal(ln_s, ln[:17]) and torch.allclose(ret_s, ret[:17], rtol=1e-6, atol=1e-6)


def _run(tmp_path, name, **kw):
    from pytorch_dppo_amd.runtime.launcher import run_worker
    path = tmp_path / f"{name}.jsonl"
    p = dppo_preset(env_name="HalfCheetah-v2", num_envs=8, exploration_size=64, batch_size=64, num_epoch=2,
                    max_episode_length=40, log_jsonl=str(path), **kw)
    w, hist = run_worker(p, DistContext(), max_iters=3, quiet=True)
    recs = [json.loads(l) for l in path.read_text().splitlines()]
    return w, hist, recs


def test_inline_eval_run_worker_cpu(tmp_path, capsys):
    w, hist, recs = _run(tmp_path, "inline", eval_mode="inline", eval_every=1, eval_envs=12)
    ev = [r for r in recs if "eval_iteration" in r]
    assert [r["eval_iteration"] for r in ev] == [1, 2, 3]          # one per iteration
    assert ev == w.eval_history
    for r in ev:
        assert set(r) == {"eval_iteration", "eval_return_mean", "eval_return_std", "eval_return_min",
                          "eval_return_max", "eval_length_mean", "eval_episodes"}
        assert all(math.isfinite(float(v)) for v in r.values())
        assert r["eval_episodes"] == 12
        assert r["eval_return_min"] <= r["eval_return_mean"] <= r["eval_return_max"]
        assert 1 <= r["eval_length_mean"] <= 40
    # the per-iteration records are untouched by the evaluation records
    its = [r for r in recs if "eval_iteration" not in r]
    assert len(its) == 3 and not any(k.startswith("eval_") for r in its for k in r)
    # the last record is what the engine's evaluate gives for the final parameters
    ret, ln = w.engine.evaluate(12, False)
    assert ev[-1]["eval_return_mean"] == pytest.approx(float(ret.double().mean()), rel=1e-12)
    assert ev[-1]["eval_length_mean"] == pytest.approx(float(ln.double().mean()), rel=1e-12)
    w0, _, recs0 = _run(tmp_path, "plain", eval_every=0)
    assert not any("eval_iteration" in r for r in recs0) and w0.eval_history == []
    assert torch.equal(w.model.flat.data, w0.model.flat.data)      # evaluation changes no training state
    assert torch.equal(w.stats.mean, w0.stats.mean) and torch.equal(w.env.state, w0.env.state)
    assert "episode reward" not in capsys.readouterr().out         # quiet


def test_inline_eval_prints_reference_line(tmp_path, capsys):
    from pytorch_dppo_amd.runtime.launcher import run_worker
    p = dppo_preset(env_name="Pendulum-v0", num_envs=4, exploration_size=16, batch_size=16, num_epoch=1,
                    max_episode_length=10, eval_mode="inline", eval_every=2, eval_envs=3, log_every=0)
    w, _ = run_worker(p, DistContext(), max_iters=4)
    lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith("Time ")]
    assert len(lines) == 2 and [r["eval_iteration"] for r in w.eval_history] == [2, 4]
    assert all(", episode reward " in l and ", episode length " in l for l in lines)


def test_eval_config_validation():
    p = Params()
    assert (p.eval_mode, p.eval_envs, p.eval_deterministic) == ("process", 256, False)
    with pytest.raises(ValueError, match="eval_mode"):
        Params(eval_mode="gpu")
    with pytest.raises(ValueError, match="gym"):
        Params(eval_mode="inline", env_backend="gym")
    with pytest.raises(ValueError, match="eval_envs"):
        Params(eval_mode="inline", eval_envs=0)
    q = Params.from_dict({**p.to_dict(), "eval_mode": "inline", "eval_envs": 45, "eval_deterministic": True})
    assert (q.eval_mode, q.eval_envs, q.eval_deterministic) == ("inline", 45, True)
    from pytorch_dppo_amd.config import params_from_args
    a = params_from_args(["--eval-mode", "inline", "--eval-envs", "1024", "--eval-every", "5", "--eval-deterministic"])
    assert (a.eval_mode, a.eval_envs, a.eval_every, a.eval_deterministic) == ("inline", 1024, 5, True)
