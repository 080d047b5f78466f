"""Categorical policies on the CPU (docs/ARCHITECTURE.md §27): the oracle (ops/oracle.py categorical_*, ppo_loss /
policy_act with dist="categorical") against scalar float64 arithmetic, the keyed Gumbel-max sample, the discrete
cart-pole ``CartPole-v1``, the torch engine, the runner, the refusals and that training learns.
tests/test_gpu_categorical.py holds the GPU engine and the two kernels to the same oracle."""
import math

import pytest
import torch

from pytorch_dppo_amd.config import Params, dppo_preset
from pytorch_dppo_amd.envs import CartPoleContinuousEnv, VecEnv, get_spec, make_vec_env, register_tensor_env
from pytorch_dppo_amd.envs.registry import KIND_TENSOR, EnvSpec
from pytorch_dppo_amd.models.actor_critic import ActorCritic
from pytorch_dppo_amd.ops import oracle
from pytorch_dppo_amd.parallel.dist import DistContext
from pytorch_dppo_amd.runtime.engine import check_discrete
from pytorch_dppo_amd.runtime.evaluator import evaluate_batch, run_episode
from pytorch_dppo_amd.utils import rng
from pytorch_dppo_amd.utils.obs_stats import RunningObsStats

CARTPOLE = "CartPole-v1"

# ---- the oracle against scalar float64 arithmetic --------------------------------------------------------------
# rows of (logits, chosen action, logp_old, advantage): K = 2, K = 3, and one logit 40 above the rest
TABLE = {
    "K2": [([0.3, -0.2], 0, -0.60, 1.5), ([-1.0, 0.5], 1, -0.10, -0.7), ([0.0, 0.0], 1, -0.80, 0.4)],
    "K3": [([0.2, -0.4, 1.1], 2, -0.70, 0.9), ([1.5, 1.5, -2.0], 0, -0.50, -1.2), ([0.1, 0.0, -0.1], 1, -1.30, 2.0),
           ([-3.0, 0.5, 0.4], 1, -0.75, -0.3)],
    "sat": [([40.0, 0.0, 0.0, 0.0], 0, -0.01, 1.0), ([0.0, 41.5, 1.5, 0.5], 1, 0.0, -2.0),
            ([0.0, 40.0, 0.0, 0.0], 2, -39.0, 0.5)],
}
CLIP, ENT = 0.2, 0.01


def _scalar_row(z, a, lpo, adv):
    """one row in python floats: (logp, H, p, clipped surrogate term, dL_row/dz without the 1/B)"""
    m = max(z)
    lse = m + math.log(sum(math.exp(x - m) for x in z))
    p = [math.exp(x - lse) for x in z]
    logp = z[a] - lse
    H = lse - sum(pk * x for pk, x in zip(p, z))
    ratio = math.exp(logp - lpo)
    s1, s2 = ratio * adv, min(max(ratio, 1.0 - CLIP), 1.0 + CLIP) * adv
    dlogp = -adv * ratio if s1 <= s2 else 0.0
    dz = [dlogp * ((1.0 if k == a else 0.0) - p[k]) + ENT * p[k] * ((z[k] - lse) + H) for k in range(len(z))]
    return logp, H, p, -min(s1, s2), dz, ratio


def _tensors(rows, dtype):
    z = torch.tensor([r[0] for r in rows], dtype=dtype)
    o = torch.zeros_like(z)
    o[torch.arange(len(rows)), torch.tensor([r[1] for r in rows])] = 1.0
    return z, o, torch.tensor([r[2] for r in rows], dtype=dtype), torch.tensor([r[3] for r in rows], dtype=dtype)


@pytest.mark.parametrize("name", list(TABLE))
@pytest.mark.parametrize("dtype,tol", [(torch.float64, 1e-12), (torch.float32, 2e-6)])
def test_oracle_matches_scalar_table(name, dtype, tol):
    """tolerances: float64 arithmetic in another order (1e-12); fp32: logits up to 41.5 carry 2^-24 * 41.5 = 2.5e-6
    absolute in lse, held relative to max(1, |want|)"""
    rows = TABLE[name]
    B = len(rows)
    ref = [_scalar_row(*r) for r in rows]
    z, o, lpo, adv = _tensors(rows, dtype)
    z.requires_grad_(True)
    close = lambda got, want, t=tol: abs(float(got.detach()) - want) <= t * max(1.0, abs(want))   # noqa: E731
    logp = oracle.categorical_logp(o, z)
    H = oracle.categorical_entropy(z)
    assert logp.shape == (B, 1) and H.shape == (B,)
    for i in range(B):
        assert close(logp[i, 0], ref[i][0]) and close(H[i], ref[i][1]), (i, float(logp[i, 0]), float(H[i]), ref[i][:2])
    assert bool(torch.isfinite(logp).all()) and bool(torch.isfinite(H).all()) and bool((H >= 0).all())
    if name == "sat":
        assert float(H.detach().max()) < 1e-14          # H -> 0: 3 * e^-40 * 40 = 5e-16
    v = torch.zeros(B, dtype=dtype)
    log_std = torch.zeros(z.shape[1], dtype=dtype, requires_grad=True)
    out = oracle.ppo_loss(z, log_std, v, o, lpo, adv, v, v, clip=CLIP, ent_coeff=ENT, dist="categorical")
    assert close(out["loss_clip"], sum(r[3] for r in ref) / B)
    assert close(out["loss_ent"], -ENT * sum(r[1] for r in ref) / B)
    assert close(out["clipfrac"], sum(abs(r[5] - 1.0) > CLIP for r in ref) / B, 1e-6)     # (an fp32 mean of 0 / 1)
    assert close(out["approx_kl"], sum((r[5] - 1.0) - math.log(r[5]) for r in ref) / B)
    # autograd of the loss against the closed form dL/dz_k = dlogp (o_k - p_k) + c p_k ((z_k - lse) + H)
    gz, gls = torch.autograd.grad(out["loss"], [z, log_std], allow_unused=True)
    assert gls is None or bool((gls == 0).all())          # log_std is unread
    assert bool(torch.isfinite(gz).all())
    gscale = max(1.0, max(abs(x) for r in ref for x in r[4]))
    for i in range(B):
        for k in range(z.shape[1]):
            assert abs(float(gz[i, k]) * B - ref[i][4][k]) <= tol * gscale, (i, k, float(gz[i, k]) * B, ref[i][4][k])


def test_ppo_loss_and_policy_act_defaults_are_gaussian():
    torch.manual_seed(0)
    mu, a = torch.randn(5, 3), torch.randn(5, 3)
    ls, v = torch.randn(3) * 0.1, torch.randn(5)
    kw = dict(clip=0.2, ent_coeff=0.01)
    d0 = oracle.ppo_loss(mu, ls, v, a, v, v, v, v, **kw)
    d1 = oracle.ppo_loss(mu, ls, v, a, v, v, v, v, dist="gaussian", **kw)
    assert all(torch.equal(d0[k], d1[k]) for k in d0)
    with pytest.raises(ValueError, match="dist"):
        oracle.ppo_loss(mu, ls, v, a, v, v, v, v, dist="softmax", **kw)


# ---- sampling -------------------------------------------------------------------------------------------------
def test_gumbel_is_finite_at_every_bucket_end():
    """uniform01 keeps 24 bits; its lowest bucket gives g = -log(17.33), the top ones (whose u rounds to 1 in fp32)
    are held at -log(2^-25) = 17.33"""
    b = torch.tensor([0, 1, 2, (1 << 23) - 1, 1 << 23, (1 << 24) - 3, (1 << 24) - 2, (1 << 24) - 1], dtype=torch.int64)
    u = rng.uniform01(b << 8)
    assert float(u[-1]) == 1.0                   # the reason for the clamp
    g = -torch.log(torch.clamp_min(-torch.log(u), rng.GUMBEL_E_MIN))
    assert bool(torch.isfinite(g).all())
    assert float(g.min()) == pytest.approx(-math.log(-math.log(0.5 / (1 << 24))), abs=1e-5)
    assert float(g.max()) == pytest.approx(25.0 * math.log(2.0), abs=1e-5)
    # the keyed function is that expression, finite over many hashes, and fp32
    env = torch.arange(4096)[:, None]
    dims = torch.arange(16)[None, :]
    gk = rng.gumbel(77, env, 5, dims)
    uk = rng.uniform01(rng.keyed(77, env, 5, dims))
    assert gk.dtype == torch.float32 and bool(torch.isfinite(gk).all())
    assert torch.equal(gk, -torch.log(torch.clamp_min(-torch.log(uk), rng.GUMBEL_E_MIN)))


def test_categorical_sample_ties_and_deterministic():
    z = torch.tensor([[0.0, 0.0, 0.0], [1.0, 2.0, 2.0], [-1.0, -5.0, -1.0], [3.0, 1.0, 2.0]])
    a, o, lp = oracle.categorical_sample(z, 9, torch.arange(4), 0, deterministic=True)
    assert a.dtype == torch.int64 and a.tolist() == [0, 1, 0, 0]          # ties: the lowest index
    assert torch.equal(o, torch.nn.functional.one_hot(a, 3).float())
    assert torch.allclose(lp, torch.log_softmax(z, -1)[torch.arange(4), a], atol=1e-6)
    torch.manual_seed(3)
    z = torch.randn(64, 5)
    a, o, lp = oracle.categorical_sample(z, 9, torch.arange(64), 0, deterministic=True)
    assert torch.equal(a, z.argmax(1))
    # sampled: the arg-max of z + g, g the keyed noise
    a, o, lp = oracle.categorical_sample(z, 9, torch.arange(64), 7)
    g = rng.gumbel(9, torch.arange(64)[:, None], 7, torch.arange(5)[None, :])
    assert torch.equal(a, (z + g).argmax(1)) and not torch.equal(a, z.argmax(1))
    assert bool((o.sum(1) == 1).all()) and torch.equal(o.argmax(1), a)
    # equal perturbed values: the lowest index too (the same noise in two columns needs the same key, so force it)
    z2 = torch.zeros(8, 4)
    g2 = rng.gumbel(9, torch.arange(8)[:, None], 1, torch.arange(4)[None, :])
    z2[:, 3] = (g2.max(1).values - g2[:, 3])              # column 3 ties the best of the others or beats it
    a2 = oracle.categorical_sample(z2, 9, torch.arange(8), 1)[0]
    s2 = z2 + g2
    for i in range(8):
        assert int(a2[i]) == min(k for k in range(4) if float(s2[i, k]) == float(s2[i].max()))


def test_sample_frequencies_match_softmax():
    """2^16 keyed draws of fixed logits: every frequency within 5 standard errors of softmax"""
    N = 1 << 16
    z = torch.tensor([0.5, -1.0, 2.0, 0.0, -3.0])
    p = torch.softmax(z.double(), 0)
    for step in (0, 123):
        a = oracle.categorical_sample(z.expand(N, 5), 4242, torch.arange(N), step)[0]
        f = torch.bincount(a, minlength=5).double() / N
        se = (p * (1 - p) / N).sqrt()
        assert bool(((f - p).abs() <= 5 * se).all()), (f.tolist(), p.tolist())


# ---- env, registry ----------------------------------------------------------------------------------------------
def test_spec_and_registry():
    spec = get_spec(CARTPOLE)
    assert (spec.obs_dim, spec.act_dim, spec.kind, spec.time_limit, spec.discrete) == (4, 2, KIND_TENSOR, 500, True)
    assert get_spec("CartPoleContinuous-v1").discrete is False and get_spec("Pendulum-v0").discrete is False
    assert EnvSpec("x", 1, 1, 0, 1).discrete is False            # the new field is last and defaults to False
    env = make_vec_env(spec, 3)
    assert type(env).__name__ == "CartPoleEnv" and isinstance(env, CartPoleContinuousEnv) and env.kernel_kind is None

    class Two(VecEnv):
        pass
    with pytest.raises(ValueError, match="at least 2 actions"):
        register_tensor_env("OneAction-v0", Two, obs_dim=2, act_dim=1, time_limit=5, discrete=True)
    s = register_tensor_env("TwoActions-v0", Two, obs_dim=2, act_dim=2, time_limit=5, discrete=True)
    assert s.discrete and get_spec("TwoActions-v0") is s
    assert not register_tensor_env("TwoActionsBox-v0", Two, obs_dim=2, act_dim=2, time_limit=5).discrete


def test_cartpole_agrees_with_continuous_fed_pm1():
    E = 33
    d = make_vec_env(get_spec(CARTPOLE), E, seed=7)
    c = make_vec_env(get_spec("CartPoleContinuous-v1"), E, seed=7)
    assert torch.equal(d.reset(), c.reset())
    g = torch.Generator().manual_seed(0)
    ended = 0
    for _ in range(40):
        a = torch.randint(0, 2, (E,), generator=g)
        od, rd, dd, _ = d.step(a)
        oc, rc, dc, _ = c.step((2.0 * a.float() - 1.0)[:, None])
        assert torch.equal(od, oc) and torch.equal(rd, rc) and torch.equal(dd, dc)
        ended += int(dd.sum())
    assert ended > 0 and torch.equal(d.ep_len, c.ep_len)
    # a force of +10 for index 1, -10 for index 0: the cart accelerates that way from rest
    d.state = torch.zeros(E, 4)
    new, _, _ = d._dynamics(torch.tensor([1, 0] * 16 + [1]), 0)
    assert bool((new[0::2, 1] > 0).all()) and bool((new[1::2, 1] < 0).all())
    # env_fused is refused for an env without an in-kernel twin, with the registry's message
    from pytorch_dppo_amd.envs.registry import kernel_kind_of
    with pytest.raises(ValueError, match="no in-kernel twin"):
        kernel_kind_of(d)


def test_gym_discrete_action_space_is_refused():
    from pytorch_dppo_amd.envs import gym_adapter

    class Space:
        def __init__(self, shape):
            self.shape = shape

    class FakeGym:
        observation_space = Space((4,))
        action_space = Space(())             # gym.spaces.Discrete

        def seed(self, s):
            pass
    gym_adapter.register_env("FakeDiscrete-v0", FakeGym)
    with pytest.raises(ValueError, match="Box action spaces only"):
        make_vec_env(None, 2, backend="gym", name="FakeDiscrete-v0")


# ---- engine and runner ----------------------------------------------------------------------------------------------
def _torch_engine(E=24, T=6, seed=3, **kw):
    from pytorch_dppo_amd.runtime.engine_torch import TorchEngine
    p = dppo_preset(env_name=CARTPOLE, num_envs=E, exploration_size=E * T, batch_size=E * T, hidden=(16, 16),
                    seed=seed, **kw)
    spec = get_spec(CARTPOLE)
    torch.manual_seed(seed)
    model = ActorCritic(spec.obs_dim, spec.act_dim, p.hidden)
    env = make_vec_env(spec, E, seed=seed)
    stats = RunningObsStats(spec.obs_dim)
    eng = TorchEngine(p, model, env, stats, torch.device("cpu"), 0)
    stats.observes(env.observe())
    return eng, model, env, stats


def test_policy_act_is_the_torch_engines_step():
    eng, model, env, stats = _torch_engine()
    T, E = eng.T, eng.E
    seen = []
    step = env.step

    def recording(a):
        seen.append((env.observe().clone(), env.t, a.clone()))
        return step(a)
    env.step = recording
    eng.rollout()
    assert len(seen) == T
    for t, (obs, k, idx) in enumerate(seen):
        a, logp, logits, x = oracle.policy_act(model, stats, obs, eng.key_action, env.env_idx, k, dist="categorical")
        assert torch.equal(a, eng.actions[t]) and torch.equal(logp, eng.logp[t]) and torch.equal(x, eng.x[t])
        assert idx.dtype == torch.int64 and idx.shape == (E,) and torch.equal(idx, a.argmax(1))   # the env got indices
        assert torch.equal(logp, torch.gather(logits, 1, idx[:, None]).squeeze(1) - (
            logits.max(1).values + torch.log(torch.exp(logits - logits.max(1, keepdim=True).values).sum(1))))
    rows = eng.actions.reshape(T * E, 2)
    assert bool(((rows == 0) | (rows == 1)).all()) and bool((rows.sum(1) == 1).all())          # one-hot rows
    assert len({tuple(r) for r in rows.tolist()}) == 2                                           # both actions taken
    assert bool((eng.logp < 0).all())
    # deterministic: the arg-max of the logits and its log-probability
    a, logp, logits, _ = oracle.policy_act(model, stats, seen[0][0], 1, env.env_idx, 0, deterministic=True,
                                           dist="categorical")
    assert torch.equal(a.argmax(1), logits.argmax(1))
    assert torch.allclose(logp, torch.log_softmax(logits, 1).max(1).values, atol=1e-6)


def _worker(max_iters, evaluator=False, **kw):
    from pytorch_dppo_amd.runtime.launcher import run_worker
    base = dict(env_name=CARTPOLE, num_envs=8, exploration_size=64, batch_size=32, num_epoch=2, hidden=(16, 16),
                seed=4, log_every=0)
    base.update(kw)
    return run_worker(dppo_preset(max_iters=max_iters, **base), DistContext(), evaluator=evaluator, quiet=True)[0]


def test_log_std_is_unchanged_by_training():
    w = _worker(2)
    torch.manual_seed(4)                       # the worker's initialisation (its seed, then the model)
    m0 = ActorCritic(4, 2, (16, 16))
    A = 2
    assert w.engine.discrete and w.engine.adam_step > 0
    assert torch.equal(w.model.view("log_std"), m0.view("log_std"))
    assert not torch.equal(w.model.flat.data, m0.flat.data)
    assert torch.equal(w.model.flat.data[:A], w.model.view("log_std").reshape(-1))
    assert bool((w.engine.grad_flat[:A] == 0).all()) and bool((w.engine.adam_m[:A] == 0).all())
    assert sorted(w.model.state_dict()) == sorted(m0.state_dict()) and "log_std" in w.model.state_dict()


def test_resume_continues_bit_identically(tmp_path):
    ck = str(tmp_path / "ck")
    w_full = _worker(3)
    _worker(2, checkpoint_dir=ck)
    w_res = _worker(3, resume=ck)
    assert w_res.iteration == 3 and w_res.engine.adam_step == w_full.engine.adam_step
    assert torch.equal(w_full.model.flat.data, w_res.model.flat.data)
    assert torch.equal(w_full.engine.adam_m, w_res.engine.adam_m) and torch.equal(w_full.engine.adam_v, w_res.engine.adam_v)
    assert torch.equal(w_full.env.state, w_res.env.state) and w_full.env.t == w_res.env.t
    assert torch.equal(w_full.stats.mean, w_res.stats.mean)


def test_play_runner_and_inline_eval(tmp_path, capsys):
    import play
    from pytorch_dppo_amd.runtime.policy import PolicyRunner
    ck = str(tmp_path / "ck")
    w = _worker(2, evaluator=True, checkpoint_dir=ck, eval_mode="inline", eval_every=1, eval_envs=6, max_episode_length=60)
    assert len(w.eval_history) >= 1 and all(1.0 <= e["eval_length_mean"] <= 60.0 for e in w.eval_history)
    r = PolicyRunner.from_checkpoint(ck, device="cpu")
    assert r.discrete and (r.O, r.A) == (4, 2)
    obs = 0.05 * torch.randn(5, 4)
    key = rng.base_key(4, rng.STREAM_EVAL, 0)
    for det in (False, True):
        a, logp = r.act(obs, deterministic=det, step_key=11)
        wa, wl, _, _ = oracle.policy_act(w.model, w.stats, obs, key, torch.arange(5), 11, "std", det, dist="categorical")
        assert a.dtype == torch.int64 and a.shape == (5,) and torch.equal(a, wa.argmax(1)) and torch.equal(logp, wl)
    out = play.main(["--checkpoint", ck, "--device", "cpu", "--episodes", "2"])
    env = make_vec_env(get_spec(CARTPOLE), 1, seed=4 + 7777, rank=0, device="cpu", max_episode_length=60)
    want = [run_episode(w.model, w.stats, env, key, "std") for _ in range(2)]
    assert out == want and all(1 <= length <= 60 for _, length in out)
    # evaluate_batch: the same loop, batched; deterministic is the arg-max policy
    ret, ln = evaluate_batch(w.model, w.stats, get_spec(CARTPOLE), 6, 4, 60, "std", True)
    assert torch.equal(ret, ln.float()) and int(ln.min()) >= 1


# ---- refusals -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw,match", [(dict(loss="dppo_ref"), "loss=dppo_ref"), (dict(compat=True), "compat"),
                                      (dict(dtype="fp8"), "dtype=fp8"), (dict(update_kernels="heads"), "update_kernels=heads"),
                                      (dict(env_backend="gym"), "env_backend=gym")])
def test_discrete_refusals(kw, match):
    from pytorch_dppo_amd.runtime.engine_torch import TorchEngine
    spec = get_spec(CARTPOLE)
    p = Params(env_name=CARTPOLE, **kw)
    with pytest.raises(ValueError, match=match) as e:
        check_discrete(p, spec)
    assert "discrete" in str(e.value) and CARTPOLE in str(e.value)
    # a continuous spec passes every one of them, and the check answers whether the policy is categorical
    assert check_discrete(p, get_spec("CartPoleContinuous-v1")) is False and check_discrete(p, None) is False
    assert check_discrete(Params(env_name=CARTPOLE), spec) is True
    # the engine is where it is called
    if "env_backend" not in kw and "dtype" not in kw:
        pp = dppo_preset(env_name=CARTPOLE, num_envs=4, exploration_size=16, batch_size=16, hidden=(8, 8), **kw)
        model = ActorCritic(4, 2, (8, 8))
        with pytest.raises(ValueError, match=match):
            TorchEngine(pp, model, make_vec_env(spec, 4), RunningObsStats(4), torch.device("cpu"), 0)


def test_worker_refuses_gym_backend_for_a_registered_discrete_env():
    from pytorch_dppo_amd.runtime.worker import DPPOWorker
    p = dppo_preset(env_name=CARTPOLE, env_backend="gym", num_envs=2, exploration_size=8, batch_size=8)
    with pytest.raises(ValueError, match="env_backend=gym"):
        DPPOWorker(p, DistContext())


# ---- learning -------------------------------------------------------------------------------------------------------
def test_dppo_learns_discrete_cartpole():
    """tests/test_tensor_env.py test_dppo_learns_cartpole's configuration and criterion on CartPole-v1: 12 CPU
    iterations at least triple the mean episode length (measured ratios at seeds 1-3: profiles/categorical/README.md)"""
    from pytorch_dppo_amd.runtime.worker import DPPOWorker
    torch.set_num_threads(2)
    p = dppo_preset(env_name=CARTPOLE, num_envs=32, exploration_size=2048, batch_size=512,
                    num_epoch=4, hidden=(32, 32), lr=3e-3, seed=1)
    w = DPPOWorker(p, DistContext())
    steps_per_episode = []
    for _ in range(12):
        w.iteration_step()
        steps_per_episode.append(p.buffer_rows / float(w.engine.dones.sum()))
    print("steps per episode:", [round(s, 1) for s in steps_per_episode])
    assert steps_per_episode[-1] >= 3.0 * steps_per_episode[0], steps_per_episode


# ---- the GPU gradient tests' fixtures (pure CPU preconditions) ----------------------------------------------------
import test_gpu_categorical as gpu_fixtures      # noqa: E402


@pytest.mark.parametrize("K,kind", gpu_fixtures.CANCEL_CASES)
def test_gradient_fixtures_have_no_cancelling_policy_block(K, kind):
    gpu_fixtures.check_no_policy_block_is_a_cancelling_sum(K, kind)
