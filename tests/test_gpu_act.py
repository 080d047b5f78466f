"""Policy inference on the GPU (csrc/act.hip, HipEngine.act, host_policy="kernel", PolicyRunner)
against its torch twin (ops/oracle.policy_act; tests/test_act_twin.py pins the twin itself to the
torch engine on the CPU).

Every test: ``log_std = -0.3`` (as test_gpu_kernels.py test_rollout_matches_torch_engine), stats
observed from random data with per-feature scales and offsets, observations with entries beyond
5 sigma so the clamp is exercised.  Tolerances are the project's rollout tolerances
(tests/test_gpu_kernels.py: fp32 / bf16x3 atol 2e-4 rtol 1e-4; bf16 max < 5e-2, mean < 5e-3; fp8 mean
action error < 0.05; logp atol 1e-4 rtol 1e-5 for every dtype: it depends only on the noise).
"""
import math

import numpy as np
import pytest
import torch

from pytorch_dppo_amd.config import dppo_preset
from pytorch_dppo_amd.envs import get_spec, make_vec_env, register_env
from pytorch_dppo_amd.models.actor_critic import ActorCritic
from pytorch_dppo_amd.ops import oracle
from pytorch_dppo_amd.parallel.dist import DistContext
from pytorch_dppo_amd.utils.obs_stats import RunningObsStats

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0) if torch.cuda.is_available() else None
DTYPES = ["fp32", "bf16x3", "bf16", "fp8"]
SHAPES = [(1, 3, 1),        # serving one row; one odd action dim = half a Box-Muller pair; d1 = 32
          (13, 5, 2),       # one partial tile
          (45, 17, 6),      # two full tiles and a tail
          (16, 376, 17)]    # Humanoid widths, odd A
STEP_KEY = 12345


def _data(E, O, n=1):
    """(stat-seeding batch, n observation batches [E,O]) with per-feature scales / offsets and, per
    batch, entries beyond 5 sigma at both ends"""
    g = torch.Generator().manual_seed(1000 * E + O)
    scale = 0.5 + 3.0 * torch.rand(O, generator=g)
    offs = torch.randn(O, generator=g)
    seed_batch = torch.randn(256, O, generator=g) * scale + offs
    out = []
    for _ in range(n):
        obs = torch.randn(E, O, generator=g) * scale + offs
        obs[0, 0] = offs[0] + 9.0 * scale[0]
        obs[E - 1, O - 1] = offs[O - 1] - 9.0 * scale[O - 1]
        out.append(obs.to(DEV))
    return seed_batch.to(DEV), out


def _engine(O, A, dtype, num_envs=16, **kw):
    from pytorch_dppo_amd.runtime.engine_hip import HipEngine
    kw.setdefault("env_name", f"Synthetic-{O}x{A}")
    p = dppo_preset(device="gpu", num_envs=num_envs, exploration_size=num_envs * 4, batch_size=num_envs * 4,
                    dtype=dtype, **kw)
    spec = get_spec(p.env_name)
    torch.manual_seed(0)
    model = ActorCritic(O, A).to(DEV)
    env = make_vec_env(spec, p.num_envs, seed=p.seed, device=DEV)
    stats = RunningObsStats(O, DEV)
    eng = HipEngine(p, model, env, stats, DEV, 0)
    with torch.no_grad():
        model.flat.data[:A] = -0.3
    eng.params_changed()
    return eng, model, env, stats


_TWIN = {}


def _twin(shape, eng, model, stats, obs, e_base, det):
    """the twin's outputs, computed once per (shape, e_base, rule) and shared by the dtypes (the
    seeded snapshot is the same for all of them: checked)"""
    key = (shape, e_base, det)
    if key not in _TWIN:
        E = obs.shape[0]
        out = oracle.policy_act(model, stats, obs, eng.key_action, torch.arange(E, device=DEV) + e_base, STEP_KEY,
                                "std", det)
        _TWIN[key] = tuple(t.clone() for t in out) + (model.flat.data.clone(), stats.mean_f32.clone(), obs.clone())
    a, logp, mu, x, flat, mean, o = _TWIN[key]
    assert torch.equal(flat, model.flat.data) and torch.equal(mean, stats.mean_f32) and torch.equal(o, obs)
    return a, logp, mu, x


def _assert_close(got, want, dtype, what, lowp=None):
    """the rollout tests' tolerance of ``dtype`` (``lowp``: the dtype whose bound applies to a
    quantity stored in another precision: fp8's bf16 buffer rows)"""
    d = (got - want).abs()
    print(f"{what} {dtype}: max {d.max().item():.3e} mean {d.mean().item():.3e}")
    kind = lowp or dtype
    if kind in ("fp32", "bf16x3"):
        assert torch.allclose(got, want, atol=2e-4, rtol=1e-4), what
    elif kind == "bf16":
        assert d.max().item() < 5e-2 and d.mean().item() < 5e-3, (what, d.max().item(), d.mean().item())
    else:
        assert d.mean().item() < 0.05, (what, d.mean().item())


def _x_bufs(eng, rows):
    return torch.zeros(rows, eng.d0, dtype=eng.sdtype, device=DEV)


# ---- 1. act against the twin ----------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_act_matches_twin(shape, dtype):
    E, O, A = shape
    eng, model, env, stats = _engine(O, A, dtype)
    seed_batch, (obs,) = _data(E, O)
    stats.observes(seed_batch)
    closed = -float(model.view("log_std").detach().sum()) - 0.5 * A * oracle.LOG_2PI
    for e_base in (0, 1000):
        a_t, logp_t, mu_t, x_t = _twin(shape, eng, model, stats, obs, e_base, False)
        assert bool((x_t.abs() == 5.0).any())            # the clamp is exercised
        x_out = _x_bufs(eng, E)
        a, logp, mu = eng.act(obs, STEP_KEY, False, e_base, x_out=x_out)
        assert a.shape == (E, A) and logp.shape == (E,) and mu.shape == (E, A) and a.device.type == "cuda"
        _assert_close(a, a_t, dtype, "actions")
        _assert_close(mu, mu_t, dtype, "mu")
        assert torch.allclose(logp, logp_t, atol=1e-4, rtol=1e-5)
        x = eng.decode(x_out)
        _assert_close(x[:, :O], x_t, dtype, "x", lowp="bf16" if dtype == "fp8" else None)
        assert bool((x[:, O] == 1.0).all()) and bool((x[:, O + 1:] == 0.0).all())
        # deterministic: the action IS this launch's mu; eps = 0 in the log-prob
        a_d, logp_d, mu_d = (t.clone() for t in eng.act(obs, STEP_KEY, True, e_base))
        assert torch.equal(a_d, mu_d) and torch.equal(mu_d, mu)
        print(f"deterministic logp gap {dtype}: {(logp_d - closed).abs().max().item():.3e}")
        assert torch.allclose(logp_d, torch.full_like(logp_d, closed), atol=1e-6, rtol=0)
    # e_base reaches the key: other rows' noise
    assert not torch.equal(_twin(shape, eng, model, stats, obs, 0, False)[0],
                           _twin(shape, eng, model, stats, obs, 1000, False)[0])


# ---- 1b. act on the rollout's own observations IS the rollout's first step -------------------------
def first_step_pair(eng, env, stats):
    """((buffer rows, actions, logp) of a T = 1 rollout launch from the env's current state, the same
    three from act() on that state's observations with the rollout's keys)"""
    E = eng.E
    obs = env.observe().to(DEV, torch.float32).clone()
    t0 = env.t
    eng.refresh_fwd_image()
    eng._launch_rollout(1, 0, t0, stats, stats.shift())
    torch.cuda.synchronize()
    roll = (eng.x_buf[:E].clone(), eng.actions[:E].clone(), eng.logp[:E].clone())
    x_out = _x_bufs(eng, E)
    a, logp, _ = eng.act(obs, step_key=t0, e_base=0, key_action=eng.key_action, x_out=x_out)
    torch.cuda.synchronize()
    return roll, (x_out, a.clone(), logp.clone())


@pytest.mark.parametrize("dtype", DTYPES)
def test_act_reproduces_rollout_first_step(dtype):
    """csrc/act.hip and csrc/rollout.hip run the same policy step (csrc/policy_step.h), so from one
    env state (two whole 16-env tiles and one of 8) the row block and the actions agree bit for bit.
    The log-prob is held to test_act_matches_twin's logp tolerance: measured 4.8e-7 (one ulp) apart
    in all four precisions, and the same between the two kernels before they shared the step's
    code.  (The rollout sums it in a loop it shares with the reward's error term; floating-point
    contraction there is the likely difference, not verified in the ISA.)"""
    E, O, A = 40, 17, 6
    eng, model, env, stats = _engine(O, A, dtype, num_envs=E)
    stats.observes(env.observe().to(DEV, torch.float32) * 3.0)    # stats near the env's own observations
    roll, act = first_step_pair(eng, env, stats)
    assert int(env.ep_len.max()) == 1                             # the rollout did step the envs
    for name, r, a in zip(("x rows", "actions", "logp"), roll, act):
        assert r.shape == a.shape and r.shape[0] == E
        if name == "logp":
            print(f"logp gap {dtype}: {(r - a).abs().max().item():.3e}")
            assert torch.allclose(a, r, atol=1e-4, rtol=1e-5)
        else:
            assert torch.equal(r.view(torch.uint8), a.view(torch.uint8)), (name, dtype)


# ---- 2. nothing outside the outputs moves ---------------------------------------------------------
@pytest.mark.parametrize("dtype", ["bf16x3", "fp8"])
def test_act_writes_only_its_outputs(dtype):
    E, O, A = 45, 17, 6
    eng, model, env, stats = _engine(O, A, dtype)
    seed_batch, (obs,) = _data(E, O)
    stats.observes(seed_batch)
    nblk, TILE = (E + 15) // 16, 16
    f32 = dict(dtype=torch.float32, device=DEV)
    outs = {"actions": torch.zeros(E + TILE, A, **f32), "logp": torch.zeros(E + TILE, **f32),
            "mu": torch.zeros(E + TILE, A, **f32), "x_out": _x_bufs(eng, E + TILE),
            "mom": torch.zeros(nblk + 1, 2, O, **f32)}
    for t in outs.values():
        t.view(torch.uint8).fill_(0x5A)                       # canary bytes
    eng._launch_act(obs, STEP_KEY, False, 0, eng.key_action, stats, stats.shift(), outs["actions"], outs["logp"],
                    outs["mu"], outs["x_out"], outs["mom"], True)
    torch.cuda.synchronize()
    for name, t in outs.items():
        n = nblk if name == "mom" else E
        assert bool((t[n:].view(torch.uint8) == 0x5A).all()), name
        assert not bool((t[:n].reshape(n, -1).view(torch.uint8) == 0x5A).all(1).any()), name   # every row written
    a, logp, mu = eng.act(obs, STEP_KEY)
    assert torch.equal(a, outs["actions"][:E]) and torch.equal(logp, outs["logp"][:E]) and torch.equal(mu, outs["mu"][:E])


@pytest.mark.parametrize("dtype", ["bf16x3", "fp8"])
def test_engine_act_leaves_training_state_untouched(dtype):
    E, O, A = 45, 17, 6
    eng, model, env, stats = _engine(O, A, dtype)
    seed_batch, (obs,) = _data(E, O)
    stats.observes(seed_batch)
    eng.rollout()            # non-trivial env state, step counter, buffers
    state = {"model.flat": model.flat.data, "wimg": eng.wimg, "wimg_fwd": eng.wimg_fwd, "stats.mean": stats.mean,
             "stats.mean_diff": stats.mean_diff, "stats.mean_f32": stats.mean_f32, "stats.inv_std_f32": stats.inv_std_f32,
             "x_buf": eng.x_buf, "actions": eng.actions, "logp": eng.logp, "rewards": eng.rewards, "dones": eng.dones,
             "mom": eng.mom, "env.state": env.state, "ep_len": env.ep_len, "ep_ret": env.ep_ret,
             "adam_m": eng.adam_m, "adam_v": eng.adam_v, "adam_state": eng.adam_state}
    before = {k: v.clone() for k, v in state.items()}
    t_before, n_before = env.t, stats.n
    first = tuple(t.clone() for t in eng.act(obs))
    second = eng.act(obs)
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(first, second))     # deterministic
    assert all(bool(torch.isfinite(t).all()) for t in second)
    eng.act(obs, deterministic=True)
    torch.cuda.synchronize()
    for k, v in state.items():
        assert torch.equal(v, before[k]), k
    assert env.t == t_before and stats.n == n_before


# ---- 3. moments -----------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_act_moments_and_rows_only(dtype):
    E, O, A = 45, 17, 6
    eng, model, env, stats = _engine(O, A, dtype)
    seed_batch, batches = _data(E, O, n=3)
    stats.observes(seed_batch)
    nblk = (E + 15) // 16
    mom = torch.full((nblk, 2, O), float("nan"), device=DEV)      # mom_init overwrites
    x_full = _x_bufs(eng, E)
    eng.act(batches[0], STEP_KEY, mom=mom, mom_init=True, x_out=x_full)
    eng.act(batches[1], STEP_KEY, mom=mom)
    eng.act(batches[2], STEP_KEY, mom=mom)
    s12 = torch.zeros(2, O, dtype=torch.float64, device=DEV)
    eng.ext.obs_reduce(mom, nblk, O, s12, torch.zeros(nblk, 2, device=DEV), torch.zeros(2, dtype=torch.float64, device=DEV))
    c, s1, s2 = RunningObsStats.moments(torch.cat(batches), stats.shift())
    assert c == 3 * E
    print("s1 gap", float((s12[0] - s1).abs().max()), "s2 gap", float((s12[1] - s2).abs().max()))
    assert torch.allclose(s12[0], s1, rtol=1e-4, atol=1e-2)
    assert torch.allclose(s12[1], s2, rtol=1e-4, atol=1e-4 * (s2.abs().max().item() + 1.0))
    # rows-only: no MLP outputs requested -> x_out (the full form's, bit for bit), mom untouched
    mom_before = mom.clone()
    x_rows = _x_bufs(eng, E)
    none = eng.no_q
    eng._launch_act(batches[0], STEP_KEY, False, 0, eng.key_action, stats, stats.shift(), none, none, none, x_rows,
                    none, False)
    torch.cuda.synchronize()
    assert torch.equal(x_rows, x_full) and torch.equal(mom, mom_before)
    # ... and with mom it accumulates there too
    eng._launch_act(batches[0], STEP_KEY, False, 0, eng.key_action, stats, stats.shift(), none, none, none, x_rows,
                    mom, True)
    only = torch.zeros_like(mom)
    eng.act(batches[0], STEP_KEY, mom=only, mom_init=True)
    assert torch.equal(mom, only)


# ---- 4. host rollout on the kernel ------------------------------------------------------------------
class _Box:
    def __init__(self, n):
        self.shape = (n,)


class _Spec:
    max_episode_steps = 12


class FakeGymNoTermEnv:
    """tests/test_gym_backend.py FakeGymEnv without its state-dependent terminal (time limit 12
    only; noise from its own seeded RandomState): the done flags do not depend on the actions"""
    O, A = 5, 2

    def __init__(self):
        self.observation_space = _Box(self.O)
        self.action_space = _Box(self.A)
        self.spec = _Spec()
        self.rs = np.random.RandomState(0)
        self.s = np.zeros(self.O)

    def seed(self, s):
        self.rs = np.random.RandomState(s)

    def reset(self):
        self.s = self.rs.randn(self.O) * 0.5
        return self.s.astype(np.float32)

    def step(self, a):
        a = np.asarray(a, dtype=np.float64)
        r = -float(((a - np.tanh(self.s[:self.A])) ** 2).sum())
        drive = np.zeros(self.O)
        drive[:self.A] = np.tanh(a)
        self.s = 0.9 * self.s + 0.1 * drive + 0.05 * self.rs.randn(self.O)
        return self.s.astype(np.float32), r, False, {}


register_env("FakeGymNoTerm-v0", FakeGymNoTermEnv)


def _host_params(dtype, **kw):
    return dppo_preset(device="gpu", env_backend="gym", env_name="FakeGymNoTerm-v0", num_envs=16,
                       exploration_size=16 * 8, batch_size=16 * 8, num_epoch=2, dtype=dtype, seed=3, **kw)


@pytest.mark.parametrize("dtype", ["fp32", "bf16x3"])
def test_host_rollout_kernel_matches_torch_path(dtype):
    from pytorch_dppo_amd.runtime.engine_hip import HipEngine
    res = {}
    for policy in ("kernel", "torch"):
        p = _host_params(dtype, host_policy=policy)
        torch.manual_seed(0)
        model = ActorCritic(5, 2).to(DEV)
        with torch.no_grad():
            model.flat.data[:2] = -0.3
        env = make_vec_env(None, p.num_envs, seed=p.seed, backend="gym", name=p.env_name)
        st = RunningObsStats(5, DEV)
        eng = HipEngine(p, model, env, st, DEV, 0)
        st.observes(eng.current_obs() * 0.1)           # narrow stats: some observations beyond 5 sigma
        ro = eng.rollout()
        assert set(ro) == {"count", "s1", "s2", "shift", "ep_return_sum", "ep_count", "ep2"}
        res[policy] = (eng, ro)
    (k, ro_k), (t, ro_t) = res["kernel"], res["torch"]
    T, E = k.T, k.E
    assert (T, E) == (8, 16) and k.env.t == t.env.t == 8
    _assert_close(k.actions, t.actions, dtype, "actions")
    assert torch.allclose(k.logp, t.logp, atol=1e-4, rtol=1e-5)
    xk, xt = k.decode(k.x_buf), t.decode(t.x_buf)
    assert bool((xt.abs() == 5.0).any())
    _assert_close(xk, xt, dtype, "x_buf")              # all T + 1 rows, pad columns included
    assert torch.equal(k.dones, t.dones) and int(k.dones.sum()) == 0
    _assert_close(k.rewards, t.rewards, dtype, "rewards")
    assert ro_k["count"] == ro_t["count"] == float(T * E)
    assert torch.allclose(ro_k["s1"], ro_t["s1"], rtol=1e-4, atol=1e-2)
    assert torch.allclose(ro_k["s2"], ro_t["s2"], rtol=1e-4, atol=1e-4 * (ro_t["s2"].abs().max().item() + 1.0))
    assert torch.equal(ro_k["shift"], ro_t["shift"])
    assert float(ro_k["ep_count"]) == float(ro_t["ep_count"])


@pytest.mark.parametrize("dtype,obs_norm", [("bf16x3", "rollout"), ("bf16x3", "step"), ("fp8", "rollout")])
def test_worker_trains_on_host_kernel_policy(dtype, obs_norm):
    from pytorch_dppo_amd.runtime.worker import DPPOWorker
    p = _host_params(dtype, host_policy="kernel", obs_norm_update=obs_norm)
    w = DPPOWorker(p, DistContext(device=DEV))
    m = w.iteration_step()
    assert math.isfinite(m["loss"]) and m["updates"] == p.num_epoch
    assert w.env.t == 8 and bool(torch.isfinite(w.model.flat.data).all())


# ---- 5. PolicyRunner on the GPU ---------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["bf16x3", "bf16"])
def test_policy_runner_gpu(dtype, tmp_path):
    from pytorch_dppo_amd.runtime.launcher import run_worker
    from pytorch_dppo_amd.runtime.policy import PolicyRunner
    p = dppo_preset(device="gpu", env_name="HalfCheetah-v2", num_envs=16, exploration_size=16 * 4, batch_size=16 * 4,
                    num_epoch=2, dtype=dtype, seed=4, checkpoint_dir=str(tmp_path), log_every=0)
    w, _ = run_worker(p, DistContext(device=DEV), max_iters=1, quiet=True)
    gpu = PolicyRunner.from_checkpoint(str(tmp_path), device="gpu")
    cpu = PolicyRunner.from_checkpoint(str(tmp_path), device="cpu")
    assert gpu.dtype == dtype and (gpu.O, gpu.A) == (17, 6) and not hasattr(gpu, "engine")
    _, batches = _data(13, 17, n=3)
    for call, obs in enumerate(batches):
        a, logp = gpu.act(obs)
        assert gpu.step == call + 1 and a.device.type == "cuda"
        ea, el, _ = w.engine.act(obs, step_key=call, key_action=gpu.key_action)
        assert torch.equal(a, ea) and torch.equal(logp, el)
        ca, cl = cpu.act(obs.cpu())
        _assert_close(a.cpu(), ca, dtype, "runner actions")
        assert torch.allclose(logp.cpu(), cl, atol=1e-4, rtol=1e-5)
    with pytest.raises(ValueError, match="fp8"):
        PolicyRunner.from_checkpoint(str(tmp_path), device="gpu", dtype="fp8")
