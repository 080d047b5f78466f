"""Batched policy evaluation on the GPU (csrc/eval.hip, HipEngine.evaluate, eval_mode="inline")
against its torch twin (runtime/evaluator.py evaluate_batch; tests/test_eval_twin.py checks the
twin itself on the CPU).

Geometry unless stated otherwise: 45 envs = two full 16-env tiles + a 13-env tail, seed 1,
max_episode_length 96 (24 for Pendulum): 6 of the 45 HalfCheetah episodes end early, the rest at
the time limit, so the first-done freeze, the masked accumulation and the early workgroup exit
are all exercised.
"""
import json

import pytest
import torch

from pytorch_dppo_amd.config import dppo_preset
from pytorch_dppo_amd.envs import get_spec, make_vec_env
from pytorch_dppo_amd.models.actor_critic import ActorCritic
from pytorch_dppo_amd.parallel.dist import DistContext
from pytorch_dppo_amd.runtime.evaluator import eval_keys, evaluate_batch
from pytorch_dppo_amd.utils.obs_stats import RunningObsStats

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0) if torch.cuda.is_available() else None
E = 45


def _limit(env_name):
    return 24 if env_name.startswith("Pendulum") else 96


def _params(env_name, dtype, num_envs=E, **kw):
    kw.setdefault("max_episode_length", _limit(env_name))
    return dppo_preset(device="gpu", env_name=env_name, num_envs=num_envs, exploration_size=num_envs * 8,
                       batch_size=num_envs * 8, dtype=dtype, **kw)


def _engine(params, seed=0):
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
        model.flat.data[:model.num_outputs] = torch.linspace(-0.5, -0.1, model.num_outputs, device=DEV)
    eng.params_changed()
    return eng, model, env, stats


_TWIN = {}


def _twin(eng, model, stats, n, det):
    """the twin's (ret, len) for this snapshot: computed once per (env, network, count, rule) and
    shared by the dtypes (the seeded snapshot is the same for all of them: checked)"""
    p = eng.p
    key = (p.env_name, p.hidden, p.max_episode_length, n, bool(det))
    if key not in _TWIN:
        ret, ln = evaluate_batch(model, stats, get_spec(p.env_name), n, p.seed, p.max_episode_length,
                                 p.std_convention, det)
        _TWIN[key] = (ret.clone(), ln.clone(), model.flat.data.clone(), stats.mean_f32.clone())
    ret, ln, flat, mean = _TWIN[key]
    assert torch.equal(flat, model.flat.data) and torch.equal(mean, stats.mean_f32)
    return ret, ln


def _assert_matches(ret, ln, ret_t, ln_t):
    """test_rollout_matches_torch_engine's per-step reward tolerance (atol 2e-4, rtol 1e-4) summed
    over the episode"""
    assert ret.dtype == torch.float32 and ln.dtype == torch.int32
    assert torch.equal(ln, ln_t)
    bound = 2e-4 * ln_t.to(torch.float32) + 1e-4 * ret_t.abs()
    gap = (ret - ret_t).abs()
    print("max |ret - twin| / bound:", float((gap / bound).max()), "max gap", float(gap.max()))
    assert bool((gap <= bound).all())


@pytest.mark.parametrize("deterministic", [True, False])
@pytest.mark.parametrize("dtype", ["fp32", "bf16x3"])
@pytest.mark.parametrize("env_name", ["HalfCheetah-v2", "Humanoid-v2", "Pendulum-v0"])
def test_eval_matches_twin(env_name, dtype, deterministic):
    eng, model, env, stats = _engine(_params(env_name, dtype))
    ret_t, ln_t = _twin(eng, model, stats, E, deterministic)
    if not env_name.startswith("Pendulum"):
        # the oracle spans early terminations and time-limit ends (tests/test_eval_twin.py)
        assert int((ln_t < 96).sum()) >= 1 and int((ln_t == 96).sum()) >= 1 and len(set(ln_t.tolist())) >= 3
    ret, ln = eng.evaluate(E, deterministic)
    assert ret.device.type == "cuda" and ret.shape == (E,) and ln.shape == (E,)
    _assert_matches(ret, ln, ret_t, ln_t)


# mean over envs of |ret - ret_fp32_gpu| / len, measured once on an MI355X against the fp32 GPU
# evaluation of the same snapshot (profiles/eval/README.md); the test allows 3x (the run is
# deterministic: the margin absorbs compiler and box differences only)
LOWP_GAP_MEASURED = {"bf16": 1.537803e-05, "fp8": 2.512902e-04}


@pytest.mark.parametrize("dtype", ["bf16", "fp8"])
def test_eval_low_precision_tracks_fp32(dtype):
    """Humanoid-v2, deterministic, 45 envs, limit 96.  Measured on an MI355X (mean over envs of
    |ret - ret_fp32_gpu| / len): bf16 1.537803e-05, fp8 2.512902e-04; the bound is 3x that."""
    eng32, model32, _, stats32 = _engine(_params("Humanoid-v2", "fp32"))
    ret_t, ln_t = _twin(eng32, model32, stats32, E, True)
    ret32, ln32 = eng32.evaluate(E, True)
    eng, model, _, stats = _engine(_params("Humanoid-v2", dtype))
    assert torch.equal(model.flat.data, model32.flat.data) and torch.equal(stats.mean_f32, stats32.mean_f32)
    ret, ln = eng.evaluate(E, True)
    assert torch.equal(ln, ln_t) and torch.equal(ln32, ln_t)
    assert bool(torch.isfinite(ret).all())
    gap = float(((ret - ret32).abs() / ln.to(torch.float32)).mean())
    print(f"low-precision return gap {dtype}: {gap:.6e}")
    assert gap <= 3.0 * LOWP_GAP_MEASURED[dtype]


def _training_state(eng, model, env, stats):
    return {"env.state": env.state, "ep_len": env.ep_len, "ep_ret": env.ep_ret,
            "env.t": torch.tensor(env.t), "x_buf": eng.x_buf, "actions": eng.actions, "logp": eng.logp,
            "rewards": eng.rewards, "dones": eng.dones, "mom": eng.mom, "epstat": eng.epstat,
            "stats.mean": stats.mean, "stats.mean_diff": stats.mean_diff, "stats.mean_f32": stats.mean_f32,
            "stats.inv_std_f32": stats.inv_std_f32, "model.flat": model.flat.data, "wimg": eng.wimg,
            "adam_m": eng.adam_m, "adam_v": eng.adam_v, "adam_state": eng.adam_state}


@pytest.mark.parametrize("dtype", ["bf16x3", "fp8"])
def test_eval_leaves_training_state_untouched(dtype):
    a = _engine(_params("HalfCheetah-v2", dtype))
    b = _engine(_params("HalfCheetah-v2", dtype))
    for eng, *_ in (a, b):
        eng.rollout()            # non-trivial env state, episode trackers, step counter, buffers
    before = {k: v.clone() for k, v in _training_state(*a).items()}
    ret, ln = a[0].evaluate(E, False)
    ret_d, _ = a[0].evaluate(E, True)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(ret).all()) and int(ln.min()) >= 1
    for k, v in _training_state(*a).items():
        assert torch.equal(v, before[k]), k
    # the evaluator owns its outputs: they are none of the training buffers
    ptrs = {v.data_ptr() for v in _training_state(*a).values() if v.is_cuda}
    assert ret.data_ptr() not in ptrs and ln.data_ptr() not in ptrs
    # ... and the next rollout is the one of an engine that never evaluated
    a[0].rollout()
    b[0].rollout()
    sa, sb = _training_state(*a), _training_state(*b)
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k


@pytest.mark.parametrize("dtype", ["bf16x3", "fp8"])
def test_eval_is_repeatable_and_follows_the_policy(dtype):
    from pytorch_dppo_amd.runtime.engine_hip import HipEngine
    from pytorch_dppo_amd.runtime.worker import DPPOWorker
    p = _params("HalfCheetah-v2", dtype, num_envs=64, num_epoch=1, eval_envs=E)
    w = DPPOWorker(p, DistContext(device=DEV))
    w.init_stats()
    eng = w.engine
    r1, l1 = (t.clone() for t in eng.evaluate(E, True))
    r2, l2 = (t.clone() for t in eng.evaluate(E, True))
    assert torch.equal(r1, r2) and torch.equal(l1, l2)
    w.iteration_step()           # one step of training (and one merge of the observation stats)
    r3, l3 = (t.clone() for t in eng.evaluate(E, True))
    assert torch.equal(l3, l1)                       # termination does not depend on the policy
    assert not torch.equal(r3, r1)
    if dtype == "bf16x3":
        # still the twin's answer for the CURRENT parameters and statistics
        ret_t, ln_t = evaluate_batch(w.model, w.stats, w.spec, E, p.seed, p.max_episode_length, p.std_convention, True)
        _assert_matches(r3, l3, ret_t, ln_t)
    else:
        # fp8: the e4m3 forward image was refreshed from the updated weights — a fresh engine
        # that packs its images from the same parameters evaluates to the same bits
        env2 = make_vec_env(w.spec, p.num_envs, seed=p.seed, device=DEV, max_episode_length=p.max_episode_length)
        eng2 = HipEngine(p, w.model, env2, w.stats, DEV, 0)
        r4, l4 = eng2.evaluate(E, True)
        assert torch.equal(r4, r3) and torch.equal(l4, l3)


@pytest.mark.parametrize("n", [1, 16, 17])
def test_eval_other_network_and_tile_edges(n):
    eng, model, env, stats = _engine(_params("Synthetic-64x8", "bf16x3", hidden=(64, 64), max_episode_length=96))
    for det in (True, False):
        ret_t, ln_t = _twin(eng, model, stats, n, det)
        ret, ln = eng.evaluate(n, det)
        assert ret.shape == (n,) and ln.shape == (n,)
        _assert_matches(ret, ln, ret_t, ln_t)


def test_inline_eval_end_to_end_gpu(tmp_path):
    from pytorch_dppo_amd.runtime.launcher import run_worker

    def run(name, **kw):
        path = tmp_path / f"{name}.jsonl"
        p = dppo_preset(device="gpu", env_name="HalfCheetah-v2", num_envs=64, exploration_size=64 * 4,
                        batch_size=64 * 4, num_epoch=2, dtype="bf16x3", max_episode_length=96,
                        log_jsonl=str(path), **kw)
        w, _ = run_worker(p, DistContext(device=DEV), max_iters=3, quiet=True)
        return w, [json.loads(l) for l in path.read_text().splitlines()]

    w, recs = run("inline", eval_mode="inline", eval_every=1, eval_envs=E)
    ev = [r for r in recs if "eval_iteration" in r]
    assert [r["eval_iteration"] for r in ev] == [1, 2, 3] and all(r["eval_episodes"] == E for r in ev)
    assert len([r for r in recs if "eval_iteration" not in r]) == 3
    ret, ln = w.engine.evaluate(E, False)
    r, l = ret.double(), ln.double()
    tol = 2e-4 * float(l.mean()) + 1e-4 * abs(float(r.mean()))
    last = ev[-1]
    assert abs(last["eval_return_mean"] - float(r.mean())) <= tol
    assert abs(last["eval_return_std"] - float(r.std(unbiased=False))) <= tol
    assert abs(last["eval_return_min"] - float(r.min())) <= 2e-4 * 96 + 1e-4 * abs(float(r.min()))
    assert abs(last["eval_return_max"] - float(r.max())) <= 2e-4 * 96 + 1e-4 * abs(float(r.max()))
    assert last["eval_length_mean"] == pytest.approx(float(l.mean()), rel=1e-12)
    w0, recs0 = run("plain", eval_every=0)
    assert not any("eval_iteration" in r for r in recs0)
    assert torch.equal(w.model.flat.data, w0.model.flat.data)
    assert torch.equal(w.env.state, w0.env.state) and torch.equal(w.stats.mean, w0.stats.mean)


def test_eval_binding_validation():
    eng, model, env, stats = _engine(_params("HalfCheetah-v2", "bf16x3"))
    k = eval_keys(1)
    keys = [k["key_env"], k["key_term"], k["key_reset"], k["key_action"]]

    def call(ret, ln, limit=96, n=E):
        ints = [env.kind, n, eng.O, eng.A, env.state_dim, limit, 0, 1]
        eng.ext.eval_rollout(eng.dt_fwd, eng.wimg_fwd, eng.layout, eng.scales, model.flat.data, stats.mean_f32,
                             stats.inv_std_f32, ret, ln, ints, keys, eng.qscale)

    f32 = lambda n: torch.full((n,), -7.0, dtype=torch.float32, device=DEV)   # noqa: E731
    i32 = lambda n: torch.full((n,), -7, dtype=torch.int32, device=DEV)       # noqa: E731
    ret, ln = f32(E), i32(E)
    with pytest.raises(RuntimeError, match="exactly E"):
        call(f32(E + 1), i32(E + 1))
    with pytest.raises(RuntimeError):
        call(f32(E - 1), ln)
    with pytest.raises(RuntimeError, match="dtype"):
        call(ret.double(), ln)
    with pytest.raises(RuntimeError, match="dtype"):
        call(ret, ln.long())
    with pytest.raises(RuntimeError, match="limit"):
        call(ret, ln, limit=0)
    with pytest.raises(RuntimeError, match="limit"):
        call(ret, ln, limit=(1 << 20) + 1)
    with pytest.raises(RuntimeError, match="E must"):
        call(ret, ln, n=0)
    with pytest.raises(RuntimeError, match="state dims"):
        eng.ext.eval_rollout(eng.dt_fwd, eng.wimg_fwd, eng.layout, eng.scales, model.flat.data, stats.mean_f32,
                             stats.inv_std_f32, ret, ln, [env.kind, E, eng.O, eng.A, env.state_dim + 1, 96, 0, 1],
                             keys, eng.qscale)
    torch.cuda.synchronize()
    # every refusal came before a launch: the outputs were never written
    assert bool((ret == -7.0).all()) and bool((ln == -7).all())
    call(ret, ln)
    assert int(ln.min()) >= 1 and bool(torch.isfinite(ret).all())


def test_evaluate_refuses_host_stepped_env():
    eng, *_ = _engine(_params("HalfCheetah-v2", "bf16x3"))
    eng.host_env = True          # (what a gym-backend env sets)
    with pytest.raises(RuntimeError, match="host-stepped"):
        eng.evaluate(E, True)
