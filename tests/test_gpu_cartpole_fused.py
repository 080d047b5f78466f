"""The continuous cart-pole INSIDE the rollout and evaluation kernels (in-kernel env kind 2, csrc/env_core.h,
``env_fused=True``): against the torch engine, against the device-stepped path, on placed states whose outcome
is fixed by construction, with the per-step observation filter, at low precision (bookkeeping only), through
evaluation, the bindings' refusals, resume, learning and ``train.py``.

Every comparison of done flags first asserts, on the reference alone, that no pre-reset state lies within 1e-3 of
a termination threshold (so no flag can flip inside the tolerance) and that the expected episode ends occurred.
The helpers, tolerances, configurations and seeds are those of tests/test_gpu_tensor_env.py."""
import json
import math
import subprocess
import sys

import pytest
import torch

from pytorch_dppo_amd.config import dppo_preset
from pytorch_dppo_amd.envs import VecEnv, get_spec, make_vec_env, register_tensor_env
from pytorch_dppo_amd.parallel.dist import DistContext
from pytorch_dppo_amd.runtime.evaluator import EVAL_ENV_SEED_OFFSET, evaluate_batch
from test_gpu_tensor_env import (CARTPOLE, DEV, EVAL_SEED, ROLLOUT_SEED, ROOT, TH_LIMIT, X_LIMIT, _balancing_policy,
                                 _compare_rollouts, _engine, _params, _record_new_states, _threshold_margin,
                                 _torch_engine, _training_state)

pytestmark = pytest.mark.gpu


def _clone(ro):
    return {k: (v.clone() if torch.is_tensor(v) else v) for k, v in ro.items()}


# ---- 1. rollout against the torch engine ------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["fp32", "bf16x3"])
def test_fused_cartpole_rollout_matches_torch_engine(dtype):
    # 45 envs: two full 16-env tiles + a 13-row partial tile
    p = _params(CARTPOLE, dtype, E=45, T=24, max_episode_length=10000, seed=ROLLOUT_SEED, env_fused=True)
    eng, model, env, stats = _engine(p)
    assert not eng.stepped_env and eng.kernel_kind == 2 and env.kind == 3
    new_states = []
    ref = _torch_engine(p, model, stats, record=new_states)
    state_ptr = (env.state.data_ptr(), env.ep_len.data_ptr(), env.ep_ret.data_ptr())
    ro_h = eng.rollout()                        # the fused rollout kernel
    ro_t = ref.rollout()
    margin = _threshold_margin(new_states)
    print("reference terminations", int(ref.dones.sum()), "threshold margin", margin)
    assert int(ref.dones.sum()) >= 5 and margin > 1e-3
    assert torch.equal(ref.rewards, torch.ones_like(ref.rewards))
    _compare_rollouts(eng, env, ro_h, ref, ro_t, dtype)
    assert torch.equal(eng.rewards, torch.ones_like(eng.rewards))
    assert state_ptr == (env.state.data_ptr(), env.ep_len.data_ptr(), env.ep_ret.data_ptr())


# ---- 2. rollout against the device-stepped path --------------------------------------------------------------
def test_fused_cartpole_rollout_matches_stepped_path():
    p = _params(CARTPOLE, "bf16x3", E=45, T=24, max_episode_length=10000, seed=ROLLOUT_SEED, env_fused=True)
    eng_f, model, env_f, stats = _engine(p)
    eng_s, model2, env_s, stats2 = _engine(p)
    assert torch.equal(model.flat.data, model2.flat.data) and torch.equal(stats.mean_f32, stats2.mean_f32)
    assert not eng_f.stepped_env
    new_states = []
    _record_new_states(env_s, new_states)       # the stepped path calls the env's own _dynamics
    ro_s = _clone(eng_s.rollout_stepped())      # works on the cart-pole whatever the flag says
    ro_f = _clone(eng_f.rollout())
    torch.cuda.synchronize()
    margin = _threshold_margin(new_states)
    print("stepped terminations", int(eng_s.dones.sum()), "threshold margin", margin)
    assert len(new_states) == 24 and int(eng_s.dones.sum()) >= 5 and margin > 1e-3
    _compare_rollouts(eng_s, env_s, ro_s, eng_f, ro_f, "bf16x3", ref_is_torch=False)
    assert float(ro_s["ep_return_sum"]) == pytest.approx(float(ro_f["ep_return_sum"]), rel=1e-6)


# ---- 3. placed states: every outcome fixed by construction --------------------------------------------------
def test_fused_cartpole_placed_states():
    """x' = x + dt x_dot and th' = th + dt th_dot do not depend on the action (explicit Euler), so which
    rows terminate at step 0 is fixed by the placed states.  The smallest shape at which a wrong sign, a
    wrong threshold or a termination taken from the OLD state shows."""
    E, T, limit = 13, 2, 50
    p = _params(CARTPOLE, "fp32", E=E, T=T, max_episode_length=limit, seed=7, env_fused=True)
    eng, model, env, stats = _engine(p)
    assert not eng.stepped_env
    new_states = []
    ref = _torch_engine(p, model, stats, record=new_states)
    placed = torch.zeros(E, 4)
    placed[0] = torch.tensor([2.39, 1.0, 0.0, 0.0])       # x' =  2.41: terminal
    placed[1] = torch.tensor([-2.39, -1.0, 0.0, 0.0])     # x' = -2.41: terminal
    placed[2] = torch.tensor([0.0, 0.0, 0.205, 0.5])      # th' =  0.215 > 0.20944: terminal
    placed[3] = torch.tensor([0.0, 0.0, -0.205, -0.5])    # th' = -0.215: terminal
    placed[4] = torch.tensor([2.39, -1.0, 0.0, 0.0])      # x' = 2.37: goes on (old |x| is the larger one)
    placed[5] = torch.tensor([0.0, 0.0, 0.205, -0.5])     # th' = 0.195: goes on
    ep_len0 = torch.zeros(E, dtype=torch.int32)
    ep_ret0 = torch.zeros(E)
    ep_len0[6], ep_ret0[6] = limit - 1, float(limit - 1)  # benign (origin), ends by the step limit
    for engine in (eng, ref):                             # rows 7..12: at the origin
        # (load_env_state: the torch engine also re-reads the observation it acts on at step 0)
        engine.load_env_state({"state": placed.clone(), "ep_len": ep_len0.clone(), "ep_ret": ep_ret0.clone(), "t": 0})
    assert torch.equal(env.state, placed.to(DEV)) and torch.equal(ref.env.state, env.state)
    reset0 = ref.env._reset_state(0)                      # the in-place reset of step 0 (step key env.t = 0)
    ro_h = _clone(eng.rollout())
    ro_t = ref.rollout()
    torch.cuda.synchronize()
    margin = _threshold_margin(new_states)
    print("threshold margin", margin)
    assert len(new_states) == T and margin > 1e-3
    want = torch.zeros(T, E, device=DEV)
    want[0, [0, 1, 2, 3, 6]] = 1.0
    assert torch.equal(ref.dones, want)                   # the reference does what the construction says
    assert torch.equal(eng.dones.view(T, E), want)
    # the second step's observations of the reset rows: the keyed reset state, within +-0.05 (fp32
    # rows, un-normalised; the stats were seeded from reset observations, so nothing is clamped)
    x1 = eng.decode(eng.x_buf).view(T + 1, E, -1)[1, :, :4]
    obs1 = x1 / stats.inv_std_f32 + stats.mean_f32
    rows = [0, 1, 2, 3, 6]
    assert float(obs1[rows].abs().max()) <= 0.05 + 1e-6
    assert torch.allclose(obs1[rows], reset0[rows], atol=1e-6, rtol=1e-5)
    _compare_rollouts(eng, env, ro_h, ref, ro_t, "fp32")
    assert torch.equal(env.ep_len, ref.env.ep_len) and torch.equal(env.ep_ret, ref.env.ep_ret)
    assert env.ep_len.tolist() == [1, 1, 1, 1, 2, 2, 1] + [2] * 6
    assert float(ro_h["ep_count"]) == float(ro_t["ep_count"]) == 5.0
    assert float(ro_h["ep_return_sum"]) == float(ro_t["ep_return_sum"]) == 4.0 + float(limit)


# ---- 4. the per-step observation filter: the same kernel through the cooperative launch -------------------
# Two cases.  (200, 3): test_rollout_stepped_step_obs_norm_matches_torch_engine as it stands, on the fused
# cart-pole at E = 45, T = 24, seed 200: that test takes `_params`' episode limit of 3, so every env ends by the
# step limit every third step (24 / 3 ends per env, 360 in all) and no pole gets anywhere near a threshold.
# (219, 10000): the filter with state-decided terminations.  Seed 200 was picked for rollout-mode statistics;
# under the per-step filter at limit 10000 the torch reference alone comes within 2.018e-4 of the theta threshold
# (26 terminations; the same figure from the CPU torch engine and on the MI355X), inside the 1e-3 a done-flag
# comparison needs, so it cannot serve there.  219 was picked by running the reference alone on the CPU over
# seeds 201..231: three met the precondition (201 at 1.58e-3, 207 at 1.63e-3, 219 at 1.71e-3, 19 terminations).
STEP_MODE_SEED = 219


@pytest.mark.parametrize("seed,limit", [(ROLLOUT_SEED, 3), (STEP_MODE_SEED, 10000)])
def test_fused_cartpole_step_obs_norm_matches_torch_engine(seed, limit):
    E, T = 45, 24
    p = _params(CARTPOLE, "fp32", E=E, T=T, max_episode_length=limit, seed=seed, env_fused=True,
                obs_norm_update="step")
    eng, model, env, stats = _engine(p)
    assert not eng.stepped_env and eng._stepnorm_fits()
    new_states = []
    ref = _torch_engine(p, model, stats, record=new_states)
    ro_h = eng.rollout()
    ro_t = ref.rollout()
    # preconditions, on the reference alone: the expected episode ends occurred, no pre-reset state within
    # 1e-3 of a threshold
    margin = _threshold_margin(new_states)
    print("reference episode ends", int(ref.dones.sum()), "threshold margin", margin)
    assert len(new_states) == T and margin > 1e-3
    if limit == 3:
        want = torch.zeros(T, E, device=DEV)
        want[2::3] = 1.0                        # by the step limit alone: a pole cannot fall in 3 steps
        assert torch.equal(ref.dones, want) and int(ref.dones.sum()) == E * (T // 3)
    else:
        assert int(ref.dones.sum()) >= 5        # state-decided terminations (no env reaches step 10000)
    _compare_rollouts(eng, env, ro_h, ref, ro_t, "fp32")
    eng.raise_if_failed(sync=True)
    assert eng.local_stats.n == pytest.approx(ref.local_stats.n)
    assert torch.allclose(eng.local_stats.mean, ref.local_stats.mean, rtol=1e-6, atol=1e-6)
    assert torch.equal(stats.mean, ref.stats.mean)


# ---- 5. low precision: no reference can share flags, the bookkeeping must still be consistent -------------
@pytest.mark.parametrize("dtype", ["bf16", "fp8"])
def test_fused_cartpole_low_precision_bookkeeping(dtype):
    E, T, limit = 45, 24, 6
    p = _params(CARTPOLE, dtype, E=E, T=T, max_episode_length=limit, seed=ROLLOUT_SEED, env_fused=True)
    eng, model, env, stats = _engine(p)
    assert not eng.stepped_env
    ro = _clone(eng.rollout())
    torch.cuda.synchronize()
    for name in ("actions", "logp", "rewards", "dones"):
        assert bool(torch.isfinite(getattr(eng, name)).all()), name
    assert bool(torch.isfinite(eng.decode(eng.x_buf)).all()) and bool(torch.isfinite(env.state).all())
    assert torch.equal(eng.rewards, torch.ones_like(eng.rewards))
    dones = eng.dones.view(T, E).cpu()
    assert bool(((dones == 0) | (dones == 1)).all())
    ep_len, ep_ret = env.ep_len.cpu(), env.ep_ret.cpu()
    for e in range(E):
        ends = [t for t in range(T) if dones[t, e] > 0]
        assert ends, e                                       # limit 6 < 24 steps: every column ends
        assert int(ep_len[e]) == T - 1 - ends[-1], e         # steps since the column's last done
        assert float(ep_ret[e]) == float(ep_len[e]), e       # reward 1 per step
        gaps = [b - a for a, b in zip([-1] + ends, ends)]
        assert max(gaps) <= limit and T - 1 - ends[-1] < limit, e
    assert float(ro["ep_count"]) == float(dones.sum()) > 0
    assert float(ro["count"]) == T * E and env.t == T


# ---- 6. evaluation against the twin ---------------------------------------------------------------------------
@pytest.mark.parametrize("deterministic", [False, True])
def test_fused_cartpole_evaluate_matches_twin(deterministic):
    E, limit = 64, 40
    p = _params(CARTPOLE, "bf16x3", E=32, T=8, max_episode_length=limit, seed=EVAL_SEED, env_fused=True)
    eng, model, env, stats = _engine(p)
    assert not eng.stepped_env
    _balancing_policy(model, log_std=0.5)
    eng.params_changed()
    eng.rollout()                               # non-trivial env state, episode trackers, step counter, buffers
    before = {k: v.clone() for k, v in _training_state(eng, model, env, stats).items()}
    ret, ln = eng.evaluate(E, deterministic)    # the evaluation kernel
    torch.cuda.synchronize()
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


# ---- 7. what the bindings and the engine refuse ---------------------------------------------------------------
class _DriftEnv(VecEnv):
    """a user's tensor env (no in-kernel twin)"""

    @property
    def state_dim(self):
        return 4

    def _reset_state(self, step_key):
        return torch.zeros(self.E, 4, device=self.device)

    def observe(self):
        return self.state.clone()

    def _dynamics(self, a, step_key):
        return (self.state + a[:, :1], torch.ones(self.E, device=self.device),
                torch.zeros(self.E, dtype=torch.bool, device=self.device))


def test_fused_cartpole_binding_validation():
    p = _params(CARTPOLE, "bf16x3", E=45, T=4, max_episode_length=6, env_fused=True)
    eng, model, env, stats = _engine(p)
    kp = env.kernel_params()
    keys = [kp["key_env"], kp["key_term"], kp["key_reset"], eng.key_action]
    std_var = 1 if p.std_convention == "var" else 0

    def rollout(kind, O=4, A=1, S=4):
        ints = [kind, eng.E, O, A, S, eng.T, 0, eng.E, 0, kp["limit"], std_var]
        eng.ext.rollout(eng.dt_fwd, 16, env.state, env.ep_len, env.ep_ret, eng.wimg_fwd, eng.layout, eng.scales,
                        model.flat.data, stats.mean_f32, stats.inv_std_f32, stats.shift(), eng.x_buf, eng.actions,
                        eng.logp, eng.rewards, eng.dones, eng.mom, eng.epstat, ints, keys, float(p.reward_clip),
                        eng.qscale, eng.empty_x, eng.x_rows[0])

    ret = torch.zeros(eng.E, dtype=torch.float32, device=DEV)
    ln = torch.zeros(eng.E, dtype=torch.int32, device=DEV)

    def evaluate(kind, O=4, A=1, S=4):
        ints = [kind, eng.E, O, A, S, kp["limit"], std_var, 0]
        eng.ext.eval_rollout(eng.dt_fwd, eng.wimg_fwd, eng.layout, eng.scales, model.flat.data, stats.mean_f32,
                             stats.inv_std_f32, ret, ln, ints, keys, eng.qscale)

    before = [t.clone() for t in (env.state, env.ep_len, eng.dones, eng.actions)]
    for call in (rollout, evaluate):
        for bad in (dict(S=3), dict(S=2), dict(O=3), dict(O=5), dict(A=2), dict(S=2, O=3)):
            with pytest.raises(RuntimeError, match="state dims"):
                call(2, **bad)
        with pytest.raises(RuntimeError, match="kind"):
            call(3)
        with pytest.raises(RuntimeError, match="kind"):
            call(-1)
    torch.cuda.synchronize()
    for x, y in zip(before, (env.state, env.ep_len, eng.dones, eng.actions)):
        assert torch.equal(x, y)                # every refusal came before a launch
    rollout(2)                                  # and the well-formed calls are taken
    evaluate(2)
    torch.cuda.synchronize()
    assert int(ln.min()) >= 1 and int(ln.max()) <= kp["limit"]
    assert torch.equal(eng.rewards, torch.ones_like(eng.rewards))           # (zeros before the launch)
    assert int(env.ep_len.max()) == eng.T       # 4 steps from the reset: a pole cannot fall that fast


def test_env_fused_refuses_an_env_without_a_kernel_kind():
    from pytorch_dppo_amd.models.actor_critic import ActorCritic
    from pytorch_dppo_amd.runtime.engine_hip import HipEngine
    from pytorch_dppo_amd.utils.obs_stats import RunningObsStats
    name = "FusedGpuTestDrift-v0"
    spec = register_tensor_env(name, _DriftEnv, obs_dim=4, act_dim=1, time_limit=20)

    def build(fused):
        p = _params(name, "bf16x3", E=16, T=2, env_fused=fused)
        model = ActorCritic(spec.obs_dim, spec.act_dim, p.hidden).to(DEV)
        env = make_vec_env(spec, p.num_envs, seed=p.seed, device=DEV, max_episode_length=p.max_episode_length)
        return HipEngine(p, model, env, RunningObsStats(spec.obs_dim, DEV), DEV, 0)

    with pytest.raises(ValueError, match=name):
        build(True)
    assert build(False).stepped_env             # without the flag it is device-stepped, as ever


# ---- 8. resume ------------------------------------------------------------------------------------------------
def test_fused_cartpole_resume_continues_bit_identically(tmp_path):
    """3 iterations straight == 2 iterations, checkpoint, a fresh worker resumed from it, 1 more"""
    from pytorch_dppo_amd.runtime.launcher import run_worker
    base = dict(device="gpu", env_name=CARTPOLE, num_processes=1, num_envs=32, exploration_size=32 * 8,
                batch_size=32 * 8, num_epoch=2, dtype="bf16x3", seed=4, env_fused=True)
    ctx = DistContext(device=DEV)
    w_full, _ = run_worker(dppo_preset(max_iters=3, **base), ctx, evaluator=False, quiet=True)
    ck = str(tmp_path / "ck")
    w_two, _ = run_worker(dppo_preset(max_iters=2, checkpoint_dir=ck, **base), ctx, evaluator=False, quiet=True)
    w_res, _ = run_worker(dppo_preset(max_iters=3, resume=ck, **base), ctx, evaluator=False, quiet=True)
    torch.cuda.synchronize()
    assert not w_full.engine.stepped_env and not w_res.engine.stepped_env and w_res.iteration == 3
    assert w_res.engine.adam_step == w_full.engine.adam_step
    assert not torch.equal(w_two.env.state, w_full.env.state)       # the third iteration moved the envs
    assert torch.equal(w_full.model.flat.data, w_res.model.flat.data)
    assert torch.equal(w_full.engine.adam_m, w_res.engine.adam_m)
    assert torch.equal(w_full.engine.adam_v, w_res.engine.adam_v)
    assert torch.equal(w_full.env.state, w_res.env.state)
    assert torch.equal(w_full.env.ep_len, w_res.env.ep_len) and torch.equal(w_full.env.ep_ret, w_res.env.ep_ret)
    assert w_full.env.t == w_res.env.t == 24
    assert torch.equal(w_full.stats.mean, w_res.stats.mean)


# ---- 9. learning ----------------------------------------------------------------------------------------------
def test_fused_cartpole_learns():
    """tests/test_tensor_env.py test_dppo_learns_cartpole on the GPU engine with the env in the kernel: 12
    iterations at least triple the steps per episode end (the CPU engine: 35.9 -> 341.3, 9.5x)"""
    from pytorch_dppo_amd.runtime.worker import DPPOWorker
    p = dppo_preset(device="gpu", env_name=CARTPOLE, num_envs=32, exploration_size=2048, batch_size=512,
                    num_epoch=4, hidden=(32, 32), lr=3e-3, seed=1, dtype="bf16x3", env_fused=True)
    w = DPPOWorker(p, DistContext(device=DEV))
    assert not w.engine.stepped_env
    steps_per_episode = []
    for _ in range(12):
        w.iteration_step()
        steps_per_episode.append(p.buffer_rows / float(w.engine.dones.sum()))
    print("steps per episode:", [round(s, 1) for s in steps_per_episode])
    assert steps_per_episode[-1] >= 3.0 * steps_per_episode[0], steps_per_episode


# ---- 10. train.py end to end ----------------------------------------------------------------------------------
def test_train_py_fused_cartpole_end_to_end(tmp_path):
    path = tmp_path / "train.jsonl"
    cmd = [sys.executable, "train.py", "--device", "gpu", "--env-name", CARTPOLE, "--eval-every", "1", "--eval-mode",
           "inline", "--max-iters", "2", "--num-processes", "1", "--num-envs", "32", "--exploration-size", "1024",
           "--batch-size", "1024", "--num-epoch", "2", "--dtype", "bf16x3", "--eval-envs", "32",
           "--max-episode-length", "50", "--log-jsonl", str(path), "--env-fused", "true"]
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
