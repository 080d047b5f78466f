"""Reward normalisation by the running std of the discounted return (Params.reward_norm) on the CPU
engine: the scan (ops/oracle.return_scan), the statistics (utils/ret_stats.py), the engine and worker
plumbing, checkpoints and a 2-rank gloo run."""
import json
import math
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch

from pytorch_dppo_amd.config import Params, dppo_preset, params_from_args
from pytorch_dppo_amd.envs import VecEnv, register_tensor_env
from pytorch_dppo_amd.ops import oracle
from pytorch_dppo_amd.parallel.dist import DistContext
from pytorch_dppo_amd.runtime.launcher import free_port, run_worker
from pytorch_dppo_amd.runtime.worker import DPPOWorker
from pytorch_dppo_amd.utils.ret_stats import RunningReturnStats

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the scan ------------------------------------------------------------------------------------------------
def loop_scan(r, d, gamma, acc, shift, f=np.float64):
    """scalar replay: R [T,E], carry [E] and (S1, S2) in float64, the recurrence in ``f`` arithmetic"""
    T, E = r.shape
    g = f(np.float32(gamma))
    R = np.zeros((T, E), dtype=f)
    carry = np.zeros(E, dtype=f)
    s1 = s2 = 0.0
    for e in range(E):
        x = f(acc[e])
        for t in range(T):
            x = f(f(g * x) + f(r[t, e]))
            R[t, e] = x
            s1 += float(x) - float(shift)
            s2 += (float(x) - float(shift)) ** 2
            if d[t, e] != 0:
                x = f(0.0)
        carry[e] = x
    return R, carry, s1, s2


def hand_case():
    # env 0: a done at t = 0; env 1: two consecutive dones; env 2: a done at T - 1; env 3: none
    r = np.array([[1.5, -2.25, 0.75, 3.0],
                  [-0.5, 4.0, 1.25, -1.0],
                  [2.0, 0.125, -3.5, 0.3],
                  [0.7, -0.9, 2.2, 1.1],
                  [1.0, 1.0, -1.0, 0.45]], dtype=np.float32)
    d = np.zeros_like(r)
    d[0, 0] = 1
    d[1, 1] = d[2, 1] = 1
    d[4, 2] = 1
    acc = np.array([3.25, -1.5, 0.6, 10.0], dtype=np.float32)
    return r, d, acc, np.float32(0.37)


def test_return_scan_matches_scalar_loop():
    r, d, acc, shift = hand_case()
    gamma = 0.99
    acc2, s1, s2, R = oracle.return_scan(torch.from_numpy(r), torch.from_numpy(d), gamma, torch.from_numpy(acc),
                                         torch.tensor([shift]), return_R=True)
    assert R.dtype == torch.float32 and acc2.dtype == torch.float32
    R32, c32, s1_32, s2_32 = loop_scan(r, d, gamma, acc, shift, np.float32)
    assert np.array_equal(R.numpy(), R32) and np.array_equal(acc2.numpy(), c32)        # bitwise
    assert acc2[2] == 0.0 and acc2[0] != 0.0                                           # done at T-1 zeroes the carry
    # 20 terms of magnitude <= ~150: any summation order agrees to ~20 * 2^-53 * sum|x| < 1e-11
    assert float(s1) == pytest.approx(s1_32, abs=1e-10) and float(s2) == pytest.approx(s2_32, abs=1e-10)
    R64, c64, s1_64, s2_64 = loop_scan(r, d, gamma, acc, shift, np.float64)
    np.testing.assert_allclose(R.numpy(), R64, rtol=5e-7, atol=1e-6)
    assert float(s1) == pytest.approx(s1_64, abs=1e-4) and float(s2) == pytest.approx(s2_64, rel=1e-5)
    # the three-value form and a float shift
    a3 = oracle.return_scan(torch.from_numpy(r), torch.from_numpy(d), gamma, torch.from_numpy(acc), float(shift))
    assert len(a3) == 3 and torch.equal(a3[0], acc2) and float(a3[1]) == float(s1)


def test_two_scans_equal_one():
    g = torch.Generator().manual_seed(3)
    r = torch.randn(24, 7, generator=g) * 30
    d = (torch.rand(24, 7, generator=g) < 0.15).float()
    acc0 = torch.randn(7, generator=g)
    one, s1, s2 = oracle.return_scan(r, d, 0.99, acc0, 0.5)
    a, p1, q1 = oracle.return_scan(r[:12], d[:12], 0.99, acc0, 0.5)
    b, p2, q2 = oracle.return_scan(r[12:], d[12:], 0.99, a, 0.5)
    assert torch.equal(one, b)
    assert float(p1 + p2) == pytest.approx(float(s1), rel=1e-12) and float(q1 + q2) == pytest.approx(float(s2), rel=1e-12)


# ---- the statistics --------------------------------------------------------------------------------------------
def test_running_return_stats_matches_numpy():
    rng = np.random.default_rng(0)
    batches = [rng.normal(-300.0, 80.0, 500), rng.normal(-150.0, 20.0, 300), rng.normal(40.0, 200.0, 700)]
    st = RunningReturnStats()
    assert float(st.scale) == 1.0 and st.n == 0
    for b in batches:
        shift = st.shift().clone()
        x = torch.from_numpy(b.astype(np.float32)).to(torch.float64) - shift.to(torch.float64)
        st.merge_moments(float(len(b)), x.sum().reshape(1), (x * x).sum().reshape(1), shift)
    allx = np.concatenate([b.astype(np.float32).astype(np.float64) for b in batches])
    assert st.n == allx.size
    assert float(st.mean) == pytest.approx(allx.mean(), rel=1e-12)
    assert float(st.mean_diff / st.n) == pytest.approx(allx.var(), rel=1e-12)
    assert float(st.std()) == pytest.approx(allx.std(), rel=1e-12)
    assert st.scale.dtype == torch.float32 and float(st.scale) == pytest.approx(1.0 / allx.std(), rel=1e-6)
    assert float(st.shift()) == np.float32(allx.mean())
    # the floor: constant samples
    z = RunningReturnStats()
    z.merge_moments(10.0, torch.zeros(1, dtype=torch.float64), torch.zeros(1, dtype=torch.float64), z.shift().clone())
    assert float(z.scale) == pytest.approx(1e4, rel=1e-6)
    # state_dict round trip
    st2 = RunningReturnStats()
    st2.load_state_dict(st.state_dict())
    assert st2.n == st.n and torch.equal(st2.mean, st.mean) and torch.equal(st2.mean_diff, st.mean_diff)
    assert torch.equal(st2.scale, st.scale) and set(st.state_dict()) == {"n", "mean", "M2"}


# ---- the engine -------------------------------------------------------------------------------------------------
def replay64(chunks, gamma, E):
    """float64 replay over consecutive rollouts' (rewards, dones): every sample R"""
    g = float(np.float32(gamma))
    carry = np.zeros(E)
    out = []
    for r, d in chunks:
        r, d = r.double().numpy(), d.numpy()
        for t in range(r.shape[0]):
            carry = g * carry + r[t]
            out.append(carry.copy())
            carry = np.where(d[t] != 0, 0.0, carry)
    return np.concatenate(out)


def scale64(samples):
    return 1.0 / math.sqrt(max(samples.var(), 1e-8))


def _pendulum(**kw):
    base = dict(env_name="Pendulum-v0", num_envs=6, exploration_size=6 * 20, batch_size=6 * 20, num_epoch=1,
                reward_clip=0.0, reward_norm=True, max_episode_length=8, normalize_adv=True)
    base.update(kw)
    return dppo_preset(**base)


@pytest.mark.parametrize("obs_norm_update", ["rollout", "step"])
def test_torch_engine_scale_follows_float64_replay(obs_norm_update):
    w = DPPOWorker(_pendulum(obs_norm_update=obs_norm_update), DistContext())
    eng = w.engine
    chunks = []
    for it in range(3):
        m = w.iteration_step()
        chunks.append((eng.rewards.clone(), eng.dones.clone()))
        assert float(eng.dones.sum()) > 0 and float(eng.rewards.abs().max()) > 1.0      # raw units, episodes end
        samples = replay64(chunks, w.p.gamma, eng.E)
        assert eng.ret_stats.n == samples.size == (it + 1) * eng.T * eng.E
        assert float(eng.ret_stats.scale) == pytest.approx(scale64(samples), rel=1e-6)
        assert m["return_std"] == pytest.approx(samples.std(), rel=1e-6)
        # GAE read the scaled reward
        r = oracle.scale_rewards(eng.rewards, eng.ret_stats.scale, w.p.reward_norm_clip)
        adv, ret = oracle.gae(r, eng.values_buf, eng.dones, w.p.gamma, w.p.gae_param, segment=w.p.gae_segment())
        assert torch.equal(eng.ret, ret)
    # the carry is the scan's
    acc = torch.zeros(eng.E)
    for r, d in chunks:
        acc = oracle.return_scan(r, d, w.p.gamma, acc, 0.0)[0]
    assert torch.equal(eng.ret_acc, acc)


def test_flag_off_holds_no_state_and_logs_no_return_std():
    w = DPPOWorker(_pendulum(reward_norm=False), DistContext())
    m = w.iteration_step()
    assert w.engine.ret_stats is None and w.engine.ret_acc is None
    assert "return_std" not in m and "ret_stats" not in w.trainer_state() and "ret_acc" not in w.engine.env_state()


def test_reward_clip_applies_before_the_scan():
    w = DPPOWorker(_pendulum(reward_clip=1.0), DistContext())
    w.iteration_step()
    eng = w.engine
    assert float(eng.rewards.abs().max()) <= 1.0
    samples = replay64([(eng.rewards, eng.dones)], w.p.gamma, eng.E)
    assert float(eng.ret_stats.scale) == pytest.approx(scale64(samples), rel=1e-6)


def test_bootstrap_time_limit_composes():
    w = DPPOWorker(_pendulum(bootstrap_time_limit=True, normalize_adv=False), DistContext())
    w.iteration_step()
    eng = w.engine
    slot = torch.arange(eng.T) // eng.env.limit
    boot = eng.trunc * eng.v_fin[slot]
    assert float(boot.abs().sum()) > 0
    r = oracle.scale_rewards(eng.rewards, eng.ret_stats.scale, w.p.reward_norm_clip)
    adv, ret = oracle.gae(r, eng.values_buf, eng.dones, w.p.gamma, w.p.gae_param, boot=boot)
    assert torch.equal(eng.adv, adv) and torch.equal(eng.ret, ret)


# ---- scale invariance --------------------------------------------------------------------------------------------
def make_point_mass(k):
    class PointMass(VecEnv):                       # the README's example, reward times k
        state_dim = 2

        def _reset_state(self, step_key):
            return torch.zeros(self.E, 2, device=self.device)

        def observe(self):
            return self.state.clone()

        def _dynamics(self, a, step_key):
            pos, vel = self.state[:, 0], self.state[:, 1]
            vel = vel + 0.1 * a[:, 0].clamp(-1, 1)
            pos = pos + 0.1 * vel
            return torch.stack([pos, vel], 1), -k * (pos - 1.0) ** 2, pos.abs() > 5.0

    return PointMass


for _k in (1, 1024):
    register_tensor_env(f"PointMassTimes{_k}-v0", make_point_mass(float(_k)), obs_dim=2, act_dim=1, time_limit=10)


def first_adv(k, reward_norm, device="cpu", **kw):
    base = dict(device=device, env_name=f"PointMassTimes{k}-v0", num_envs=8, exploration_size=8 * 24,
                batch_size=8 * 24, num_epoch=1, reward_clip=0.0, reward_norm=reward_norm, reward_norm_clip=0.0, seed=5)
    base.update(kw)
    dev = torch.device("cuda", 0) if device == "gpu" else torch.device("cpu")
    w = DPPOWorker(dppo_preset(**base), DistContext(device=dev))
    w.iteration_step()
    eng = w.engine
    return eng.adv.detach().cpu().clone().reshape(-1), eng.rewards.detach().cpu().clone().reshape(-1)


def test_scale_invariance():
    a1, r1 = first_adv(1, True)
    ak, rk = first_adv(1024, True)
    assert torch.equal(rk, r1 * 1024) and float(r1.abs().max()) > 0       # the stored rewards keep raw units
    assert float((ak - a1).abs().max()) <= 1e-5 * float(a1.abs().max())
    b1, _ = first_adv(1, False)
    bk, _ = first_adv(1024, False)
    assert float((bk - b1).abs().max()) > 100 * float(b1.abs().max())    # without the flag the scale goes through


# ---- refusals, CLI -----------------------------------------------------------------------------------------------
def test_refusals():
    with pytest.raises(ValueError, match="compat"):
        Params(reward_norm=True, compat=True)
    for mode in ("on", "auto"):
        with pytest.raises(ValueError, match="stats_stream"):
            Params(reward_norm=True, stats_stream=mode)
    Params(reward_norm=False, compat=True, stats_stream="on")
    p = Params(reward_norm=True, bootstrap_time_limit=True, normalize_adv=True, obs_norm_update="rollout")
    assert p.reward_norm and p.reward_norm_clip == 10.0


def test_cli_flags():
    p = params_from_args(["--reward-norm", "true", "--reward-norm-clip", "5", "--reward-clip", "0"])
    assert p.reward_norm is True and p.reward_norm_clip == 5.0 and p.reward_clip == 0.0
    assert params_from_args([]).reward_norm is False
    assert params_from_args(["--reward-norm"]).reward_norm is True
    assert Params.from_dict(p.to_dict()).reward_norm is True


# ---- checkpoints -------------------------------------------------------------------------------------------------
def _run(tmp=None, **kw):
    base = dict(env_name="Pendulum-v0", num_processes=1, num_envs=6, exploration_size=6 * 20, batch_size=6 * 20,
                num_epoch=2, reward_clip=0.0, reward_norm=True, max_episode_length=8, seed=4)
    base.update(kw)
    return run_worker(dppo_preset(**base), DistContext(), evaluator=False, quiet=True)[0]


def test_resume_continues_bit_identically(tmp_path):
    ck = str(tmp_path / "ck")
    w_full = _run(max_iters=3)
    w_two = _run(max_iters=2, checkpoint_dir=ck)
    st = torch.load(os.path.join(ck, "trainer_state.pt"), weights_only=True)
    es = torch.load(os.path.join(ck, "env_rank0.pt"), weights_only=True)
    assert set(st["ret_stats"]) == {"n", "mean", "M2"} and st["ret_stats"]["n"] == 2 * 120
    assert torch.equal(es["ret_acc"], w_two.engine.ret_acc)
    w_res = _run(max_iters=3, resume=ck, checkpoint_dir="")
    assert w_res.iteration == 3
    for a, b in ((w_full.model.flat.data, w_res.model.flat.data), (w_full.engine.ret_acc, w_res.engine.ret_acc),
                 (w_full.engine.ret_stats.mean, w_res.engine.ret_stats.mean),
                 (w_full.engine.ret_stats.mean_diff, w_res.engine.ret_stats.mean_diff),
                 (w_full.engine.ret_stats.scale, w_res.engine.ret_stats.scale), (w_full.engine.adv, w_res.engine.adv)):
        assert torch.equal(a, b)
    assert w_full.engine.ret_stats.n == w_res.engine.ret_stats.n == 360
    assert not torch.equal(w_two.engine.ret_acc, w_full.engine.ret_acc)


def test_resume_without_the_keys_warns_and_starts_empty(tmp_path):
    ck = str(tmp_path / "ck")
    _run(max_iters=1, checkpoint_dir=ck, reward_norm=False)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        w = _run(max_iters=1, resume=ck, checkpoint_dir="")
    msgs = [str(x.message) for x in rec]
    assert any("no return statistics" in m for m in msgs) and any("no ret_acc" in m for m in msgs)
    assert w.iteration == 1 and w.engine.ret_stats.n == 0 and float(w.engine.ret_acc.abs().sum()) == 0.0
    with pytest.warns(UserWarning, match="reward_norm"):
        w2 = _run(max_iters=2, resume=ck, checkpoint_dir="")
    assert w2.engine.ret_stats.n == 120
    # and the other way round: a checkpoint with the keys resumes with the flag off
    ck2 = str(tmp_path / "ck2")
    _run(max_iters=1, checkpoint_dir=ck2)
    w3 = _run(max_iters=2, resume=ck2, checkpoint_dir="", reward_norm=False)
    assert w3.iteration == 2 and w3.engine.ret_stats is None


def test_train_py_logs_return_std(tmp_path):
    path, csv = tmp_path / "train.jsonl", tmp_path / "train.csv"
    cmd = [sys.executable, "train.py", "--env-name", "Pendulum-v0", "--max-iters", "2", "--num-processes", "1",
           "--num-envs", "4", "--exploration-size", "64", "--batch-size", "64", "--num-epoch", "1", "--reward-clip", "0",
           "--reward-norm", "true", "--log-jsonl", str(path), "--log-csv", str(csv)]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=170)
    assert r.returncode == 0, r.stderr[-3000:]
    recs = [json.loads(l) for l in path.read_text().splitlines()]
    assert len(recs) == 2 and all(x["return_std"] > 1.0 and math.isfinite(x["return_std"]) for x in recs)
    assert "return_std" not in csv.read_text().splitlines()[0]           # the CSV columns are fixed
    assert "return_std" not in r.stdout


# ---- two ranks -------------------------------------------------------------------------------------------------
def _rank_main(rank, world, port, out_dir):
    from pytorch_dppo_amd.parallel.dist import init_distributed
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.set_num_threads(1)
    ctx = init_distributed("cpu", rank=rank, world_size=world, timeout_s=60.0)
    w = DPPOWorker(_pendulum(num_processes=world), ctx)
    chunks = []
    for _ in range(2):
        w.iteration_step()
        chunks.append((w.engine.rewards.clone(), w.engine.dones.clone()))
    rs = w.engine.ret_stats
    torch.save({"n": rs.n, "mean": rs.mean.clone(), "M2": rs.mean_diff.clone(), "scale": rs.scale.clone(),
                "chunks": chunks, "flat": w.model.flat.data.clone()}, os.path.join(out_dir, f"r{rank}.pt"))
    ctx.destroy()


@pytest.mark.slow
def test_two_ranks_hold_identical_global_statistics(tmp_path):
    import torch.multiprocessing as mp
    port = free_port()
    mpc = mp.get_context("spawn")
    procs = [mpc.Process(target=_rank_main, args=(r, 2, port, str(tmp_path))) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(240)
    for p in procs:
        if p.is_alive():
            p.terminate()
    assert [p.exitcode for p in procs] == [0, 0]
    r0 = torch.load(tmp_path / "r0.pt", weights_only=True)
    r1 = torch.load(tmp_path / "r1.pt", weights_only=True)
    assert r0["n"] == r1["n"] == 2 * 2 * 120
    assert torch.equal(r0["mean"], r1["mean"]) and torch.equal(r0["M2"], r1["M2"]) and torch.equal(r0["scale"], r1["scale"])
    assert torch.equal(r0["flat"], r1["flat"])
    assert not torch.equal(r0["chunks"][0][0], r1["chunks"][0][0])                 # different data per rank
    samples = np.concatenate([replay64(r["chunks"], 0.99, 6) for r in (r0, r1)])
    assert float(r0["mean"]) == pytest.approx(samples.mean(), rel=1e-6)
    assert float(r0["M2"]) / r0["n"] == pytest.approx(samples.var(), rel=1e-6)
    assert float(r0["scale"]) == pytest.approx(scale64(samples), rel=1e-6)
