"""Advantage normalisation scopes (Params.adv_norm_scope global | minibatch) on the CPU engine: the oracle
(ops/oracle.adv_sums / adv_block / adv_apply), the engine and worker plumbing, the record's fields, checkpoints
and a 2-rank gloo run."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from pytorch_dppo_amd.config import Params, dppo_preset, params_from_args
from pytorch_dppo_amd.envs import VecEnv, register_tensor_env
from pytorch_dppo_amd.ops import oracle
from pytorch_dppo_amd.parallel.dist import DistContext
from pytorch_dppo_amd.runtime.launcher import free_port, run_worker
from pytorch_dppo_amd.runtime.worker import DPPOWorker

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the oracle --------------------------------------------------------------------------------------------------
def block64(adv, ret):
    """[mean, inv, std, ev] worked in numpy float64 from the float32 samples, rounded to float32 here"""
    a, r = np.asarray(adv, np.float32).astype(np.float64), np.asarray(ret, np.float32).astype(np.float64)
    n = a.size
    mean = a.sum() / n
    var = max((a * a).sum() - a.sum() * mean, 0.0) / (n - 1)
    rvar = max((r * r).sum() - r.sum() * (r.sum() / n), 0.0) / (n - 1)
    std = math.sqrt(var)
    ev = 1.0 - var / rvar if rvar > 0 else float("nan")
    return np.array([mean, 1.0 / (std + 1e-8), std, ev]).astype(np.float32)


def same_bits(a, b):
    """bitwise equality of two fp32 vectors, a NaN equal to a NaN"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    nan = np.isnan(a) & np.isnan(b)
    return a.shape == b.shape and bool(np.all(nan | (a.view(np.int32) == b.view(np.int32))))


def _block(adv, ret):
    a, r = torch.tensor(adv, dtype=torch.float32), torch.tensor(ret, dtype=torch.float32)
    return oracle.adv_block(oracle.adv_sums(a, r), a.numel())


def test_adv_block_hand_table():
    # [1, 2, 3, 4] / [2, 4, 6, 8]: mean 2.5, var 5/3, var(ret) 20/3, ev 0.75
    b = _block([1, 2, 3, 4], [2, 4, 6, 8])
    assert b.dtype == torch.float32 and b.shape == (4,)
    std = math.sqrt(5.0 / 3.0)
    want = np.array([2.5, 1.0 / (std + 1e-8), std, 0.75]).astype(np.float32)
    assert same_bits(b.numpy(), want) and same_bits(b.numpy(), block64([1, 2, 3, 4], [2, 4, 6, 8]))
    # n = 2: mean 2, var 8 (unbiased), var(ret) 0.5, ev -15
    b = _block([0, 4], [1, 2])
    std = math.sqrt(8.0)
    assert same_bits(b.numpy(), np.array([2.0, 1.0 / (std + 1e-8), std, 1.0 - 8.0 / 0.5]).astype(np.float32))
    # a constant advantage: std 0, inv = 1 / 1e-8, every normalised value exactly 0, ev 1
    adv = torch.full((7,), 3.25)
    b = oracle.adv_block(oracle.adv_sums(adv, torch.arange(7.0)), 7)
    assert float(b[0]) == 3.25 and float(b[2]) == 0.0 and float(b[1]) == float(np.float32(1e8)) and float(b[3]) == 1.0
    assert bool((oracle.adv_apply(adv, b) == 0).all())
    # a constant return: explained variance undefined
    b = _block([1, 2, 3, 4], [5, 5, 5, 5])
    assert math.isnan(float(b[3])) and float(b[0]) == 2.5
    # mean / std = 1e3: the fp64 sums keep the variance that an fp32 sum of squares would lose
    g = torch.Generator().manual_seed(0)
    adv = 1e3 + torch.randn(4096, generator=g)
    ret = torch.randn(4096, generator=g)
    b = oracle.adv_block(oracle.adv_sums(adv, ret), 4096)
    assert same_bits(b.numpy(), block64(adv.numpy(), ret.numpy()))
    a64 = adv.double().numpy()
    assert float(b[2]) == pytest.approx(a64.std(ddof=1), rel=1e-6) and float(b[0]) == pytest.approx(a64.mean(), rel=1e-7)
    # adv_apply: two separately rounded fp32 operations
    x = oracle.adv_apply(adv, b)
    want = ((adv.numpy() - b.numpy()[0]).astype(np.float32) * b.numpy()[1]).astype(np.float32)
    assert x.dtype == torch.float32 and np.array_equal(x.numpy(), want)
    # shift invariance: a constant added to every advantage moves the mean alone
    b2 = oracle.adv_block(oracle.adv_sums(adv - 1e3, ret), 4096)
    assert float(b2[2]) == pytest.approx(float(b[2]), rel=1e-6)
    assert float((oracle.adv_apply(adv - 1e3, b2) - x).abs().max()) <= 1e-3      # fl32(1e3 + x) lost ~6e-5 of x


def test_adv_sums_with_idx_counts_duplicates():
    g = torch.Generator().manual_seed(1)
    adv, ret = torch.randn(5, 8, generator=g) * 3, torch.randn(5, 8, generator=g) + 2
    idx = torch.tensor([39, 39, 0, 7, 7, 7, 12, 3, 38])
    s = oracle.adv_sums(adv, ret, idx)
    assert s.dtype == torch.float64 and s.shape == (4,)
    a, r = adv.reshape(-1).double().numpy()[idx.numpy()], ret.reshape(-1).double().numpy()[idx.numpy()]
    np.testing.assert_allclose(s.numpy(), [a.sum(), (a * a).sum(), r.sum(), (r * r).sum()], rtol=1e-14)
    full = oracle.adv_sums(adv, ret)
    np.testing.assert_allclose(full.numpy()[:2], [adv.double().sum(), (adv.double() ** 2).sum()], rtol=1e-14)
    assert not np.allclose(s.numpy(), oracle.adv_sums(adv, ret, torch.unique(idx)).numpy())


# ---- the torch worker against a twin fed the pre-normalised buffer ----------------------------------------------------
def _pendulum(**kw):
    base = dict(env_name="Pendulum-v0", num_envs=6, exploration_size=6 * 20, batch_size=6 * 20, num_epoch=2,
                reward_clip=0.0, max_episode_length=8, normalize_adv=True, seed=7)
    base.update(kw)
    return dppo_preset(**base)


def _twin(scope, **kw):
    """a worker without normalize_adv whose engine the test drives: ``global``: after GAE the buffer is overwritten
    with adv_apply(adv, block of the whole buffer); ``minibatch``: around every grad(idx) the buffer holds
    adv_apply(adv, block of that step's rows)"""
    w = DPPOWorker(_pendulum(normalize_adv=False, **kw), DistContext())
    eng = w.engine
    gae, grad = eng.gae, eng.grad
    raw = {}

    def gae_then_normalise():
        gae()
        raw["adv"] = eng.adv.clone()
        if scope == "global":
            eng.adv.copy_(oracle.adv_apply(eng.adv, oracle.adv_block(oracle.adv_sums(eng.adv, eng.ret), eng.adv.numel())))

    def grad_on_step_rows(idx):
        if scope == "minibatch":
            n = eng.adv.numel() if idx is None else idx.numel()
            eng.adv.copy_(oracle.adv_apply(raw["adv"], oracle.adv_block(oracle.adv_sums(raw["adv"], eng.ret, idx), n)))
        return grad(idx)
    eng.gae, eng.grad = gae_then_normalise, grad_on_step_rows
    return w, raw


@pytest.mark.parametrize("scope", ["global", "minibatch"])
@pytest.mark.parametrize("geometry", [dict(), dict(batch_size=32, minibatches_per_epoch=5)], ids=["full", "minibatches"])
def test_torch_worker_equals_the_twin_on_the_prenormalised_buffer(scope, geometry):
    w = DPPOWorker(_pendulum(adv_norm_scope=scope, **geometry), DistContext())
    t, raw = _twin(scope, **geometry)
    for _ in range(2):
        m, mt = w.iteration_step(), t.iteration_step()
        assert torch.equal(w.model.flat.data, t.model.flat.data)
        assert torch.equal(w.engine.adv, raw["adv"]) and torch.equal(w.engine.ret, t.engine.ret)   # adv stays raw
        assert m["loss"] == mt["loss"] and m["grad_norm"] == mt["grad_norm"]
        assert float(w.engine.adv.std()) > 0 and abs(float(w.engine.adv.mean())) > 1e-3
    if geometry:       # the wrap-around of 5 x 32 rows over 120 repeats rows inside a step
        assert w.p.num_minibatches() * w.p.minibatch_rows() > w.p.buffer_rows


def test_minibatch_block_is_the_steps_own():
    """the two scopes differ where a step is not the whole buffer, and agree where it is"""
    geo = dict(batch_size=32, minibatches_per_epoch=2, num_epoch=1)
    a = DPPOWorker(_pendulum(adv_norm_scope="global", **geo), DistContext())
    b = DPPOWorker(_pendulum(adv_norm_scope="minibatch", **geo), DistContext())
    a.iteration_step(), b.iteration_step()
    assert torch.equal(a.engine.adv, b.engine.adv) and not torch.equal(a.model.flat.data, b.model.flat.data)
    a = DPPOWorker(_pendulum(adv_norm_scope="global"), DistContext())
    b = DPPOWorker(_pendulum(adv_norm_scope="minibatch"), DistContext())
    a.iteration_step(), b.iteration_step()
    assert torch.equal(a.model.flat.data, b.model.flat.data) and torch.equal(a.engine.adv_block, b.engine.adv_block)


def test_world_size_one_global_agrees_with_rank():
    r = DPPOWorker(_pendulum(adv_norm_scope="rank", num_epoch=1), DistContext())
    g = DPPOWorker(_pendulum(adv_norm_scope="global", num_epoch=1), DistContext())
    r.iteration_step(), g.iteration_step()
    want = oracle.adv_apply(g.engine.adv, g.engine.adv_block)
    # the mean and std are fp64 here and torch's fp32 reductions there: 4 fp32 ulp of the largest |a'|
    top = float(want.abs().max())
    assert float((r.engine.adv - want).abs().max()) <= 4 * np.spacing(np.float32(top))
    assert float(g.engine.adv.abs().max()) > 2 * top or float(g.engine.adv.mean().abs()) > 0.1     # raw units kept


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


for _k in (0, 1, 1024):
    register_tensor_env(f"AdvPointMassTimes{_k}-v0", make_point_mass(float(_k)), obs_dim=2, act_dim=1, time_limit=10)


def _zero_value_output(w):
    """V == 0 everywhere: the advantages are then a function of the rewards alone"""
    for k in ("v.weight", "v.bias"):
        w.model.view(k).data.zero_()
    w.engine.params_changed()


def first_policy_grad(k, device="cpu", **kw):
    base = dict(device=device, env_name=f"AdvPointMassTimes{k}-v0", num_envs=8, exploration_size=8 * 24,
                batch_size=8 * 24, num_epoch=1, reward_clip=0.0, seed=5)
    base.update(kw)
    dev = torch.device("cuda", 0) if device == "gpu" else torch.device("cpu")
    w = DPPOWorker(dppo_preset(**base), DistContext(device=dev))
    _zero_value_output(w)
    w.iteration_step()
    lo, hi = w.model.head_ranges["policy"]
    return w.engine.grad_flat[lo:hi].detach().cpu().clone(), w


def test_scale_invariance_of_the_policy_gradient():
    on = dict(normalize_adv=True, adv_norm_scope="global")
    g1, w1 = first_policy_grad(1, **on)
    gk, wk = first_policy_grad(1024, **on)
    assert torch.equal(wk.engine.rewards, w1.engine.rewards * 1024) and torch.equal(wk.engine.adv, w1.engine.adv * 1024)
    # a' differs by the 1e-8 beside the std (relative 1e-8 / std ~ 1e-7) and one fp32 rounding; the gradient is a
    # mean of terms linear in a', with cancellation allowed for: 1e-5 of its largest element
    top = float(g1.abs().max())
    assert top > 0 and float((gk - g1).abs().max()) <= 1e-5 * top
    b1, _ = first_policy_grad(1)
    bk, _ = first_policy_grad(1024)
    assert float((bk - b1 * 1024).abs().max()) <= 1e-5 * float(bk.abs().max())     # without the flag the scale goes through
    assert float(bk.abs().max()) > 100 * float(b1.abs().max())


# ---- refusals, CLI -----------------------------------------------------------------------------------------------
def test_refusals():
    with pytest.raises(ValueError, match="adv_norm_scope must be rank\\|global\\|minibatch"):
        Params(normalize_adv=True, adv_norm_scope="batch")
    for scope in ("global", "minibatch"):
        with pytest.raises(ValueError, match="normalize_adv"):
            Params(adv_norm_scope=scope)
    with pytest.raises(ValueError, match="at least 2 rows"):
        Params(normalize_adv=True, adv_norm_scope="minibatch", batch_size=1)
    with pytest.raises(ValueError, match="at least 2 advantages"):
        Params(normalize_adv=True, adv_norm_scope="global", exploration_size=1, num_envs=1, num_processes=1)
    Params(normalize_adv=True, adv_norm_scope="global", exploration_size=1, num_envs=1, num_processes=2)
    assert Params().adv_norm_scope == "rank" and Params().adv_scope() == "" and Params(normalize_adv=True).adv_scope() == ""
    p = Params(normalize_adv=True, adv_norm_scope="minibatch", target_kl=0.02, lr_schedule="adaptive", reward_norm=True,
               bootstrap_time_limit=True)
    assert p.adv_scope() == "minibatch"


def test_cli_flags():
    p = params_from_args(["--normalize-adv", "true", "--adv-norm-scope", "global"])
    assert p.normalize_adv is True and p.adv_norm_scope == "global" and p.adv_scope() == "global"
    assert params_from_args([]).adv_norm_scope == "rank"
    assert Params.from_dict(p.to_dict()).adv_norm_scope == "global"
    with pytest.raises(ValueError, match="normalize_adv"):
        params_from_args(["--adv-norm-scope", "minibatch"])


# ---- the record ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scope", ["global", "minibatch"])
def test_record_fields(scope):
    w = DPPOWorker(_pendulum(adv_norm_scope=scope, batch_size=40), DistContext())
    m = w.iteration_step()
    eng = w.engine
    a, r = eng.adv.double().numpy().ravel(), eng.ret.double().numpy().ravel()
    assert m["adv_mean"] == pytest.approx(a.mean(), rel=1e-6) and m["adv_std"] == pytest.approx(a.std(ddof=1), rel=1e-6)
    assert m["explained_variance"] == pytest.approx(1.0 - a.var(ddof=1) / r.var(ddof=1), rel=1e-5, abs=1e-6)
    assert m["adv_mean"] == float(eng.adv_block[0]) and m["adv_std"] == float(eng.adv_block[2])
    assert math.isfinite(m["loss"]) and m["ep_count"] > 0       # the tails behind the vector did not shift it


def test_record_composes_with_the_other_tails():
    w = DPPOWorker(_pendulum(adv_norm_scope="global", reward_norm=True, target_kl=0.5, lr_schedule="adaptive"),
                   DistContext())
    m = w.iteration_step()
    a = w.engine.adv.double().numpy().ravel()
    assert m["adv_std"] == pytest.approx(a.std(ddof=1), rel=1e-6) and m["return_std"] > 0
    assert m["lr"] > 0 and m["steps_applied"] >= 1 and "lr_ups" in m


def test_explained_variance_is_null_for_a_constant_return():
    w = DPPOWorker(dppo_preset(env_name="AdvPointMassTimes0-v0", num_envs=4, exploration_size=32, batch_size=32,
                               num_epoch=1, normalize_adv=True, adv_norm_scope="global"), DistContext())
    _zero_value_output(w)
    m = w.iteration_step()
    assert m["explained_variance"] is None and m["adv_std"] == 0.0 and m["adv_mean"] == 0.0
    assert json.loads(json.dumps(m))["explained_variance"] is None
    assert math.isfinite(m["loss"]) and bool(torch.isfinite(w.model.flat.data).all())


def test_fields_absent_and_nothing_held_with_the_flag_off():
    for kw in (dict(normalize_adv=False), dict(normalize_adv=True), dict(normalize_adv=True, adv_norm_scope="rank")):
        w = DPPOWorker(_pendulum(**kw), DistContext())
        m = w.iteration_step()
        assert not any(k in m for k in ("adv_mean", "adv_std", "explained_variance")) and w.engine.adv_block is None
    # scope rank normalises the buffer in place, as ever
    assert abs(float(w.engine.adv.mean())) < 1e-6 and float(w.engine.adv.std()) == pytest.approx(1.0, rel=1e-5)


# ---- checkpoints -------------------------------------------------------------------------------------------------
def _run(**kw):
    base = dict(env_name="Pendulum-v0", num_processes=1, num_envs=6, exploration_size=6 * 20, batch_size=40,
                num_epoch=2, reward_clip=0.0, max_episode_length=8, seed=4, normalize_adv=True)
    base.update(kw)
    return run_worker(dppo_preset(**base), DistContext(), evaluator=False, quiet=True)[0]


@pytest.mark.parametrize("scope", ["global", "minibatch"])
def test_resume_continues_bit_identically(tmp_path, scope):
    ck = str(tmp_path / "ck")
    w_full = _run(max_iters=3, adv_norm_scope=scope)
    _run(max_iters=2, checkpoint_dir=ck, adv_norm_scope=scope)
    st = torch.load(os.path.join(ck, "trainer_state.pt"), weights_only=True)
    assert not any("adv" in k for k in st if k not in ("adam_m", "adam_v", "adam_step"))    # nothing new is checkpointed
    w_res = _run(max_iters=3, resume=ck, checkpoint_dir="", adv_norm_scope=scope)
    assert w_res.iteration == 3
    for a, b in ((w_full.model.flat.data, w_res.model.flat.data), (w_full.engine.adv, w_res.engine.adv),
                 (w_full.engine.adv_block, w_res.engine.adv_block)):
        assert torch.equal(a, b)
    assert w_full.last_metrics["adv_std"] == w_res.last_metrics["adv_std"]


def test_train_py_logs_the_three_fields(tmp_path):
    path, csv = tmp_path / "train.jsonl", tmp_path / "train.csv"
    cmd = [sys.executable, "train.py", "--env-name", "Pendulum-v0", "--max-iters", "2", "--num-processes", "1",
           "--num-envs", "4", "--exploration-size", "64", "--batch-size", "16", "--num-epoch", "1", "--reward-clip", "0",
           "--normalize-adv", "true", "--adv-norm-scope", "minibatch", "--log-jsonl", str(path), "--log-csv", str(csv)]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=170)
    assert r.returncode == 0, r.stderr[-3000:]
    recs = [json.loads(l) for l in path.read_text().splitlines()]
    assert len(recs) == 2
    for x in recs:
        assert x["adv_std"] > 0 and math.isfinite(x["adv_mean"]) and x["explained_variance"] < 1.0
    assert "adv_std" not in csv.read_text().splitlines()[0]           # the CSV columns are fixed


# ---- two ranks -------------------------------------------------------------------------------------------------
def _rank_main(rank, world, port, out_dir):
    from pytorch_dppo_amd.parallel.dist import init_distributed
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.set_num_threads(1)
    ctx = init_distributed("cpu", rank=rank, world_size=world, timeout_s=60.0)
    w = DPPOWorker(_pendulum(num_processes=world, adv_norm_scope="global", batch_size=40, verify_sync_every=1), ctx)
    out = []
    for _ in range(2):
        m = w.iteration_step()
        eng = w.engine
        out.append({"block": eng.adv_block.clone(), "adv": eng.adv.clone(), "ret": eng.ret.clone(),
                    "rank_block": oracle.adv_block(oracle.adv_sums(eng.adv, eng.ret), eng.adv.numel()),
                    "in_sync": bool(m["replicas_in_sync"]), "adv_std": m["adv_std"]})
    torch.save({"its": out, "flat": w.model.flat.data.clone()}, os.path.join(out_dir, f"r{rank}.pt"))
    ctx.destroy()


@pytest.mark.slow
def test_two_ranks_hold_one_global_block(tmp_path):
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
    assert torch.equal(r0["flat"], r1["flat"])
    for a, b in zip(r0["its"], r1["its"]):
        assert a["in_sync"] and b["in_sync"]
        assert torch.equal(a["block"], b["block"]) and not torch.equal(a["adv"], b["adv"])
        adv, ret = torch.cat([a["adv"], b["adv"]]), torch.cat([a["ret"], b["ret"]])
        # the all-reduce adds the two ranks' fp64 sums: one more rounding than the sum over the concatenation
        want = oracle.adv_block(oracle.adv_sums(a["adv"], a["ret"]) + oracle.adv_sums(b["adv"], b["ret"]), adv.numel())
        assert same_bits(a["block"].numpy(), want.numpy())
        cat = oracle.adv_block(oracle.adv_sums(adv, ret), adv.numel())
        np.testing.assert_allclose(a["block"].numpy(), cat.numpy(), rtol=1e-6)
        assert not torch.equal(a["rank_block"], b["rank_block"]) and not torch.equal(a["rank_block"], a["block"])
        assert a["adv_std"] == float(a["block"][2])
