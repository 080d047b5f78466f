"""``reward_norm`` on the GPU engine: the return scan's two kernels (csrc/retnorm.hip) against the CPU twin
(ops/oracle.return_scan), the scaled GAE kernels (csrc/optim.hip, RN) against the plain ones on a pre-scaled buffer,
and the engine / worker plumbing: statistics, scale invariance, no host sync, resume, ``train.py``."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from pytorch_dppo_amd.config import dppo_preset
from pytorch_dppo_amd.ops import oracle
from pytorch_dppo_amd.parallel.dist import DistContext
from pytorch_dppo_amd.runtime.worker import DPPOWorker
from test_reward_norm import first_adv, replay64, scale64

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0) if torch.cuda.is_available() else None
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYN, PEND, CARTPOLE = "Synthetic-17x6", "Pendulum-v0", "CartPoleContinuous-v1"
U = 2.0 ** -53


def _ext():
    from pytorch_dppo_amd.ops import native
    return native.load()


# ---- the scan kernels --------------------------------------------------------------------------------------------
def scan_inputs(T, E, mag, seed):
    """rewards up to ``mag``, ~15 % dones plus a done at t = 0, two consecutive ones and one at T - 1 where the
    shape has room, a nonzero carry and shift (CPU tensors)"""
    g = torch.Generator().manual_seed(seed)
    r = (torch.rand(T, E, generator=g) * 2 - 1) * mag
    d = (torch.rand(T, E, generator=g) < 0.15).float()
    d[0, 0] = 1
    d[T - 1, E - 1] = 1
    if T >= 3 and E >= 2:
        d[1, 1] = d[2, 1] = 1
    acc = torch.randn(E, generator=g) * mag * 0.01
    shift = torch.tensor([0.3 * mag + 0.123], dtype=torch.float32)
    return r, d, acc, shift


def run_scan(r, d, acc, shift, gamma, mode, want_R=True):
    ext = _ext()
    T, E = r.shape
    acc_d = acc.to(DEV).clone()
    part = torch.zeros(2 * ext.ret_scan_nblk(T, E, mode), dtype=torch.float64, device=DEV)
    s12 = torch.full((2,), float("nan"), dtype=torch.float64, device=DEV)
    R = torch.full((T, E), float("nan"), device=DEV) if want_R else torch.empty(0, device=DEV)
    ext.ret_scan(r.to(DEV), d.to(DEV), acc_d, shift.to(DEV), part, s12, R, gamma, mode)
    torch.cuda.synchronize()
    return acc_d.cpu(), s12.cpu(), R.cpu()


def assert_moments_of(R, shift, s12):
    """|dS1| <= 2 n 2^-53 sum|R - shift| (likewise S2 with the squares): the worst case of any summation order"""
    x = R.double() - float(shift)
    n = x.numel()
    s1, s2 = float(x.sum()), float((x * x).sum())
    print("moments", float(s12[0]), s1, float(s12[1]), s2)
    assert abs(float(s12[0]) - s1) <= 2 * n * U * float(x.abs().sum())
    assert abs(float(s12[1]) - s2) <= 2 * n * U * float((x * x).sum())


@pytest.mark.parametrize("gamma", [0.99, 1.0])
@pytest.mark.parametrize("T,E", [(1, 1), (7, 45), (8, 64), (24, 130), (16, 1024)])
def test_ret_scan_lane_form_is_the_twin(T, E, gamma):
    r, d, acc, shift = scan_inputs(T, E, 1e4, T * 1000 + E)
    acc_t, s1_t, s2_t, R_t = oracle.return_scan(r, d, gamma, acc, shift, return_R=True)
    acc_k, s12, R_k = run_scan(r, d, acc, shift, gamma, 1)
    assert torch.equal(R_k, R_t) and torch.equal(acc_k, acc_t)
    assert_moments_of(R_k, shift, s12)
    # mode 0 takes this form at these shapes
    acc_0, s12_0, R_0 = run_scan(r, d, acc, shift, gamma, 0)
    assert torch.equal(R_0, R_k) and torch.equal(acc_0, acc_k) and torch.equal(s12_0, s12)


@pytest.mark.parametrize("T,E", [(600, 3), (512, 64)])
def test_ret_scan_time_form(T, E):
    gamma = 0.99
    r, d, acc, shift = scan_inputs(T, E, 1.0, T + E)
    g = float(np.float32(gamma))
    R64 = torch.empty(T, E, dtype=torch.float64)
    c = acc.double()
    for t in range(T):
        c = g * c + r[t].double()
        R64[t] = c
        c = torch.where(d[t] != 0, torch.zeros_like(c), c)
    acc_k, s12, R_k = run_scan(r, d, acc, shift, gamma, 2)
    assert torch.allclose(R_k.double(), R64, atol=2e-5, rtol=2e-5)
    assert torch.allclose(acc_k.double(), c, atol=2e-5, rtol=2e-5)
    assert_moments_of(R_k, shift, s12)
    # the lane form holds the same tolerance on these inputs, and mode 0 takes the time form at these shapes
    acc_l, s12_l, R_l = run_scan(r, d, acc, shift, gamma, 1)
    assert torch.allclose(R_l.double(), R64, atol=2e-5, rtol=2e-5)
    assert_moments_of(R_l, shift, s12_l)
    acc_0, s12_0, R_0 = run_scan(r, d, acc, shift, gamma, 0)
    assert torch.equal(R_0, R_k) and torch.equal(acc_0, acc_k) and torch.equal(s12_0, s12)


@pytest.mark.parametrize("mode", [1, 2])
def test_ret_scan_halves_equal_the_whole_and_R_out_is_optional(mode):
    # (unit rewards for the time form: its 2e-5 tolerance is the one of test_ret_scan_time_form)
    r, d, acc, shift = scan_inputs(24, 45, 100.0 if mode == 1 else 1.0, 11)
    whole, s12_w, R_w = run_scan(r, d, acc, shift, 0.99, mode)
    a, s12_a, R_a = run_scan(r[:12].contiguous(), d[:12].contiguous(), acc, shift, 0.99, mode)
    b, s12_b, R_b = run_scan(r[12:].contiguous(), d[12:].contiguous(), a, shift, 0.99, mode)
    if mode == 1:
        assert torch.equal(b, whole) and torch.equal(torch.cat([R_a, R_b]), R_w)
        # the same samples in two groupings: each sum within the order bound of the exact one
        x = R_w.double() - float(shift)
        for k, y in ((0, x.abs()), (1, x * x)):
            assert abs(float(s12_a[k] + s12_b[k] - s12_w[k])) <= 4 * x.numel() * U * float(y.sum())
    else:
        assert torch.allclose(b, whole, atol=2e-5, rtol=2e-5)
        assert torch.allclose(torch.cat([R_a, R_b]), R_w, atol=2e-5, rtol=2e-5)
        assert_moments_of(R_a, shift, s12_a)
        assert_moments_of(R_b, shift, s12_b)
    # an empty R_out: the carry and the moments keep their bits
    whole2, s12_2, R_2 = run_scan(r, d, acc, shift, 0.99, mode, want_R=False)
    assert R_2.numel() == 0 and torch.equal(whole2, whole) and torch.equal(s12_2, s12_w)


def test_ret_scan_binding_refusals():
    ext = _ext()
    T, E = 8, 20
    ok = dict(r=torch.zeros(T, E, device=DEV), d=torch.zeros(T, E, device=DEV), acc=torch.zeros(E, device=DEV),
              shift=torch.zeros(1, device=DEV), part=torch.zeros(2, dtype=torch.float64, device=DEV),
              s12=torch.zeros(2, dtype=torch.float64, device=DEV), R=torch.empty(0, device=DEV))

    def call(mode=1, **kw):
        a = dict(ok, **kw)
        ext.ret_scan(a["r"], a["d"], a["acc"], a["shift"], a["part"], a["s12"], a["R"], 0.99, mode)

    call()
    bad = [dict(r=torch.zeros(T * E, device=DEV)), dict(r=torch.zeros(T, E, dtype=torch.float64, device=DEV)),
           dict(d=torch.zeros(T - 1, E, device=DEV)), dict(acc=torch.zeros(E - 1, device=DEV)),
           dict(acc=torch.zeros(E)), dict(shift=torch.zeros(1)), dict(shift=torch.zeros(1, dtype=torch.float64, device=DEV)),
           dict(s12=torch.zeros(2, device=DEV)), dict(s12=torch.zeros(1, dtype=torch.float64, device=DEV)),
           dict(R=torch.zeros(T - 1, E, device=DEV)), dict(R=torch.zeros(T, E)), dict(mode=3),
           dict(mode=2)]              # the time form needs E x 2 doubles of scratch, not 1 x 2
    for kw in bad:
        with pytest.raises(RuntimeError):
            call(**kw)
    torch.cuda.synchronize()


# ---- the scaled GAE kernels --------------------------------------------------------------------------------------
@pytest.mark.parametrize("T_,E_", [(24, 45), (300, 3)])
@pytest.mark.parametrize("clip", [10.0, 0.0])
@pytest.mark.parametrize("boot_on", [False, True])
@pytest.mark.parametrize("seg", [0, 5])
@pytest.mark.parametrize("mode", [1, 2])
def test_gae_rn_equals_gae_on_a_prescaled_buffer(mode, seg, boot_on, clip, T_, E_):
    ext = _ext()
    g = torch.Generator().manual_seed(T_ * 7 + E_)
    r = (torch.randn(T_, E_, generator=g) * 50).to(DEV)
    v = torch.randn(T_ + 1, E_, generator=g).to(DEV)
    d = (torch.rand(T_, E_, generator=g) < 0.15).float().to(DEV)
    boot = (d * torch.randn(T_, E_, generator=g).to(DEV)) if boot_on else torch.empty(0, device=DEV)
    scale = torch.tensor([0.37], device=DEV)
    rs = r * scale
    if clip > 0:
        rs = rs.clamp(-clip, clip)
        assert int((rs.abs() == clip).sum()) > 5 and int((rs.abs() < clip).sum()) > 5
    adv, ret = torch.empty(T_, E_, device=DEV), torch.empty(T_, E_, device=DEV)
    adv0, ret0 = torch.empty_like(adv), torch.empty_like(ret)
    ext.gae_rn(r, v, d, boot, scale, clip, adv, ret, 0.99, 0.95, mode, seg)
    ext.gae_boot(rs, v, d, boot, adv0, ret0, 0.99, 0.95, mode, seg)
    assert torch.equal(adv, adv0) and torch.equal(ret, ret0)
    if not boot_on:
        # scale 1, no clip: ext.gae's bits
        one = torch.ones(1, device=DEV)
        ext.gae_rn(r, v, d, boot, one, 0.0, adv, ret, 0.99, 0.95, mode, seg)
        ext.gae(r, v, d, adv0, ret0, 0.99, 0.95, mode, seg)
        assert torch.equal(adv, adv0) and torch.equal(ret, ret0)


def test_gae_rn_binding_refusals():
    ext = _ext()
    T, E = 8, 20
    z = lambda *s, **k: torch.zeros(*s, device=k.pop("device", DEV), **k)
    ok = dict(r=z(T, E), v=z(T + 1, E), d=z(T, E), boot=torch.empty(0, device=DEV), scale=torch.ones(1, device=DEV),
              adv=z(T, E), ret=z(T, E))

    def call(mode=1, seg=0, **kw):
        a = dict(ok, **kw)
        ext.gae_rn(a["r"], a["v"], a["d"], a["boot"], a["scale"], 10.0, a["adv"], a["ret"], 0.99, 0.95, mode, seg)

    call()
    bad = [dict(r=z(T * E)), dict(r=z(T, E, dtype=torch.float64)), dict(v=z(T, E)), dict(d=z(T - 1, E)),
           dict(boot=z(T - 1, E)), dict(boot=z(T, E, device="cpu")), dict(scale=torch.ones(1)),
           dict(scale=torch.empty(0, device=DEV)), dict(scale=torch.ones(1, dtype=torch.float64, device=DEV)),
           dict(adv=z(T - 1, E)), dict(ret=z(T, E, device="cpu")), dict(mode=3), dict(seg=-1)]
    for kw in bad:
        with pytest.raises(RuntimeError):
            call(**kw)
    torch.cuda.synchronize()


# ---- the engine ----------------------------------------------------------------------------------------------------
def _worker(env_name, dtype, E=37, T=12, **kw):
    base = dict(device="gpu", env_name=env_name, num_envs=E, exploration_size=E * T, batch_size=E * T, num_epoch=1,
                dtype=dtype, hidden=(32, 32), reward_clip=0.0, reward_norm=True, max_episode_length=5,
                seed=30 if env_name == SYN else 1)
    base.update(kw)
    return DPPOWorker(dppo_preset(**base), DistContext(device=DEV))


@pytest.mark.parametrize("dtype", ["fp32", "bf16x3", "bf16", "fp8"])
@pytest.mark.parametrize("env_name", [SYN, PEND, CARTPOLE])
def test_engine_statistics_and_advantages(env_name, dtype):
    ext = _ext()
    w = _worker(env_name, dtype)
    eng = w.engine
    T, E = eng.T, eng.E
    assert eng.stepped_env == (env_name == CARTPOLE)
    acc = torch.zeros(E)
    chunks = []
    for it in range(3):
        shift = eng.ret_stats.shift().cpu().clone()
        m = w.iteration_step()
        torch.cuda.synchronize()
        r, d = eng.rewards.view(T, E).cpu().clone(), eng.dones.view(T, E).cpu().clone()
        assert float(d.sum()) >= E
        acc = oracle.return_scan(r, d, w.p.gamma, acc, shift)[0]
        assert torch.equal(eng.ret_acc.cpu(), acc)
        chunks.append((r, d))
        samples = replay64(chunks, w.p.gamma, E)
        assert eng.ret_stats.n == samples.size
        assert float(eng.ret_stats.scale) == pytest.approx(scale64(samples), rel=1e-6)
        assert m["return_std"] == pytest.approx(samples.std(), rel=1e-6)
        rs = (eng.rewards * eng.ret_stats.scale).clamp(-w.p.reward_norm_clip, w.p.reward_norm_clip).view(T, E)
        adv, ret = torch.empty(T, E, device=DEV), torch.empty(T, E, device=DEV)
        ext.gae(rs, eng.values_buf.view(T + 1, E), eng.dones.view(T, E), adv, ret, w.p.gamma, w.p.gae_param, 0,
                w.p.gae_segment())
        assert torch.equal(eng.adv.view(T, E), adv) and torch.equal(eng.ret.view(T, E), ret)


def test_engine_composes_with_bootstrap_time_limit_and_step_obs_norm():
    w = _worker(PEND, "bf16x3", bootstrap_time_limit=True)
    w.iteration_step()
    eng = w.engine
    T, E = eng.T, eng.E
    rs = (eng.rewards * eng.ret_stats.scale).clamp(-10, 10).view(T, E)
    adv, ret = torch.empty(T, E, device=DEV), torch.empty(T, E, device=DEV)
    _ext().gae_boot(rs, eng.values_buf.view(T + 1, E), eng.dones.view(T, E), eng.boot_buf.view(T, E), adv, ret,
                    w.p.gamma, w.p.gae_param, 0, 0)
    assert float(eng.boot_buf.abs().sum()) > 0 and torch.equal(eng.adv.view(T, E), adv)
    w2 = _worker(PEND, "bf16x3", obs_norm_update="step")
    m = w2.iteration_step()
    samples = replay64([(w2.engine.rewards.view(T, E).cpu(), w2.engine.dones.view(T, E).cpu())], w2.p.gamma, E)
    assert m["return_std"] == pytest.approx(samples.std(), rel=1e-6)


def test_scale_invariance_on_the_device_stepped_path():
    kw = dict(device="gpu", num_envs=64, exploration_size=64 * 16, batch_size=64 * 16, dtype="bf16x3")
    a1, r1 = first_adv(1, True, **kw)
    ak, rk = first_adv(1024, True, **kw)
    assert torch.equal(rk, r1 * 1024) and float(r1.abs().max()) > 0
    print("max |adv_k - adv_1|", float((ak - a1).abs().max()), "max |adv_1|", float(a1.abs().max()))
    assert float((ak - a1).abs().max()) <= 1e-5 * float(a1.abs().max())
    b1, _ = first_adv(1, False, **kw)
    bk, _ = first_adv(1024, False, **kw)
    assert float((bk - b1).abs().max()) > 100 * float(b1.abs().max())


def test_flag_off_is_the_plain_gae_and_holds_nothing():
    w = _worker(PEND, "bf16x3", reward_norm=False)
    eng = w.engine
    T, E = eng.T, eng.E
    w.init_stats()
    eng.rollout()
    eng.values()
    eng.gae()
    adv, ret = torch.empty(T, E, device=DEV), torch.empty(T, E, device=DEV)
    _ext().gae(eng.rewards.view(T, E), eng.values_buf.view(T + 1, E), eng.dones.view(T, E), adv, ret, w.p.gamma,
               w.p.gae_param, 0, w.p.gae_segment())
    assert torch.equal(eng.adv.view(T, E), adv) and torch.equal(eng.ret.view(T, E), ret)
    assert eng.ret_stats is None and eng.ret_acc is None
    assert not hasattr(eng, "ret_s12") and not hasattr(eng, "ret_part") and eng.metrics_buf.numel() == 11
    assert "return_std" not in w.iteration_step()


def _sync_mode_raises():
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        torch.ones(1, device=DEV).item()
        return False
    except RuntimeError:
        return True
    finally:
        torch.cuda.set_sync_debug_mode(prev)


@pytest.mark.parametrize("env_name", [PEND, CARTPOLE])
def test_iteration_step_does_not_sync(env_name):
    w = _worker(env_name, "bf16x3", phase_timing=0)
    w.iteration_step(defer=True)                 # (first call: allocations, kernel loads)
    torch.cuda.synchronize()
    if not _sync_mode_raises():
        pytest.skip("torch.cuda.set_sync_debug_mode('error') does not raise on .item() in this build")
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        m = w.iteration_step(defer=True)
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    torch.cuda.synchronize()
    assert m["return_std"] > 0 and w.engine.ret_stats.n == 2 * w.engine.T * w.engine.E
    assert w.finish_metrics()["return_std"] > 0


def test_resume_continues_bit_identically(tmp_path):
    from pytorch_dppo_amd.runtime.launcher import run_worker
    base = dict(device="gpu", env_name=PEND, num_processes=1, num_envs=32, exploration_size=32 * 8, batch_size=32 * 8,
                num_epoch=2, dtype="bf16x3", seed=4, hidden=(32, 32), reward_clip=0.0, reward_norm=True,
                max_episode_length=5)
    ctx = DistContext(device=DEV)
    w_full, _ = run_worker(dppo_preset(max_iters=3, **base), ctx, evaluator=False, quiet=True)
    ck = str(tmp_path / "ck")
    w_two, _ = run_worker(dppo_preset(max_iters=2, checkpoint_dir=ck, **base), ctx, evaluator=False, quiet=True)
    w_res, _ = run_worker(dppo_preset(max_iters=3, resume=ck, **base), ctx, evaluator=False, quiet=True)
    torch.cuda.synchronize()
    a, b = w_full.engine, w_res.engine
    assert w_res.iteration == 3 and a.ret_stats.n == b.ret_stats.n == 3 * 256
    assert not torch.equal(w_two.engine.ret_acc, a.ret_acc)
    for x, y in ((w_full.model.flat.data, w_res.model.flat.data), (a.adam_m, b.adam_m), (a.ret_acc, b.ret_acc),
                 (a.ret_stats.mean, b.ret_stats.mean), (a.ret_stats.mean_diff, b.ret_stats.mean_diff),
                 (a.ret_stats.scale, b.ret_stats.scale), (a.ret_stats.mean_f32, b.ret_stats.mean_f32), (a.adv, b.adv)):
        assert torch.equal(x, y)


def test_train_py_logs_return_std(tmp_path):
    path = tmp_path / "train.jsonl"
    cmd = [sys.executable, "train.py", "--device", "gpu", "--env-name", PEND, "--max-iters", "2", "--num-processes", "1",
           "--num-envs", "32", "--exploration-size", "1024", "--batch-size", "1024", "--num-epoch", "2", "--dtype",
           "bf16x3", "--reward-clip", "0", "--reward-norm", "true", "--normalize-adv", "true", "--log-jsonl", str(path)]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=170)
    assert r.returncode == 0, r.stderr[-3000:]
    recs = [json.loads(l) for l in path.read_text().splitlines()]
    assert len(recs) == 2
    for m in recs:
        assert all(math.isfinite(m[k]) for k in ("loss", "loss_value", "grad_norm", "return_std")), m
        assert m["return_std"] > 1.0
