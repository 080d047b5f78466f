"""``bootstrap_time_limit`` on the GPU engine: the fused rollout kernel's ``trunc`` / ``x_fin`` outputs (csrc/rollout.hip
FIN), the GAE kernels' ``boot`` operand, the device-stepped path (``env_advance_fin``), the engine's
``rollout -> values -> gae`` against ``TorchEngine``, the bindings' refusals and ``train.py`` end to end.

Geometry of the rollout cases, as tests/test_gpu_rollout_episodes.py: 45 envs = two full 16-env tiles + 13 rows, 24
steps, limit 7 (so ``x_fin`` has K = 4 slots), episode lengths placed in [0, limit) so that the truncations of a tile
fall on different steps.  The fp64 reference is tests/test_time_limit_bootstrap.py's."""
import json
import math
import subprocess
import sys

import pytest
import torch

from pytorch_dppo_amd.ops import oracle
from test_gpu_tensor_env import CARTPOLE, DEV, ROOT, _close, _engine, _params, _sync_mode_raises, _torch_engine
from test_rollout_replay import copy_start, placement
from test_time_limit_bootstrap import (PEND, SYN, SYN_SEED, assert_truncation_preconditions, compare_boot,
                                       expected_boot)

pytestmark = pytest.mark.gpu

E, T, LIMIT, K = 45, 24, 7, 4
KINDS = {0: SYN, 1: PEND, 2: CARTPOLE}
DTYPES = ["fp32", "bf16x3", "bf16", "fp8"]


def _ext():
    from pytorch_dppo_amd.ops import native
    return native.load()


def _case_params(kind, dtype, flag, limit=LIMIT, E=E, T=T, env_name=None, **kw):
    name = env_name or KINDS[kind]
    if kind == 2:
        kw.setdefault("env_fused", True)
    return _params(name, dtype, E=E, T=T, max_episode_length=limit, seed=SYN_SEED if name == SYN else 1,
                   bootstrap_time_limit=flag, **kw)


def _snapshot(eng, env, ro):
    """everything a rollout leaves behind, as clones of the raw tensors"""
    torch.cuda.synchronize()
    out = {"x_buf": eng.x_buf, "actions": eng.actions, "logp": eng.logp, "rewards": eng.rewards, "dones": eng.dones,
           "env.state": env.state, "ep_len": env.ep_len, "ep_ret": env.ep_ret, "mom": eng.mom, "epstat": eng.epstat,
           "s1": ro["s1"], "s2": ro["s2"], "ep_return_sum": ro["ep_return_sum"], "ep_count": ro["ep_count"]}
    out = {k: v.detach().clone() for k, v in out.items()}
    out["t"] = env.t
    if eng.boot:
        out["trunc"], out["x_fin"] = eng.trunc.clone(), eng.x_fin.clone()
    return out


_RUNS = {}


def _fused_run(kind, dtype, flag, limit=LIMIT, E=E, T=T, env_name=None, place_limit=LIMIT):
    """one fused rollout from the placed start (shared by the tests below; never modified)"""
    key = (kind, dtype, flag, limit, E, T, env_name, place_limit)
    if key not in _RUNS:
        p = _case_params(kind, dtype, flag, limit, E, T, env_name)
        eng, model, env, stats = _engine(p)
        assert not eng.stepped_env and eng.boot == flag
        start = placement(env, place_limit, 0, 0)
        eng.load_env_state(copy_start(start))
        ro = eng.rollout()
        _RUNS[key] = (_snapshot(eng, env, ro), start, eng, model, env, stats, p)
    return _RUNS[key]


def _assert_same_rollout(on, off):
    for k, v in off.items():
        if torch.is_tensor(v):
            assert torch.equal(on[k], v), k
        else:
            assert on[k] == v, k


# ---- nothing else moves ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", [0, 1, 2])
def test_flag_leaves_the_rollout_bit_identical(kind, dtype):
    on, off = _fused_run(kind, dtype, True)[0], _fused_run(kind, dtype, False)[0]
    assert float(off["dones"].sum()) >= 3 * E and "x_fin" in on and "x_fin" not in off
    _assert_same_rollout(on, off)
    # the kernel did take its cold branch: truncations were flagged
    assert float(on["trunc"].sum()) > 100 and bool((on["trunc"] <= on["dones"]).all())


def test_flag_leaves_the_rollout_bit_identical_at_humanoid_widths():
    kw = dict(limit=3, E=16, T=8, env_name="Humanoid-v2", place_limit=3)
    on, off = _fused_run(0, "bf16x3", True, **kw)[0], _fused_run(0, "bf16x3", False, **kw)[0]
    _assert_same_rollout(on, off)
    assert float(on["trunc"].sum()) >= 2 * 16


def test_flag_leaves_the_rollout_bit_identical_on_the_four_wave_form():
    ext = _ext()
    ext.set_rollout_waves(4)
    try:
        runs = []
        for flag in (True, False):
            p = _case_params(0, "bf16x3", flag)
            eng, model, env, stats = _engine(p)
            eng.load_env_state(copy_start(placement(env, LIMIT, 0, 0)))
            runs.append(_snapshot(eng, env, eng.rollout()))
        torch.cuda.synchronize()
    finally:
        ext.set_rollout_waves(8)
    _assert_same_rollout(runs[0], runs[1])
    # and the four-wave form writes the final rows the eight-wave form writes
    ref = _fused_run(0, "bf16x3", True)[0]
    assert torch.equal(runs[0]["trunc"], ref["trunc"]) and torch.equal(runs[0]["x_fin"], ref["x_fin"])


# ---- the final rows are the rows the kernel would have stored ---------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", [0, 1, 2])
def test_final_rows_equal_the_next_rows_of_a_run_without_the_limit(kind, dtype):
    """Under a limit no env reaches, the synthetic env's keyed ends and every state up to an env's first limit end are
    those of the limit-7 run, so that run's next buffer row is the final row, bit for bit (for a truncation at the
    last step it is the bootstrap row)."""
    on = _fused_run(kind, dtype, True)[0]
    free = _fused_run(kind, dtype, False, limit=10000)[0]
    trunc = on["trunc"].view(T, E) > 0.5
    # (the free run ends by keyed draws alone; the cart-pole, never reset by a limit, also falls over later on:
    # until an env's first limit end both runs hold the same states either way)
    assert kind == 2 or float(free["dones"].sum()) <= 10
    d0 = on["x_fin"].shape[-1]
    xf, xb = on["x_fin"].view(K, E, d0), free["x_buf"].view(T + 1, E, d0)
    first = torch.where(trunc.any(0), trunc.float().argmax(0), torch.full((E,), -1, device=DEV))
    assert bool((first >= 0).all()) and int(first.max()) >= LIMIT - 1 and int(first.min()) == 0
    for e in range(E):
        t = int(first[e])
        assert torch.equal(xf[t // LIMIT, e], xb[t + 1, e]), (t, e)


@pytest.mark.parametrize("kind", [0, 1, 2])
def test_truncation_at_the_last_step_takes_the_bootstrap_row(kind):
    """T = limit and fresh episodes: every env is truncated at step T - 1, and its final row is row T of the run
    without the limit"""
    kw = dict(limit=LIMIT, E=E, T=LIMIT, place_limit=1)
    on = _fused_run(kind, "bf16x3", True, **kw)[0]
    free = _fused_run(kind, "bf16x3", False, **{**kw, "limit": 10000})[0]
    tr = on["trunc"].view(LIMIT, E)
    last = tr[LIMIT - 1] > 0.5
    # (the synthetic env 20 draws its keyed end at step 5 and starts a new episode: it alone is not truncated)
    assert float(tr[:LIMIT - 1].sum()) == 0 and int(last.sum()) == (E - 1 if kind == 0 else E)
    d0 = on["x_fin"].shape[-1]
    assert on["x_fin"].shape[0] == E                              # K = 1
    assert torch.equal(on["x_fin"].view(E, d0)[last], free["x_buf"].view(LIMIT + 1, E, d0)[LIMIT][last])
    assert bool((on["x_fin"].view(E, d0)[~last] == 0).all())


# ---- against the fp64 replay -------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", [0, 1])
def test_trunc_and_final_rows_match_replay(kind, dtype):
    on, start, eng, model, env, stats, p = _fused_run(kind, dtype, True)
    exp = expected_boot(env, model, stats, p, eng.key_action, start, on["actions"].view(T, E, -1))
    assert_truncation_preconditions(exp, kind == 0)
    got = {"trunc": on["trunc"], "x_fin": eng.decode(on["x_fin"])}
    compare_boot(got, exp, lowp=dtype in ("bf16", "fp8"))


def test_fused_cartpole_terminal_on_the_limit_step_is_not_truncated():
    """the placed states of the CPU test: row 0 crosses 12 degrees on the step its episode reaches the limit"""
    limit = 4
    p = _case_params(2, "fp32", True, limit=limit, E=3, T=1)
    eng, model, env, stats = _engine(p)
    with torch.no_grad():
        model.flat.data[model.num_outputs:] = 0.0                   # mu = 0, sigma = exp(-0.3): |force| stays small
    eng.params_changed()
    state = torch.tensor([[0.0, 0.0, 0.2090, 1.0], [0.1, 0.0, 0.01, 0.0], [0.0, 0.0, 0.0, 0.0]])
    start = {"state": state, "ep_len": torch.tensor([limit - 1, limit - 1, 0], dtype=torch.int32),
             "ep_ret": torch.zeros(3), "t": 0}
    eng.load_env_state(copy_start(start))
    eng.rollout()
    torch.cuda.synchronize()
    assert eng.dones.tolist() == [1.0, 1.0, 0.0] and eng.trunc.tolist() == [0.0, 1.0, 0.0]
    x = eng.decode(eng.x_fin).view(1, 3, -1)
    assert bool((x[0, 0] == 0).all()) and bool((x[0, 2] == 0).all()) and float(x[0, 1, 4]) == 1.0


# ---- the GAE kernels ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T_,E_", [(24, 45), (300, 3)])
@pytest.mark.parametrize("seg", [0, 5])
@pytest.mark.parametrize("mode", [1, 2])
def test_gae_boot_kernels_match_oracle(mode, seg, T_, E_):
    ext = _ext()
    g = torch.Generator(device="cpu").manual_seed(T_ * 7 + E_)
    r = torch.randn(T_, E_, generator=g).to(DEV)
    v = torch.randn(T_ + 1, E_, generator=g).to(DEV)
    d = (torch.rand(T_, E_, generator=g) < 0.15).float().to(DEV)
    # two thirds of the ends truncated, each with a value of its own
    boot = (d * (torch.rand(T_, E_, generator=g) < 0.67).float().to(DEV) * torch.randn(T_, E_, generator=g).to(DEV))
    assert int((boot != 0).sum()) >= 3 and int(((boot == 0) & (d == 1)).sum()) >= 1
    adv, ret = torch.empty(T_, E_, device=DEV), torch.empty(T_, E_, device=DEV)
    ext.gae_boot(r, v, d, boot, adv, ret, 0.99, 0.95, mode, seg)
    a_ref, r_ref = oracle.gae(r.double(), v.double(), d.double(), 0.99, 0.95, segment=seg, boot=boot.double())
    assert torch.allclose(adv.double(), a_ref, atol=2e-5, rtol=2e-5)
    assert torch.allclose(ret.double(), r_ref, atol=2e-5, rtol=2e-5)
    a_plain, _ = oracle.gae(r.double(), v.double(), d.double(), 0.99, 0.95, segment=seg)
    assert float((a_ref - a_plain).abs().max()) > 1e-2              # the operand matters
    # a null boot: ext.gae's bits
    adv0, ret0 = torch.empty_like(adv), torch.empty_like(ret)
    adv1, ret1 = torch.empty_like(adv), torch.empty_like(ret)
    ext.gae(r, v, d, adv0, ret0, 0.99, 0.95, mode, seg)
    ext.gae_boot(r, v, d, torch.empty(0, device=DEV), adv1, ret1, 0.99, 0.95, mode, seg)
    assert torch.equal(adv0, adv1) and torch.equal(ret0, ret1)


# ---- the device-stepped path against the fused kernel ----------------------------------------------------------------
@pytest.mark.parametrize("kind", [0, 1, 2])
def test_rollout_stepped_bootstrap_matches_fused(kind):
    dtype = "bf16x3"
    on, start, eng_f, model_f, env_f, stats_f, p_f = _fused_run(kind, dtype, True)
    p = _case_params(kind, dtype, True, env_fused=False)
    eng, model, env, stats = _engine(p)
    assert eng.stepped_env == (kind == 2)
    assert torch.equal(model.flat.data, model_f.flat.data)
    eng.load_env_state(copy_start(start))
    eng.rollout_stepped()
    eng.values()
    eng.gae()
    # (the fused engine's buffers still hold the shared run: nothing above wrote them)
    eng_f.values()
    eng_f.gae()
    torch.cuda.synchronize()
    assert torch.equal(eng.dones, on["dones"]) and torch.equal(eng.trunc, on["trunc"])
    w = (on["trunc"].view(T, E) > 0.5)
    written = torch.zeros(K, E, dtype=torch.bool, device=DEV)
    for t in range(T):
        written[t // LIMIT] |= w[t]
    xs, xf = eng.decode(eng.x_fin).view(K, E, -1), eng_f.decode(on["x_fin"]).view(K, E, -1)
    assert int(written.sum()) == int(w.sum()) > 100
    _close(xs[written], xf[written], dtype, "x_fin")
    assert bool((xs[~written] == 0).all()) and bool((xf[~written] == 0).all())
    _close(eng.v_fin.view(K, E)[written], eng_f.v_fin.view(K, E)[written], dtype, "v_fin")
    _close(eng.adv, eng_f.adv, dtype, "adv")
    _close(eng.ret, eng_f.ret, dtype, "ret")


def test_stepped_rollout_with_the_flag_does_not_sync():
    p = _params(CARTPOLE, "bf16x3", E=45, T=8, max_episode_length=3, bootstrap_time_limit=True)
    eng, model, env, stats = _engine(p)
    assert eng.stepped_env
    eng.rollout_stepped()                       # (first call: allocations, kernel loads)
    eng.values()
    eng.gae()
    torch.cuda.synchronize()
    if not _sync_mode_raises():
        pytest.skip("torch.cuda.set_sync_debug_mode('error') does not raise on .item() in this build")
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        ro = eng.rollout_stepped()
        eng.values()
        eng.gae()
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    torch.cuda.synchronize()
    assert float(ro["ep_count"]) == float(eng.trunc.sum()) >= 2 * 45 and bool(torch.isfinite(eng.adv).all())


# ---- engine against engine -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["fp32", "bf16x3"])
def test_engine_bootstrap_matches_torch_engine(dtype):
    p = _params(PEND, dtype, E=32, T=8, max_episode_length=5, bootstrap_time_limit=True)
    eng, model, env, stats = _engine(p)
    ref = _torch_engine(p, model, stats)
    assert ref.boot and eng.boot and eng.fin_K == ref.fin_K == 2
    for e in (eng, ref):
        e.rollout()
        e.values()
        e.gae()
    torch.cuda.synchronize()
    # precondition, on the oracle alone: at the truncated steps the flag moves the advantages beyond the tolerance
    tr = ref.trunc > 0.5
    plain, _ = oracle.gae(ref.rewards, ref.values_buf, ref.dones, p.gamma, p.gae_param, segment=p.gae_segment())
    # (a truncated step moves by gamma |V(final row)|, and a value may happen to lie near 0: nine in ten must clear it)
    moved = (ref.adv - plain).abs()[tr]
    tol = 2e-4 + 1e-4 * float(ref.adv.abs().max())
    assert int(tr.sum()) >= 32 and float((moved > tol).float().mean()) >= 0.9 and float(moved.max()) > 100 * tol
    print("advantages moved by", float(moved.min()), "..", float(moved.max()))
    assert torch.equal(eng.trunc.view(8, 32), ref.trunc) and torch.equal(eng.dones.view(8, 32), ref.dones)
    _close(eng.v_fin.view(2, 32), ref.v_fin, dtype, "v_fin")
    _close(eng.adv.view(8, 32), ref.adv, dtype, "adv")
    _close(eng.ret.view(8, 32), ref.ret, dtype, "ret")


# ---- the bindings refuse what the grid does not cover --------------------------------------------------------------
def test_bindings_refuse_bad_final_buffers():
    p = _case_params(1, "bf16x3", True)
    eng, model, env, stats = _engine(p)
    watched = [eng.x_buf, eng.actions, eng.dones, eng.trunc, eng.x_fin, env.state, env.ep_len]
    before = [t.clone() for t in watched]
    good = (eng.x_fin, eng.fin_K)

    def launch():
        eng._launch_rollout(eng.T, 0, env.t, eng.stats, eng.stats.shift())

    bad = [(eng.x_fin[:-1], K),                                         # x_fin one row short of fin_K * E rows
           (eng.x_fin, K - 1),                                          # fin_K below ceil(T / limit)
           (torch.zeros(K * E + E, eng.d0, dtype=eng.sdtype, device=DEV), K + 2),   # fin_K beyond the buffer
           (eng.x_fin.view(torch.float32), K),                          # wrong dtype
           (eng.x_fin.view(K * E, -1).t(), K)]                          # not contiguous
    try:
        for x_fin, fin_K in bad:
            eng.x_fin, eng.fin_K = x_fin, fin_K
            with pytest.raises(RuntimeError):
                launch()
        eng.x_fin, eng.fin_K = good
        tr = eng.trunc
        for t_bad in (tr[:-1], tr.double()):
            eng.trunc = t_bad
            with pytest.raises(RuntimeError):
                launch()
        eng.trunc = tr
    finally:
        eng.x_fin, eng.fin_K = good
    torch.cuda.synchronize()
    for x, y in zip(before, watched):                                   # every refusal came before a launch
        assert torch.equal(x, y)
    launch()
    torch.cuda.synchronize()
    assert float(eng.trunc.sum()) > 100
    # env_advance_fin and gae_boot
    ext = _ext()
    f = lambda *s: torch.zeros(*s, device=DEV)   # noqa: E731
    n = 37
    ok = [f(n), torch.zeros(n, dtype=torch.bool, device=DEV), f(n, 4), f(n, 4), f(n, 4),
          torch.zeros(n, dtype=torch.int32, device=DEV), f(n), f(n), f(n), f(3, 2), 3, 1.0, True]
    rows = lambda k=n, w=32: torch.zeros(k, w, dtype=torch.bfloat16, device=DEV)   # noqa: E731
    for src, dst, trow in [(rows(n - 1), rows(), f(n)), (rows(), rows(n - 1), f(n)), (rows(), rows().float(), f(n)),
                           (rows(), rows(), f(n - 1)), (rows(), rows(), f(n).double()), (rows(w=12), rows(w=12), f(n)),
                           (rows(), rows(n, 64)[:, :32], f(n))]:
        with pytest.raises(RuntimeError):
            ext.env_advance_fin(*ok, src, dst, trow)
    ext.env_advance_fin(*ok, rows(), rows(), f(n))
    a, r_ = f(5, 3), f(5, 3)
    for boot in (f(4, 3), f(5, 3).double()):
        with pytest.raises(RuntimeError):
            ext.gae_boot(f(5, 3), f(6, 3), f(5, 3), boot, a, r_, 0.99, 0.95, 1, 0)
    torch.cuda.synchronize()


def test_env_advance_fin_copies_exactly_the_truncated_rows():
    ext = _ext()
    n, S, limit, W = 300, 3, 4, 32                                      # two workgroups, the second partial
    g = torch.Generator(device="cpu").manual_seed(3)
    reward = torch.rand(n, generator=g).to(DEV)
    terminal = (torch.rand(n, generator=g) < 0.3).to(DEV)
    ep_len = (torch.arange(n, dtype=torch.int32) % limit).to(DEV)
    mk = lambda: dict(state=torch.zeros(n, S, device=DEV), ep_len=ep_len.clone(), ep_ret=torch.zeros(n, device=DEV),   # noqa: E731
                      rew=torch.zeros(n, device=DEV), done=torch.zeros(n, device=DEV),
                      epstat=torch.zeros((n + 15) // 16, 2, device=DEV))
    new_state, reset_state = torch.randn(n, S, generator=g).to(DEV), torch.randn(n, S, generator=g).to(DEV)
    src = torch.randn(n, W, generator=g).to(DEV).to(torch.bfloat16)
    dst = torch.full((n + 16, W), -7.0, dtype=torch.bfloat16, device=DEV)
    trow = torch.full((n + 16,), -7.0, device=DEV)
    a, b = mk(), mk()
    ext.env_advance_fin(reward, terminal, new_state, reset_state, a["state"], a["ep_len"], a["ep_ret"], a["rew"],
                        a["done"], a["epstat"], limit, 1.0, True, src, dst[:n], trow[:n])
    ext.env_advance(reward, terminal, new_state, reset_state, b["state"], b["ep_len"], b["ep_ret"], b["rew"], b["done"],
                    b["epstat"], limit, 1.0, True)
    torch.cuda.synchronize()
    for k in a:
        assert torch.equal(a[k], b[k]), k                               # everything else as env_advance
    want = (ep_len + 1 >= limit) & ~terminal
    assert int(want.sum()) > 20 and int(((ep_len + 1 >= limit) & terminal).sum()) > 5
    assert torch.equal(trow[:n], want.float()) and bool((trow[n:] == -7.0).all())
    assert torch.equal(dst[:n][want], src[want]) and bool((dst[:n][~want] == -7.0).all()) and bool((dst[n:] == -7).all())


# ---- end to end ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env_name,extra", [(PEND, []), (CARTPOLE, []), (CARTPOLE, ["--env-fused", "true"])])
def test_train_py_with_the_flag(tmp_path, env_name, extra):
    path = tmp_path / "train.jsonl"
    cmd = [sys.executable, "train.py", "--device", "gpu", "--env-name", env_name, "--bootstrap-time-limit", "true",
           "--max-iters", "3", "--num-processes", "1", "--num-envs", "32", "--exploration-size", "1024", "--batch-size",
           "1024", "--num-epoch", "2", "--dtype", "bf16x3", "--max-episode-length", "20", "--log-jsonl", str(path)] + extra
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=170)
    assert r.returncode == 0, r.stderr[-3000:]
    its = [json.loads(l) for l in path.read_text().splitlines()]
    its = [x for x in its if "eval_iteration" not in x]
    assert len(its) == 3
    for m in its:
        assert all(math.isfinite(m[k]) for k in ("loss", "loss_clip", "loss_value", "grad_norm", "mean_ep_return")), m
        assert m["ep_count"] > 0
