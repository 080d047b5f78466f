"""Dump what every rollout path of HipEngine leaves behind, for a byte-wise comparison of two commits.

    python scripts/rollout_paths_dump.py --out DIR [--only SUBSTRING]

The file uses only the engine's public surface (plus ``_sn_cap``, which forces the per-step fallback of the
fused step-mode rollout), so the same file runs at either commit: run it once in each tree, each in a fresh
process, and ``cmp`` the two directories file by file.  For every configuration below it builds a HipEngine
with a fixed seed and runs two iterations of ``rollout()`` (or ``rollout_stepped()``), the worker's stats
merge, ``values()`` and ``gae()``; after each iteration it writes, as ``DIR/<config>/it<k>_<name>.npy``:
``x_buf`` (raw storage bytes), ``actions``, ``logp``, ``rewards``, ``dones``, ``values_buf``, ``adv``, ``ret``,
``trunc`` / ``x_fin`` / ``v_fin`` when they exist, the env's state / ``ep_len`` / ``ep_ret`` / step counter, the
returned ``s1`` / ``s2`` / ``shift`` / ``ep2``, and the fp32 images of ``stats`` and (step mode) ``local_stats``.

Sizes: 48 envs (three 16-env tiles), 6 steps, ``max_episode_length`` 4 (episodes end by the limit inside a
rollout; ``fin_K`` = 2).  Configurations:

  host-stepped env (a small env of gym's API, registered here)  x  dtype  x  host_policy torch | kernel
      x  obs_norm_update rollout | step
  Synthetic-17x6 | Pendulum-v0 | CartPoleContinuous-v1 with env_fused on | off  x  dtype
      x  path ``rollout()`` (the fused kernel; the stepped loop for the unfused cart-pole) | ``rollout_stepped()``
      x  obs_norm_update rollout | step (fused kernel: the cooperative launch, and the per-step fallback)
      x  bootstrap_time_limit off | on
  extras: ``rollout(stats_stream=...)`` on each path, ``compat`` (the raw bootstrap rows of ``values()``), and a
      full-batch geometry (8 steps) at which the fused rollout also writes the x^T operand (dumped too)

A combination the configuration or the engine refuses is skipped; ``DIR/skips.json`` lists each with the
refusal's text and ``DIR/configs.json`` the ones that ran.
"""
import argparse
import contextlib
import itertools
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from pytorch_dppo_amd.config import dppo_preset  # noqa: E402
from pytorch_dppo_amd.envs import get_spec, make_vec_env, register_env  # noqa: E402
from pytorch_dppo_amd.models.actor_critic import ActorCritic  # noqa: E402
from pytorch_dppo_amd.runtime.engine_hip import HipEngine  # noqa: E402
from pytorch_dppo_amd.utils.obs_stats import RunningObsStats  # noqa: E402

E, T, LIMIT, ITERS = 48, 6, 4, 2
DTYPES = ("bf16x3", "bf16", "fp8")
SYN, PEND, CARTPOLE, HOST = "Synthetic-17x6", "Pendulum-v0", "CartPoleContinuous-v1", "DumpGym-v0"


class _Box:
    def __init__(self, n):
        self.shape = (n,)


class _Spec:
    max_episode_steps = 12


class DumpGymEnv:
    """old-gym-API env: s' = 0.9 s + 0.1 tanh(a) (padded) + noise, r = -|a - tanh(s[:A])|^2, terminal when
    |s0| > 0.9 (some episodes end before the step limit, most by it)"""
    O, A = 5, 2

    def __init__(self):
        self.observation_space, self.action_space, self.spec = _Box(self.O), _Box(self.A), _Spec()
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
        return self.s.astype(np.float32), r, bool(abs(self.s[0]) > 0.9), {}


register_env(HOST, DumpGymEnv)


def configs():
    """(name, Params keywords, how to run it) of every configuration, in a fixed order"""
    out = []
    for dtype, pol, mode in itertools.product(DTYPES, ("torch", "kernel"), ("rollout", "step")):
        out.append((f"host-{pol}-{mode}-{dtype}",
                    dict(env_backend="gym", env_name=HOST, dtype=dtype, host_policy=pol, obs_norm_update=mode), {}))
    envs = (("syn", SYN, False), ("pend", PEND, False), ("cartfused", CARTPOLE, True), ("cart", CARTPOLE, False))
    for (tag, env, fused), dtype, path, boot in itertools.product(envs, DTYPES, ("rollout", "stepped"), (False, True)):
        # (the per-step fallback belongs to the fused kernel: the unfused cart-pole's rollout() is the stepped loop)
        modes = ("rollout", "step", "stepfb") if path == "rollout" and tag != "cart" else ("rollout", "step")
        for mode in modes:
            out.append((f"{tag}-{path}-{mode}-{'boot' if boot else 'noboot'}-{dtype}",
                        dict(env_name=env, env_fused=fused, dtype=dtype, bootstrap_time_limit=boot,
                             obs_norm_update="rollout" if mode == "rollout" else "step"),
                        dict(path=path, fallback=mode == "stepfb")))
    for dtype in DTYPES:
        out.append((f"extra-syn-fused-stream-{dtype}", dict(env_name=SYN, dtype=dtype), dict(path="rollout", stream=True)))
        out.append((f"extra-syn-fused-compat-{dtype}", dict(env_name=SYN, dtype=dtype, compat=True), dict(path="rollout")))
        out.append((f"extra-syn-fused-compat-heads-{dtype}",
                    dict(env_name=SYN, dtype=dtype, compat=True, update_kernels="heads"), dict(path="rollout")))
        out.append((f"extra-syn-fused-fullbatch-{dtype}", dict(env_name=SYN, dtype=dtype), dict(path="rollout", T=8, xT=True)))
    out.append(("extra-cart-stepped-stream-bf16x3", dict(env_name=CARTPOLE, dtype="bf16x3"), dict(path="rollout", stream=True)))
    out.append(("extra-host-kernel-stream-bf16x3",
                dict(env_backend="gym", env_name=HOST, dtype="bf16x3", host_policy="kernel"), dict(stream=True)))
    return out


def build(kw, steps, dev):
    """engine with stats seeded from the reset observations and a non-trivial log_std"""
    p = dppo_preset(device="gpu", num_envs=E, exploration_size=E * steps, batch_size=E * steps, max_episode_length=LIMIT,
                    seed=3, **kw)
    torch.manual_seed(0)
    if kw.get("env_backend") == "gym":
        env = make_vec_env(None, E, seed=p.seed, backend="gym", name=HOST)
        O, A = env.O, env.A
    else:
        spec = get_spec(p.env_name)
        env = make_vec_env(spec, E, seed=p.seed, device=dev, max_episode_length=LIMIT)
        O, A = spec.obs_dim, spec.act_dim
    model = ActorCritic(O, A, p.hidden).to(dev)
    stats = RunningObsStats(O, dev)
    eng = HipEngine(p, model, env, stats, dev, 0)
    stats.observes(eng.current_obs().to(dev))
    with torch.no_grad():
        model.flat.data[:model.num_outputs] = -0.3
    eng.params_changed()
    return eng


def raw(t):
    t = torch.as_tensor(t).detach().contiguous()
    if t.dtype == torch.bfloat16 or t.dtype == torch.bool:
        t = t.view(torch.uint8)
    return t.cpu().numpy()


def snapshot(eng, ro, how):
    env, st = eng.env, eng.stats
    out = {"x_buf": eng.x_buf.view(torch.uint8), "actions": eng.actions, "logp": eng.logp, "rewards": eng.rewards,
           "dones": eng.dones, "values_buf": eng.values_buf, "adv": eng.adv, "ret": eng.ret,
           "ep_len": env.ep_len, "ep_ret": env.ep_ret, "env_t": [env.t],
           "env_state": env.state if hasattr(env, "state") else env.observe(),
           "s1": ro["s1"], "s2": ro["s2"], "shift": ro["shift"], "ep2": ro["ep2"],
           "stats_mean_f32": st.mean_f32, "stats_inv_std_f32": st.inv_std_f32}
    if getattr(eng, "boot", False):
        out.update(trunc=eng.trunc, x_fin=eng.x_fin.view(torch.uint8), v_fin=eng.v_fin)
    if eng.p.obs_norm_update == "step":
        out.update(local_mean_f32=eng.local_stats.mean_f32, local_inv_std_f32=eng.local_stats.inv_std_f32)
    if how.get("xT"):
        out["xT"] = eng.xT.view(torch.uint8)
    return out


def run(name, eng, how, dev, root):
    if how.get("fallback"):
        eng._sn_cap = 0         # no env tile fits co-resident: rollout() takes the per-step launches
    side = torch.cuda.Stream(dev) if how.get("stream") else None
    meta = {"stepped_env": bool(eng.stepped_env), "host_env": bool(eng.host_env), "heads": bool(eng.heads)}
    os.makedirs(os.path.join(root, name), exist_ok=True)
    for it in range(ITERS):
        if how.get("path") == "stepped":
            ro = eng.rollout_stepped()
        elif side is not None:
            ro = eng.rollout(stats_stream=side)
        else:
            ro = eng.rollout()
        # the worker's merge (on the stats stream when the reduce ran there)
        with torch.cuda.stream(side) if side is not None else contextlib.nullcontext():
            eng.stats.merge_moments(ro["count"], ro["s1"], ro["s2"], ro["shift"])
        if side is not None:
            torch.cuda.current_stream(dev).wait_stream(side)
        eng.values()
        eng.gae()
        torch.cuda.synchronize(dev)
        eng.raise_if_failed()
        for k, v in snapshot(eng, ro, how).items():
            np.save(os.path.join(root, name, f"it{it}_{k}.npy"), raw(v))
    return meta


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--only", default="", help="run the configurations whose name contains this")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    os.makedirs(a.out, exist_ok=True)
    ran, skips = {}, {}
    for name, kw, how in configs():
        if a.only not in name:
            continue
        try:
            eng = build(kw, how.get("T", T), dev)
        except ValueError as e:          # the configuration or the engine's constructor refuses the combination
            skips[name] = str(e)
            print(name, "skipped: " + skips[name], flush=True)
            continue
        ran[name] = run(name, eng, how, dev, a.out)   # (an error past the constructor is a failure, not a skip)
        print(name, "ok", flush=True)
    for fn, d in (("configs.json", ran), ("skips.json", skips)):
        with open(os.path.join(a.out, fn), "w") as f:
            json.dump(d, f, indent=1, sort_keys=True)
    print(json.dumps({"ran": len(ran), "skipped": len(skips)}))


if __name__ == "__main__":
    main()
