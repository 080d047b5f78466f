"""Time what ``reward_norm`` adds (diagnostics; the numbers of profiles/reward_norm/README.md).

    python scripts/reward_norm_time.py [--out reward_norm_time.json] [--rounds 5] [--reps 20]

One process, interleaved round by round, HIP events around windows of ``--reps`` calls:

  * bench geometry (Humanoid-v2, 4096 envs x 16 steps, bf16x3), two engines with the same weights, flag off and on:
    ``gae()`` of each; with the flag on also the return scan + moment reduce (``return_moments()``), the merge
    (``merge_return_moments``: obs_merge with O = 1) and the two together.
  * the scan's two forms at 1 env x 2048 steps (ppo.py's geometry) and, for scale, at the bench geometry: the
    ``ret_scan`` binding with mode 1 (per-env lanes) and mode 2 (parallel in time), beside ``gae`` mode 1 / 2 at the
    same shape.

Prints one JSON line (median, min, max over the rounds, microseconds).  No threshold.
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from pytorch_dppo_amd.config import dppo_preset  # noqa: E402
from pytorch_dppo_amd.envs import get_spec, make_vec_env  # noqa: E402
from pytorch_dppo_amd.models.actor_critic import ActorCritic  # noqa: E402
from pytorch_dppo_amd.runtime.engine_hip import HipEngine  # noqa: E402
from pytorch_dppo_amd.utils.obs_stats import RunningObsStats  # noqa: E402

E, T, DTYPE = 4096, 16, "bf16x3"


def build(dev, flag):
    p = dppo_preset(device="gpu", env_name="Humanoid-v2", num_envs=E, exploration_size=E * T, batch_size=E * T,
                    dtype=DTYPE, reward_clip=0.0, reward_norm=flag)
    spec = get_spec(p.env_name)
    torch.manual_seed(0)
    model = ActorCritic(spec.obs_dim, spec.act_dim, p.hidden).to(dev)
    env = make_vec_env(spec, E, seed=p.seed, device=dev, max_episode_length=p.max_episode_length)
    stats = RunningObsStats(spec.obs_dim, dev)
    eng = HipEngine(p, model, env, stats, dev, 0)
    stats.observes(env.observe())
    eng.params_changed()
    eng.rollout()
    eng.values()
    return eng


def window_us(fn, reps):
    s, t = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    torch.cuda.synchronize()
    s.record()
    for _ in range(reps):
        fn()
    t.record()
    torch.cuda.synchronize()
    return s.elapsed_time(t) / reps * 1e3


def summary(v):
    return {"median": round(statistics.median(v), 2), "min": round(min(v), 2), "max": round(max(v), 2)}


def kernel_cases(dev, ext, t, e):
    g = torch.Generator().manual_seed(t + e)
    r = torch.randn(t, e, generator=g).to(dev)
    d = (torch.rand(t, e, generator=g) < 0.01).float().to(dev)
    v = torch.randn(t + 1, e, generator=g).to(dev)
    acc, shift = torch.zeros(e, device=dev), torch.zeros(1, device=dev)
    s12 = torch.zeros(2, dtype=torch.float64, device=dev)
    adv, ret, none = torch.empty(t, e, device=dev), torch.empty(t, e, device=dev), torch.empty(0, device=dev)
    out = {}
    for mode, name in ((1, "lane"), (2, "time")):
        part = torch.zeros(2 * ext.ret_scan_nblk(t, e, mode), dtype=torch.float64, device=dev)
        out[f"{t}x{e}.ret_scan_{name}_us"] = lambda mode=mode, part=part: ext.ret_scan(r, d, acc, shift, part, s12, none, 0.99, mode)
        out[f"{t}x{e}.gae_{name}_us"] = lambda mode=mode: ext.gae(r, v, d, adv, ret, 0.99, 0.95, mode, 0)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    off, on = build(dev, False), build(dev, True)
    n = float(T * E)

    def scan_merge():
        on.merge_return_moments(n, on.return_moments())

    s12 = on.return_moments()
    cases = {"off.gae_us": off.gae, "on.gae_rn_us": on.gae, "on.ret_scan_us": on.return_moments,
             "on.merge_us": lambda: on.merge_return_moments(n, s12), "on.ret_scan_merge_us": scan_merge}
    cases.update(kernel_cases(dev, on.ext, 2048, 1))
    cases.update(kernel_cases(dev, on.ext, T, E))
    res = {k: [] for k in cases}
    for _ in range(a.rounds + 1):          # (the first round is the warm-up: dropped below)
        for k, fn in cases.items():
            res[k].append(window_us(fn, a.reps))
    out = {"geometry": f"{E} envs x {T} steps, {DTYPE}", "rounds": a.rounds, "reps": a.reps,
           **{k: summary(v[1:]) for k, v in res.items()}}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
