"""Time what ``bootstrap_time_limit`` adds (diagnostics; the numbers of profiles/time_limit/README.md).

    python scripts/time_limit_time.py [--out time_limit_time.json] [--rounds 5] [--reps 20]

One process, interleaved round by round, HIP events around windows of ``--reps`` calls:

  * bench geometry (Humanoid-v2, 4096 envs x 16 steps, bf16x3), three engines with the same weights: flag off; flag on
    with the env's own limit (1000: a rollout of 16 steps almost never meets it, the cold branch stays cold); flag
    on with ``max_episode_length`` 8 (every env is truncated twice per rollout, every tile takes the cold branch on
    two of the 16 steps).  Per engine: ``rollout()``, ``values()``, ``gae()`` in microseconds.
  * the device-stepped path (CartPoleContinuous-v1, 4096 envs x 16 steps, bf16x3): ``rollout_stepped()`` per env step
    with and without the flag.

Prints one JSON line (median, min, max over the rounds).  No threshold.
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


def build(dev, env_name, flag, limit=10000):
    p = dppo_preset(device="gpu", env_name=env_name, num_envs=E, exploration_size=E * T, batch_size=E * T, dtype=DTYPE,
                    max_episode_length=limit, bootstrap_time_limit=flag)
    spec = get_spec(env_name)
    torch.manual_seed(0)
    model = ActorCritic(spec.obs_dim, spec.act_dim, p.hidden).to(dev)
    env = make_vec_env(spec, E, seed=p.seed, device=dev, max_episode_length=limit)
    stats = RunningObsStats(spec.obs_dim, dev)
    eng = HipEngine(p, model, env, stats, dev, 0)
    stats.observes(env.observe())
    eng.params_changed()
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    fused = {"off": build(dev, "Humanoid-v2", False), "on_limit_1000": build(dev, "Humanoid-v2", True),
             "on_limit_8": build(dev, "Humanoid-v2", True, limit=8), "off_limit_8": build(dev, "Humanoid-v2", False, limit=8)}
    stepped = {"off": build(dev, "CartPoleContinuous-v1", False, limit=8),
               "on": build(dev, "CartPoleContinuous-v1", True, limit=8)}
    res = {f"{k}.{ph}": [] for k in fused for ph in ("rollout_us", "values_us", "gae_us")}
    res.update({f"stepped_{k}.step_us": [] for k in stepped})
    for _ in range(a.rounds + 1):          # (the first round is the warm-up: dropped below)
        for k, eng in fused.items():
            for ph in ("rollout", "values", "gae"):
                res[f"{k}.{ph}_us"].append(window_us(getattr(eng, ph), a.reps))
        for k, eng in stepped.items():
            res[f"stepped_{k}.step_us"].append(window_us(eng.rollout_stepped, max(1, a.reps // 4)) / T)
    out = {"geometry": f"{E} envs x {T} steps, {DTYPE}", "rounds": a.rounds, "reps": a.reps,
           "truncated_per_rollout": {k: float(eng.trunc.sum()) for k, eng in fused.items() if eng.boot},
           **{k: summary(v[1:]) for k, v in res.items()}}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
