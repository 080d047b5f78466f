"""Time CartPole-v0's rollout and evaluation: fused (one launch each, the kernels' categorical head) against the
same env device-stepped, in one process.

    python scripts/categorical_fused_time.py [--out categorical_fused_time.json] [--reps 5]

E = 1024, T = 16, hidden 100,100, bf16x3; two engines with the same weights and statistics, one with ``env_fused``.
Per repetition and variant: device events around a window of back-to-back calls (``--stepped-window`` rollouts of the
device-stepped path, 16x as many of the fused kernel's, so that neither window is a few milliseconds), the variants
interleaved repetition by repetition; two warm-up windows each.  The same for one evaluation of 1024 envs (at the
env's 200-step limit, the policy at its initialisation).  Prints one JSON line (and writes it to ``--out``):
microseconds per rollout / per evaluation, the median, min and max over the repetitions.  No threshold.
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

ENV, E, T, DTYPE, HIDDEN = "CartPole-v0", 1024, 16, "bf16x3", (100, 100)
FUSED_X = 16     # the fused variant's calls per window, as a multiple of the stepped variant's


def build(dev, env_fused):
    p = dppo_preset(device="gpu", env_name=ENV, num_envs=E, exploration_size=E * T, batch_size=E * T, dtype=DTYPE,
                    hidden=HIDDEN, env_fused=env_fused)
    spec = get_spec(ENV)
    torch.manual_seed(0)
    model = ActorCritic(spec.obs_dim, spec.act_dim, p.hidden).to(dev)
    env = make_vec_env(spec, E, seed=p.seed, device=dev, max_episode_length=p.max_episode_length)
    stats = RunningObsStats(spec.obs_dim, dev)
    eng = HipEngine(p, model, env, stats, dev, 0)
    stats.observes(env.observe())
    eng.params_changed()
    return eng


def window_us(fn, calls):
    """microseconds per call: device events around ``calls`` back-to-back calls"""
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(calls):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1e3 / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--stepped-window", type=int, default=64, help="calls per window of the device-stepped variant")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    stepped, fused = build(dev, False), build(dev, True)
    assert stepped.stepped_env and not fused.stepped_env and fused.kernel_dist == 1
    variants = {
        "rollout": {"stepped": stepped.rollout, "fused": fused.rollout},
        "evaluate": {"stepped": lambda: stepped.evaluate(E, False), "fused": lambda: fused.evaluate(E, False)},
    }
    calls = {"stepped": a.stepped_window, "fused": a.stepped_window * FUSED_X}
    res = {"env": ENV, "E": E, "T": T, "dtype": DTYPE, "hidden": list(HIDDEN), "reps": a.reps, "calls_per_window": calls,
           "device": torch.cuda.get_device_properties(dev).name, "unit": "us per call (device events)"}
    for what, fns in variants.items():
        for k, fn in fns.items():            # warm-up (allocations, code objects, lazy inits)
            window_us(fn, 2)
            window_us(fn, 2)
        if what == "rollout":                # same seed, same keys, same number of rollouts: the same envs
            res["rollout_state_max_gap"] = float((stepped.env.state - fused.env.state).abs().max())
            res["rollout_dones_equal"] = bool(torch.equal(stepped.dones, fused.dones))
            res["rollout_actions_equal"] = bool(torch.equal(stepped.actions, fused.actions))
        else:
            (rs, ls), (rf, lf) = stepped.evaluate(E, False), fused.evaluate(E, False)
            res["evaluate_lengths_equal"] = bool(torch.equal(ls, lf))
            res["evaluate_length_mean"] = float(lf.float().mean())
        times = {k: [] for k in fns}
        for _ in range(a.reps):              # interleaved
            for k, fn in fns.items():
                times[k].append(window_us(fn, calls[k]))
        res[what] = {k: {"median": statistics.median(v), "min": min(v), "max": max(v)} for k, v in times.items()}
        res[what]["stepped_over_fused"] = res[what]["stepped"]["median"] / res[what]["fused"]["median"]
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
