"""Time the host-env rollout's policy step: per-step torch ops against one csrc/act.hip launch.

    python scripts/act_time.py [--out profiles/act/README.md] [--rounds 5] [--reps 4] [--tree LABEL]

One process, one commit: ``Params.host_policy`` "torch" (the default path: fp64 moments, normalise,
three linear layers, counter RNG, sample, log-prob as separate torch launches plus the fp32 staging
tensor and its encode copy) and "kernel" (one launch per step) alternate, round by round, on engines
with the same weights.  The env is a null host env whose ``step`` returns preallocated arrays, so
the policy step is what is timed; ``d2h`` rows copy the actions to the host every step first, as any
real host simulator must.  Humanoid dims, bf16x3, T = 64, E in {16, 256, 1024}; two warm-up
rollouts, then a host clock around each window of ``--reps`` rollouts, which ends in a device
synchronise.  The launch counts come from a ``torch.profiler`` window over one rollout of each path.

No threshold: the numbers are written between the ``act_time`` markers of ``--out`` (the rest of
the file is kept) and printed as one JSON line.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from pytorch_dppo_amd.config import dppo_preset  # noqa: E402
from pytorch_dppo_amd.models.actor_critic import ActorCritic  # noqa: E402
from pytorch_dppo_amd.runtime.engine_hip import HipEngine  # noqa: E402
from pytorch_dppo_amd.utils.obs_stats import RunningObsStats  # noqa: E402

BEGIN, END = "<!-- act_time:begin -->", "<!-- act_time:end -->"
O, A, T = 376, 17, 64


class NullHostEnv:
    """a host-stepped env that does no work: ``step`` returns preallocated tensors (``d2h``: after
    copying the actions to the host, the one thing every real host env needs from the device)"""
    host_stepped = True

    def __init__(self, E, d2h):
        g = torch.Generator().manual_seed(E)
        self.E, self.O, self.A, self.limit, self.t, self.d2h = E, O, A, 1000, 0, d2h
        self.device = torch.device("cpu")
        self.env_idx = torch.arange(E, dtype=torch.int64)
        self._obs = torch.randn(E, O, generator=g)
        self._rew = torch.zeros(E)
        self._done = torch.zeros(E, dtype=torch.bool)
        self._info = {"ep_return_sum": torch.tensor(0.0), "ep_count": torch.tensor(0)}

    def reset(self):
        return self._obs

    def observe(self):
        return self._obs

    def step(self, actions):
        if self.d2h:
            actions.to("cpu")
        self.t += 1
        return self._obs, self._rew, self._done, self._info

    def state_dict(self):
        return {"t": self.t}


def build(E, policy, d2h, dev):
    p = dppo_preset(device="gpu", env_backend="gym", env_name="Null-v0", num_envs=E, exploration_size=E * T,
                    batch_size=E * T, dtype="bf16x3", host_policy=policy)
    torch.manual_seed(0)
    model = ActorCritic(O, A).to(dev)
    env = NullHostEnv(E, d2h)
    stats = RunningObsStats(O, dev)
    eng = HipEngine(p, model, env, stats, dev, 0)
    stats.observes(eng.current_obs())
    return eng


def timed_rollout(eng, reps=1):
    """seconds per rollout: a host clock around ``reps`` rollouts that end in a device synchronise"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        eng.rollout()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


def launches_per_step(eng):
    """(kernels, copies / memsets) per env step of one rollout, from a torch.profiler window"""
    from torch.profiler import ProfilerActivity, profile
    try:
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            eng.rollout()
            torch.cuda.synchronize()
        dev_evts = [e for e in prof.events() if str(e.device_type).endswith("CUDA")]
    except Exception as e:   # no device tracing on this box
        print(f"torch.profiler window failed: {e}", file=sys.stderr)
        return None
    copies = sum(1 for e in dev_evts if "memcpy" in e.name.lower() or "memset" in e.name.lower())
    return {"kernels": (len(dev_evts) - copies) / T, "copies": copies / T}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/act/README.md")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=4, help="rollouts per timed window")
    ap.add_argument("--tree", default="", help="name of the measured tree (default: git describe)")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    res = {"dims": [O, A], "dtype": "bf16x3", "T": T, "rounds": a.rounds, "reps": a.reps, "rows": []}
    for d2h in (False, True):
        for E in (16, 256, 1024):
            engs = {pol: build(E, pol, d2h, dev) for pol in ("torch", "kernel")}
            for eng in engs.values():       # warm-up (allocations, LDS attribute, lazy inits)
                timed_rollout(eng)
                timed_rollout(eng)
            times = {pol: [] for pol in engs}
            for _ in range(a.rounds):       # alternate the two paths round by round
                for pol, eng in engs.items():
                    times[pol].append(timed_rollout(eng, a.reps) / T * 1e6)
            row = {"E": E, "d2h": d2h}
            for pol, eng in engs.items():
                ts = times[pol]
                row[pol] = {"us_per_step_median": statistics.median(ts), "us_min": min(ts), "us_max": max(ts),
                            "launches": launches_per_step(eng) if not d2h else None}
            res["rows"].append(row)
            del engs
            torch.cuda.empty_cache()
    res["tree"] = a.tree
    if not res["tree"]:
        try:
            res["tree"] = subprocess.run(["git", "describe", "--always", "--dirty"], capture_output=True, text=True,
                                         cwd=os.path.dirname(os.path.abspath(__file__))).stdout.strip() or "unknown"
        except OSError:
            res["tree"] = "unknown"
    props = torch.cuda.get_device_properties(dev)
    arch = getattr(props, "gcnArchName", "").split(":")[0]
    res["device"] = f"{props.name} ({arch}, {props.multi_processor_count} CUs)" if arch else props.name
    print(json.dumps(res))

    def cell(r):
        return f"{r['us_per_step_median']:.0f} us (min {r['us_min']:.0f}, max {r['us_max']:.0f})"

    def launches(r):
        n = r["launches"]
        return "n/a" if n is None else f"{n['kernels']:.1f} kernels + {n['copies']:.1f} copies"

    lines = [BEGIN, "", f"Measured by `scripts/act_time.py` on {res['device']} (tree `{res['tree']}`): Humanoid dims "
             f"({O} x {A}), bf16x3, T = {T}, a null host env; host clock around {a.reps} whole rollouts that end in a "
             f"device synchronise, divided by their steps; median of {a.rounds} alternating rounds after two warm-up "
             "rollouts (min / max = the spread).  `null`: the env ignores the actions; `d2h`: it copies them to the host every step first.",
             "", "| env | E | torch path / step | kernel path / step | kernel / torch |", "|---|---|---|---|---|"]
    for r in res["rows"]:
        ratio = r["kernel"]["us_per_step_median"] / r["torch"]["us_per_step_median"]
        lines.append(f"| {'d2h' if r['d2h'] else 'null'} | {r['E']} | {cell(r['torch'])} | {cell(r['kernel'])} | "
                     f"{ratio:.2f} |")
    lines += ["", "Device launches per env step (`torch.profiler` window over one rollout, divided by T; the copies "
              "include the host env's observation / reward / done uploads; the kernel path's per-rollout rows-only "
              "launch and `obs_reduce` are 2 / T):", "", "| E | torch path | kernel path |", "|---|---|---|"]
    for r in res["rows"]:
        if not r["d2h"]:
            lines.append(f"| {r['E']} | {launches(r['torch'])} | {launches(r['kernel'])} |")
    lines += ["", END]
    block = "\n".join(lines)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    text = open(a.out).read() if os.path.exists(a.out) else ""
    if BEGIN in text and END in text:
        text = text[:text.index(BEGIN)] + block + text[text.index(END) + len(END):]
    else:
        text = text + ("\n" if text and not text.endswith("\n") else "") + block + "\n"
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
