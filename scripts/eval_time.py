"""Time the batched GPU evaluation against the CPU evaluator's episode loop, same snapshot, same box.

    python scripts/eval_time.py [--out profiles/eval/README.md] [--reps 5] [--tree LABEL]

* ``HipEngine.evaluate`` (csrc/eval.hip): Humanoid-v2 dims, bf16x3, max_episode_length 1000,
  256 and 4096 evaluation envs, stochastic (the reference's rule); HIP events around each call
  after a warm-up, median of ``--reps``.
* ``run_episode`` (runtime/evaluator.py, what the evaluator process runs per snapshot): one env at
  batch 1 through torch CPU ops, on a CPU copy of the same parameters and statistics.

``--tree``: the name of the measured tree where ``git describe`` cannot give one (a copy of the
sources without their repository).

No threshold: the numbers are written between the ``eval_time`` markers of ``--out`` (the rest of
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
from pytorch_dppo_amd.envs import make_vec_env  # noqa: E402
from pytorch_dppo_amd.models.actor_critic import ActorCritic  # noqa: E402
from pytorch_dppo_amd.parallel.dist import DistContext  # noqa: E402
from pytorch_dppo_amd.runtime.evaluator import run_episode  # noqa: E402
from pytorch_dppo_amd.runtime.worker import DPPOWorker  # noqa: E402
from pytorch_dppo_amd.utils import rng  # noqa: E402
from pytorch_dppo_amd.utils.obs_stats import RunningObsStats  # noqa: E402

BEGIN, END = "<!-- eval_time:begin -->", "<!-- eval_time:end -->"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/eval/README.md")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cpu-episodes", type=int, default=3)
    ap.add_argument("--tree", default="", help="name of the measured tree (default: git describe)")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    p = dppo_preset(device="gpu", env_name="Humanoid-v2", num_envs=1024, exploration_size=16384, batch_size=16384,
                    dtype="bf16x3", max_episode_length=1000)
    w = DPPOWorker(p, DistContext(device=dev))
    for _ in range(2):                      # a trained-a-little snapshot with merged statistics
        w.iteration_step()
    eng = w.engine
    res = {"env": p.env_name, "dtype": p.dtype, "max_episode_length": p.max_episode_length, "gpu": []}
    for n in (256, 4096):
        eng.evaluate(n, False)              # warm-up (LDS attribute, output buffers)
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            ret, ln = eng.evaluate(n, False)
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        steps = int(ln.sum())
        med = statistics.median(ms)
        res["gpu"].append({"eval_envs": n, "ms_median": med, "ms_min": min(ms), "ms_max": max(ms),
                           "episodes": n, "env_steps": steps, "env_steps_per_s": steps / (med * 1e-3),
                           "return_mean": float(ret.mean()), "length_mean": float(ln.double().mean())})
    # the CPU evaluator's loop on the same snapshot
    torch.set_num_threads(1)                # as evaluator_main
    model = ActorCritic(w.spec.obs_dim, w.spec.act_dim, p.hidden, p.value_mult)
    model.load_state_dict({k: v.cpu() for k, v in w.model.state_dict().items()})
    stats = RunningObsStats(w.spec.obs_dim)
    stats.load_state_dict(w.stats.state_dict())
    env = make_vec_env(w.spec, 1, seed=p.seed + 7777, rank=0, device="cpu", max_episode_length=p.max_episode_length)
    key = rng.base_key(p.seed, rng.STREAM_EVAL, 0)
    cpu = []
    for _ in range(a.cpu_episodes):
        t0 = time.perf_counter()
        total, length = run_episode(model, stats, env, key, p.std_convention)
        cpu.append({"s": time.perf_counter() - t0, "length": length, "return": total})
    res["cpu_run_episode"] = cpu
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

    cpu_s = statistics.median(c["s"] for c in cpu)
    cpu_len = statistics.median(c["length"] for c in cpu)
    lines = [BEGIN, "", f"Measured by `scripts/eval_time.py` on {res['device']} (tree `{res['tree']}`): {p.env_name} dims, "
             f"{p.dtype}, `max_episode_length` {p.max_episode_length}, stochastic actions; HIP events, median of "
             f"{a.reps} after a warm-up. The snapshot is the policy after two training iterations ({p.num_envs} envs x "
             f"{p.rollout_len} steps): the same parameters and statistics for every row.", "",
             "| path | episodes | env steps | time | env steps/s |", "|---|---|---|---|---|"]
    for g in res["gpu"]:
        lines.append(f"| `HipEngine.evaluate`, {g['eval_envs']} envs | {g['episodes']} | {g['env_steps']} | "
                     f"{g['ms_median']:.2f} ms (min {g['ms_min']:.2f}, max {g['ms_max']:.2f}) | {g['env_steps_per_s']:.3g} |")
    lines.append(f"| CPU `run_episode` (1 thread, batch 1) | 1 | {int(cpu_len)} | {cpu_s * 1e3:.0f} ms | "
                 f"{cpu_len / cpu_s:.3g} |")
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
