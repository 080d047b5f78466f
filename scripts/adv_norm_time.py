"""Time what ``adv_norm_scope`` costs (diagnostics; the numbers of profiles/adv_norm/README.md).

    python scripts/adv_norm_time.py [--out adv_norm_time.json] [--warmup 2] [--iters 20] [--block 5]
    python scripts/adv_norm_time.py --only global --iters 10      # one configuration (a kernel-trace run)

One process at the bench geometry (Humanoid-v2, 4096 envs x 16 steps, 10 full-batch epochs, bf16x3), three workers
with the same seed: ``normalize_adv`` off, scope ``rank`` (torch ops that rewrite the buffer) and scope ``global``
(csrc/advnorm.hip's two launches and the operand of the policy kernel).  After ``--warmup`` iterations each, the
``--iters`` timed iterations of every worker are run in blocks of ``--block``, the workers taking turns block by
block; a block is the bench's loop (``iteration_step(defer=True)``) between two device synchronisations, timed on the
host clock.  Prints one JSON line: ms per iteration per configuration (mean over all timed iterations, and the
minimum / maximum block).  No threshold.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from pytorch_dppo_amd.config import dppo_preset  # noqa: E402
from pytorch_dppo_amd.parallel.dist import DistContext  # noqa: E402
from pytorch_dppo_amd.runtime.worker import DPPOWorker  # noqa: E402

E, T, DTYPE = 4096, 16, "bf16x3"
CONFIGS = {"off": dict(), "rank": dict(normalize_adv=True), "global": dict(normalize_adv=True, adv_norm_scope="global")}


def worker(dev, name):
    p = dppo_preset(device="gpu", env_name="Humanoid-v2", num_envs=E, exploration_size=E * T, batch_size=E * T,
                    num_epoch=10, dtype=DTYPE, seed=1, phase_timing=0, **CONFIGS[name])
    return DPPOWorker(p, DistContext(device=dev))


def block_ms(w, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        w.iteration_step(defer=True)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--block", type=int, default=5)
    ap.add_argument("--only", default="", choices=[""] + sorted(CONFIGS))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    names = [a.only] if a.only else list(CONFIGS)
    ws = {k: worker(dev, k) for k in names}
    for w in ws.values():
        for _ in range(a.warmup):
            w.iteration_step()
    res = {k: [] for k in names}
    for _ in range(max(1, a.iters // a.block)):
        for k in names:
            res[k].append(block_ms(ws[k], a.block))
    for w in ws.values():
        w.finish_metrics()
    out = {"geometry": f"{E} envs x {T} steps, 10 full-batch epochs, {DTYPE}", "warmup": a.warmup,
           "iters": a.block * len(res[names[0]]), "block": a.block,
           **{f"{k}.ms_per_iter": {"mean": sum(v) / len(v), "min_block": min(v), "max_block": max(v)}
              for k, v in res.items()}}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
