"""Where the fused gather + Adam time goes (diagnostics): the joint world-1 launch at the bench
geometry, timed back to back as is, without the slab elements (reduce items only), and without
the reduce items (slab elements only), with the bytes the launch moves (from the plan) and the rate
they make of its time.   python scripts/probe_gather.py [bf16x3|bf16] [stream|elem]

``elem``: the per-element form on its own grid (ext.set_gather_stream(0); docs/ARCHITECTURE.md §26)."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from pytorch_dppo_amd.config import dppo_preset  # noqa: E402
from pytorch_dppo_amd.parallel.dist import DistContext  # noqa: E402
from pytorch_dppo_amd.runtime.worker import DPPOWorker  # noqa: E402


def launch_bytes(eng, stream: bool) -> dict:
    """bytes one joint gather + Adam launch moves, from the plan: the slab chunks its elements read (whole
    16-byte quads in the streaming form), the partial rows under the reduce items, the per-element state and
    index reads, and the writes (g, p, m, v and the weight images)"""
    b = eng.joint_bucket
    slab = elems = 0
    for tb, nch, size, n0, k0, kq, fan_in, fan_out, woff, boff, nq, q0 in b["tile_rows"]:
        rows, cols = min(nq * 64, fan_out - n0), min(kq * 64, fan_in + 1 - k0)
        slab += rows * (-(-cols // 4) * 4 if stream else cols) * nch * 4
        elems += rows * cols
    nitems = int(eng.items["joint"][0].numel())
    upd = elems + int((eng.items["joint"][1] >= 0).sum())           # elements that take an Adam step
    imgs = int((eng.w_map >= 0).sum()) + int((eng.wt_map >= 0).sum())
    isz = eng.wimg.element_size()
    out = {"slab_read": slab, "slab_written_by_wgrad": int(b["slab"].numel()) * 4,
           "part_rows": nitems * eng.nhead_blk * 4,
           "state_read": upd * 3 * 4, "index_read": upd * 2 * 4 + nitems * 2 * 4 + (0 if stream else elems * 2 * 4),
           "writes": upd * 4 * 4 + imgs * isz}
    out["total"] = sum(v for k, v in out.items() if k != "slab_written_by_wgrad")
    return out


def main():
    dt = sys.argv[1] if len(sys.argv) > 1 else "bf16x3"
    form = sys.argv[2] if len(sys.argv) > 2 else "stream"
    dev = torch.device("cuda", 0)
    p = dppo_preset(device="gpu", env_name="Humanoid-v2", num_envs=4096, exploration_size=65536, batch_size=65536,
                    dtype=dt, seed=1)
    w = DPPOWorker(p, DistContext(device=dev))
    w.iteration_step()
    eng = w.engine
    if form == "elem":
        eng.ext.set_gather_stream(0)
        eng.norm_n_whole = eng.norm_n_elem
    b = eng.joint_bucket
    rc, rd = eng.items["joint"]
    n = eng.model.num_params
    empty_i = torch.empty(0, dtype=torch.int32, device=dev)
    eng.p.lr = 0.0          # (the launches of the window leave the parameters where they are)
    no_slab = dict(b, runs=[n, n], tile_rows=[], tiles={})   # (no slab element: no tile table either)

    def run(items, bucket):
        eng._gather_adam(bucket, *eng.joint_src, eng.part_joint, eng.nhead_blk, (rc, rd) if items else (empty_i, empty_i))
    arms = {"full": (True, b), "items_only": (True, no_slab), "slab_only": (False, b)}
    res = {}
    for name, (items, bucket) in arms.items():
        for _ in range(3):
            run(items, bucket)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(50):
            run(items, bucket)
        e1.record()
        torch.cuda.synchronize()
        res[name] = round(e0.elapsed_time(e1) * 1e3 / 50, 2)
    res["nitems"] = int(rc.numel())
    res["grid"] = int(eng.norm_n_whole)
    by = launch_bytes(eng, form != "elem")
    tbs = by["total"] / (res["full"] * 1e-6) / 1e12
    print(json.dumps({"dtype": dt, "form": form, "us": res, "bytes": by, "TB_per_s": round(tbs, 2),
                      "of_6_TB_per_s": round(tbs / 6.0, 2)}))
    eng.ext.set_gather_stream(1)


if __name__ == "__main__":
    main()
