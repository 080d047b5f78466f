"""Dump what the worker loop leaves behind on either engine, for a byte-wise comparison of two commits.

    python scripts/worker_records_dump.py --device cpu|gpu --out DIR [--only SUBSTRING]

The file drives only DPPOWorker.iteration_step and finish_metrics, so the same file runs at either commit: run it
once in each tree, each in a fresh process, and ``cmp`` the two directories file by file.  For every configuration
below it builds a worker with a fixed seed and runs three iterations of two epochs; after each it writes, into
``DIR/<config>/``: ``it<k>_record.json`` (the metrics record iteration_step returned — under ``defer`` the previous
iteration's, ``{}`` first — floats as ``float.hex()``, without the phase timings and the iter_s / steps_per_s
keys), ``it<k>_flat.npy`` / ``_adam_m.npy`` / ``_adam_v.npy`` and ``it<k>_state.json`` (the Adam step count and
``worker.updates``); at the end ``final_record.json`` (finish_metrics).

Sizes: Pendulum-v0 dims, 16 envs x 8 steps = 128 rows.  Minibatch 128: the full batch; 48: gathered rows, the last
minibatch wrapped.  Configurations (normalize_adv on throughout):

  minibatch 128 | 48  x  reward_norm off | on  x  target_kl off | on (trips in the second epoch)
      x  lr_schedule constant | linear | adaptive  x  adv_norm_scope rank | global | minibatch
  minibatch 48: each of them again with iteration_step(defer=True)
  num_epoch 0 with every feature on, and with the linear schedule: the metrics vector without a loss vector
  gpu: Humanoid-v2 dims, 64 envs x 8 steps, bf16x3 (the per-head kernels; pack_metrics with a loss vector), plain
      and with every feature on
  cpu: two gloo ranks — target_kl, target_kl with grad_reduce=mean, overlap_rollout (the deferred last step), and
      grad_reduce=mean; each rank writes ``DIR/<config>/rank<r>/``

A combination the configuration or the engine refuses is skipped; ``DIR/skips.json`` lists each with the refusal's
text and ``DIR/configs.json`` the ones that ran, with the iterations whose gate stopped.
"""
import argparse
import itertools
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from pytorch_dppo_amd.config import dppo_preset  # noqa: E402
from pytorch_dppo_amd.parallel.dist import DistContext  # noqa: E402
from pytorch_dppo_amd.runtime.worker import DPPOWorker  # noqa: E402

E, T, ITERS, EPOCHS = 16, 8, 3, 2
# confirmed on the CPU engine: 2.43e-3 stops steps of the second epoch at minibatch 48 (6 steps an iteration); the full
# batch has 2 steps, the second epoch's being the last: 2e-5 lies under its KL in every iteration, so the gate trips
# there (kl_stopped, kl_trip) with no step left to stop
TARGET_KL = 2.43e-3
TARGET_KL_FULL = 2e-5
DROP = ("iter_s", "steps_per_s", "host_s")
ALL_ON = dict(reward_norm=True, target_kl=TARGET_KL, lr_schedule="adaptive", adv_norm_scope="minibatch")


def configs(device):
    """(name, Params keywords, defer, ranks) of every configuration, in a fixed order"""
    out = []
    for mb, rn, gate, lr, scope in itertools.product((128, 48), (False, True), (False, True),
                                                     ("constant", "linear", "adaptive"),
                                                     ("rank", "global", "minibatch")):
        kl = 0.0 if not gate else (TARGET_KL_FULL if mb == 128 else TARGET_KL)
        kw = dict(batch_size=mb, reward_norm=rn, target_kl=kl, lr_schedule=lr, adv_norm_scope=scope)
        if mb == 48:
            kw["minibatches_per_epoch"] = 3      # 3 x 48 rows out of 128: the last minibatch wraps
        name = f"mb{mb}-rn{int(rn)}-kl{int(gate)}-{lr}-{scope}"
        out.append((name, kw, False, 1))
        if mb == 48:
            out.append((name + "-defer", kw, True, 1))
    # no update step at all: no loss vector exists, so the GPU engine's pack_metrics declines and the worker fills the
    # vector from metrics_tails() on either engine
    out.append(("noepoch-all", dict(batch_size=48, num_epoch=0, **ALL_ON), False, 1))
    out.append(("noepoch-linear", dict(batch_size=48, num_epoch=0, reward_norm=True, lr_schedule="linear",
                                       adv_norm_scope="global"), True, 1))
    if device == "gpu":
        big = dict(env_name="Humanoid-v2", num_envs=64, exploration_size=64 * T, dtype="bf16x3")
        for mb in (512, 200):
            out.append((f"humanoid-mb{mb}", dict(big, batch_size=mb), False, 1))
            out.append((f"humanoid-mb{mb}-all-defer", dict(big, batch_size=mb, **ALL_ON), True, 1))
    else:
        for name, kw in (("kl", dict(target_kl=TARGET_KL)), ("kl-mean", dict(target_kl=TARGET_KL, grad_reduce="mean")),
                         ("overlap", dict(overlap_rollout=True)), ("mean", dict(grad_reduce="mean"))):
            kw = dict(batch_size=48, minibatches_per_epoch=3, num_processes=2, **kw)
            out.append((f"ranks2-{name}", kw, False, 2))
    return out


def lossless(rec):
    return {k: (v.hex() if isinstance(v, float) else v) for k, v in rec.items()
            if not (k.startswith("ms_") or k in DROP)}


def dump_json(path, obj):
    with open(path, "w") as f:
        json.dump(obj, f, indent=1, sort_keys=True)


def run(device, kw, defer, ctx, out):
    p = dppo_preset(**{**dict(device=device, env_name="Pendulum-v0", num_envs=E, exploration_size=E * T,
                              num_epoch=EPOCHS, seed=3, normalize_adv=True, max_iters=ITERS), **kw})
    torch.manual_seed(0)
    w = DPPOWorker(p, ctx)
    eng = w.engine
    assert eng.name == ("hip" if device == "gpu" else "torch")
    os.makedirs(out, exist_ok=True)
    stopped = []
    for it in range(ITERS):
        rec = w.iteration_step(defer=defer)
        eng.sync()
        if rec.get("kl_stopped"):
            stopped.append(int(rec["iteration"]))
        dump_json(os.path.join(out, f"it{it}_record.json"), lossless(rec))
        for k, v in (("flat", w.model.flat.data), ("adam_m", eng.adam_m), ("adam_v", eng.adam_v)):
            np.save(os.path.join(out, f"it{it}_{k}.npy"), v.detach().cpu().numpy())
        dump_json(os.path.join(out, f"it{it}_state.json"), {"adam_step": int(eng.adam_step), "updates": int(w.updates)})
    dump_json(os.path.join(out, "final_record.json"), lossless(w.finish_metrics()))
    return {"adam_step": int(eng.adam_step), "updates": int(w.updates), "kl_stopped_iterations": stopped}


def rank_main(rank, world, port, kw, defer, out, q):
    from pytorch_dppo_amd.parallel.dist import init_distributed
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    torch.set_num_threads(1)
    ctx = init_distributed("cpu", rank=rank, world_size=world, timeout_s=60.0)
    try:
        res = run("cpu", kw, defer, ctx, os.path.join(out, f"rank{rank}"))
    except ValueError as e:
        res = {"refused": str(e).split("\n")[0]}
    if rank == 0:
        q.put(res)
    ctx.destroy()


def run_ranks(world, kw, defer, out):
    import torch.multiprocessing as mp
    from pytorch_dppo_amd.runtime.launcher import free_port
    mpc = mp.get_context("spawn")
    q, port = mpc.Queue(), free_port()
    procs = [mpc.Process(target=rank_main, args=(r, world, port, kw, defer, out, q)) for r in range(world)]
    for pr in procs:
        pr.start()
    for pr in procs:
        pr.join(240)
    if any(pr.is_alive() or pr.exitcode != 0 for pr in procs):
        for pr in procs:
            pr.terminate()
        raise SystemExit(f"a rank of {out} failed: exit codes {[pr.exitcode for pr in procs]}")
    res = q.get(timeout=10)
    if "refused" in res:
        raise ValueError(res["refused"])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--device", choices=("cpu", "gpu"), required=True)
    ap.add_argument("--out", required=True)
    ap.add_argument("--only", default="", help="run the configurations whose name contains this")
    a = ap.parse_args()
    dev = torch.device("cpu")
    if a.device == "gpu":
        dev = torch.device("cuda", 0)
        torch.cuda.set_device(dev)
    os.makedirs(a.out, exist_ok=True)
    ran, skips = {}, {}
    for name, kw, defer, ranks in configs(a.device):
        if a.only not in name:
            continue
        out = os.path.join(a.out, name)
        try:
            ran[name] = run_ranks(ranks, kw, defer, out) if ranks > 1 else run(a.device, kw, defer,
                                                                              DistContext(device=dev), out)
        except (ValueError, RuntimeError) as e:   # the configuration, the engine or a binding's host check refuses it
            if "HIP" in str(e) or "hip" in str(e):  # (a launch or device error is a failure, not a skip)
                raise
            skips[name] = str(e).split("\n")[0]
            print(name, "skipped: " + skips[name], flush=True)
            continue
        print(name, "ok", ran[name], flush=True)
    dump_json(os.path.join(a.out, "configs.json"), ran)
    dump_json(os.path.join(a.out, "skips.json"), skips)
    print(json.dumps({"ran": len(ran), "skipped": len(skips)}))


if __name__ == "__main__":
    main()
