"""Dump what every world-size-1 update path of HipEngine leaves behind, for a byte-wise comparison of two commits.

    python scripts/update_paths_dump.py --out DIR [--only SUBSTRING]

The file drives the engine only through DPPOWorker.iteration_step (rollout -> values -> gae -> the epochs of
HipEngine.step), so the same file runs at either commit: run it once in each tree, each in a fresh process, and
``cmp`` the two directories file by file.  For every configuration below it builds a worker with a fixed seed and
runs two iterations of two epochs; after each it writes, as ``DIR/<config>/it<k>_<name>.npy``: the flat parameters,
``adam_m``, ``adam_v``, ``adam_state``, ``grad_flat``, ``loss_sums``, ``norm_part[:_norm_n]``, ``wimg`` (raw storage
bytes), ``wimg_fwd`` and ``q8_amax`` in fp8 mode, and ``mu_prev`` / ``v_prev`` under the reference loss.

Sizes: Humanoid-v2 dims (the per-head kernels need the reference network; CartPole-v1 its own), 64 envs x 8 steps
= 512 rows.
Minibatch 512: the full batch, whole 128-row workgroups, the x^T-ready path; 200: gathered rows, masked rows in the
last workgroup.  Two epochs: ``first_step`` on and off, and all three slots of the fp8 amax ring.  Configurations:

  dtype fp32 | bf16 | bf16x3 | fp8  x  update_kernels tile | heads  x  minibatch 512 | 200
  heads: also phead_kernel on | off  x  phead_fused_dw2 on | off
  heads at fp8: also fp8_wgrad_operands on | off  x  fp8_policy_gemms on | off
  extras, on both kernel families at bf16x3 and bf16: loss dppo_ref, value_loss clipped_half, max_grad_norm 0.5,
      compat (the extra gradient), fused_apply off, target_kl, adv_norm_scope minibatch (advnorm)
  CartPole-v1 (a discrete env: the categorical head, the tile kernel alone) at fp32 | bf16x3 | bf16, minibatch 200

A combination the configuration or the engine refuses is skipped; ``DIR/skips.json`` lists each with the refusal's
text and ``DIR/configs.json`` the ones that ran.  The multi-rank branches of ``step()`` (in-stream, side-stream
split, process-group chains) have no driver here: tests/test_gpu_kernels.py and tests/test_distributed.py cover them.
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

E, T, ITERS, EPOCHS = 64, 8, 2, 2
TARGET_KL = 2.43e-3
EXTRAS = (("dpporef", dict(loss="dppo_ref", std_convention="var")), ("vclip", dict(value_loss="clipped_half")),
          ("clip", dict(max_grad_norm=0.5)), ("compat", dict(compat=True)), ("unfused", dict(fused_apply=False)),
          ("kl", dict(target_kl=TARGET_KL)), ("advnorm", dict(normalize_adv=True, adv_norm_scope="minibatch")))


def configs():
    """(name, Params keywords) of every configuration, in a fixed order"""
    out = []
    for dtype, mb in itertools.product(("fp32", "bf16", "bf16x3", "fp8"), (512, 200)):
        out.append((f"tile-{dtype}-mb{mb}", dict(dtype=dtype, update_kernels="tile", batch_size=mb)))
        for ph, p2 in itertools.product((True, False), ("on", "off")):
            out.append((f"heads-{dtype}-mb{mb}-phead{int(ph)}-dw2{p2}",
                        dict(dtype=dtype, update_kernels="heads", batch_size=mb, phead_kernel=ph, phead_fused_dw2=p2)))
        if dtype == "fp8":
            for q8, pg in itertools.product((True, False), (True, False)):
                out.append((f"heads-fp8-mb{mb}-q8{int(q8)}-pgemm{int(pg)}",
                            dict(dtype=dtype, update_kernels="heads", batch_size=mb, fp8_wgrad_operands=q8,
                                 fp8_policy_gemms=pg)))
    for (tag, kw), fam, dtype in itertools.product(EXTRAS, ("tile", "heads"), ("bf16x3", "bf16")):
        out.append((f"extra-{tag}-{fam}-{dtype}", dict(dtype=dtype, update_kernels=fam, batch_size=200, **kw)))
    for dtype in ("fp32", "bf16x3", "bf16"):
        out.append((f"cartpole-tile-{dtype}-mb200",
                    dict(env_name="CartPole-v1", dtype=dtype, update_kernels="tile", batch_size=200)))
    return out


def raw(t):
    t = torch.as_tensor(t).detach().contiguous()
    if t.dtype == torch.bfloat16:
        t = t.view(torch.uint8)
    return t.cpu().numpy()


def snapshot(eng):
    out = {"flat": eng.model.flat.data, "adam_m": eng.adam_m, "adam_v": eng.adam_v, "adam_state": eng.adam_state,
           "grad_flat": eng.grad_flat, "loss_sums": eng.loss_sums, "norm_part": eng.norm_part[:eng._norm_n],
           "wimg": eng.wimg.view(torch.uint8)}
    if eng.fp8:
        out.update(wimg_fwd=eng.wimg_fwd, q8_amax=eng.q8_amax)
    if eng.p.loss == "dppo_ref":
        out.update(mu_prev=eng.mu_prev, v_prev=eng.v_prev)
    return out


def run(name, kw, dev, root):
    p = dppo_preset(**{**dict(device="gpu", env_name="Humanoid-v2", num_envs=E, exploration_size=E * T,
                              num_epoch=EPOCHS, seed=3, value_loss="mse"), **kw})
    torch.manual_seed(0)
    w = DPPOWorker(p, DistContext(device=dev))
    eng = w.engine
    assert eng.name == "hip"
    os.makedirs(os.path.join(root, name), exist_ok=True)
    for it in range(ITERS):
        w.iteration_step()
        torch.cuda.synchronize(dev)
        eng.raise_if_failed()
        for k, v in snapshot(eng).items():
            np.save(os.path.join(root, name, f"it{it}_{k}.npy"), raw(v))
    return {"heads": bool(eng.heads), "phead": bool(eng.phead), "phead_p2": bool(eng.phead_p2), "q8": bool(eng.q8),
            "adam_step": int(eng.adam_step)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--only", default="", help="run the configurations whose name contains this")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    os.makedirs(a.out, exist_ok=True)
    ran, skips = {}, {}
    for name, kw in configs():
        if a.only not in name:
            continue
        try:
            ran[name] = run(name, kw, dev, a.out)
        except (ValueError, RuntimeError) as e:   # the configuration, the engine or a binding's host check refuses it
            if "HIP" in str(e) or "hip" in str(e):  # (a launch or device error is a failure, not a skip)
                raise
            skips[name] = str(e).split("\n")[0]
            print(name, "skipped: " + skips[name], flush=True)
            continue
        print(name, "ok", flush=True)
    for fn, d in (("configs.json", ran), ("skips.json", skips)):
        with open(os.path.join(a.out, fn), "w") as f:
            json.dump(d, f, indent=1, sort_keys=True)
    print(json.dumps({"ran": len(ran), "skipped": len(skips)}))


if __name__ == "__main__":
    main()
