"""Time what ``target_kl`` adds (diagnostics; the numbers of profiles/target_kl/README.md).

    python scripts/target_kl_time.py [--out target_kl_time.json] [--rounds 5] [--reps 20]

One process, interleaved round by round, HIP events around windows of ``--reps`` calls, bench geometry
(Humanoid-v2, 4096 envs x 16 steps, bf16x3, full batch), two engines with the same weights, flag off and on (the
gated one with a target it never reaches, so every step is applied, and once more with the gate closed by hand):

  * the ``kl_gate`` launch (once per step) and the zeroing of ``gate`` (once per iteration);
  * the joint gather + Adam launch alone on the buffers of a step: ungated, gated and applied, gated and stopped;
  * a whole ``step()``: ungated, gated (= the gated launch + ``kl_gate``), gated and stopped.

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


def build(dev, target_kl):
    p = dppo_preset(device="gpu", env_name="Humanoid-v2", num_envs=E, exploration_size=E * T, batch_size=E * T,
                    dtype=DTYPE, target_kl=target_kl)
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
    eng.gae()
    eng.begin_update()
    eng.step(None)          # the slab and the partial rows of a step, for the gather + Adam launch alone
    return eng


def gather_adam(eng):
    """the joint gather + Adam launch of HipEngine._joint_step, alone (ungated: the host counts every launch)"""
    return lambda: eng._gather_adam(eng.joint_bucket, *eng.joint_src, eng.part_joint, eng.nhead_blk,
                                    eng.items["joint"])


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
    off, on = build(dev, 0.0), build(dev, 1e9)
    assert off.heads and on.heads and off.gate is None and on.gate is not None
    ga_off, ga_on = gather_adam(off), gather_adam(on)

    # (no launch of a window writes gate[0]: the gated Adam launches only read it, and kl_gate neither trips at
    # this target nor reopens a closed gate; so the flag is set once, ahead of the window)
    def close():
        on.gate[0] = 1.0

    cases = {"kl_gate_us": (on.gate.zero_, lambda: on.ext.kl_gate(on.loss_sums, on.gate, on.adam_state, 1e9)),
             "gate_zero_us": (None, on.gate.zero_),
             "gather_adam.ungated_us": (None, ga_off), "gather_adam.gated_applied_us": (on.gate.zero_, ga_on),
             "gather_adam.gated_stopped_us": (close, ga_on),
             "step.ungated_us": (None, lambda: off.step(None)),
             "step.gated_applied_us": (on.gate.zero_, lambda: on.step(None)),
             "step.gated_stopped_us": (close, lambda: on.step(None))}
    res = {k: [] for k in cases}
    for _ in range(a.rounds + 1):          # (the first round is the warm-up: dropped below)
        for k, (setup, fn) in cases.items():
            if setup is not None:
                setup()
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
