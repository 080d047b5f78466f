"""Time what ``lr_schedule=adaptive`` adds (diagnostics; the numbers of profiles/lr_schedule/README.md).

    python scripts/lr_schedule_time.py [--out lr_schedule_time.json] [--rounds 5] [--reps 20]

One process, interleaved round by round, HIP events around windows of ``--reps`` calls, bench geometry
(Humanoid-v2, 4096 envs x 16 steps, bf16x3, full batch), two gated engines with the same weights: one with the host
rate (``target_kl`` at a value it never reaches) and one with ``lr_schedule=adaptive`` (the rate in ``lr_state``):

  * the ``kl_gate`` launch without and with the rate block;
  * each gated Adam launch on the buffers of a step, host rate against device rate: the joint gather + Adam
    launch, the no-clip Adam launch and the clipping pair (sumsq + adam) over the whole vector.

Prints one JSON line (median, min, max over the rounds, microseconds).  No threshold.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from pytorch_dppo_amd.config import dppo_preset  # noqa: E402
from pytorch_dppo_amd.envs import get_spec, make_vec_env  # noqa: E402
from pytorch_dppo_amd.models.actor_critic import ActorCritic  # noqa: E402
from pytorch_dppo_amd.runtime.engine_hip import HipEngine  # noqa: E402
from pytorch_dppo_amd.utils.obs_stats import RunningObsStats  # noqa: E402
from target_kl_time import DTYPE, E, T, gather_adam, summary, window_us  # noqa: E402


def build(dev, **flags):
    p = dppo_preset(device="gpu", env_name="Humanoid-v2", num_envs=E, exploration_size=E * T, batch_size=E * T,
                    dtype=DTYPE, **flags)
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
    eng.step(None)          # the slab, the partial rows and the gradient of a step, for the Adam launches alone
    return eng


def whole_adam(eng, max_norm):
    """HipEngine.apply's launch over the whole vector, alone: the no-clip kernel, or the sumsq + adam pair"""
    n = eng.grad_flat.numel()
    return lambda: eng._adam(0, n, eng.norm_part[:eng.norm_n_elem], max_norm, 0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    host, devr = build(dev, target_kl=1e9), build(dev, lr_schedule="adaptive")
    assert host.heads and devr.heads and host.lr_state is None and devr.lr_state is not None
    lr0 = devr.lr_state.clone()

    def reset():            # (the kl_gate windows move the rate: every window starts from the initial one)
        devr.gate.zero_()
        devr.lr_state.copy_(lr0)

    cases = {"kl_gate.plain_us": (host.gate.zero_, lambda: host.ext.kl_gate(host.loss_sums, host.gate, host.adam_state, 1e9)),
             "kl_gate.rate_block_us": (reset, lambda: devr.ext.kl_gate(devr.loss_sums, devr.gate, devr.adam_state,
                                                                       float("inf"), *devr._rate_block))}
    for name, fn in (("gather_adam", gather_adam), ("adam_noclip", lambda e: whole_adam(e, 0.0)),
                     ("clip_pair", lambda e: whole_adam(e, 0.5))):
        cases[f"{name}.host_rate_us"] = (host.gate.zero_, fn(host))
        cases[f"{name}.device_rate_us"] = (reset, fn(devr))
    res = {k: [] for k in cases}
    for _ in range(a.rounds + 1):          # (the first round is the warm-up: dropped below)
        for k, (setup, fn) in cases.items():
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
