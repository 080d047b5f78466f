"""Time the device-stepped rollout (HipEngine.rollout_stepped) per env step, three ways.

    python scripts/tensor_env_time.py [--out tensor_env_time.json] [--rounds 7] [--reps 64] [--env pendulum|cartpole]

Pendulum-v0 (a kind the fused kernel also runs), E = 4096, T = 16, bf16x3, one process, three engines
with the same weights, alternating round by round:

  (a) ``rollout_stepped()``: per step one csrc/act.hip launch, the env's torch ops, one
      csrc/envstep.hip launch (``env_advance``)
  (b) the same loop with ``VecEnv.step`` in place of the env's ops + ``env_advance``: its torch
      bookkeeping (~12 small ops), the reward clip, the row copies and the episode-stat adds.  This
      variant lives here only: it is what the ``env_advance`` launch replaces.
  (c) ``rollout()``: the fused rollout kernel, the whole rollout in one launch — the price of the
      general path is (a) against (c).

Two warm-up rollouts each, then a host clock around each window of ``--reps`` rollouts (16x as many
of the fused kernel's, so that its window is not a few milliseconds), which ends in a device
synchronise, divided by the window's env steps.  Prints one JSON line (and writes it to
``--out``): the median, min and max over the rounds.  No threshold.

``--env cartpole``: CartPoleContinuous-v1, the same sizes and method, variants (a) ``rollout_stepped()``
(its default path) and (c) ``rollout()`` with ``env_fused`` (in-kernel env kind 2); there is no (b).
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from pytorch_dppo_amd.config import dppo_preset  # noqa: E402
from pytorch_dppo_amd.envs import get_spec, make_vec_env  # noqa: E402
from pytorch_dppo_amd.models.actor_critic import ActorCritic  # noqa: E402
from pytorch_dppo_amd.runtime.engine_hip import HipEngine  # noqa: E402
from pytorch_dppo_amd.utils import rng  # noqa: E402
from pytorch_dppo_amd.utils.obs_stats import RunningObsStats  # noqa: E402

ENV, E, T, DTYPE = "Pendulum-v0", 4096, 16, "bf16x3"
ENVS = {"pendulum": "Pendulum-v0", "cartpole": "CartPoleContinuous-v1"}
FUSED_REPS_X = 16    # the fused kernel's rollouts per window, as a multiple of --reps


def build(dev, env_fused=False):
    p = dppo_preset(device="gpu", env_name=ENV, num_envs=E, exploration_size=E * T, batch_size=E * T, dtype=DTYPE,
                    env_fused=env_fused)
    spec = get_spec(ENV)
    torch.manual_seed(0)
    model = ActorCritic(spec.obs_dim, spec.act_dim, p.hidden).to(dev)
    env = make_vec_env(spec, E, seed=p.seed, device=dev, max_episode_length=p.max_episode_length)
    stats = RunningObsStats(spec.obs_dim, dev)
    eng = HipEngine(p, model, env, stats, dev, 0)
    stats.observes(env.observe())
    eng.params_changed()
    return eng


@torch.no_grad()
def rollout_stepped_torch(eng):
    """variant (b): rollout_stepped's loop with VecEnv.step (torch bookkeeping), the reward clip, the
    row copies and the episode-stat adds where the product has one env_advance launch"""
    p, env, none = eng.p, eng.env, eng.no_q
    shift = eng.stats.shift()
    ep = torch.zeros(2, dtype=torch.float64, device=eng.device)
    obs = env.observe().contiguous()
    for t in range(T):
        rows = slice(t * E, (t + 1) * E)
        a = eng.actions[rows]
        eng._launch_act(obs, env.t & rng.MASK32, False, 0, eng.key_action, eng.stats, shift, a, eng.logp[rows], none,
                        eng.x_buf[rows], eng.mom, t == 0)
        obs, r, done, info = env.step(a)
        if p.reward_clip > 0:
            r = r.clamp(-p.reward_clip, p.reward_clip)
        eng.rewards[rows].copy_(r)
        eng.dones[rows].copy_(done.to(torch.float32))
        ep[0] += info["ep_return_sum"]
        ep[1] += info["ep_count"]
        obs = obs.contiguous()
    eng._launch_act(obs, env.t, False, 0, eng.key_action, eng.stats, shift, none, none, none, eng.x_buf[T * E:], none,
                    False)
    eng.ext.obs_reduce(eng.mom, eng.mom.shape[0], eng.O, eng.s12, eng.epstat, eng.ep_sum)
    return ep


def timed(fn, reps):
    """microseconds per env step: a host clock around ``reps`` rollouts that end in a device synchronise"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / (reps * T) * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=64, help="rollouts per timed window")
    ap.add_argument("--env", choices=sorted(ENVS), default="pendulum")
    a = ap.parse_args()
    global ENV
    ENV = ENVS[a.env]
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    if a.env == "cartpole":
        engs = {"a_env_advance": build(dev), "c_fused_kernel": build(dev, env_fused=True)}
        assert engs["a_env_advance"].stepped_env and not engs["c_fused_kernel"].stepped_env
        fns = {"a_env_advance": engs["a_env_advance"].rollout_stepped, "c_fused_kernel": engs["c_fused_kernel"].rollout}
    else:
        engs = {k: build(dev) for k in ("a_env_advance", "b_torch_bookkeeping", "c_fused_kernel")}
        fns = {"a_env_advance": engs["a_env_advance"].rollout_stepped,
               "b_torch_bookkeeping": lambda: rollout_stepped_torch(engs["b_torch_bookkeeping"]),
               "c_fused_kernel": engs["c_fused_kernel"].rollout}
    for fn in fns.values():          # warm-up (allocations, code objects, lazy inits)
        timed(fn, 2)
    # same seed, same keys: after the same number of rollouts the three engines hold the same env
    st = [engs[k].env.state for k in fns]
    same = {"a_vs_c_state_max_gap": float((st[0] - st[-1]).abs().max())}
    if "b_torch_bookkeeping" in fns:
        same["a_vs_b_state_equal"] = bool(torch.equal(st[0], st[1]))
    times = {k: [] for k in fns}
    for _ in range(a.rounds):        # alternate the variants round by round
        for k, fn in fns.items():
            times[k].append(timed(fn, a.reps * (FUSED_REPS_X if k == "c_fused_kernel" else 1)))
    props = torch.cuda.get_device_properties(dev)
    res = {"env": ENV, "E": E, "T": T, "dtype": DTYPE, "rounds": a.rounds, "reps": a.reps,
           "fused_reps": a.reps * FUSED_REPS_X, "device": props.name,
           "unit": "us per env step (all E envs)", **same,
           **{k: {"median": statistics.median(v), "min": min(v), "max": max(v)} for k, v in times.items()}}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
