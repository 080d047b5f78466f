#!/usr/bin/env python3
"""Roll out a trained checkpoint (the reference's ``test.py`` loop, from a saved run).

    python play.py --checkpoint ckpt --device cpu --episodes 3
    python play.py --checkpoint ckpt --device gpu --env-name Pendulum-v0 --deterministic
    python play.py --checkpoint ckpt --env-backend gym --env-name Hopper-v2

Builds one evaluation env (seed + 7777, as the evaluator does), loops ``PolicyRunner.act`` ->
``env.step`` to the end of each episode and prints the reference's line per episode
(``test.py:56-59``).  The env name, seed and network come from the checkpoint's saved config.
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from pytorch_dppo_amd.envs import get_spec, import_env_module, make_vec_env  # noqa: E402
from pytorch_dppo_amd.runtime.evaluator import EVAL_ENV_SEED_OFFSET  # noqa: E402
from pytorch_dppo_amd.runtime.policy import PolicyRunner  # noqa: E402
from pytorch_dppo_amd.utils import checkpoint  # noqa: E402


def main(argv=None):
    """returns [(return, length)] of the episodes played"""
    ap = argparse.ArgumentParser(description="roll out a trained DPPO / PPO checkpoint")
    ap.add_argument("--checkpoint", required=True, help="directory with model.pt + trainer_state.pt")
    ap.add_argument("--device", choices=("cpu", "gpu"), default="cpu")
    ap.add_argument("--dtype", default=None, help="GPU operand precision (default: the run's)")
    ap.add_argument("--episodes", type=int, default=1)
    ap.add_argument("--env-backend", choices=("builtin", "gym"), default=None)
    ap.add_argument("--env-name", default=None, help="default: the run's env")
    ap.add_argument("--env-module", default=None, help="module that registers the env (default: the run's)")
    ap.add_argument("--deterministic", action="store_true", help="act with mu (the reference acts stochastically)")
    ns = ap.parse_args(argv)

    st = checkpoint.load_trainer_state(ns.checkpoint)
    if st is None:
        raise FileNotFoundError(f"{ns.checkpoint}: no trainer_state.pt")
    cfg = st["config"]
    runner = PolicyRunner.from_checkpoint(ns.checkpoint, device=ns.device, dtype=ns.dtype)
    import_env_module(ns.env_module if ns.env_module is not None else cfg.get("env_module", ""))
    name = ns.env_name or cfg["env_name"]
    backend = ns.env_backend or cfg.get("env_backend", "builtin")
    seed = int(cfg.get("seed", 1)) + EVAL_ENV_SEED_OFFSET
    max_len = int(cfg.get("max_episode_length", 10000))
    if backend == "gym":
        env = make_vec_env(None, 1, seed=seed, rank=0, max_episode_length=max_len, backend="gym", name=name)
    else:
        env = make_vec_env(get_spec(name), 1, seed=seed, rank=0, device="cpu", max_episode_length=max_len)
    # a discrete env: the runner's action is the index the env's step takes (the distribution follows the env played)
    runner.discrete = bool(getattr(getattr(env, "spec", None), "discrete", False))
    if (env.O, env.A) != (runner.O, runner.A):
        raise ValueError(f"env {name} has obs/act dims ({env.O}, {env.A}), the checkpoint's policy ({runner.O}, {runner.A})")

    out = []
    start = time.time()
    for _ in range(max(1, ns.episodes)):
        obs = env.reset()
        total, length = 0.0, 0
        while True:
            # the noise key's step is the env's step counter, as the evaluator's loop (run_episode)
            a, _ = runner.act(obs, deterministic=ns.deterministic, step_key=env.t)
            obs, r, done, _ = env.step(a.to("cpu"))
            total += float(r[0])
            length += 1
            if bool(done[0]):
                break
        print("Time {}, episode reward {}, episode length {}".format(
            time.strftime("%Hh %Mm %Ss", time.gmtime(time.time() - start)), total, length), flush=True)
        out.append((total, length))
    return out


if __name__ == "__main__":
    main()
