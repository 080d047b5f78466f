"""Online evaluator — the reference ``test.py`` process (``test.py:24-65``).

Reference behaviour: reload the shared weights every env step (torn reads while the chief
writes, Q18), update the SHARED obs stats from the evaluator too (Q5), act stochastically
``mu + sqrt(sigma_sq)*eps``, print ``Time …, episode reward …, episode length …`` per
episode and sleep 10 s.

Here rank 0 hands the evaluator a consistent snapshot (reference-format state_dict + frozen
obs stats) every ``eval_every`` iterations through a bounded queue (dropped if the evaluator
is busy — the trainer never blocks on it).  The evaluator runs on the CPU in its own process,
keeps the print format, and never writes training state.

``eval_mode="inline"`` replaces the process by a batched evaluation inside the trainer's engine
(``csrc/eval.hip`` through ``HipEngine.evaluate``; runtime/launcher.py): ``evaluate_batch`` below
is that kernel's torch twin — the CPU engine's path and the GPU tests' oracle.
"""
from __future__ import annotations

import queue
import time
from typing import Dict, Optional

import torch

from ..envs import get_spec, host_spec, import_env_module, make_vec_env
from ..models.actor_critic import ActorCritic
from ..ops import oracle
from ..utils import rng
from ..utils.obs_stats import RunningObsStats


def is_discrete(env_or_spec) -> bool:
    """a discrete-action env (EnvSpec.discrete): a categorical policy, the env takes action indices"""
    spec = getattr(env_or_spec, "spec", env_or_spec)
    return bool(getattr(spec, "discrete", False))


def run_episode(model: ActorCritic, stats: RunningObsStats, env, key_action: int,
                convention: str, max_steps: int = 100000, deterministic: bool = False):
    obs = env.reset()
    total, length = 0.0, 0
    dims = torch.arange(env.A, dtype=torch.int64)
    with torch.no_grad():
        while length < max_steps:
            x = stats.normalize(obs)
            mu, log_std, _ = model(x)
            if is_discrete(env):
                a = oracle.categorical_sample(mu, key_action, env.env_idx, env.t, deterministic)[0]
            elif deterministic:
                a = mu
            else:
                sig = torch.exp(log_std if convention == "std" else 0.5 * log_std)
                eps = rng.gauss(key_action, env.env_idx[:, None], env.t, dims[None, :])
                a = mu + sig * eps
            obs, r, done, info = env.step(a)
            total += float(r[0])
            length += 1
            if bool(done[0]):
                break
    return total, length


EVAL_ENV_SEED_OFFSET = 7777   # the evaluator's env seed is Params.seed + this (evaluator_main)


def eval_keys(seed: int) -> Dict[str, int]:
    """RNG keys of an evaluation: the env streams of seed + 7777, rank 0 (as ``evaluator_main``
    builds its env) and the evaluator's action stream of ``seed``."""
    es = int(seed) + EVAL_ENV_SEED_OFFSET
    return {"key_env": rng.base_key(es, rng.STREAM_ENV, 0), "key_term": rng.base_key(es, rng.STREAM_TERM, 0),
            "key_reset": rng.base_key(es, rng.STREAM_RESET, 0),
            "key_action": rng.base_key(int(seed), rng.STREAM_EVAL, 0)}


@torch.no_grad()
def evaluate_batch(model: ActorCritic, stats: RunningObsStats, spec_or_env, num_envs: int, seed: int,
                   max_episode_length: int, convention: str = "std", deterministic: bool = False,
                   act_fn=None, early_exit: bool = True):
    """Batched evaluation, the torch twin of ``csrc/eval.hip``: ``num_envs`` fresh builtin envs
    (seed ``seed + 7777``, rank 0; action key ``base_key(seed, STREAM_EVAL, 0)``) each run from
    their reset to the end of their FIRST episode (terminal or time limit) under the frozen
    ``stats``.  Finished envs keep stepping (and auto-resetting) in lockstep — the keys depend on
    the shared step counter — but are masked out of the sums.

    ``spec_or_env``: an ``EnvSpec``, or a builtin ``VecEnv`` of ``num_envs`` envs to use (reset
    here).  Returns ``(ret fp32 [E], len int32 [E])``: the sum of the unclipped rewards, added in
    step order in fp32 as ``VecEnv.ep_ret`` does, and the episode length.

    A discrete env (``EnvSpec.discrete``) takes ``oracle.categorical_sample`` of the logits and is stepped with the
    indices.  ``act_fn(obs, step_key) -> actions [E, A]`` (a discrete env: the indices ``[E]``): the policy step, in place of the torch one below
    (``model``, ``stats``, ``convention`` and ``deterministic`` are then its business;
    HipEngine.evaluate passes one ``csrc/act.hip`` launch).  ``early_exit=False`` drops the
    ``active.any()`` break — the loop's only host sync — and runs all ``limit`` steps; the masked
    sums are the same."""
    dev = model.flat.device
    if hasattr(spec_or_env, "step"):
        env = spec_or_env
        if getattr(env, "host_stepped", False):
            raise ValueError("evaluate_batch steps the builtin tensor envs, not a host-stepped (gym) env")
        if env.E != int(num_envs):
            raise ValueError(f"env has {env.E} envs, num_envs is {num_envs}")
    else:
        env = make_vec_env(spec_or_env, int(num_envs), seed=int(seed) + EVAL_ENV_SEED_OFFSET, rank=0, device=dev,
                           max_episode_length=max_episode_length)
    key_action = rng.base_key(int(seed), rng.STREAM_EVAL, 0)
    E = env.E
    obs = env.reset()
    env.t = 0
    ret = torch.zeros(E, dtype=torch.float32, device=env.device)
    length = torch.zeros(E, dtype=torch.int32, device=env.device)
    active = torch.ones(E, dtype=torch.bool, device=env.device)
    dims = torch.arange(env.A, dtype=torch.int64, device=env.device)
    discrete = is_discrete(env)
    for _ in range(env.limit):      # every first episode ends by step limit - 1
        if act_fn is not None:
            a = act_fn(obs, env.t)
        else:
            x = stats.normalize(obs.to(dev))
            mu, log_std, _ = model(x)
            if discrete:
                a = oracle.categorical_sample(mu, key_action, env.env_idx.to(dev), env.t, deterministic)[0]
            elif deterministic:
                a = mu
            else:
                sig = torch.exp(log_std if convention == "std" else 0.5 * log_std)
                eps = rng.gauss(key_action, env.env_idx[:, None], env.t, dims[None, :]).to(dev)
                a = mu + sig * eps
        obs, r, done, _ = env.step(a)
        ret = torch.where(active, ret + r.to(torch.float32), ret)
        length = torch.where(active, length + 1, length)
        active = active & ~done
        if early_exit and not bool(active.any()):
            break
    return ret, length


def evaluator_main(params_dict: Dict, q, stop_event=None, out_q=None) -> None:
    from ..config import Params
    p = Params.from_dict(params_dict)
    torch.set_num_threads(1)
    import_env_module(p.env_module)   # this is a spawned process: the user's registrations are made here
    if p.env_backend == "gym":   # test.py:28 gym.make
        env = make_vec_env(None, 1, seed=p.seed + 7777, rank=0, max_episode_length=p.max_episode_length,
                           backend="gym", name=p.env_name)
        spec = host_spec(p.env_name, env.O, env.A, env.limit)
    else:
        spec = get_spec(p.env_name)
        env = make_vec_env(spec, 1, seed=p.seed + 7777, rank=0, device="cpu",
                           max_episode_length=p.max_episode_length)
    model = ActorCritic(spec.obs_dim, spec.act_dim, p.hidden, p.value_mult)
    stats = RunningObsStats(spec.obs_dim)
    key = rng.base_key(p.seed, rng.STREAM_EVAL, 0)
    start = time.time()
    while True:
        if stop_event is not None and stop_event.is_set():
            break
        try:
            snap = q.get(timeout=0.5)
        except queue.Empty:
            continue
        if snap is None:
            break
        model.load_state_dict(snap["model"])
        stats.load_state_dict(snap["obs_stats"])
        for _ in range(max(1, p.eval_episodes)):
            ret, length = run_episode(model, stats, env, key, p.std_convention)
            # test.py:56-59 print format
            print("Time {}, episode reward {}, episode length {}".format(
                time.strftime("%Hh %Mm %Ss", time.gmtime(time.time() - start)), ret, length),
                flush=True)
            if out_q is not None:
                out_q.put({"iteration": snap.get("iteration", -1), "return": ret, "length": length})
            if p.eval_sleep > 0:
                time.sleep(p.eval_sleep)


class EvaluatorHandle:
    """rank-0 side: spawn the evaluator process and push snapshots without blocking."""

    def __init__(self, params, results: bool = False):
        import torch.multiprocessing as mp
        ctx = mp.get_context("spawn")
        self.q = ctx.Queue(maxsize=1)
        self.out_q = ctx.Queue() if results else None
        self.stop = ctx.Event()
        self.proc = ctx.Process(target=evaluator_main, args=(params.to_dict(), self.q, self.stop, self.out_q),
                                daemon=True)
        self.proc.start()

    def push(self, model_sd: Dict, stats_sd: Dict, iteration: int) -> bool:
        try:
            self.q.put_nowait({"model": model_sd, "obs_stats": stats_sd, "iteration": iteration})
            return True
        except queue.Full:
            return False

    def close(self, timeout: float = 10.0) -> None:
        try:
            self.q.put(None, timeout=timeout)
        except Exception:
            pass
        self.stop.set()
        self.proc.join(timeout)
        if self.proc.is_alive():
            self.proc.terminate()
