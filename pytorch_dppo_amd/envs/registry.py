"""Env registry: every env name the reference mentions, with gym's observation/action dims.

The reference picks an env by commenting lines (``main.py:33-39``, ``ppo.py:35-42``) and
runs it through ``gym.make`` (MuJoCo / PyBullet).  Neither is installed in this image, so an
env name resolves to

* ``pendulum`` — a faithful vectorised Pendulum-v0 (gym's dynamics; CPU torch + HIP), or
* ``synthetic`` — an obs/act-dim-faithful synthetic locomotion task (CPU torch + HIP),
  used for every MuJoCo/Bullet name, or
* ``tensor`` — a ``VecEnv`` subclass registered with :func:`register_tensor_env` (by this package:
  ``CartPoleContinuous-v1`` and the discrete-action ``CartPole-v1``; by a user's ``--env-module``): torch ops on device tensors, stepped on
  the device by the GPU engine (``HipEngine.rollout_stepped``); the cart-pole also has an in-kernel
  twin (kernel kind ``KIND_CARTPOLE``, ``--env-fused true``), or
* ``gym`` — the real env through :mod:`pytorch_dppo_amd.envs.gym_adapter` with
  ``--env-backend gym`` (``gym.make``, or a factory installed with ``register_env``); its dims
  come from the env's spaces (:func:`host_spec`).

Dims are gym facts (SURVEY.md §2.6 [ext]).
"""
from __future__ import annotations

from dataclasses import dataclass

KIND_SYNTHETIC = 0
KIND_PENDULUM = 1
KIND_HOST = 2          # a host-stepped env (gym backend): dims come from the env itself
KIND_TENSOR = 3        # a registered tensor env (register_tensor_env): a VecEnv subclass the rollout kernel
                       # does not know; the GPU engine steps it on the device (HipEngine.rollout_stepped)
# In-kernel env kinds of the rollout / evaluation kernels (csrc/env_core.h): KIND_SYNTHETIC, KIND_PENDULUM and
KIND_CARTPOLE = 2      # the continuous cart-pole.  A kernel kind is what a VecEnv class can run as
                       # (VecEnv.kernel_kind); it is not a spec kind: the cart-pole's spec stays KIND_TENSOR, and
                       # the spec kind with the same number, KIND_HOST, never reaches a kernel.


@dataclass(frozen=True)
class EnvSpec:
    name: str
    obs_dim: int
    act_dim: int
    kind: int
    time_limit: int       # gym TimeLimit max_episode_steps
    # a discrete action space of act_dim actions: the policy's act_dim outputs are logits of a categorical
    # distribution, the rollout buffer's action rows are one-hot, and the env's step / _dynamics receive the
    # chosen index [E] int64 (docs/ARCHITECTURE.md §27).  Registered tensor envs only.
    discrete: bool = False


_SPECS = {}
_TENSOR_ENVS = {}      # name -> VecEnv subclass of the KIND_TENSOR specs


def _reg(names, obs, act, kind, limit):
    for n in names:
        _SPECS[n] = EnvSpec(n, obs, act, kind, limit)


_reg(["Pendulum-v0", "Pendulum-v1"], 3, 1, KIND_PENDULUM, 200)
_reg(["InvertedPendulum-v1", "InvertedPendulum-v2"], 4, 1, KIND_SYNTHETIC, 1000)
_reg(["InvertedDoublePendulum-v1", "InvertedDoublePendulum-v2"], 11, 1, KIND_SYNTHETIC, 1000)
_reg(["Reacher-v1", "Reacher-v2"], 11, 2, KIND_SYNTHETIC, 50)
_reg(["Hopper-v1", "Hopper-v2"], 11, 3, KIND_SYNTHETIC, 1000)
_reg(["HalfCheetah-v1", "HalfCheetah-v2"], 17, 6, KIND_SYNTHETIC, 1000)
_reg(["Walker2d-v1", "Walker2d-v2"], 17, 6, KIND_SYNTHETIC, 1000)
_reg(["Ant-v1", "Ant-v2"], 111, 8, KIND_SYNTHETIC, 1000)
_reg(["Humanoid-v1", "Humanoid-v2"], 376, 17, KIND_SYNTHETIC, 1000)
_reg(["HalfCheetahBulletEnv-v0"], 26, 6, KIND_SYNTHETIC, 1000)
_reg(["HopperBulletEnv-v0"], 15, 3, KIND_SYNTHETIC, 1000)
_reg(["AntBulletEnv-v0"], 28, 8, KIND_SYNTHETIC, 1000)


def host_spec(name: str, obs_dim: int, act_dim: int, limit: int) -> EnvSpec:
    """spec of a host-stepped env (``--env-backend gym``) built from the env's own spaces"""
    return EnvSpec(name, int(obs_dim), int(act_dim), KIND_HOST, int(limit))


def register_tensor_env(name: str, cls, obs_dim: int, act_dim: int, time_limit: int, discrete: bool = False) -> EnvSpec:
    """Register ``cls`` (a ``VecEnv`` subclass: ``state_dim``, ``_reset_state``, ``observe``,
    ``_dynamics`` as torch ops on its device tensors) under ``name``; ``make_vec_env`` builds it for
    the returned spec.  The names of the built-in table cannot be re-registered; registering the same
    tensor env again (a module imported twice) replaces it.  ``discrete``: ``act_dim`` is the number of
    actions (at least 2) and ``_dynamics(a, step_key)`` receives the chosen indices ``a [E] int64``."""
    if name in _SPECS and _SPECS[name].kind != KIND_TENSOR:
        raise ValueError(f"env {name!r} is a built-in entry and cannot be re-registered")
    if name.startswith("Synthetic-"):
        raise ValueError("the Synthetic-<obs>x<act> names are reserved")
    if int(obs_dim) < 1 or int(act_dim) < 1 or int(time_limit) < 1:
        raise ValueError("obs_dim, act_dim and time_limit must be positive")
    if discrete and int(act_dim) < 2:
        raise ValueError(f"a discrete env has at least 2 actions (act_dim is their number), got act_dim={act_dim}")
    spec = EnvSpec(name, int(obs_dim), int(act_dim), KIND_TENSOR, int(time_limit), bool(discrete))
    _SPECS[name] = spec
    _TENSOR_ENVS[name] = cls
    return spec


def tensor_env_class(name: str):
    """the class registered for a KIND_TENSOR spec"""
    if name not in _TENSOR_ENVS:
        raise KeyError(f"no tensor env registered as {name!r}; registered: {sorted(_TENSOR_ENVS)}")
    return _TENSOR_ENVS[name]


def kernel_kind_of(env) -> int:
    """the in-kernel kind (KIND_SYNTHETIC / KIND_PENDULUM / KIND_CARTPOLE) ``env`` can run as inside the
    rollout and evaluation kernels; ``ValueError`` naming the env when it has none"""
    kind = getattr(env, "kernel_kind", None)
    if kind is None:
        spec = getattr(env, "spec", None)
        name = getattr(spec, "name", "") or type(env).__name__
        raise ValueError(f"env {name!r} ({type(env).__name__}) has no in-kernel twin (kernel_kind is None): "
                         "it runs device-stepped (HipEngine.rollout_stepped), not with env_fused")
    return int(kind)


def import_env_module(module: str) -> None:
    """``Params.env_module``: import a dotted module path once so that it can call
    ``register_tensor_env`` (the worker, the evaluator process and play.py call this at start;
    spawned processes do not inherit the parent's registrations).  Empty: nothing is imported."""
    if module:
        import importlib
        importlib.import_module(module)


def get_spec(name: str) -> EnvSpec:
    if name in _SPECS:
        return _SPECS[name]
    if name.startswith("Synthetic-"):
        # Synthetic-<obs>x<act>
        o, a = name[len("Synthetic-"):].split("x")
        return EnvSpec(name, int(o), int(a), KIND_SYNTHETIC, 1000)
    raise KeyError(f"unknown env {name!r}; known: {sorted(_SPECS)}")


def known_envs():
    return sorted(_SPECS)
