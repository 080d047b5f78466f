"""Vectorised environments with explicit state tensors.

The reference steps ONE gym env per worker at batch 1 (``train.py:82-106``).  Here a worker
owns ``E`` envs whose whole state lives in tensors (``state [E,S]``, ``ep_len``, ``ep_ret``)
so the GPU rollout kernel (``csrc/rollout.hip``) can step them in-kernel, and the torch
``step`` below is the bit-compatible oracle used on the CPU path and in tests.

Episode semantics follow gym: ``done`` = terminal OR ``ep_len >= min(time_limit,
max_episode_length)`` counted per step (the reference counts per outer iteration, SURVEY Q7;
``compat`` is not needed for that quirk because it almost never fires).  The env resets
in place on ``done`` and returns the post-reset observation, like ``train.py:98-105``.
"""
from __future__ import annotations

import math
from typing import Dict, Tuple

import torch

from ..utils import rng
from .registry import KIND_CARTPOLE, KIND_PENDULUM, KIND_SYNTHETIC, KIND_TENSOR, EnvSpec, register_tensor_env, tensor_env_class

SYN_DECAY = 0.9
SYN_DRIVE = 0.1
SYN_NOISE = 0.05
SYN_RESET = 0.1
SYN_TERM_P = 0.002


def syn_weights(obs_dim: int, device) -> torch.Tensor:
    i = torch.arange(obs_dim, device=device)
    return 0.5 + (i % 7).to(torch.float32) / 7.0


class VecEnv:
    """Base: E envs of one spec, keyed RNG (seed, rank)."""
    # the in-kernel kind this class can run as inside the rollout / evaluation kernels (csrc/env_core.h),
    # None when the kernels have no twin of it (every user env; envs.registry.kernel_kind_of).  A subclass
    # that changes the dynamics of an env with a twin sets it back to None.
    kernel_kind = None

    def __init__(self, spec: EnvSpec, num_envs: int, seed: int = 1, rank: int = 0,
                 device="cpu", max_episode_length: int = 10000):
        self.spec = spec
        self.E = int(num_envs)
        self.O = spec.obs_dim
        self.A = spec.act_dim
        self.kind = spec.kind
        self.seed = int(seed)
        self.rank = int(rank)
        self.device = torch.device(device)
        self.limit = int(min(spec.time_limit, max_episode_length))
        self.t = 0  # global step counter: RNG key, advances once per vector step
        self.env_idx = torch.arange(self.E, device=self.device, dtype=torch.int64)
        self.key_env = rng.base_key(self.seed, rng.STREAM_ENV, self.rank)
        self.key_term = rng.base_key(self.seed, rng.STREAM_TERM, self.rank)
        self.key_reset = rng.base_key(self.seed, rng.STREAM_RESET, self.rank)
        self.state = torch.zeros(self.E, self.state_dim, device=self.device, dtype=torch.float32)
        self.ep_len = torch.zeros(self.E, device=self.device, dtype=torch.int32)
        self.ep_ret = torch.zeros(self.E, device=self.device, dtype=torch.float32)
        # bootstrap_time_limit: step() also reports which envs ended by the step limit alone and the
        # observation each env reached before the in-place reset (info "truncated" / "final_obs")
        self.report_final = False

    # -- subclass API ----------------------------------------------------------------------
    @property
    def state_dim(self) -> int:
        raise NotImplementedError

    def _reset_state(self, step_key: int) -> torch.Tensor:
        raise NotImplementedError

    def observe(self) -> torch.Tensor:
        raise NotImplementedError

    def _dynamics(self, a: torch.Tensor, step_key: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """returns (new_state, reward, terminal)"""
        raise NotImplementedError

    # -- common ------------------------------------------------------------------------------
    def reset(self) -> torch.Tensor:
        self.state = self._reset_state(0xFFFFFFFF)
        self.ep_len.zero_()
        self.ep_ret.zero_()
        return self.observe()

    @torch.no_grad()
    def step(self, actions: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, Dict]:
        if self.spec.discrete:    # the chosen action's index per env
            a = actions.to(self.device, torch.int64).reshape(self.E)
        else:
            a = actions.to(self.device, torch.float32).reshape(self.E, self.A)
        k = self.t & rng.MASK32
        new_state, reward, terminal = self._dynamics(a, k)
        self.ep_len += 1
        self.ep_ret += reward
        done = terminal | (self.ep_len >= self.limit)
        finished_ret = torch.where(done, self.ep_ret, torch.zeros_like(self.ep_ret))
        finished_len = torch.where(done, self.ep_len, torch.zeros_like(self.ep_len))
        reset_state = self._reset_state(k)
        extra = {}
        if self.report_final:
            # terminal wins when both hold; the final observation is observe() of the stepped state
            self.state = new_state
            extra = {"truncated": done & ~terminal, "final_obs": self.observe()}
        self.state = torch.where(done[:, None], reset_state, new_state)
        self.ep_len = torch.where(done, torch.zeros_like(self.ep_len), self.ep_len)
        self.ep_ret = torch.where(done, torch.zeros_like(self.ep_ret), self.ep_ret)
        self.t += 1
        info = {"ep_return_sum": finished_ret.sum(), "ep_count": done.sum(),
                "finished_ret": finished_ret, "finished_len": finished_len, **extra}
        return self.observe(), reward, done, info

    def kernel_params(self) -> Dict:
        return dict(kind=self.kind, limit=self.limit, key_env=self.key_env,
                    key_term=self.key_term, key_reset=self.key_reset)

    def state_dict(self):
        return {"state": self.state.cpu(), "ep_len": self.ep_len.cpu(), "ep_ret": self.ep_ret.cpu(),
                "t": self.t}

    def load_state_dict(self, d):
        self.state = d["state"].to(self.device)
        self.ep_len = d["ep_len"].to(self.device)
        self.ep_ret = d["ep_ret"].to(self.device)
        self.t = int(d["t"])


class SyntheticEnv(VecEnv):
    """Obs/act-dim-faithful synthetic locomotion task (one per MuJoCo/Bullet name).

    state == observation s in R^O.  With a_c = clamp(a, -1, 1) and w_i = 0.5 + (i mod 7)/7:
        r    = 1 - mean_{j<A} (a_c[j] - tanh(s[j]))^2           (learnable: target is a function of s)
        s'_i = 0.9 s_i + 0.1 tanh(w_i a_c[i mod A]) + 0.05 N(0,1)
        terminal with probability 0.002 per step; reset s ~ 0.1 N(0,1)
    All noise is keyed (seed, rank, env, step, dim) — identical in ``csrc/rollout.hip``.
    """
    kernel_kind = KIND_SYNTHETIC

    @property
    def state_dim(self) -> int:
        return self.O

    def _reset_state(self, step_key: int) -> torch.Tensor:
        d = torch.arange(self.O, device=self.device, dtype=torch.int64)
        g = rng.gauss(self.key_reset, self.env_idx[:, None], step_key, d[None, :])
        return SYN_RESET * g

    def observe(self) -> torch.Tensor:
        return self.state.clone()

    def _dynamics(self, a, step_key):
        s = self.state
        ac = a.clamp(-1.0, 1.0)
        na = min(self.A, self.O)
        err = ac[:, :na] - torch.tanh(s[:, :na])
        reward = 1.0 - (err * err).sum(1) / float(na)
        d = torch.arange(self.O, device=self.device, dtype=torch.int64)
        w = syn_weights(self.O, self.device)
        drive = torch.tanh(w[None, :] * ac[:, (d % self.A)])
        noise = rng.gauss(self.key_env, self.env_idx[:, None], step_key, d[None, :])
        new_s = SYN_DECAY * s + SYN_DRIVE * drive + SYN_NOISE * noise
        u = rng.uniform01(rng.keyed(self.key_term, self.env_idx, step_key,
                                    torch.zeros_like(self.env_idx)))
        terminal = u < SYN_TERM_P
        return new_s, reward, terminal


class PendulumEnv(VecEnv):
    """gym Pendulum-v0 dynamics (g=10, m=l=1, dt=.05, max_speed 8, max_torque 2, 200 steps)."""
    G, M, L, DT, MAX_SPEED, MAX_TORQUE = 10.0, 1.0, 1.0, 0.05, 8.0, 2.0
    kernel_kind = KIND_PENDULUM

    @property
    def state_dim(self) -> int:
        return 2

    def _reset_state(self, step_key: int) -> torch.Tensor:
        d = torch.zeros(self.E, dtype=torch.int64, device=self.device)
        u0 = rng.uniform01(rng.keyed(self.key_reset, self.env_idx, step_key, d))
        u1 = rng.uniform01(rng.keyed(self.key_reset, self.env_idx, step_key, d + 1))
        th = (2.0 * u0 - 1.0) * math.pi
        thdot = 2.0 * u1 - 1.0
        return torch.stack([th, thdot], 1)

    def observe(self) -> torch.Tensor:
        th, thdot = self.state[:, 0], self.state[:, 1]
        return torch.stack([torch.cos(th), torch.sin(th), thdot], 1)

    def _dynamics(self, a, step_key):
        th, thdot = self.state[:, 0], self.state[:, 1]
        u = a[:, 0].clamp(-self.MAX_TORQUE, self.MAX_TORQUE)
        thn = torch.remainder(th + math.pi, 2.0 * math.pi) - math.pi
        costs = thn * thn + 0.1 * thdot * thdot + 0.001 * u * u
        newthdot = thdot + (-3.0 * self.G / (2.0 * self.L) * torch.sin(th + math.pi)
                            + 3.0 / (self.M * self.L * self.L) * u) * self.DT
        newth = th + newthdot * self.DT
        newthdot = newthdot.clamp(-self.MAX_SPEED, self.MAX_SPEED)
        terminal = torch.zeros(self.E, dtype=torch.bool, device=self.device)
        return torch.stack([newth, newthdot], 1), -costs, terminal


class CartPoleContinuousEnv(VecEnv):
    """Cart-pole with a continuous force: gym CartPole-v1's physics (Barto, Sutton & Anderson 1983
    as gym integrates them: g = 9.8, cart 1.0, pole 0.1, pole half-length 0.5, explicit Euler,
    dt = 0.02), the force ``10 * clamp(a, -1, 1)`` instead of the two discrete pushes.

    state == observation (x, x_dot, theta, theta_dot).  Reward 1 per step; terminal when the NEW
    state has |x| > 2.4 or |theta| > 12 degrees; reset draws every state dim uniform in +-0.05 from
    the keyed reset stream (dims 0..3).  A registered tensor env (``CartPoleContinuous-v1``, spec kind
    KIND_TENSOR): by default the GPU engine steps it on the device (HipEngine.rollout_stepped).  It
    also has an in-kernel twin, kernel kind KIND_CARTPOLE (csrc/env_core.h ``cartpole_next``: this
    ``_dynamics`` operation for operation, compiled without FMA contraction), which ``env_fused``
    (``--env-fused true``) selects: rollout and evaluation then run in the fused kernels, the done flag
    of a step coming from the very four values the kernel stores as the new state."""
    kernel_kind = KIND_CARTPOLE
    GRAVITY, MASS_CART, MASS_POLE, HALF_LEN, FORCE_MAG, DT = 9.8, 1.0, 0.1, 0.5, 10.0, 0.02
    X_LIMIT = 2.4
    THETA_LIMIT = 12.0 * 2.0 * math.pi / 360.0
    RESET_RANGE = 0.05

    @property
    def state_dim(self) -> int:
        return 4

    def _reset_state(self, step_key: int) -> torch.Tensor:
        d = torch.arange(4, device=self.device, dtype=torch.int64)
        u = rng.uniform01(rng.keyed(self.key_reset, self.env_idx[:, None], step_key, d[None, :]))
        return (2.0 * u - 1.0) * self.RESET_RANGE

    def observe(self) -> torch.Tensor:
        return self.state.clone()

    def _dynamics(self, a, step_key):
        x, x_dot, th, th_dot = self.state.unbind(1)
        force = self.FORCE_MAG * a[:, 0].clamp(-1.0, 1.0)
        total_mass = self.MASS_CART + self.MASS_POLE
        pml = self.MASS_POLE * self.HALF_LEN
        cos, sin = torch.cos(th), torch.sin(th)
        temp = (force + pml * th_dot * th_dot * sin) / total_mass
        th_acc = (self.GRAVITY * sin - cos * temp) / (
            self.HALF_LEN * (4.0 / 3.0 - self.MASS_POLE * cos * cos / total_mass))
        x_acc = temp - pml * th_acc * cos / total_mass
        new = torch.stack([x + self.DT * x_dot, x_dot + self.DT * x_acc,
                           th + self.DT * th_dot, th_dot + self.DT * th_acc], 1)
        terminal = (new[:, 0].abs() > self.X_LIMIT) | (new[:, 2].abs() > self.THETA_LIMIT)
        return new, torch.ones(self.E, device=self.device, dtype=torch.float32), terminal


register_tensor_env("CartPoleContinuous-v1", CartPoleContinuousEnv, obs_dim=4, act_dim=1, time_limit=500)


class CartPoleEnv(CartPoleContinuousEnv):
    """gym CartPole-v1: the parent's physics, reset and termination under the two discrete pushes — action
    index 1 is the force +10, index 0 the force -10.  A discrete tensor env (``CartPole-v1``, 2 actions): its
    policy is categorical and ``_dynamics`` receives the indices ``a [E] int64``.  No in-kernel twin
    (``kernel_kind`` None): the GPU engine steps it on the device (HipEngine.rollout_stepped)."""
    kernel_kind = None

    def _dynamics(self, a, step_key):
        # +-1 is exact in fp32 and the parent's clamp keeps it: FORCE_MAG * (+-1), its own equations
        return super()._dynamics((2.0 * a.to(torch.float32) - 1.0)[:, None], step_key)


register_tensor_env("CartPole-v1", CartPoleEnv, obs_dim=4, act_dim=2, time_limit=500, discrete=True)


class CartPoleV0Env(CartPoleEnv):
    """gym CartPole-v0: CartPole-v1 with a 200-step limit — the same class but for one attribute.  It owns the
    in-kernel twin of the discrete cart-pole: kernel kind KIND_CARTPOLE (the parent's physics, csrc/env_core.h
    ``cartpole_next``) under the categorical head (``dist`` 1 of the rollout / evaluation kernels: index 1 pushes
    +1, index 0 pushes -1, this ``_dynamics``' own ``2 a - 1``), which ``env_fused`` selects.  Without the flag it
    is device-stepped like ``CartPole-v1``, whose name stays unfused."""
    kernel_kind = KIND_CARTPOLE


register_tensor_env("CartPole-v0", CartPoleV0Env, obs_dim=4, act_dim=2, time_limit=200, discrete=True)


def make_vec_env(spec: EnvSpec, num_envs: int, seed: int = 1, rank: int = 0, device="cpu",
                 max_episode_length: int = 10000, backend: str = "builtin", name: str = ""):
    """``builtin``: the tensor envs above and the registered ones (``register_tensor_env``) — stepped
    in-kernel on the GPU engine when the rollout kernel knows the kind, device-stepped otherwise;
    ``gym``: real gym envs stepped on the host (envs/gym_adapter.py, ``gym.make`` as main.py:45; ``name`` or
    ``spec.name``)."""
    if backend == "gym":
        from .gym_adapter import GymVecEnv
        return GymVecEnv(name or spec.name, num_envs, seed=seed, rank=rank, max_episode_length=max_episode_length)
    if backend != "builtin":
        raise ValueError(f"env backend must be builtin|gym, got {backend!r}")
    if spec.kind == KIND_TENSOR:
        cls = tensor_env_class(spec.name)
    else:
        cls = PendulumEnv if spec.kind == KIND_PENDULUM else SyntheticEnv
    return cls(spec, num_envs, seed=seed, rank=rank, device=device,
               max_episode_length=max_episode_length)
