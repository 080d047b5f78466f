"""Hyper-parameters and CLI.

One dataclass carries every knob of both reference programs:

* preset ``dppo`` reproduces ``Params`` of ``main.py:18-39`` (batch 1000, lr 3e-4,
  4 workers, ``update_treshold = N-1`` …),
* preset ``ppo`` reproduces ``Params`` of ``ppo.py:21-42`` (batch 64, lr 7e-4,
  ent 0.01, max grad norm 0.5, 2048 steps …).

Field names are the reference's (``gae_param``, ``ent_coeff``, ``num_epoch``,
``exploration_size``, ``update_treshold`` — sic, ``main.py:30``; the correctly spelled
``update_threshold`` is accepted as an alias).  The fields after the reference block are
the MI355X-native additions listed in SURVEY.md §5.6.
"""
from __future__ import annotations

import argparse
import dataclasses
import json
import warnings
from dataclasses import dataclass, field, fields
from typing import Any, Dict, Optional


@dataclass
class Params:
    # ---- reference fields (main.py:18-39 / ppo.py:21-42) -------------------------------
    batch_size: int = 1000
    lr: float = 3e-4
    gamma: float = 0.99
    gae_param: float = 0.95
    clip: float = 0.2
    ent_coeff: float = 0.0
    num_epoch: int = 10
    num_steps: int = 1000
    exploration_size: int = 1000
    num_processes: int = 4
    update_treshold: Optional[int] = None  # sic (main.py:30); None -> num_processes - 1
    max_episode_length: int = 10000
    seed: int = 1
    env_name: str = "InvertedPendulum-v1"
    time_horizon: int = 1000000          # ppo.py:31 (outer iterations)
    max_grad_norm: Optional[float] = None  # ppo.py:33 uses 0.5; DPPO path has no clipping

    # ---- MI355X-native additions --------------------------------------
    device: str = "cpu"                  # cpu | gpu
    env_backend: str = "builtin"         # builtin (tensor envs: in-kernel on GPU when the rollout kernel knows the
                                         # kind, device-stepped otherwise) | gym (gym.make, host-stepped)
    env_fused: bool = False              # GPU engine: run an env that has an in-kernel twin (VecEnv.kernel_kind) inside the
                                         # rollout / evaluation kernels; changes nothing for the synthetic envs and the
                                         # pendulum (always in-kernel), moves CartPoleContinuous-v1 and the discrete
                                         # CartPole-v0 (the kernels' categorical head) off the device-stepped path; an env
                                         # without a kernel kind (CartPole-v1 among them) is refused.  The CPU engine ignores it.
    env_module: str = ""                 # dotted module path imported once at start (worker, evaluator process,
                                         # play.py) so that it can call envs.register_tensor_env; "" = none
    host_policy: str = "torch"           # env_backend gym on the GPU engine, the per-step policy: torch (fp32 tensor
                                         # ops: the path tests/test_gym_backend.py holds to the torch engine at 1e-6,
                                         # so it stays the default and that test's reference) | kernel (one
                                         # csrc/act.hip launch per step, buffer rows written in storage precision).
                                         # Making kernel the default and retiring the torch path is a later change.
    num_envs: int = 1                    # E vectorised envs per worker
    dtype: str = "fp32"                  # fp32 | bf16x3 | bf16 | fp8  (GEMM operand precision;
                                         # bf16x3 = fp32-accurate split-bf16 on the bf16 MFMA)
    hidden: tuple = (100, 100)           # model.py:11-12
    value_mult: int = 5                  # model.py:17 (value fc1 = hidden[0]*5)
    loss: str = "ppo"                    # ppo (corrected, ppo.py:148-167) | dppo_ref (train.py:142-161)
    value_loss: str = "mse"              # mse (ppo.py:164) | clipped_half (train.py:154-157)
    std_convention: str = "std"          # std: exp(log_std) is sigma (ppo.py:93) | var: it is sigma^2 (train.py:89)
    compat: bool = False                 # reproduce reference quirks Q1 (ones grad buffers), Q6 (same seed), Q8 (raw bootstrap)
    grad_reduce: str = "sum"             # sum (model.py:55, chief.py:16) | mean
    obs_norm_update: str = "rollout"     # step (model.py:68 per step) | rollout (one merge per rollout)
    reward_clip: float = 1.0             # train.py:96 clips to +-1; <=0 disables
    normalize_adv: bool = False
    adv_norm_scope: str = "rank"         # read with normalize_adv only.  rank: each rank normalises its own T*E
                                         # advantages in place (torch ops) | global: one mean / std over the T*E*W
                                         # advantages of all W ranks | minibatch: over this rank's rows of the current
                                         # update step, recomputed before every step, no collective (the CleanRL /
                                         # Stable-Baselines3 rule).  global and minibatch leave adv raw — the update
                                         # kernels apply the statistics at their advantage load (csrc/advnorm.hip,
                                         # ops/oracle.adv_block) — and log adv_mean, adv_std and explained_variance.
    bootstrap_time_limit: bool = False   # an episode ended by the step limit alone (truncated, not terminal) is
                                         # bootstrapped with V of the observation the env reached before its reset:
                                         # delta_t = r_t + gamma * V(s_{t+1}^true) - V_t, recursion still cut.  False: the
                                         # reference's GAE, which zeroes V_{t+1} at every episode end (train.py:98-112).
                                         # Refused with obs_norm_update=step, compat and env_backend=gym.
    reward_norm: bool = False            # GAE reads r' = r / (running std of the discounted return) (the
                                         # VecNormalize(norm_reward=True) rule; ops/oracle.return_scan).  The stored
                                         # rewards, episode returns and evaluation keep raw units.  Use with
                                         # reward_clip 0.  Refused with compat and with stats_stream on|auto.
    reward_norm_clip: float = 10.0       # r' clamped to +-this; <=0 disables
    target_kl: float = 0.0               # > 0: after each step of an iteration, kl = approx_kl of that step's
                                         # minibatch (summed over ranks); the first step with not (kl <= target_kl) is
                                         # still applied, the iteration's later steps are not (ops/oracle.kl_gate; the
                                         # decision is taken on the device).  Stopped steps still run their gradient
                                         # kernels: no time is saved.  0: off.  Refused with loss=dppo_ref, compat,
                                         # overlap_rollout and overlap_value_epochs.
    lr_schedule: str = "constant"        # constant | linear (annealed per iteration to lr * lr_final_frac at the end
                                         # of the run: needs max_iters or total_env_steps) | adaptive (after every applied
                                         # step the rate is divided by lr_adapt_factor when that step's KL is above
                                         # 2 * lr_kl_target and multiplied by it when below half, inside [lr_min, lr_max];
                                         # ops/oracle.lr_adapt, decided and read on the device).  adaptive is refused with
                                         # loss=dppo_ref, compat, overlap_rollout and overlap_value_epochs.
    lr_final_frac: float = 0.0           # linear: the rate at the run's last iteration, as a fraction of lr
    lr_kl_target: float = 0.008          # adaptive: the KL the rate is steered to
    lr_adapt_factor: float = 1.5         # adaptive: the divisor / multiplier (> 1)
    lr_min: float = 1e-6                 # adaptive: the rate's bounds; lr starts inside them
    lr_max: float = 1e-2
    minibatches_per_epoch: int = 0       # 0 = buffer // batch_size (full pass); reference ppo.py uses 1
    total_env_steps: int = 0             # 0 = unbounded (use max_iters)
    max_iters: int = 0                   # 0 = unbounded
    eval_every: int = 0                  # evaluator snapshot period in iterations (0 = off)
    eval_episodes: int = 1
    eval_sleep: float = 0.0              # test.py:63 sleeps 10 s per episode; default no sleep
    eval_mode: str = "process"           # process (the CPU evaluator process, one env) | inline (batched, in the
                                         # trainer's engine: csrc/eval.hip on the GPU engine, its torch twin on the CPU one)
    eval_envs: int = 256                 # inline: evaluation envs (one first episode each)
    eval_deterministic: bool = False     # inline: act with mu (the reference acts stochastically, test.py:40-44)
    checkpoint_dir: str = ""
    checkpoint_every: int = 0
    resume: str = ""
    log_jsonl: str = ""
    log_every: int = 1
    # the last gradient all-reduce overlaps the next rollout.  GPU engine: the value
    # head's last step stays pending until after the next rollout (which reads only the policy:
    # exact); CPU engine: the whole last step (option b, a 1-update policy lag)
    overlap_rollout: bool = False
    # GPU engine, in-stream communicator (the default at N > 1): EVERY epoch's value-head all-reduce
    # + Adam on a side stream (second communicator), joined just before the next value kernel, so
    # it runs beside the next epoch's policy Adam + policy kernel (chief.py:13-20's sum -> Adam ->
    # release off the critical path, once per epoch).  Exact (the policy chain reads no value
    # parameter).  False: stream order (only the last epoch's, with overlap_rollout)
    overlap_value_epochs: bool = False
    dist_timeout_s: float = 300.0
    verify_sync_every: int = 0           # debug param-checksum all-reduce period
    adam_betas: tuple = (0.9, 0.999)
    adam_eps: float = 1e-8
    # ---- observability / failure detection ----------------------
    log_csv: str = ""                    # learning-curve CSV (rank 0), the figs/*.png analogue
    profile_dir: str = ""                # torch.profiler chrome traces (host + HIP timeline) per rank
    profile_iters: str = "2:4"           # [start:stop) iterations captured when profile_dir is set
    heartbeat_s: float = -1.0            # per-rank heartbeat in the rendezvous store every N s (<0: auto =
                                         # 5 s whenever world_size > 1; 0: off)
    heartbeat_timeout_s: float = 60.0    # a peer silent this long is reported dead: abort + exit 75
    check_finite: bool = False           # debug: stop with the failing phase when loss/params go non-finite
    phase_timing: int = 1                # per-phase HIP-event timing every N iterations (0 = off; each
                                         # event record idles the GPU ~10 us, see PhaseTimer)
    # ---- execution options (the GPU engine's paths; A/B switches of earlier rounds) ----------
    dist_backend: str = "auto"           # auto: nccl (RCCL) on gpu, gloo on cpu | nccl | gloo (GPU ranks
                                         # sharing one device: the 1-GPU box's multi-rank runs)
    grad_comm: str = "auto"              # auto: in-stream communicator when available (csrc/comm.cpp RCCL;
                                         # gloo adapter) | native (required) | process_group (torch's)
    update_kernels: str = "auto"         # auto | heads (per-head streaming kernels, csrc/mlp_head.hip) |
                                         # tile (one-kernel update, csrc/mlp.hip)
    fused_apply: bool = True             # world size 1: gradient gather + Adam in one launch
    fp8_wgrad_operands: bool = True      # dtype fp8 on the per-head path: e4m3 wgrad operands (else bf16)
    fp8_policy_gemms: bool = False       # dtype fp8: the policy head's fc1 / fc2 on the e4m3 x128 MFMA too (opt-in:
                                         # speed-neutral and 3x the policy-gradient error, profiles/r4/fp8_heads.md)
    stats_stream: str = "off"            # off | on | auto (on when an all-reduce sits in the chain): the
                                         # obs-stat reduce / all-reduce / merge on a side stream
    wgrad_wgs: int = 0                   # wgrad tasks per launch (0: one per CU of the device)
    wgrad_wide: bool = True              # wgrad tiles of up to 16 quadrants, two per wave (split-bf16 / bf16;
                                         # csrc/wgrad.hip)
    phead_kernel: bool = True            # the policy head on the 32x32 kernel (csrc/phead.hip)
    phead_fused_dw2: str = "auto"        # auto | on | off: ... summing p_fc2's weight gradient in the kernel
                                         # (auto: at bf16x3 only, the measured-faster choice per dtype)
    mlp_rows: int = 0                    # diagnostics: force the tile update kernel's row tile (0: auto)

    # ------------------------------------------------------------------------------------
    def __post_init__(self):
        if self.update_treshold is None:
            self.update_treshold = self.num_processes - 1
        elif self.update_treshold != self.num_processes - 1:
            # chief.py:13 fires when counter > threshold, i.e. with threshold+1 of N workers'
            # gradients.  The synchronous RCCL all-reduce always combines all N ranks, so a
            # smaller threshold (straggler tolerance) cannot be honoured: say so, do not no-op.
            warnings.warn(f"update_treshold={self.update_treshold} is inert: the gradient all-reduce is "
                          f"synchronous over all num_processes={self.num_processes} ranks (reference "
                          f"default N-1 = {self.num_processes - 1})", UserWarning, stacklevel=3)
        self.hidden = tuple(int(h) for h in self.hidden)
        self.adam_betas = tuple(float(b) for b in self.adam_betas)
        if self.device not in ("cpu", "gpu"):
            raise ValueError(f"device must be cpu|gpu, got {self.device}")
        if self.env_backend not in ("builtin", "gym"):
            raise ValueError(f"env_backend must be builtin|gym, got {self.env_backend}")
        if self.env_fused and self.env_backend == "gym":
            raise ValueError("env_fused runs a builtin env inside the rollout kernel; env_backend=gym is host-stepped")
        if self.host_policy not in ("torch", "kernel"):
            raise ValueError(f"host_policy must be torch|kernel, got {self.host_policy}")
        if self.dtype not in ("fp32", "bf16x3", "bf16", "fp8"):
            raise ValueError(f"dtype must be fp32|bf16x3|bf16|fp8, got {self.dtype}")
        if self.phead_fused_dw2 not in ("auto", "on", "off"):
            raise ValueError(f"phead_fused_dw2 must be auto|on|off, got {self.phead_fused_dw2}")
        if self.loss not in ("ppo", "dppo_ref"):
            raise ValueError(f"loss must be ppo|dppo_ref, got {self.loss}")
        if self.value_loss not in ("mse", "clipped_half"):
            raise ValueError(f"value_loss must be mse|clipped_half, got {self.value_loss}")
        if self.std_convention not in ("std", "var"):
            raise ValueError("std_convention must be std|var")
        if self.grad_reduce not in ("sum", "mean"):
            raise ValueError("grad_reduce must be sum|mean")
        if self.loss == "dppo_ref":
            # train.py:88-89,143-146 treat exp(log_std) as the variance everywhere
            self.std_convention = "var"
        if self.obs_norm_update not in ("step", "rollout"):
            raise ValueError("obs_norm_update must be step|rollout")
        if self.bootstrap_time_limit:
            if self.obs_norm_update == "step":
                raise ValueError("bootstrap_time_limit is not built for obs_norm_update=step (the per-step filter's "
                                 "launches); use obs_norm_update=rollout")
            if self.compat:
                raise ValueError("bootstrap_time_limit cannot be combined with compat: compat reproduces the "
                                 "reference, which zeroes the value at every episode end")
            if self.env_backend == "gym":
                raise ValueError("bootstrap_time_limit needs the final observation of a truncated step; "
                                 "env_backend=gym auto-resets on the host and does not keep it")
        if self.eval_mode not in ("process", "inline"):
            raise ValueError(f"eval_mode must be process|inline, got {self.eval_mode}")
        if int(self.eval_envs) < 1:
            raise ValueError(f"eval_envs must be >= 1, got {self.eval_envs}")
        if self.eval_mode == "inline" and self.env_backend == "gym":
            raise ValueError("eval_mode=inline evaluates the builtin envs; env_backend=gym needs eval_mode=process")
        for name, ok in (("dist_backend", ("auto", "nccl", "gloo")), ("grad_comm", ("auto", "native", "process_group")),
                         ("update_kernels", ("auto", "heads", "tile")), ("stats_stream", ("off", "on", "auto"))):
            if getattr(self, name) not in ok:
                raise ValueError(f"{name} must be {'|'.join(ok)}, got {getattr(self, name)}")
        if self.reward_norm:
            if self.compat:
                raise ValueError("reward_norm cannot be combined with compat: compat reproduces the reference, "
                                 "whose only reward scaling is the clip to +-1")
            if self.stats_stream != "off":
                raise ValueError("reward_norm is not built for stats_stream=on|auto: the return scale is merged on "
                                 "the compute stream before GAE reads it; use stats_stream=off")
        if self.adv_norm_scope not in ("rank", "global", "minibatch"):
            raise ValueError(f"adv_norm_scope must be rank|global|minibatch, got {self.adv_norm_scope}")
        if self.adv_norm_scope != "rank":
            if not self.normalize_adv:
                raise ValueError(f"adv_norm_scope={self.adv_norm_scope} is a scope of normalize_adv: set normalize_adv "
                                 "true")
            if self.adv_norm_scope == "minibatch" and self.minibatch_rows() < 2:
                raise ValueError("adv_norm_scope=minibatch needs a minibatch of at least 2 rows (the unbiased std), got "
                                 f"{self.minibatch_rows()}")
            if self.adv_norm_scope == "global" and self.buffer_rows * self.num_processes < 2:
                raise ValueError("adv_norm_scope=global needs at least 2 advantages per iteration (the unbiased std), "
                                 f"got {self.buffer_rows * self.num_processes}")

        self.target_kl = float(self.target_kl)
        if not self.target_kl >= 0:
            raise ValueError(f"target_kl must be >= 0 (0 = off): a KL estimate is never below a negative "
                             f"target, got {self.target_kl}")
        if self.target_kl > 0:
            if self.loss == "dppo_ref":
                raise ValueError("target_kl cannot be combined with loss=dppo_ref: that loss reports approx_kl = 0 by "
                                 "construction, so the gate would never trip")
            if self.compat:
                raise ValueError("target_kl cannot be combined with compat: compat reproduces the reference, which "
                                 "applies every update step")
            if self.overlap_rollout or self.overlap_value_epochs:
                raise ValueError("target_kl cannot be combined with overlap_rollout / overlap_value_epochs: they move "
                                 "a value step to a side stream or behind the next rollout, and a gated step reads and "
                                 "advances one device counter in stream order")

        if self.lr_schedule not in ("constant", "linear", "adaptive"):
            raise ValueError(f"lr_schedule must be constant|linear|adaptive, got {self.lr_schedule}")
        if self.lr_schedule == "linear":
            if not (self.max_iters > 0 or self.total_env_steps > 0):
                raise ValueError("lr_schedule=linear anneals to the end of the run: set max_iters or total_env_steps")
            if not 0.0 <= float(self.lr_final_frac) <= 1.0:
                raise ValueError(f"lr_final_frac must be in [0, 1], got {self.lr_final_frac}")
        if self.lr_schedule == "adaptive":
            if not self.lr_kl_target > 0:
                raise ValueError(f"lr_kl_target must be > 0, got {self.lr_kl_target}")
            if not self.lr_adapt_factor > 1:
                raise ValueError(f"lr_adapt_factor must be > 1, got {self.lr_adapt_factor}")
            if not 0 < self.lr_min <= self.lr_max:
                raise ValueError(f"lr_schedule=adaptive needs 0 < lr_min <= lr_max, got [{self.lr_min}, {self.lr_max}]")
            if not self.lr_min <= self.lr <= self.lr_max:
                raise ValueError(f"lr_schedule=adaptive: the initial lr {self.lr} is outside [lr_min, lr_max] = "
                                 f"[{self.lr_min}, {self.lr_max}]")
            if self.loss == "dppo_ref":
                raise ValueError("lr_schedule=adaptive cannot be combined with loss=dppo_ref: that loss reports "
                                 "approx_kl = 0 by construction, so the rate would only ever go up")
            if self.compat:
                raise ValueError("lr_schedule=adaptive cannot be combined with compat: compat reproduces the reference, "
                                 "whose rate is constant")
            if self.overlap_rollout or self.overlap_value_epochs:
                raise ValueError("lr_schedule=adaptive cannot be combined with overlap_rollout / overlap_value_epochs: "
                                 "they move a value step to a side stream or behind the next rollout, and an adaptive "
                                 "step reads the device rate and counter in stream order")

    def adv_scope(self) -> str:
        """the advantage normalisation applied at the loss: "global" | "minibatch", or "" (off, and scope rank, which
        normalises the buffer in place)"""
        return self.adv_norm_scope if (self.normalize_adv and self.adv_norm_scope != "rank") else ""

    def gated(self) -> bool:
        """the update steps run through the KL gate (target_kl, or the adaptive rate, which lives behind it)"""
        return self.target_kl > 0 or self.lr_schedule == "adaptive"

    def gate_target(self) -> float:
        """the KL the gate trips on: target_kl, else +inf (lr_schedule=adaptive alone: only a NaN KL trips)"""
        return float(self.target_kl) if self.target_kl > 0 else float("inf")

    def schedule_iters(self, world_size: int = 1) -> int:
        """the run's iteration count n of lr_schedule=linear: max_iters, else the iterations total_env_steps takes"""
        if self.max_iters > 0:
            return int(self.max_iters)
        return max(1, -(-int(self.total_env_steps) // (self.buffer_rows * max(1, world_size))))

    def linear_lr(self, iteration: int, world_size: int = 1) -> float:
        """lr_schedule=linear: the rate of iteration ``iteration`` (0-based), a pure function of the index"""
        n = self.schedule_iters(world_size)
        return self.lr * (1.0 - (1.0 - self.lr_final_frac) * min(iteration, n) / n)

    def heartbeat_interval(self, world_size: int) -> float:
        """the heartbeat period in effect: heartbeat_s, or 5 s (auto) whenever there are peers"""
        if self.heartbeat_s >= 0:
            return float(self.heartbeat_s)
        return 5.0 if world_size > 1 else 0.0

    # alias with the correct spelling
    @property
    def update_threshold(self) -> int:
        return self.update_treshold

    @update_threshold.setter
    def update_threshold(self, v: int) -> None:
        self.update_treshold = v

    # rollout geometry: T steps x E envs per worker --------------------------------------
    @property
    def rollout_len(self) -> int:
        """T: steps per env per iteration so that T*E ~= exploration_size."""
        return max(1, -(-self.exploration_size // max(1, self.num_envs)))

    @property
    def buffer_rows(self) -> int:
        return self.rollout_len * self.num_envs

    def gae_segment(self) -> int:
        """the reference's segment length num_steps (train.py:82, ppo.py:87) when it cuts the
        T-step rollout (0 otherwise): GAE restarts after every num_steps steps, bootstrapping
        the not-done state (ops/oracle.gae, csrc/optim.hip gae kernels)"""
        return self.num_steps if 0 < self.num_steps < self.rollout_len else 0

    def minibatch_rows(self) -> int:
        return max(1, min(self.batch_size, self.buffer_rows))

    def num_minibatches(self) -> int:
        if self.minibatches_per_epoch > 0:
            return self.minibatches_per_epoch
        return max(1, self.buffer_rows // self.minibatch_rows())

    def to_dict(self) -> Dict[str, Any]:
        d = dataclasses.asdict(self)
        d["hidden"] = list(self.hidden)
        d["adam_betas"] = list(self.adam_betas)
        return d

    def to_json(self) -> str:
        return json.dumps(self.to_dict(), sort_keys=True)

    @classmethod
    def from_dict(cls, d: Dict[str, Any]) -> "Params":
        d = dict(d)
        if "update_threshold" in d:
            d["update_treshold"] = d.pop("update_threshold")
        names = {f.name for f in fields(cls)}
        return cls(**{k: v for k, v in d.items() if k in names})


def dppo_preset(**overrides) -> Params:
    """``main.py:18-39`` values."""
    p = dict(batch_size=1000, lr=3e-4, gamma=0.99, gae_param=0.95, clip=0.2, ent_coeff=0.0,
             num_epoch=10, num_steps=1000, exploration_size=1000, num_processes=4,
             max_episode_length=10000, seed=1, env_name="InvertedPendulum-v1",
             max_grad_norm=None, loss="ppo", value_loss="clipped_half", std_convention="std")
    p.update(overrides)
    return Params(**p)


def ppo_preset(**overrides) -> Params:
    """``ppo.py:21-42`` values (single process)."""
    p = dict(batch_size=64, lr=7e-4, gamma=0.99, gae_param=0.95, clip=0.2, ent_coeff=0.01,
             num_epoch=10, num_steps=2048, exploration_size=2048, time_horizon=1000000,
             max_episode_length=10000, max_grad_norm=0.5, seed=1, env_name="HalfCheetah-v1",
             num_processes=1, loss="ppo", value_loss="mse", std_convention="std",
             minibatches_per_epoch=1)
    p.update(overrides)
    return Params(**p)


PRESETS = {"dppo": dppo_preset, "ppo": ppo_preset}


def _parse_bool(s: str) -> bool:
    return str(s).lower() in ("1", "true", "yes", "y", "on")


def build_arg_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description="MI355X-native DPPO / PPO trainer")
    ap.add_argument("--preset", choices=sorted(PRESETS), default="dppo")
    for f in fields(Params):
        flag = "--" + f.name.replace("_", "-")
        default = None
        if f.name == "hidden" or f.name == "adam_betas":
            ap.add_argument(flag, type=str, default=default, help=f"comma list (default preset)")
        elif f.type in ("bool", bool):
            ap.add_argument(flag, type=_parse_bool, default=default, nargs="?", const=True)
        elif f.name in ("update_treshold",):
            ap.add_argument(flag, "--update-threshold", type=int, default=default)
        elif f.name == "max_grad_norm":
            ap.add_argument(flag, type=float, default=default)
        else:
            t = {"int": int, "float": float, "str": str}.get(str(f.type), None)
            if t is None:
                t = type(f.default) if f.default is not None else str
            ap.add_argument(flag, type=t, default=default)
    return ap


def params_from_args(argv=None) -> Params:
    ap = build_arg_parser()
    ns = ap.parse_args(argv)
    overrides = {}
    for f in fields(Params):
        v = getattr(ns, f.name, None)
        if v is None:
            continue
        if f.name in ("hidden", "adam_betas"):
            v = tuple(float(x) if f.name == "adam_betas" else int(x) for x in str(v).split(","))
        overrides[f.name] = v
    return PRESETS[ns.preset](**overrides)
