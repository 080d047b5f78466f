"""Policy inference: ``PolicyRunner`` answers "here are E observations, give me the actions".

A runner holds a trained policy and its frozen observation statistics and nothing else — no
``HipEngine``, env, rollout buffers or optimizer state.  On the GPU one ``csrc/act.hip`` launch per
call normalises the observations, evaluates the policy on MFMA and samples with the keyed RNG; on
the CPU the torch twin (``ops/oracle.policy_act``) does the same.  The action noise is keyed by the
evaluator's stream (``rng.base_key(seed, STREAM_EVAL, 0)``), the row index and a step counter that
advances once per call, so a run is reproducible.

    runner = PolicyRunner.from_checkpoint("ckpt", device="gpu")
    action, logp = runner.act(obs)            # obs [E, O] (or [O]), fp32; a discrete policy: action indices [E]
"""
from __future__ import annotations

from typing import Dict, Optional

import torch

from ..models.actor_critic import ActorCritic
from ..ops import native, oracle
from ..utils import checkpoint, rng
from ..utils.obs_stats import RunningObsStats

GPU_DTYPES = ("fp32", "bf16x3", "bf16")


class PolicyRunner:
    def __init__(self, model_sd: Dict, obs_stats_sd: Dict, *, hidden=(100, 100), value_mult: int = 5,
                 device: str = "gpu", dtype: str = "bf16x3", seed: int = 1, std_convention: str = "std",
                 discrete: bool = False):
        if device not in ("cpu", "gpu"):
            raise ValueError(f"device must be cpu|gpu, got {device}")
        if dtype == "fp8":
            raise ValueError("PolicyRunner does not run fp8: the e4m3 policy image needs the engine's per-layer "
                             "scale refresh (HipEngine.act covers fp8); use fp32, bf16x3 or bf16")
        if dtype not in GPU_DTYPES:
            raise ValueError(f"dtype must be {'|'.join(GPU_DTYPES)}, got {dtype}")
        if std_convention not in ("std", "var"):
            raise ValueError("std_convention must be std|var")
        A, H2 = model_sd["mu.weight"].shape
        H1, O = model_sd["p_fc1.weight"].shape
        if (int(H1), int(H2)) != tuple(int(h) for h in hidden):
            raise ValueError(f"hidden={tuple(hidden)} does not match the state dict's ({int(H1)}, {int(H2)})")
        self.O, self.A = int(O), int(A)
        self.dtype, self.seed, self.std_convention = dtype, int(seed), std_convention
        # a discrete-action policy (EnvSpec.discrete): the A outputs are logits, act() returns action indices
        self.discrete = bool(discrete)
        if self.discrete and self.A < 2:
            raise ValueError(f"a discrete policy has at least 2 actions, the state dict's mu layer has {self.A}")
        self.gpu = device == "gpu"
        self.device = torch.device("cuda", torch.cuda.current_device()) if self.gpu else torch.device("cpu")
        self.model = ActorCritic(self.O, self.A, hidden, value_mult).to(self.device)
        self.model.load_state_dict(model_sd)
        self.model.requires_grad_(False)
        self.stats = RunningObsStats(self.O, self.device)
        self.stats.load_state_dict(obs_stats_sd)
        self.key_action = rng.base_key(self.seed, rng.STREAM_EVAL, 0)
        self.step = 0                      # the default step key: advances once per act()
        self._bufs: Dict[int, tuple] = {}  # GPU: (action, logp) outputs per row count
        if self.gpu:
            self.ext = native.load()
            self.dt = native.DT_CODE[dtype]
            L = self.model.packed_layout()
            ls = L.layers
            self.layout = ([L.w_off[l.name] for l in ls] + [L.wt_off[l.name] for l in ls] +
                           [l.d_in for l in ls] + [l.d_out for l in ls] + [l.fan_out for l in ls])
            from ..ops.storage import STORAGE
            self.wimg = torch.zeros(L.total, dtype=STORAGE[self.dt], device=self.device)
            self._none = torch.empty(0, dtype=torch.float32, device=self.device)
            # the packed image of the weights, as HipEngine.params_changed builds it
            self.ext.pack(self.model.flat.data, self.wimg, L.flat_to_w.to(self.device), L.flat_to_wt.to(self.device),
                          self.dt, self._none)

    @classmethod
    def from_checkpoint(cls, ckpt_dir: str, device: str = "gpu", dtype: Optional[str] = None) -> "PolicyRunner":
        """A runner for ``model.pt`` + ``trainer_state.pt`` of a training run: the network shape,
        seed, std convention and (unless given) the dtype come from the run's saved config."""
        model_sd = checkpoint.load_model_state(ckpt_dir)
        st = checkpoint.load_trainer_state(ckpt_dir)
        if st is None:
            raise FileNotFoundError(f"{ckpt_dir}: no trainer_state.pt (the observation statistics live there)")
        cfg = st["config"]
        if dtype is None:
            dtype = cfg.get("dtype", "bf16x3")
            if device == "cpu" and dtype == "fp8":
                dtype = "fp32"    # the CPU twin is fp32 whatever the run's GEMM precision was
        discrete = False
        if cfg.get("env_backend", "builtin") != "gym" and cfg.get("env_name"):
            # the action distribution follows the run's env (its module registers a user's env first)
            # A run whose module or env is not known here loads as before, with the Gaussian head (a caller that
            # serves a discrete policy without its env passes ``discrete=True`` to the constructor).
            from ..envs import get_spec, import_env_module
            try:
                import_env_module(cfg.get("env_module", ""))
                discrete = bool(get_spec(cfg["env_name"]).discrete)
            except (ImportError, KeyError):
                discrete = False
        return cls(model_sd, st["obs_stats"], hidden=tuple(cfg.get("hidden", (100, 100))),
                   value_mult=int(cfg.get("value_mult", 5)), device=device, dtype=dtype, seed=int(cfg.get("seed", 1)),
                   std_convention=cfg.get("std_convention", "std"), discrete=discrete)

    @torch.no_grad()
    def act(self, obs: torch.Tensor, deterministic: bool = False, step_key: Optional[int] = None):
        """``(action [E,A], logp [E])`` for ``obs`` ``[E,O]`` (a single ``[O]`` observation is one
        row).  The noise of row r is keyed (evaluator stream, r, ``step_key``); ``step_key``
        defaults to the runner's step counter, which advances once per call either way.  On the GPU
        the outputs are device tensors the runner owns (rewritten by the next call for the same E).
        A discrete policy returns ``(index [E] int64, logp [E])``: the Gumbel-max sample of the logits
        (``deterministic``: their arg-max), which a discrete env's ``step`` takes as it is."""
        obs = torch.as_tensor(obs, dtype=torch.float32).reshape(-1, self.O)
        key = self.step if step_key is None else int(step_key)
        self.step += 1
        E = int(obs.shape[0])
        if not self.gpu:
            a, logp, _, _ = oracle.policy_act(self.model, self.stats, obs, self.key_action,
                                              torch.arange(E, dtype=torch.int64), key, self.std_convention,
                                              deterministic, dist="categorical" if self.discrete else "gaussian")
            return (a.argmax(1), logp) if self.discrete else (a, logp)
        obs = obs.to(self.device).contiguous()
        bufs = self._bufs.get(E)
        if bufs is None:
            bufs = self._bufs[E] = (torch.zeros(E, self.A, dtype=torch.float32, device=self.device),
                                    torch.zeros(E, dtype=torch.float32, device=self.device))
        action, logp = bufs
        none = self._none
        ints = [E, self.O, self.A, 1 if self.std_convention == "var" else 0, 1 if deterministic else 0, 0,
                1 if self.discrete else 0]
        keys = [self.key_action & 0xFFFFFFFF, 0, key & 0xFFFFFFFF]
        self.ext.policy_act(self.dt, self.wimg, self.layout, [1.0] * 6, self.model.flat.data, self.stats.mean_f32,
                            self.stats.inv_std_f32, none, obs, action, logp, none, none, none, ints, keys, none)
        return (action.argmax(1), logp) if self.discrete else (action, logp)
