"""Eager-PyTorch engine: the CPU execution path (BASELINE config 1) and the end-to-end oracle
for the HIP engine.

One *engine* owns the device-side state of one DPPO worker — the vectorised envs, the
``[T,E]`` rollout buffer, the flat parameters / gradient / Adam moments — and exposes the
phases the worker loop (``runtime/worker.py``) sequences:

    rollout()  ->  values()  ->  gae()  ->  for each minibatch: step(idx) = grad(idx) -> [all-reduce] -> apply()

Reference mapping: rollout = ``train.py:60-106``; values/bootstrap = ``train.py:109-112``;
gae = ``train.py:117-122``; grad = ``train.py:140-166``; apply = ``chief.py:15-19``.
"""
from __future__ import annotations

import math
import warnings
from typing import Dict, Optional

import torch

from ..config import Params
from ..models.actor_critic import ActorCritic
from ..ops import oracle
from ..utils import rng
from ..utils.obs_stats import RunningObsStats
from ..utils.ret_stats import RunningReturnStats
from .engine import Engine, check_discrete


class TorchEngine(Engine):
    name = "torch"

    def __init__(self, params: Params, model: ActorCritic, env, stats: RunningObsStats,
                 device: torch.device, action_rank: int):
        self.p = params
        self.model = model
        self.env = env
        self.stats = stats
        self.device = device
        # a discrete env: the policy's A outputs are logits, `actions` holds one-hot rows, the env takes indices
        self.discrete = check_discrete(params, getattr(env, "spec", None))
        self.dist = "categorical" if self.discrete else "gaussian"
        T, E = params.rollout_len, env.E
        O, A = env.O, env.A
        self.T, self.E, self.O, self.A = T, E, O, A
        f32 = dict(device=device, dtype=torch.float32)
        self.x = torch.zeros(T + 1, E, O, **f32)         # normalised observations (update input)
        self.raw_last = torch.zeros(E, O, **f32)          # raw bootstrap obs (compat Q8)
        self.actions = torch.zeros(T, E, A, **f32)
        self.logp = torch.zeros(T, E, **f32)
        self.values_buf = torch.zeros(T + 1, E, **f32)
        self.rewards = torch.zeros(T, E, **f32)
        self.dones = torch.zeros(T, E, **f32)
        self.adv = torch.zeros(T, E, **f32)
        self.ret = torch.zeros(T, E, **f32)
        # bootstrap_time_limit: which steps ended by the step limit alone, the normalised observation
        # each reached before its reset (slot t // limit: an env's truncations are >= limit steps
        # apart) and its value
        self.boot = bool(params.bootstrap_time_limit)
        if self.boot:
            env.report_final = True
            self.fin_K = -(-T // env.limit)
            self.trunc = torch.zeros(T, E, **f32)
            self.x_fin = torch.zeros(self.fin_K, E, O, **f32)
            self.v_fin = torch.zeros(self.fin_K, E, **f32)
        # reward_norm: the carry of the discounted-return scan (per rank, checkpointed with the env) and
        # the running statistics of the return (global); allocated only with the flag on
        self.ret_stats: Optional[RunningReturnStats] = None
        self.ret_acc: Optional[torch.Tensor] = None
        if bool(params.reward_norm):
            self.ret_stats = RunningReturnStats(device)
            self.ret_acc = torch.zeros(E, **f32)
        n = model.num_params
        self.grad_flat = torch.zeros(n, **f32)
        self.adam_m = torch.zeros(n, **f32)
        self.adam_v = torch.zeros(n, **f32)
        self.adam_step = 0
        # target_kl: [stop, applied, trip_kl, last_kl] of the current iteration (ops/oracle.kl_gate) and
        # the last step's (KL sum, row count); only with the flag on
        self.gate: Optional[list] = [0.0, 0.0, 0.0, 0.0] if params.gated() else None
        self.kl_pair: Optional[torch.Tensor] = None
        # lr_schedule: the rate apply() reads.  linear: the worker sets it once per iteration; adaptive:
        # lr_state = [lr, downs, ups, reserved] as fp32 values (the HIP engine's device state), moved by
        # adapt() after every applied step and never reset
        self.lr = float(params.lr)
        self.lr_state: Optional[list] = None
        if params.lr_schedule == "adaptive":
            self.lr = float(torch.tensor(params.lr, dtype=torch.float32))
            self.lr_state = [self.lr, 0.0, 0.0, 0.0]
        # adv_norm_scope global | minibatch: adv stays raw; adv_block = fp32 [mean, inv, std, explained variance] of
        # the whole buffer (global: of every rank's), set after gae() through adv_sums() / set_adv_sums(); grad()
        # applies it to the gathered rows (minibatch: the block of the step's own rows).  Only with the flag on.
        self.adv_scope = params.adv_scope()
        self.adv_block: Optional[torch.Tensor] = None
        self.flat_old = model.flat.detach().clone()  # dppo_ref "model_old" (train.py:128-129,164)
        self.key_action = rng.base_key(params.seed, rng.STREAM_ACTION, action_rank)
        self.obs = env.reset().to(device)
        self.local_stats: Optional[RunningObsStats] = None
        self._pending = None          # (async all-reduce work, extra) of a step deferred under --overlap-rollout

    # -- rollout ---------------------------------------------------------------------------
    @torch.no_grad()
    def rollout(self) -> Dict:
        p, T, E = self.p, self.T, self.E
        shift = self.stats.shift().clone()
        s1 = torch.zeros(self.O, dtype=torch.float64, device=self.device)
        s2 = torch.zeros(self.O, dtype=torch.float64, device=self.device)
        count = 0.0
        norm_stats = self.stats
        if p.obs_norm_update == "step":
            self.local_stats = RunningObsStats(self.O, self.device)
            self.local_stats.copy_from(self.stats)
            norm_stats = self.local_stats
        ep_ret_sum = torch.zeros((), dtype=torch.float64, device=self.device)
        ep_count = torch.zeros((), dtype=torch.float64, device=self.device)
        eidx = self.env.env_idx.to(self.device)
        dims = torch.arange(self.A, device=self.device, dtype=torch.int64)
        log_std = self.model.view("log_std")
        log_sigma = log_std if p.std_convention == "std" else 0.5 * log_std
        sigma = torch.exp(log_sigma)
        for t in range(T):
            raw = self.obs
            c, a1, a2 = RunningObsStats.moments(raw, shift)
            count += c
            s1 += a1
            s2 += a2
            if p.obs_norm_update == "step":
                norm_stats.observes(raw)
            x = norm_stats.normalize(raw)
            mu, _, _ = self.model(x)
            if self.discrete:
                ai, a, logp = oracle.categorical_sample(mu, self.key_action, eidx, self.env.t)
            else:
                eps = rng.gauss(self.key_action, eidx[:, None], self.env.t, dims[None, :])
                ai = a = mu + sigma * eps
                logp = (-0.5 * eps * eps - 0.5 * oracle.LOG_2PI - log_sigma).sum(-1)
            obs, r, done, info = self.env.step(ai)
            if p.reward_clip > 0:
                r = r.clamp(-p.reward_clip, p.reward_clip)
            self.x[t] = x
            self.actions[t] = a
            self.logp[t] = logp
            self.rewards[t] = r
            self.dones[t] = done.to(torch.float32)
            if self.boot:
                tr = info["truncated"].to(self.device)
                self.trunc[t] = tr.to(torch.float32)
                slot = self.x_fin[t // self.env.limit]
                slot[tr] = norm_stats.normalize(info["final_obs"].to(self.device))[tr]
            ep_ret_sum += info["ep_return_sum"].to(torch.float64)
            ep_count += info["ep_count"].to(torch.float64)
            self.obs = obs.to(self.device)
        self.x[T] = norm_stats.normalize(self.obs)
        self.raw_last.copy_(self.obs)
        return {"count": count, "s1": s1, "s2": s2, "shift": shift,
                "ep_return_sum": float(ep_ret_sum), "ep_count": float(ep_count)}

    @torch.no_grad()
    def values(self) -> None:
        T, E = self.T, self.E
        _, _, v = self.model(self.x.reshape((T + 1) * E, self.O))
        self.values_buf.copy_(v.reshape(T + 1, E))
        if self.p.compat:  # Q8: bootstrap with the raw, un-normalised state (train.py:111)
            _, _, vb = self.model(self.raw_last)
            self.values_buf[T] = vb.reshape(E)
        if self.boot:
            _, _, vf = self.model(self.x_fin.reshape(self.fin_K * E, self.O))
            self.v_fin.copy_(vf.reshape(self.fin_K, E))

    @torch.no_grad()
    def return_moments(self) -> torch.Tensor:
        """reward_norm, after a rollout: the discounted-return scan over the rollout's rewards / dones
        (``ret_acc`` advanced) -> fp64 [2] = (S1, S2) of its T*E samples about the statistics' shift;
        the worker sums it over ranks and hands it to ``merge_return_moments``."""
        acc, s1, s2 = oracle.return_scan(self.rewards, self.dones, self.p.gamma, self.ret_acc, self.ret_stats.shift())
        self.ret_acc.copy_(acc)
        return torch.stack([s1, s2])

    def merge_return_moments(self, count: float, s12: torch.Tensor) -> None:
        rs = self.ret_stats
        rs.merge_moments(float(count), s12[0:1], s12[1:2], rs.shift())

    @torch.no_grad()
    def gae(self) -> None:
        boot = None
        if self.boot:
            slot = torch.arange(self.T, device=self.device) // self.env.limit
            boot = self.trunc * self.v_fin[slot]
        rewards = self.rewards
        if self.ret_stats is not None:
            rewards = oracle.scale_rewards(rewards, self.ret_stats.scale, float(self.p.reward_norm_clip))
        adv, ret = oracle.gae(rewards, self.values_buf, self.dones, self.p.gamma, self.p.gae_param,
                              segment=self.p.gae_segment(), boot=boot)
        if self.p.normalize_adv and not self.adv_scope:
            adv = (adv - adv.mean()) / (adv.std() + 1e-8)
        self.adv.copy_(adv)
        self.ret.copy_(ret)

    @torch.no_grad()
    def adv_sums(self, finish: bool = True) -> torch.Tensor:
        """adv_norm_scope global | minibatch, after gae(): fp64 [sum a, sum a^2, sum r, sum r^2] of this rank's whole
        buffer (ops/oracle.adv_sums).  ``finish``: they are the iteration's (no other rank's join them) and become
        the block here; else the worker sums them over the ranks and hands them to ``set_adv_sums``."""
        sums = oracle.adv_sums(self.adv, self.ret)
        if finish:
            self.set_adv_sums(sums, float(self.T * self.E))
        return sums

    def set_adv_sums(self, sums: torch.Tensor, n: float) -> None:
        self.adv_block = oracle.adv_block(sums, n)

    def current_obs(self) -> torch.Tensor:
        return self.obs

    @torch.no_grad()
    def evaluate(self, num_envs: int, deterministic: bool = False):
        """Batched evaluation of the current policy under the current observation statistics on
        fresh evaluation envs (runtime/evaluator.py evaluate_batch — the twin of the GPU engine's
        kernel): ``(ret fp32 [E], len int32 [E])``.  Touches no training state."""
        from .evaluator import evaluate_batch
        if getattr(self.env, "host_stepped", False):
            raise RuntimeError("evaluate() steps the builtin envs; a host-stepped (gym) env has no batched evaluation")
        p = self.p
        return evaluate_batch(self.model, self.stats, self.env.spec, num_envs, p.seed, p.max_episode_length,
                              p.std_convention, deterministic)

    def env_state(self) -> Dict:
        d = self.env.state_dict()
        if self.ret_acc is not None:
            d = dict(d, ret_acc=self.ret_acc.detach().cpu().clone())
        return d

    def load_env_state(self, d: Dict) -> None:
        d = load_ret_acc(self, d)
        self.env.load_state_dict(d)
        self.obs = self.env.observe().to(self.device)

    def begin_update(self) -> None:
        self.flat_old.copy_(self.model.flat.detach())
        if self.gate is not None:
            self.gate = [0.0, 0.0, 0.0, 0.0]

    # -- update ----------------------------------------------------------------------------
    def grad(self, idx: torch.Tensor) -> Dict[str, float]:
        """loss + backward on rows ``idx`` of the flattened [T*E] buffer -> self.grad_flat."""
        p = self.p
        N = self.T * self.E
        full = idx is None
        if full:
            idx = torch.arange(N, device=self.device)
        x = self.x[:self.T].reshape(N, self.O)[idx]
        a = self.actions.reshape(N, self.A)[idx]
        adv = self.adv.reshape(N)[idx]
        ret = self.ret.reshape(N)[idx]
        if self.adv_scope:
            block = self.adv_block
            if self.adv_scope == "minibatch" and not full:
                block = oracle.adv_block(oracle.adv_sums(self.adv, self.ret, idx), idx.numel())
            adv = oracle.adv_apply(adv, block)
        self.model.flat.grad = None
        mu, log_std, v = self.model(x)
        if p.loss == "ppo":
            logp_old = self.logp.reshape(N)[idx]
            v_old = self.values_buf[:self.T].reshape(N)[idx]
            out = oracle.ppo_loss(mu, log_std, v, a, logp_old, adv, ret, v_old, clip=p.clip,
                                  ent_coeff=p.ent_coeff, value_loss=p.value_loss,
                                  convention=p.std_convention, dist=self.dist)
        else:
            with torch.no_grad():
                mu_o, ls_o, v_o = _forward_with(self.model, self.flat_old, x)
            out = oracle.dppo_ref_loss(mu, log_std, v, mu_o, ls_o, v_o, a, adv, ret,
                                       clip=p.clip, ent_coeff=p.ent_coeff)
            # train.py:164 model_old <- model (pre-update params of this step)
            self.flat_old.copy_(self.model.flat.detach())
        out["loss"].backward()
        self.grad_flat.copy_(self.model.flat.grad)
        self._last = {k: float(v.detach()) for k, v in out.items()}
        if self.gate is not None:
            # target_kl: slots 3 and 5 of the HIP engine's loss sums (the estimator's sum, the row count)
            M = float(idx.numel())
            self.kl_pair = torch.stack([out["approx_kl"].detach().to(torch.float32) * M,
                                        torch.tensor(M, dtype=torch.float32, device=self.device)])
        return self._last

    @torch.no_grad()
    def skip(self) -> float:
        """target_kl, a stopped step: nothing moves; the reported gradient norm is this step's, as the
        HIP engine's stopped launches leave it"""
        self._norm = float(torch.linalg.vector_norm(self.grad_flat))
        return self._norm

    @torch.no_grad()
    def apply(self, extra_grad: float = 0.0) -> float:
        """clip (optional) + Adam on the flat buffers; returns the pre-clip grad norm."""
        g = self.grad_flat
        if extra_grad:
            g.add_(extra_grad)
        norm = float(torch.linalg.vector_norm(g))
        if self.p.max_grad_norm is not None and self.p.max_grad_norm > 0:
            oracle.clip_grad_norm_(g, self.p.max_grad_norm)
        self.adam_step += 1
        oracle.adam_step_(self.model.flat.data, g, self.adam_m, self.adam_v, self.adam_step,
                          self.lr, self.p.adam_betas, self.p.adam_eps)
        self._norm = norm
        return norm

    def adapt(self, kl: float) -> None:
        """lr_schedule=adaptive, after an APPLIED step whose KL was ``kl`` (the gate's last_kl):
        ops/oracle.lr_adapt moves the rate the next step runs at"""
        p, st = self.p, self.lr_state
        st[0] = oracle.lr_adapt(st[0], kl, p.lr_kl_target, p.lr_adapt_factor, p.lr_min, p.lr_max)
        d = oracle.lr_adapt_dir(kl, p.lr_kl_target)
        if d:
            st[1 if d < 0 else 2] += 1.0
        self.lr = st[0]

    # -- one global step ------------------------------------------------------------------------
    def step(self, idx: Optional[torch.Tensor], extra_grad: float = 0.0, allreduce=None,
             mean: bool = False, last: bool = False) -> bool:
        """ONE global step (runtime/engine.py): grad(idx), the all-reduce, apply().  --overlap-rollout: the
        iteration's last step stays deferred — its all-reduce runs beside the next rollout and finish_steps()
        applies it (a 1-update policy lag, safe for PPO because logp_old is recorded at rollout)."""
        p = self.p
        self.grad(idx)
        if self.gate is not None:
            # target_kl (ops/oracle.kl_gate): the step is applied while the gate is open, then the gate sees its KL
            self._reduce(allreduce, self.grad_flat, mean)
            self._reduce(allreduce, self.kl_pair, False)
            if self.gate[0] == 0.0:
                self.apply(extra_grad)
            else:
                self.skip()
            self.gate, applied = oracle.kl_gate(self.kl_pair[0], self.kl_pair[1], p.gate_target(), self.gate)
            if applied and self.lr_state is not None:
                self.adapt(self.gate[3])           # the next step's rate (ops/oracle.lr_adapt)
            return applied
        if p.overlap_rollout and last and not mean and allreduce is not None:
            self._pending = (allreduce(self.grad_flat), extra_grad)
            return True
        self._reduce(allreduce, self.grad_flat, mean)
        self.apply(extra_grad)
        return True

    def _reduce(self, allreduce, t: torch.Tensor, mean: bool) -> None:
        """``t`` summed (``mean``: averaged) over the ranks in place; no collective: untouched"""
        if allreduce is None:
            return
        allreduce(t).wait()
        if mean:
            t.mul_(1.0 / torch.distributed.get_world_size())

    def finish_steps(self) -> None:
        """apply the step step() left deferred, if any"""
        pend, self._pending = self._pending, None
        if pend is not None:
            work, extra = pend
            work.wait()
            self.apply(extra)

    def metrics_tails(self) -> Dict[str, torch.Tensor]:
        """the metrics vector's tails by field name (runtime/metrics_layout.py)"""
        out = {}
        if self.ret_stats is not None:
            out["return_std"] = self.ret_stats.std()
        if self.gate is not None:
            out["gate"] = torch.tensor(list(self.gate[:3]) + [float(self.adam_step)], dtype=torch.float64)
        if self.p.lr_schedule != "constant":
            out["lr"] = torch.tensor(self.lr_state[:3] if self.lr_state is not None else [self.lr], dtype=torch.float64)
        if self.adv_scope:                 # of the raw whole-buffer advantages
            out["adv"] = self.adv_block[[0, 2, 3]]
        return out

    def lr_state_dict(self) -> torch.Tensor:
        return torch.tensor(self.lr_state, dtype=torch.float32)

    def load_lr_state(self, t: torch.Tensor) -> None:
        self.lr_state = [float(x) for x in t.to(torch.float32).tolist()]
        self.lr = self.lr_state[0]

    def last_losses(self) -> Dict[str, float]:
        out = dict(getattr(self, "_last", {}))
        out["grad_norm"] = getattr(self, "_norm", 0.0)
        return out

    def sync(self) -> None:
        pass


def load_ret_acc(engine, d: Dict) -> Dict:
    """the env state without the ``ret_acc`` entry (reward_norm's per-rank carry), which goes into
    the engine; an env state without one, loaded with the flag on, starts the carry at 0 and warns"""
    if "ret_acc" not in d:
        if engine.ret_acc is not None:
            warnings.warn("reward_norm: the env state has no ret_acc; the return scan starts from 0", UserWarning,
                          stacklevel=3)
            engine.ret_acc.zero_()
        return d
    d = dict(d)
    acc = d.pop("ret_acc")
    if engine.ret_acc is not None:
        engine.ret_acc.copy_(acc.to(engine.ret_acc.device, torch.float32))
    return d


def _forward_with(model: ActorCritic, flat: torch.Tensor, x: torch.Tensor):
    saved = model.flat.data
    try:
        model.flat.data = flat
        return model(x)
    finally:
        model.flat.data = saved
