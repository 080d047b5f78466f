"""Pure-PyTorch math: the CPU execution path and the numerical oracle for every HIP kernel.

Each function documents which reference lines it reproduces.  GPU kernels in ``csrc/`` are
tested against these at fp32 (tight) and bf16/fp8 (loose) tolerances.
"""
from __future__ import annotations

import math
from typing import Dict, Optional, Tuple

import torch

from ..utils import rng

LOG_2PI = math.log(2.0 * math.pi)


def sigma_from_log_std(log_std: torch.Tensor, convention: str) -> torch.Tensor:
    """'std': sigma = exp(log_std) (ppo.py:93).  'var': exp(log_std) is sigma^2 (train.py:89)."""
    return torch.exp(log_std) if convention == "std" else torch.exp(0.5 * log_std)


def gaussian_logp(a: torch.Tensor, mu: torch.Tensor, log_std: torch.Tensor,
                  convention: str = "std") -> torch.Tensor:
    """joint diagonal-Gaussian log-density [B,1] (ppo.py:95-97 for 'std')."""
    log_sigma = log_std if convention == "std" else 0.5 * log_std
    z = (a - mu) * torch.exp(-log_sigma)
    return (-0.5 * z * z - 0.5 * LOG_2PI - log_sigma).sum(-1, keepdim=True)


def _check_dist(dist: str) -> bool:
    """True for a categorical head"""
    if dist not in ("gaussian", "categorical"):
        raise ValueError(f"dist must be gaussian|categorical, got {dist!r}")
    return dist == "categorical"


def categorical_logp(onehot: torch.Tensor, logits: torch.Tensor) -> torch.Tensor:
    """log-probability [B,1] of the one-hot rows ``onehot`` [B,K] under softmax(``logits``):
    ``sum_k o_k z_k - lse``, ``lse = m + log sum_k exp(z_k - m)``, ``m = max_k z_k``."""
    m = logits.max(-1, keepdim=True).values
    lse = m + torch.log(torch.exp(logits - m).sum(-1, keepdim=True))
    return (onehot * logits).sum(-1, keepdim=True) - lse


def categorical_entropy(logits: torch.Tensor) -> torch.Tensor:
    """entropy [B] of softmax(``logits``): ``H = lse - sum_k p_k z_k``, summed as ``-sum_k p_k (z_k - lse)``
    (no cancellation between large logits; ``z_k - lse`` and never ``log p_k``: ``p_k`` may underflow to 0)."""
    m = logits.max(-1, keepdim=True).values
    lz = logits - (m + torch.log(torch.exp(logits - m).sum(-1, keepdim=True)))
    return -(torch.exp(lz) * lz).sum(-1)


def categorical_sample(logits: torch.Tensor, key_action: int, env_idx: torch.Tensor, step_key,
                       deterministic: bool = False):
    """Gumbel-max sample of softmax(``logits`` [E,K]), keyed like the Gaussian noise: ``a`` is the lowest ``k``
    attaining ``max_k (z_k + g_k)``, ``g_k = rng.gumbel(key_action, env, step_key, k)``; ``deterministic``:
    ``g = 0``, the arg-max of the logits.  Returns ``(index [E] int64, one-hot [E,K], logp [E])``."""
    K = logits.shape[-1]
    dims = torch.arange(K, device=logits.device, dtype=torch.int64)
    s = logits
    if not deterministic:
        s = logits + rng.gumbel(key_action, env_idx.to(logits.device)[:, None], step_key, dims[None, :])
    top = s == s.max(-1, keepdim=True).values
    a = torch.where(top, dims[None, :], torch.full_like(dims, K)[None, :]).min(-1).values.clamp_max(K - 1)
    onehot = torch.zeros_like(logits).scatter_(-1, a[:, None], 1.0)
    return a, onehot, categorical_logp(onehot, logits).squeeze(-1)


@torch.no_grad()
def policy_act(model, stats, obs: torch.Tensor, key_action: int, env_idx: torch.Tensor, step_key: int,
               convention: str = "std", deterministic: bool = False, dist: str = "gaussian"):
    """One policy step for a batch of observations — the torch twin of ``csrc/act.hip``, the CPU
    path of ``runtime/policy.PolicyRunner`` and the GPU tests' oracle.  The expressions are
    ``TorchEngine.rollout``'s (normalise, policy forward, keyed noise, sample, log-prob), so a rollout
    step and this function agree bit for bit.  ``deterministic``: ``a = mu`` and ``eps = 0``.

    Returns ``(action [E,A], logp [E], mu [E,A], x [E,O])``.  ``dist="categorical"``: the network's outputs are
    the logits of ``A`` actions; returns ``(one-hot [E,A], logp [E], logits [E,A], x [E,O])`` of
    ``categorical_sample`` (``log_std`` is unread)."""
    x = stats.normalize(obs)
    mu, log_std, _ = model(x)
    if _check_dist(dist):
        _, onehot, logp = categorical_sample(mu, key_action, env_idx, step_key, deterministic)
        return onehot, logp, mu, x
    log_sigma = log_std if convention == "std" else 0.5 * log_std
    if deterministic:
        a = mu
        logp = (-log_sigma.sum() - 0.5 * mu.shape[-1] * LOG_2PI).expand(mu.shape[0]).clone()
        return a, logp, mu, x
    sigma = torch.exp(log_sigma)
    dims = torch.arange(mu.shape[-1], device=mu.device, dtype=torch.int64)
    eps = rng.gauss(key_action, env_idx.to(mu.device)[:, None], step_key, dims[None, :])
    a = mu + sigma * eps
    logp = (-0.5 * eps * eps - 0.5 * LOG_2PI - log_sigma).sum(-1)
    return a, logp, mu, x


def gaussian_entropy(log_std: torch.Tensor, convention: str = "std") -> torch.Tensor:
    """analytic entropy sum_j (0.5 + 0.5 log 2pi + log sigma_j) (ppo.py:152-153)."""
    log_sigma = log_std if convention == "std" else 0.5 * log_std
    return (0.5 + 0.5 * LOG_2PI + log_sigma).sum(-1)


def normal_pdf_var(x: torch.Tensor, mu: torch.Tensor, var: torch.Tensor) -> torch.Tensor:
    """per-dim density whose 3rd arg is the VARIANCE (train.py:41-44)."""
    return torch.exp(-(x - mu) ** 2 / (2 * var)) / torch.sqrt(2 * var * math.pi)


def gae(rewards: torch.Tensor, values: torch.Tensor, dones: torch.Tensor, gamma: float,
        lam: float, segment: int = 0, boot: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """GAE(lambda) over a [T,E] rollout (train.py:109-122, ppo.py:119-133, vectorised).

    ``values`` is [T+1,E] (row T = bootstrap V(s_T)); ``dones[t]`` = episode ended at step t
    (so V_{t+1} and A_{t+1} are masked, which is the reference's segment break + R=0).
    ``segment`` > 0 (the reference's ``num_steps``, train.py:82-106 / ppo.py:87): a segment
    ends at a done OR after ``segment`` steps, and the next segment starts fresh (its step count
    restarts after a done).  Where a segment ends by length without a done the recursion
    restarts (A_{t+1} masked) while the bootstrap V_{t+1} of the not-done state is kept
    (train.py:109-112 per segment).
    ``boot`` [T,E] (``bootstrap_time_limit``): the value of the observation a step-limit ("truncated")
    episode end reached before its reset, 0 elsewhere.  It enters ``delta`` only,
    ``delta_t = r_t + gamma * (V_{t+1} * (1 - d_t) + boot_t) - V_t``; the recursion stays cut at the done.
    ``None`` is the function without it, bit for bit.
    Returns (advantages [T,E], returns [T,E]) with returns = A + V.
    """
    T = rewards.shape[0]
    cont = torch.ones_like(rewards)
    if segment > 0:
        # forward: steps since the current segment started, per env (train.py:82 `for step`)
        s = torch.zeros_like(rewards[0], dtype=torch.int64)
        for t in range(T):
            d = dones[t] != 0
            end_len = (s + 1 == segment) & ~d
            cont[t] = torch.where(end_len, torch.zeros_like(cont[t]), cont[t])
            s = torch.where(d | (s + 1 == segment), torch.zeros_like(s), s + 1)
    adv = torch.zeros_like(rewards)
    nxt = torch.zeros_like(rewards[0])
    for t in range(T - 1, -1, -1):
        nonterm = 1.0 - dones[t].to(rewards.dtype)
        if boot is None:
            delta = rewards[t] + gamma * values[t + 1] * nonterm - values[t]
        else:
            delta = rewards[t] + gamma * (values[t + 1] * nonterm + boot[t]) - values[t]
        nxt = delta + gamma * lam * nonterm * cont[t] * nxt
        adv[t] = nxt
    return adv, adv + values[:T]


def return_scan(rewards: torch.Tensor, dones: torch.Tensor, gamma: float, acc: torch.Tensor, shift,
                return_R: bool = False):
    """Forward scan of the discounted return over a [T,E] rollout (``reward_norm``; the
    VecNormalize(norm_reward=True) statistic)::

        R = fl32(fl32(gamma32 * R) + r[t]);  the sample R joins the moments;  R = 0 where done[t]

    from the carry ``acc`` [E] fp32 (two separately rounded fp32 operations: a device twin must not
    contract them into an FMA).  ``shift`` is the fp32 image of the running mean (a float or a
    1-element tensor).  Only dones reset the scan: ``gae``'s segment does not cut it.
    Returns ``(acc', S1, S2)`` — the new carry and, as 0-d fp64 tensors, ``sum(R - shift)`` and
    ``sum((R - shift)^2)`` over the T*E samples — plus the samples ``R`` [T,E] fp32 with ``return_R``."""
    T = rewards.shape[0]
    g32 = torch.tensor(float(gamma), dtype=torch.float32, device=rewards.device)
    sh = float(shift.reshape(-1)[0]) if torch.is_tensor(shift) else float(torch.tensor(shift, dtype=torch.float32))
    R = acc.to(torch.float32).clone()
    out = torch.empty_like(rewards, dtype=torch.float32)
    zero = torch.zeros_like(R)
    for t in range(T):
        R = (g32 * R) + rewards[t].to(torch.float32)
        out[t] = R
        R = torch.where(dones[t] != 0, zero, R)
    d = out.to(torch.float64) - sh
    s1, s2 = d.sum(), (d * d).sum()
    return (R, s1, s2, out) if return_R else (R, s1, s2)


def scale_rewards(rewards: torch.Tensor, scale: torch.Tensor, clip: float) -> torch.Tensor:
    """``reward_norm``'s reward as GAE reads it: ``fl32(r * scale)`` clamped to +-clip (clip <= 0: not)."""
    r = rewards * scale.to(rewards.device, torch.float32).reshape(())
    return r.clamp(-clip, clip) if clip > 0 else r


def ppo_loss(mu, log_std, v, actions, logp_old, adv, ret, v_old, *, clip: float,
             ent_coeff: float, value_loss: str = "mse", convention: str = "std",
             dist: str = "gaussian") -> Dict[str, torch.Tensor]:
    """Corrected PPO loss (ppo.py:148-167).

    ratio = exp(logp - logp_old) with logp_old recorded at rollout; clipped surrogate;
    value loss 'mse' = mean((v-R)^2) (ppo.py:164) or 'clipped_half' =
    0.5*mean(max((v-R)^2, (v_old+clip(v-v_old,+-eps)-R)^2)) (train.py:154-157);
    entropy bonus -ent_coeff * H (ppo.py:167).
    ``dist="categorical"``: ``mu`` holds logits and ``actions`` one-hot rows; logp and the entropy (the batch mean
    of the rows') are the categorical ones, ``log_std`` is unread, everything else is as for the Gaussian head.
    """
    cat = _check_dist(dist)
    adv = adv.reshape(-1, 1)
    ret = ret.reshape(-1, 1)
    logp = categorical_logp(actions, mu) if cat else gaussian_logp(actions, mu, log_std, convention)
    ratio = torch.exp(logp - logp_old.reshape(-1, 1))
    surr1 = ratio * adv
    surr2 = ratio.clamp(1.0 - clip, 1.0 + clip) * adv
    loss_clip = -torch.min(surr1, surr2).mean()
    v = v.reshape(-1, 1)
    if value_loss == "mse":
        loss_value = ((v - ret) ** 2).mean()
    else:
        v_old = v_old.reshape(-1, 1)
        vc = v_old + (v - v_old).clamp(-clip, clip)
        loss_value = 0.5 * torch.max((v - ret) ** 2, (vc - ret) ** 2).mean()
    ent = (categorical_entropy(mu) if cat else gaussian_entropy(log_std, convention)).mean()
    loss_ent = -ent_coeff * ent
    with torch.no_grad():
        lr = (logp - logp_old.reshape(-1, 1))
        approx_kl = ((torch.exp(lr) - 1.0) - lr).mean()
        clipfrac = ((ratio - 1.0).abs() > clip).float().mean()
    return {"loss": loss_clip + loss_value + loss_ent, "loss_clip": loss_clip,
            "loss_value": loss_value, "loss_ent": loss_ent, "approx_kl": approx_kl,
            "clipfrac": clipfrac}


def dppo_ref_loss(mu, log_std, v, mu_old, log_std_old, v_old, actions, adv, ret, *, clip: float,
                  ent_coeff: float) -> Dict[str, torch.Tensor]:
    """The reference DPPO worker loss, verbatim semantics (train.py:142-161).

    sigma_sq = exp(log_std) is used as a VARIANCE; ratio is per action dim
    p/(1e-10+p_old) of the per-dim densities; advantages broadcast over action dims;
    clipped value loss with the same clip eps; entropy term -c*mean(p log(p+1e-5)).
    """
    var = torch.exp(log_std)
    var_old = torch.exp(log_std_old)
    p_old = normal_pdf_var(actions, mu_old, var_old)
    p = normal_pdf_var(actions, mu, var)
    ratio = p / (1e-10 + p_old)
    A = adv.reshape(-1, 1).expand_as(ratio)
    surr1 = ratio * A
    surr2 = ratio.clamp(1.0 - clip, 1.0 + clip) * A
    loss_clip = -torch.min(surr1, surr2).mean()
    v = v.reshape(-1, 1)
    ret = ret.reshape(-1, 1)
    v_old = v_old.reshape(-1, 1)
    vf1 = (v - ret) ** 2
    vc = v_old + (v - v_old).clamp(-clip, clip)
    vf2 = (vc - ret) ** 2
    loss_value = 0.5 * torch.max(vf1, vf2).mean()
    loss_ent = -ent_coeff * (p * torch.log(p + 1e-5)).mean()
    with torch.no_grad():
        clipfrac = ((ratio - 1.0).abs() > clip).float().mean()
    return {"loss": loss_clip + loss_value + loss_ent, "loss_clip": loss_clip,
            "loss_value": loss_value, "loss_ent": loss_ent,
            "approx_kl": torch.zeros((), device=mu.device), "clipfrac": clipfrac}


def clip_grad_norm_(g: torch.Tensor, max_norm: float) -> torch.Tensor:
    """global-norm clip on a flat gradient (nn.utils.clip_grad_norm, ppo.py:173)."""
    norm = torch.linalg.vector_norm(g)
    coef = max_norm / (norm + 1e-6)
    if coef < 1.0:
        g.mul_(coef)
    return norm


def kl_gate(kl_sum, count, target_kl: float, gate) -> Tuple[list, bool]:
    """``target_kl``'s gate after one step of an iteration (the twin of ``csrc/optim.hip`` kl_gate_kernel).

    ``gate`` = ``[stop, applied, trip_kl, last_kl]`` (all 0 at the start of an iteration); ``kl_sum`` /
    ``count`` are slots 3 and 5 of the step's 8 loss sums, summed over the ranks.  The step was applied
    iff ``stop`` was 0 before this call (the caller applies it, or not, by that rule); then::

        kl = fl32(kl_sum / max(count, 1))
        if stop == 0 and not (kl <= target_kl):  stop = 1, trip_kl = kl      # a NaN KL also trips

    so the step whose KL trips the gate is still applied and every later step of the iteration is not
    (CleanRL's rule: the threshold is ``target_kl`` itself); a set ``stop`` stays set.
    Returns ``(new gate as 4 python floats, applied)``; the fp32 roundings are the kernel's."""
    f32 = lambda x: torch.as_tensor(x, dtype=torch.float32).reshape(())   # noqa: E731
    stop, applied_n, trip, _ = (float(f32(x)) for x in gate)
    applied = stop == 0.0
    if applied:
        applied_n = float(f32(applied_n) + 1.0)
    n = f32(count)
    n = n if bool(n > 1.0) else f32(1.0)            # fmaxf(count, 1): a NaN count gives 1
    kl = float(f32(kl_sum) / n)
    if applied and not (kl <= float(f32(target_kl))):
        stop, trip = 1.0, kl
    return [stop, applied_n, trip, kl], applied


def lr_adapt(lr, kl, kl_target: float, factor: float, lr_min: float, lr_max: float) -> float:
    """``lr_schedule=adaptive``: the rate after one APPLIED step whose KL was ``kl`` (the twin of the rate
    block of ``csrc/optim.hip`` kl_gate_kernel; ``kl`` is ``kl_gate``'s ``last_kl``, an fp32 value)::

        if   kl > fl32(2 * kl_target):    lr = max(fl32(lr / factor), lr_min)
        elif kl < fl32(0.5 * kl_target):  lr = min(fl32(lr * factor), lr_max)

    otherwise unchanged; a NaN ``kl`` fails both comparisons.  The caller does not call it for a step
    that was not applied (the gate was already stopped): the parameters did not move, its KL is the
    previous step's, and the rule would compound.  Every operand is rounded to fp32 first, as the
    kernel receives it; returns the new rate as a python float holding an fp32 value."""
    f32 = lambda x: torch.as_tensor(x, dtype=torch.float32).reshape(())   # noqa: E731
    lr, kl, t, fac = f32(lr), f32(kl), f32(kl_target), f32(factor)
    if bool(kl > f32(2.0) * t):
        return float(torch.maximum(lr / fac, f32(lr_min)))
    if bool(kl < f32(0.5) * t):
        return float(torch.minimum(lr * fac, f32(lr_max)))
    return float(lr)


def lr_adapt_dir(kl, kl_target: float) -> int:
    """the branch ``lr_adapt`` takes: -1 down, +1 up, 0 unchanged (the cumulative ``lr_downs`` / ``lr_ups``
    count the branches, a clamped one included)"""
    f32 = lambda x: torch.as_tensor(x, dtype=torch.float32).reshape(())   # noqa: E731
    kl, t = f32(kl), f32(kl_target)
    return -1 if bool(kl > f32(2.0) * t) else (1 if bool(kl < f32(0.5) * t) else 0)


def adv_sums(adv: torch.Tensor, ret: torch.Tensor, idx: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``adv_norm_scope`` global | minibatch: fp64 ``[sum a, sum a^2, sum r, sum r^2]`` over the rows of ``adv`` /
    ``ret`` (the twin of ``csrc/advnorm.hip`` adv_stats_kernel + adv_moments_kernel; the kernels' order of summation
    differs, within fp64 rounding).  With ``idx`` the rows are gathered first, so a duplicated row counts twice."""
    a = adv.reshape(-1).to(torch.float64)
    r = ret.reshape(-1).to(torch.float64)
    if idx is not None:
        i = idx.reshape(-1).to(torch.int64)
        a, r = a[i], r[i]
    return torch.stack([a.sum(), (a * a).sum(), r.sum(), (r * r).sum()])


def adv_block(sums: torch.Tensor, n) -> torch.Tensor:
    """fp32 ``[mean, inv, std, explained_variance]`` of ``n`` advantages (and returns) from their ``adv_sums`` (the
    twin of ``csrc/advnorm.hip`` adv_finish), in fp64 with every operation rounded on its own, rounded to fp32 once::

        mean = S1 / n;  var = max(S2 - S1 * mean, 0) / (n - 1);  std = sqrt(var);  inv = 1 / (std + 1e-8)
        explained_variance = 1 - var / var_ret      (var_ret likewise from S3, S4; NaN when var_ret = 0)

    The variance is the unbiased estimator, as ``torch.std`` uses under scope ``rank``."""
    S1, S2, R1, R2 = (float(x) for x in sums.to(torch.float64).reshape(-1).tolist())
    n = float(n)
    mean = S1 / n
    var = max(S2 - S1 * mean, 0.0) / (n - 1.0)
    std = math.sqrt(var)
    inv = 1.0 / (std + 1e-8)
    rmean = R1 / n
    rvar = max(R2 - R1 * rmean, 0.0) / (n - 1.0)
    ev = 1.0 - var / rvar if rvar > 0.0 else float("nan")
    return torch.tensor([mean, inv, std, ev], dtype=torch.float64).to(torch.float32)


def adv_apply(adv: torch.Tensor, block: torch.Tensor) -> torch.Tensor:
    """the advantage the loss reads under ``adv_norm_scope`` global | minibatch: ``(adv - mean) * inv`` as two
    separately rounded fp32 operations (csrc/common.h adv_norm_apply); ``adv`` itself is left raw"""
    b = block.to(device=adv.device, dtype=torch.float32)
    return (adv.to(torch.float32) - b[0]) * b[1]


def adam_step_(p: torch.Tensor, g: torch.Tensor, m: torch.Tensor, v: torch.Tensor, step: int,
               lr: float, betas=(0.9, 0.999), eps: float = 1e-8) -> None:
    """torch.optim.Adam (default, non-amsgrad, no weight decay) on flat buffers."""
    b1, b2 = betas
    m.mul_(b1).add_(g, alpha=1 - b1)
    v.mul_(b2).addcmul_(g, g, value=1 - b2)
    bc1 = 1 - b1 ** step
    bc2 = 1 - b2 ** step
    denom = (v.sqrt() / math.sqrt(bc2)).add_(eps)
    p.addcdiv_(m, denom, value=-lr / bc1)
