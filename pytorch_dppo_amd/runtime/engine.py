"""The engine contract: what the worker loop and the launcher ask of ``TorchEngine`` and ``HipEngine``."""
from __future__ import annotations


def check_discrete(params, spec) -> bool:
    """Whether ``spec`` (an ``EnvSpec`` or None) is a discrete-action env, i.e. the policy is categorical
    (docs/ARCHITECTURE.md §27) — after refusing the settings a categorical policy is not built for, each with its
    reason.  Both engines call it when they are built (and the worker before it builds a gym env)."""
    if spec is None or not bool(getattr(spec, "discrete", False)):
        return False
    name = getattr(spec, "name", "?")
    why = None
    if params.loss == "dppo_ref":
        why = "loss=dppo_ref is the reference's per-dimension Gaussian density ratio; a categorical policy has no such density (use loss=ppo)"
    elif params.compat:
        why = "compat reproduces the reference's Gaussian-policy quirks (the variance convention, the shared noise stream)"
    elif params.dtype == "fp8":
        why = "dtype=fp8 gains from the per-head e4m3 update path, which a categorical policy does not take (use fp32, bf16x3 or bf16)"
    elif params.update_kernels == "heads":
        why = "update_kernels=heads: the per-head and 32x32 policy kernels have the Gaussian head; the categorical loss runs on the tile kernel"
    elif params.env_backend == "gym":
        why = "env_backend=gym: the gym adapter steps Box action spaces only (gym Discrete spaces are not supported)"
    if why is not None:
        raise ValueError(f"env {name!r} has discrete actions (a categorical policy): {why}")
    return True


class Engine:
    """One engine owns the device-side state of one DPPO worker: the envs, the ``[T, E]`` rollout buffer, the flat
    parameters / gradient / Adam moments.  ``runtime/worker.py`` and ``runtime/launcher.py`` call exactly this:

    state       T, E; grad_flat, adam_m, adam_v, adam_step; lr (lr_schedule=linear: set by the worker);
                ret_stats (reward_norm); lr_state_dict() / load_lr_state() (lr_schedule=adaptive)
    rollout     rollout([stats_stream]) -> dict; current_obs(); return_moments() / merge_return_moments()
                (reward_norm)
    advantages  values(); gae(); adv_sums(finish) / set_adv_sums(sums, n) (Params.adv_scope())
    update      begin_update(); then per minibatch
                step(idx, extra_grad, allreduce=ctx.grad_allreduce_fn(mean), mean=, last=) -> bool:
                ONE global step — gradient, its sum (mean) over the ranks, Adam; under Params.gated() through the
                KL gate, whose (KL sum, count) pair is summed, never averaged.  True: the host counts one applied
                update; False: none was applied, or the device counts them (the gate field of the metrics vector
                carries the count).  A process-group ``allreduce(t)`` returns an async work handle: the engine
                waits and scales for ``mean``.  A step may stay deferred (overlap_rollout):
    deferred    finish_steps(): every deferred step applied (end of the epochs, behind the next rollout launch
                under overlap_rollout, checkpoints, shutdown);
                quiesce(): the parameters are the synchronous ones, for a snapshot, a checksum or an evaluation
                (default: they are)
    metrics     pack_metrics(ep2, reduce) -> the whole vector in one device buffer (``reduce``: sums ``ep2`` over
                the ranks first), or None: the worker fills it (runtime/metrics_layout.py) from loss_vector()
                (device [loss sums | grad norm], or None: last_losses() has them on the host) and metrics_tails();
                metrics_stream(): the stream the vector is staged on (None: the current one);
                losses_from_vector() where loss_vector() is not None
    other       evaluate(); env_state() / load_env_state(); sync(); params_changed(): the flat parameters were
                written from outside (resume, broadcast); raise_if_failed(sync): a launch failed on the device

    The hooks and attributes only one engine gives a meaning to have their trivial form here."""
    name = "engine"
    ext = None                  # the native extension module (the in-stream communicators are created from it)
    q8 = False                  # fp8 wgrad operands: a gradient-maxima ring travels with the trainer state
    has_stats_stream = False    # rollout(stats_stream=...): the observation moments may be reduced on a side stream

    def raise_if_failed(self, sync: bool = False) -> None:
        pass

    def params_changed(self) -> None:
        pass

    def quiesce(self) -> None:
        pass

    def metrics_stream(self):
        return None

    def pack_metrics(self, ep2, reduce=None):
        return None

    def loss_vector(self):
        return None
