"""The layout of the per-iteration metrics vector: the one fp64 vector an iteration stages into host
memory (``DPPOWorker._stage_metrics``) and the record is built from (``_resolve_metrics``).

Fields, in order; a field that is off has width 0:

    ep          2   [episode return sum, episode count], summed over the ranks
    loss        9   the 8 loss sums (NPART_FIXED) of the last step, then its gradient norm; absent
                    (``has_loss`` false) when the losses come from ``engine.last_losses()`` on the host
    return_std  1   reward_norm
    gate        4   Params.gated(): [stop, applied, trip_kl, steps applied since the start of training]
    lr          1   lr_schedule linear: [lr];  3 under adaptive: [lr, downs, ups]
    adv         3   Params.adv_scope(): [adv_mean, adv_std, explained_variance]

``HipEngine.pack_metrics`` writes ``metrics_buf`` through these slices, the worker's staging path fills a vector
of the same layout from ``engine.metrics_tails()``, and ``decode`` names the fields again.
"""
from __future__ import annotations

NPART_FIXED = 8      # the loss sums of one update step (csrc/kernels.h LS_FIXED: the fixed slots of a loss partial)
# the used slots by name, in the order of csrc/kernels.h LossSlot (LS_CLIP .. LS_COUNT); the rest stay 0
LOSS_SLOTS = ("clip", "value", "ent", "kl", "clipfrac", "count")


class MetricsLayout:
    def __init__(self, params, has_loss: bool = True):
        widths = (("ep", 2),
                  ("loss", NPART_FIXED + 1 if has_loss else 0),
                  ("return_std", 1 if params.reward_norm else 0),
                  ("gate", 4 if params.gated() else 0),
                  ("lr", {"constant": 0, "linear": 1, "adaptive": 3}[params.lr_schedule]),
                  ("adv", 3 if params.adv_scope() else 0))
        self._slices = {}
        lo = 0
        for name, w in widths:
            self._slices[name] = slice(lo, lo + w)
            lo += w
        self.size = lo

    def __getitem__(self, name: str) -> slice:
        """the slots of field ``name`` (empty when the field is off)"""
        return self._slices[name]

    def decode(self, v) -> dict:
        """field name -> its values out of a vector of this layout (None: the field is off)"""
        if len(v) != self.size:
            raise ValueError(f"metrics vector has {len(v)} slots, the layout {self.size}")
        return {name: (list(v[s]) if s.stop > s.start else None) for name, s in self._slices.items()}
