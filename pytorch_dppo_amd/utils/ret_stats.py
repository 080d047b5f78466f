"""Running statistics of the discounted return (``Params.reward_norm``).

One more running moment: :class:`RunningObsStats` with a single column and its own variance floor.
The state ``(n, mean, M2)`` is fp64, global and identical on every rank (the ranks' moments about
the common fp32 shift are summed before the Chan merge); ``scale`` is the fp32 image
``1 / sqrt(max(M2 / n, 1e-8))`` the GAE kernels multiply the reward by.
"""
from __future__ import annotations

from typing import Dict

import torch

from .obs_stats import RunningObsStats

VAR_FLOOR = 1e-8


class RunningReturnStats(RunningObsStats):
    def __init__(self, device="cpu"):
        super().__init__(1, device)

    @property
    def var(self) -> torch.Tensor:
        if self.n <= 0:
            return torch.ones_like(self.mean)          # empty statistics: scale 1
        return torch.clamp(self.mean_diff / self.n, min=VAR_FLOOR)

    def _refresh(self) -> None:
        self.mean_f32.copy_(self.mean.to(torch.float32))
        self.inv_std_f32.copy_((1.0 / torch.sqrt(self.var)).to(torch.float32))

    @property
    def scale(self) -> torch.Tensor:
        """fp32 [1]: what the reward is multiplied by"""
        return self.inv_std_f32

    def std(self) -> torch.Tensor:
        """fp64 [1]: sqrt(M2 / n) (no floor; 0 while empty) — the logged ``return_std``"""
        return torch.sqrt(self.mean_diff / max(self.n, 1.0))

    def state_dict(self) -> Dict[str, torch.Tensor]:
        return {"n": float(self.n), "mean": self.mean.cpu().clone(), "M2": self.mean_diff.cpu().clone()}

    def load_state_dict(self, d: Dict[str, torch.Tensor]) -> None:
        self.n = float(d["n"])
        self.mean.copy_(d["mean"].to(self.device, torch.float64))
        self.mean_diff.copy_(d["M2"].to(self.device, torch.float64))
        self._refresh()
