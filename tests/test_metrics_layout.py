"""The metrics vector's layout (runtime/metrics_layout.py): sizes, slices and decode over every feature combination."""
import itertools
import os
import re

import pytest

from pytorch_dppo_amd.config import dppo_preset
from pytorch_dppo_amd.runtime.metrics_layout import LOSS_SLOTS, NPART_FIXED, MetricsLayout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORDER = ("ep", "loss", "return_std", "gate", "lr", "adv")
LR_WIDTH = {"constant": 0, "linear": 1, "adaptive": 3}


def params(reward_norm=False, target_kl=0.0, lr_schedule="constant", adv_scope=False):
    return dppo_preset(env_name="Pendulum-v0", num_envs=4, exploration_size=16, max_iters=2, reward_norm=reward_norm,
                       target_kl=target_kl, lr_schedule=lr_schedule, normalize_adv=True,
                       adv_norm_scope="global" if adv_scope else "rank")


@pytest.mark.parametrize("has_loss", (True, False))
@pytest.mark.parametrize("reward_norm,target_kl,lr_schedule,adv_scope",
                         list(itertools.product((False, True), (0.0, 0.01), tuple(LR_WIDTH), (False, True))))
def test_layout_size_slices_and_decode(reward_norm, target_kl, lr_schedule, adv_scope, has_loss):
    p = params(reward_norm, target_kl, lr_schedule, adv_scope)
    gated = target_kl > 0 or lr_schedule == "adaptive"
    assert p.gated() == gated and bool(p.adv_scope()) == adv_scope
    # the widths as the layout is specified: head 2 + (8 loss sums + grad norm), then the tails
    want = {"ep": 2, "loss": 8 + 1 if has_loss else 0, "return_std": 1 if reward_norm else 0, "gate": 4 if gated else 0,
            "lr": LR_WIDTH[lr_schedule], "adv": 3 if adv_scope else 0}
    lay = MetricsLayout(p, has_loss=has_loss)
    assert lay.size == sum(want.values())
    lo = 0
    for name in ORDER:                      # disjoint, contiguous, in the stated order
        s = lay[name]
        assert (s.start, s.stop, s.step) == (lo, lo + want[name], None), name
        lo = s.stop
    assert lo == lay.size
    v = [100.0 + i for i in range(lay.size)]
    f = lay.decode(v)
    assert tuple(f) == ORDER
    for name in ORDER:
        assert f[name] == (v[lay[name]] if want[name] else None), name
    with pytest.raises(ValueError):
        lay.decode(v + [0.0])


def test_loss_slots_match_the_kernels_enum():
    """LOSS_SLOTS names the slots of the loss row in the order of csrc/kernels.h's LossSlot, and NPART_FIXED is its
    LS_FIXED: the enum is read from the header's text (C rule: an enumerator without a value is its predecessor + 1)."""
    with open(os.path.join(ROOT, "csrc", "kernels.h")) as f:
        m = re.search(r"enum\s+LossSlot\s*\{([^}]*)\}", f.read())
    assert m is not None
    slots, nxt = {}, 0
    for item in m.group(1).split(","):
        e = re.fullmatch(r"\s*(LS_[A-Z]+)\s*(?:=\s*(\d+))?\s*", item)
        assert e is not None, item
        nxt = int(e.group(2)) if e.group(2) is not None else nxt
        slots[e.group(1)] = nxt
        nxt += 1
    assert slots.pop("LS_FIXED") == NPART_FIXED
    assert slots == {"LS_" + name.upper(): i for i, name in enumerate(LOSS_SLOTS)}
    assert list(slots) == ["LS_" + name.upper() for name in LOSS_SLOTS]      # written in that order, too
    assert len(LOSS_SLOTS) <= NPART_FIXED


def test_sizes_the_gpu_tests_pin():
    assert MetricsLayout(params()).size == 11
    assert MetricsLayout(params(lr_schedule="linear")).size == 12
    assert MetricsLayout(params(adv_scope=True)).size == 14
    assert MetricsLayout(params(target_kl=0.01)).size == 15
