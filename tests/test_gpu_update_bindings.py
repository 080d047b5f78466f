"""The three update bindings (csrc/bindings.cpp train_args: ext.mlp_train, ext.mlp_head_train, ext.phead_train)
called through HipEngine._update_args: an illegal argument is refused on the host, before any launch, and a legal
call of each form leaves the gradient the engine's own path leaves."""
import pytest
import torch

from pytorch_dppo_amd.config import dppo_preset
from pytorch_dppo_amd.envs import get_spec, make_vec_env
from pytorch_dppo_amd.models.actor_critic import ActorCritic
from pytorch_dppo_amd.utils.obs_stats import RunningObsStats

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0) if torch.cuda.is_available() else None
# positions in HipEngine._update_args' block
DT, TBUFS, LDT = 0, 2, 20


def _engine(update_kernels):
    from pytorch_dppo_amd.runtime.engine_hip import HipEngine
    p = dppo_preset(device="gpu", env_name="Humanoid-v2", num_envs=64, exploration_size=64 * 4, batch_size=64 * 4,
                    dtype="bf16", update_kernels=update_kernels, ent_coeff=0.01, seed=3)
    spec = get_spec(p.env_name)
    torch.manual_seed(0)
    model = ActorCritic(spec.obs_dim, spec.act_dim, p.hidden).to(DEV)
    env = make_vec_env(spec, p.num_envs, seed=p.seed, device=DEV)
    stats = RunningObsStats(spec.obs_dim, DEV)
    eng = HipEngine(p, model, env, stats, DEV, 0)
    stats.observes(eng.current_obs().to(DEV))
    with torch.no_grad():
        model.flat.data[:model.num_outputs] = -0.3
    eng.params_changed()
    eng.rollout()
    eng.values()
    eng.gae()
    torch.cuda.synchronize()
    return eng


@pytest.fixture(scope="module")
def heads():
    eng = _engine("heads")
    assert eng.heads and eng.phead and not eng.phead_p2 and eng.mb == 256 and eng.ldT == 256
    return eng


def _args(eng, part, idx=None, xt_ready=False, change=()):
    """the engine's argument block for a first step over `part`, with the (position, value) pairs of `change` put in"""
    a = list(eng._update_args(eng.empty if idx is None else idx, True, xt_ready, part))
    for k, v in change:
        a[k] = v
    return a


def _head(eng, h, a, part_dw=None, w8=None, qscale=None, q8_amax=None):
    eng.ext.mlp_head_train(*a, h, eng.part_dw[h] if part_dw is None else part_dw, eng.no_u8 if w8 is None else w8,
                           eng.no_q if qscale is None else qscale, eng.empty if q8_amax is None else q8_amax, 0)


def _short_xT(eng):
    t = list(eng.tbufs)
    t[0] = eng.xT.view(-1)[:-eng.ldT]         # x^T one row of ldT elements short
    return t


CASES = {
    "part_dw_policy": (lambda e: _head(e, 0, _args(e, e.part_h[0]), part_dw=e.part_h[0].shape[1] - 32 * 128 + 4),
                       "part_dw: policy dW_mu block"),
    "part_dw_policy_phead": (lambda e: e.ext.phead_train(*_args(e, e.part_h[0]), 8 + e.A - 1, False),
                             "part_dw: policy dW_mu block"),
    "part_dw_value": (lambda e: _head(e, 1, _args(e, e.part_h[1]), part_dw=e.part_h[1].shape[1] - 128 + 4),
                      "part_dw: value dW_v block"),
    "xt_ready_idx_tile": (lambda e: e.ext.mlp_train(*_args(e, e.part, idx=e.idx_dev, xt_ready=True)),
                          "xT_ready needs a full-batch call"),
    "xt_ready_idx_head": (lambda e: _head(e, 1, _args(e, e.part_h[1], idx=e.idx_dev, xt_ready=True)),
                          "xT_ready needs a full-batch call"),
    "xt_ready_idx_phead": (lambda e: e.ext.phead_train(*_args(e, e.part_h[0], idx=e.idx_dev, xt_ready=True),
                                                       e.part_dw[0], False),
                           "xT_ready needs a full-batch call"),
    "w8_not_bf16": (lambda e: _head(e, 1, _args(e, e.part_h[1], change=[(DT, 3)]), qscale=torch.ones(6, device=DEV),
                                    w8=torch.zeros(e.L.total, dtype=torch.uint8, device=DEV)),
                    "w8: the fp8 mode's per-head bf16 update only"),
    "q8_amax_size": (lambda e: _head(e, 1, _args(e, e.part_h[1]), q8_amax=e.q8_amax[:-1]),
                     "q8_amax has .* elements, kernel needs"),
    "operand_row_short": (lambda e: _head(e, 1, _args(e, e.part_h[1], change=[(TBUFS, _short_xT(e))])),
                          "transposed buffer has .* elements, kernel needs"),
    "ldT_short": (lambda e: _head(e, 1, _args(e, e.part_h[1], change=[(LDT, e.ldT - 32)])),
                  "ldT must cover M padded to the row tile"),
    "ldT_short_tile": (lambda e: e.ext.mlp_train(*_args(e, e.part, change=[(LDT, e.ldT - 32)])),
                       "ldT must cover M padded to the row tile"),
    "phead_partial_row": (lambda e: e.ext.phead_train(*_args(e, e.part_h[0]), e.part_dw[0], True),
                          r"phead: the dW_mu \(and dW_p2\) blocks must fit the partial row"),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_illegal_argument_is_refused_before_the_launch(heads, case):
    call, msg = CASES[case]
    heads.part_h[0].fill_(7.0)
    heads.part_h[1].fill_(7.0)
    heads.part.fill_(7.0)
    with pytest.raises(RuntimeError, match=msg):
        call(heads)
    torch.cuda.synchronize()
    # no kernel ran: an update launch writes its workgroups' partial rows
    assert all(bool((t == 7.0).all()) for t in (heads.part_h[0], heads.part_h[1], heads.part))


def _manual_grad(eng):
    """HipEngine._grad_chain's launches, each binding called here through _update_args"""
    eng.begin_update()
    idx_t, first, xt_ready, xmode = eng._minibatch(None)
    if not eng.heads:
        eng.ext.mlp_train(*eng._update_args(idx_t, first, xt_ready, eng.part))
        b = eng.buckets[0]
        eng._wgrad(b, "fm")
        eng._gather(b, eng.src_off, eng.src_meta, eng.part, eng.ntrain_blk, eng.items["legacy"])
        return
    for h in (0, 1):
        a = eng._update_args(idx_t, first, xt_ready, eng.part_h[h])
        if h == 0:
            eng.ext.phead_train(*a, eng.part_dw[0], eng.phead_p2)
        else:
            _head(eng, 1, a)
        b = eng.buckets[h]
        eng._wgrad(b, xmode)
        eng._gather(b, eng.src_off, eng.src_meta, eng.part_h[h], eng.nhead_blk, eng.items["policy" if h == 0 else "value"],
                    *eng.head_range[h])


@pytest.mark.parametrize("kernels", ["heads", "tile"])
def test_legal_call_of_each_form_leaves_the_engines_gradient(heads, kernels):
    """runs after the refusals above (same module-scoped engine): phead_train + mlp_head_train on the per-head engine,
    mlp_train on a tile engine of the same geometry"""
    eng = heads if kernels == "heads" else _engine("tile")
    assert eng.heads == (kernels == "heads")
    eng.begin_update()
    eng.grad(None)
    ref, ref_loss = eng.grad_flat.clone(), eng.loss_sums.clone()
    assert bool(torch.isfinite(ref).all()) and float(ref.abs().max()) > 0
    eng.grad_flat.zero_()
    eng.loss_sums.zero_()
    _manual_grad(eng)
    torch.cuda.synchronize()
    assert torch.equal(eng.grad_flat, ref) and torch.equal(eng.loss_sums, ref_loss)
