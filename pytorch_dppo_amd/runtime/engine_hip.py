"""HIP engine: the MI355X execution path of one DPPO worker (one process per GPU).

Per iteration (all device work on the current HIP stream, no host sync until the end):

  rollout   1 launch  csrc/rollout.hip   T env steps of E envs fused (norm, policy MFMA, sample,
                                         log-prob, env physics) -> [T][E] buffer in HBM
  values    1 launch  csrc/mlp.hip       V(s) for all (T+1)*E rows (value head on MFMA)
  gae       1 launch  csrc/optim.hip     one lane per env reverse scan
  per minibatch (= one synchronous global step, train.py:133-175 / chief.py:13-20), step():
    split-bf16 + the reference network (the headline): the two heads are independent chains,
      per head  mlp_head (fwd+loss+dgrad, csrc/mlp_head.hip) -> wgrad (its layers) -> gather+Adam
      world size > 1: gather -> async RCCL all-reduce of the head's flat range -> Adam, with each
      head's all-reduce in flight while the other head's kernels run (policy step e's beside
      value step e's kernels, value step e's beside policy step e+1's)
    otherwise: mlp_train (both heads) -> wgrad -> grad_gather [-> all-reduce] -> Adam
    with clipping (ppo preset): gathers -> all-reduce -> sumsq + Adam over the whole vector

The packed weight images (PackedLayout) hold every layer as [d_out][d_in] and its transpose
in the MFMA operand precision (fp32 / bf16), the bias folded into column K.
"""
from __future__ import annotations

import contextlib
import math
from typing import Dict, Optional

import torch

from ..config import Params
from ..envs.registry import KIND_PENDULUM, KIND_SYNTHETIC, kernel_kind_of
from ..models.actor_critic import ActorCritic, PackedLayout, fm_index
from ..ops import native, storage
from ..utils import rng
from ..utils.obs_stats import RunningObsStats
from ..utils.ret_stats import VAR_FLOOR as RET_VAR_FLOOR, RunningReturnStats
from .engine import Engine, check_discrete
from .engine_torch import load_ret_acc
from .metrics_layout import LOSS_SLOTS, NPART_FIXED, MetricsLayout

# the loss row's slots (csrc/kernels.h LossSlot) as indices, for losses_from_vector
_LS_CLIP, _LS_VALUE, _LS_ENT, _LS_KL, _LS_CLIPFRAC, _LS_COUNT = (
    LOSS_SLOTS.index(k) for k in ("clip", "value", "ent", "kl", "clipfrac", "count"))

STORAGE = storage.STORAGE
Q8_SX, Q8_SH = 64.0, 256.0   # fixed e4m3 operand scales of the observations / tanh activations (csrc/common.h)
Q8_SUB = 64                  # sub-slots per tensor of the gradient-amax ring (csrc/kernels.h)
WT = 128            # operand-buffer row padding (csrc/kernels.h WGRAD_TILE)


def wgrad_tile_ok(nq: int, kq: int, wide: bool = False) -> bool:
    """the quadrant tiles the wgrad kernel runs (csrc/wgrad.hip wgrad_task_ok): one quadrant per wave
    of the 8-wave workgroup (nq*kq <= 8, nq + kq <= 6: 24 fragment slots per ring stage), or with
    ``wide`` (split-bf16 / bf16) two per wave (9-16 quadrants, nq even, nq + kq <= 10: 40 slots)"""
    if nq < 1 or kq < 1:
        return False
    if nq * kq <= 8:
        return nq + kq <= 6
    return wide and nq * kq <= 16 and nq % 2 == 0 and nq + kq <= 10


def wgrad_tiles(li: int, n: int, k: int, wide: bool = False):
    """Output tiles of one layer's weight gradient ([n][k], k including the bias column) for the
    wgrad kernel: (layer, n0, k0, nq, kq), a tile = nq x kq quadrants of 64x64 (wgrad_tile_ok).  The
    kernel streams (nq + kq) * 64 operand rows per 32-row k-step, so the (nq, kq) minimising the
    layer's total rows read wins (ties: fewer tasks, then wider n).  Humanoid v_fc1 (512 x 377):
    4x2 tiles, 2304 rows per step instead of 3072 with 128x128 tiles; ``wide``: 4x4 + 4x2 tiles,
    1792 rows per step."""
    N, K = -(-n // 64), -(-k // 64)
    best = None
    for nq in range(1, 17):
        for kq in range(1, 17):
            if nq > N or kq > K or not wgrad_tile_ok(nq, kq, wide):
                continue
            tl = []
            for a in range(0, N, nq):
                for b in range(0, K, kq):
                    tl.append((li, a * 64, b * 64, min(nq, N - a), min(kq, K - b)))
            if not all(wgrad_tile_ok(t[3], t[4], wide) for t in tl):
                continue
            cost = sum(t[3] + t[4] for t in tl)
            key = (cost, len(tl), -nq)
            if best is None or key < best[0]:
                best = (key, tl)
    return best[1]


ROLL_ROWS = 16
WGRAD_TARGET_WGS = 0     # wgrad tasks per launch; 0: one per CU of the device (256 on MI355X)


def _r(x: int, m: int) -> int:
    return (x + m - 1) // m * m


class HipEngine(Engine):
    name = "hip"
    has_stats_stream = True

    def __init__(self, params: Params, model: ActorCritic, env, stats: RunningObsStats,
                 device: torch.device, action_rank: int):
        if device.type != "cuda":
            raise RuntimeError("HipEngine needs a HIP device")
        self.ext = native.load()
        self.p = params
        self.model = model
        self.env = env
        self.stats = stats
        self.device = device
        # a discrete env (docs/ARCHITECTURE.md §27): the policy's A outputs are logits of a categorical distribution,
        # `actions` holds one-hot rows, the env takes indices; act launches with dist 1, the update on the tile
        # kernel with loss_kind 2 (the per-head and 32x32 policy kernels have the Gaussian head)
        self.discrete = check_discrete(params, getattr(env, "spec", None))
        # dtype fp8 (BASELINE config 5): the forward GEMMs of the rollout policy and of the value
        # pass run on the OCP e4m3 MFMA (v_mfma_f32_16x16x32_fp8_fp8) with per-layer weight
        # scales; on the per-head path the value head's fc1 in the update and every weight-gradient
        # GEMM (e4m3 operands with power-of-two scales, delayed per-tensor for the gradients: self.q8)
        # too; the loss, dgrad and the rest of the update run in bf16.  fp32 / bf16 use one
        # precision throughout.
        self.fp8 = params.dtype == "fp8"
        self.dt = native.DT_CODE["bf16"] if self.fp8 else native.DT_CODE[params.dtype]
        self.dt_fwd = native.DT_CODE[params.dtype]
        self.sdtype = STORAGE[self.dt]
        T, E, O, A = params.rollout_len, env.E, env.O, env.A
        self.T, self.E, self.O, self.A = T, E, O, A
        self.N = T * E
        L = model.packed_layout()
        self.L = L
        ls = L.layers
        self.layout = ([L.w_off[l.name] for l in ls] + [L.wt_off[l.name] for l in ls] +
                       [l.d_in for l in ls] + [l.d_out for l in ls] + [l.fan_out for l in ls])
        self.scales = [1.0] * 6
        dev = dict(device=device)
        f32 = dict(device=device, dtype=torch.float32)
        self.w_map = L.flat_to_w.to(device)
        self.wt_map = L.flat_to_wt.to(device)
        self.wimg = torch.zeros(L.total, dtype=self.sdtype, **dev)
        self.qscale = torch.empty(0, **f32)
        if self.fp8:
            self.wimg_fwd = torch.zeros(L.total, dtype=torch.uint8, **dev)
            self.qscale = torch.ones(6, **f32)
            # layer id of every flat parameter (-1: log_std) for the per-layer amax
            lid = torch.full((model.num_params,), -1, dtype=torch.int64)
            for li, l in enumerate(ls):
                for suffix in ("weight", "bias"):
                    o, n_ = model.offsets[f"{l.name}.{suffix}"]
                    lid[o:o + n_] = li
            # the device refresh indexes qscale[lid]: validate the static map once here
            assert bool(((lid >= 0) == (L.flat_to_w >= 0)).all()) and int(lid.max()) < 6
            self.layer_id = lid.to(torch.int32).to(device)
            self.fp8_part = torch.zeros(128 * 6, **f32)   # per-block layer maxima (fp8_amax_kernel)
        else:
            self.wimg_fwd = self.wimg
        self.d0 = ls[0].d_in
        self.x_buf = torch.zeros((T + 1) * E, self.d0, dtype=self.sdtype, **dev)
        self.actions = torch.zeros(self.N, A, **f32)
        self.logp = torch.zeros(self.N, **f32)
        self.rewards = torch.zeros(self.N, **f32)
        self.dones = torch.zeros(self.N, **f32)
        self.values_buf = torch.zeros((T + 1) * E, **f32)
        self.adv = torch.zeros(self.N, **f32)
        self.ret = torch.zeros(self.N, **f32)
        self.mu_prev = torch.zeros(self.N, A, **f32)
        self.v_prev = torch.zeros(self.N, **f32)
        self.log_std_old = torch.zeros(A, **f32)
        nroll = (E + ROLL_ROWS - 1) // ROLL_ROWS
        self.mom = torch.zeros(nroll, 2, O, **f32)
        self.epstat = torch.zeros(nroll, 2, **f32)
        self.ep_sum = torch.zeros(2, dtype=torch.float64, device=device)
        self._step_bufs = None     # per-step obs-norm mode: the steps' rollout moments / episode stats
        self._sn_cap = None        # per-step obs-norm launch: co-resident grid cap of this device
        self._sn_bufs = None       # its granule buffers, timeout word (+ pinned copy)
        self._sn_epoch = 1         # its next granule tag (never reused)
        self._obs_scratch = None   # obs_observe partials + fp64 sums
        self._eval_bufs: Dict[int, tuple] = {}   # evaluate(): (ret, len) outputs per env count
        self._act_bufs: Dict[int, tuple] = {}    # act(): (action, logp, mu) outputs per row count
        self._eval_act_bufs: Dict[int, torch.Tensor] = {}   # evaluate() of a device-stepped env: its action rows
        # ---- update geometry ----
        self.mb = params.minibatch_rows()
        # per-head streaming kernels (csrc/mlp_head.hip, 128 rows per workgroup): split-bf16 and
        # the reference network, at minibatches of at least one full round of 128-row workgroups
        # (one per CU): below that the two-head tile kernel's smaller workgroups fill the chip better
        # (measured, 16,384 rows: 0.716 vs 0.836 ms per iteration at bf16, 1.61 vs 1.71 at bf16x3;
        # 65,536 rows: 4.2 vs 4.9 ms at bf16x3).  Params.update_kernels heads / tile force one path.
        mode = params.update_kernels
        ncu = (torch.cuda.get_device_properties(device).multi_processor_count if device.type == "cuda" else 256)
        self.heads = (mode != "tile" and not self.discrete and bool(self.ext.head_applies(self.dt, self.layout, A))
                      and (mode == "heads" or params.minibatch_rows() >= 128 * ncu))
        # fp8 mode on the per-head path: the wgrad operands (x^T, h1^T, g1^T, g2^T of both heads)
        # are e4m3 bytes with power-of-two scales — fixed for the activations, delayed per-tensor
        # for the gradients (csrc/common.h Q8) — and the wgrad runs on the e4m3 MFMA: half the
        # operand bytes of the bf16 update's HBM round trip.  fp8_wgrad_operands=False: bf16 operands.
        self.q8 = self.fp8 and self.heads and bool(params.fp8_wgrad_operands)
        # (the value head's update stays on the 16x16 head kernel: its 32x32 one-wave-per-SIMD form
        # measured slower at every step, docs/ARCHITECTURE.md §13)
        # the policy head's update on the transposed-chain kernel too (csrc/phead.hip): h1p / g1p /
        # g2p row-major, and the observation operand of p_fc1 AND v_fc1 row-major — x_buf itself
        # for a full-batch step (no x^T anywhere: the rollout skips writing it), the kernel's
        # gathered rows in xT for a minibatch
        self.phead = (self.heads and not self.fp8 and bool(params.phead_kernel)
                      and bool(self.ext.phead_train_applies(self.dt, self.layout, A)))
        # ... summing p_fc2's weight gradient itself at bf16x3 (h1p / g2p never reach HBM: 4.26 ->
        # 4.15 ms per iteration); at bf16 their round trip is half the bytes and storing them for
        # the wgrad is faster (2.27 vs 2.36 ms; same box, profiles/r5/ab_p2_by_dtype.log)
        fused = params.phead_fused_dw2
        self.phead_p2 = self.phead and (fused == "on" or (fused == "auto" and self.dt == native.DT_CODE["bf16x3"]))
        # the gradient-amax ring: 3 slots x 4 tensors x 64 sub-slot lines of 32 dwords (csrc/kernels.h)
        self.q8_amax = torch.zeros(3 * 4 * Q8_SUB * 32, dtype=torch.int32, device=device)
        self._q8_next = 0          # step counter of the amax ring
        self._q8_step = 0
        self._q8_cal = [False, False]   # per head: the calibration pass ran
        # operand rows: a multiple of the update kernel's row tile (every row it writes has a
        # column) and of 64 (wgrad consumes k-steps in pairs, csrc/wgrad.hip)
        self.ldT = _r(self.mb, 128 if self.heads else 64)
        self.npart = NPART_FIXED + A
        # per-workgroup partials, sized for the smallest row tile (16) so a tile change
        # (set_mlp_rows, A/B diagnostics) never outgrows it
        self.part = torch.zeros(self.ldT // 16, self.npart, **f32)
        # per-head partial rows (one per 128-row workgroup): policy [8 loss terms | A dlog_std],
        # value [8 loss terms]; the loss columns each head's gather owns
        # policy [loss terms (its columns) | A dlog_std | pad | dW_mu [32][128]], value [loss
        # column 1 | .. | dW_v [128]] — the narrow output layers' weight gradients are summed in
        # the head kernels (csrc/mlp_head.hip) instead of streaming two more operand pairs through
        # the wgrad
        self.nhead_blk = self.ldT // 128
        self.part_dw = [_r(8 + A, 4), 8]
        # (the 32x32 policy head at bf16x3 also sums p_fc2's weight gradient [128][128] right after
        # dW_mu: p_fc2 leaves the wgrad, and h1p / g2p their HBM round trip)
        np_pol = self.part_dw[0] + 32 * 128 + (128 * 128 if self.phead_p2 else 0)
        nv_val = 128
        self.part_h = [torch.zeros(self.nhead_blk, np_pol, **f32), torch.zeros(self.nhead_blk, 8 + nv_val, **f32)]
        # world size 1: both head kernels write ONE partial buffer (policy its columns, value
        # column 1 and its dW_v after the policy's block) and one wgrad + gather/Adam launch
        # covers both heads (the observation^T operand is streamed once for p_fc1 and v_fc1)
        self.part_joint = torch.zeros(self.nhead_blk, np_pol + nv_val, **f32)
        self.part_dw_joint = [self.part_dw[0], np_pol]
        self.head_range = [model.head_ranges["policy"], model.head_ranges["value"]]
        self.head_order = (0, 1)     # launch order of the joint head kernels (A/B: scripts/ab_iter.py)
        if params.mlp_rows:                     # diagnostics: force the fused-kernel row tile
            self.ext.set_mlp_rows(int(params.mlp_rows))
        self.sync_tile()
        # transposed operand buffers (feature-major), heights padded to the wgrad tile
        lp1, lp2, lmu, lv1, lv2, lv = ls
        x_rows = [lp1.d_in, lp2.d_in, lmu.d_in, lv1.d_in, lv2.d_in, lv.d_in]
        g_rows = [lp1.fan_out, lp2.fan_out, lmu.fan_out, lv1.fan_out, lv2.fan_out, lv.fan_out]
        self.x_rows = [_r(r, WT) for r in x_rows]
        self.g_rows = [_r(r, WT) for r in g_rows]
        opd = torch.uint8 if self.q8 else self.sdtype
        mk = lambda rows: torch.zeros(rows, self.ldT, dtype=opd, **dev)
        self.xT = mk(self.x_rows[0])                       # shared by p_fc1 and v_fc1
        self.h1pT, self.h2pT = mk(self.x_rows[1]), mk(self.x_rows[2])
        self.h1vT, self.h2vT = mk(self.x_rows[4]), mk(self.x_rows[5])
        self.g1pT, self.g2pT, self.g3pT = mk(self.g_rows[0]), mk(self.g_rows[1]), mk(self.g_rows[2])
        self.g1vT, self.g2vT, self.g3vT = mk(self.g_rows[3]), mk(self.g_rows[4]), mk(self.g_rows[5])
        self.tbufs = [self.xT, self.h1pT, self.h2pT, self.h1vT, self.h2vT,
                      self.g1pT, self.g2pT, self.g3pT, self.g1vT, self.g2vT, self.g3vT]
        self.wg_g = [self.g1pT, self.g2pT, self.g3pT, self.g1vT, self.g2vT, self.g3vT]
        self.wg_x = [self.xT, self.h1pT, self.h2pT, self.xT, self.h1vT, self.h2vT]
        # constant bias rows of the hidden-activation operands (the kernel writes rows < n_out;
        # row n_out == 1 makes the wgrad GEMM emit the bias gradient as column K).  The operand
        # buffers are fragment-major, so "row r" is a scattered index set.
        cols = torch.arange(self.ldT, device=device)
        # (row-major h1v / h1p: the t32 kernels write their bias columns themselves)
        bias_rows = [(self.h2pT, lp2.fan_out), (self.h2vT, lv2.fan_out), (self.h1vT, lv1.fan_out)]
        if not self.phead:
            bias_rows.append((self.h1pT, lp1.fan_out))
        # wgrad operand layout flags (dY side of the 6 layers, then X side; 1 row-major [ldT][features]):
        # under the 32x32 policy head p_fc1's / p_fc2's dY (g1p, g2p), p_fc2's X (h1p) and the
        # observation operand of both fc1 layers
        self.rm = [0] * 12
        self.wg_x_full = self.wg_x
        if self.phead:
            self.rm[0] = self.rm[1] = self.rm[6 + 0] = self.rm[6 + 1] = self.rm[6 + 3] = 1
            assert self.x_rows[0] == self.d0, "row-major observation operand: x_buf rows are d0 wide"
            # a full-batch step reads the observation rows straight from x_buf (rows [0, ldT) of
            # its N + E rows)
            if self.ldT <= self.x_buf.shape[0]:
                xb = self.x_buf.view(-1)
                self.wg_x_full = [xb, self.h1pT, self.h2pT, xb, self.h1vT, self.h2vT]
        # X side of p_fc1 / v_fc1 per step under the 32x32 policy head: "fm" = the rollout's
        # fragment-major x^T (full batch), "buf" = x_buf's rows (full batch without it), "mb" = the
        # rows the policy kernel gathered into xT (minibatch); rm_xfm = the flags of "fm"
        self.rm_xfm = list(self.rm)
        self.rm_xfm[6 + 0] = self.rm_xfm[6 + 3] = 0
        self._x_mode = "fm"
        for buf, r in bias_rows:
            if self.q8:       # e4m3 bytes of the activation scale (Q8_SH = 256: exact)
                storage.set_elements(buf, fm_index(torch.full_like(cols, r), cols, self.ldT), Q8_SH, 2)
            else:
                storage.set_elements(buf, fm_index(torch.full_like(cols, r), cols, self.ldT), 1.0, self.dt)
        # wgrad tiles of up to 16 quadrants, two per wave (csrc/wgrad.hip; split-bf16 / bf16 operands):
        # fewer operand rows streamed per output (v_fc1 1792 instead of 2304 rows per k-step), more
        # slab chunks for the gather; per iteration −0.4 % at bf16x3, −2 % at bf16 (same process,
        # profiles/r6/ab_heads_wide_*.log).  Restricting it to the fc1 layers was slower than both.
        self.wgrad_wide = bool(params.wgrad_wide) and self.dt in (native.DT_CODE["bf16x3"], native.DT_CODE["bf16"]) \
            and not self.q8
        self._build_wgrad_plan(model)
        if self.heads:
            # the joint (one-bucket) plan of world size 1 beside the per-head buckets
            heads_buckets, heads_src = self.buckets, (self.src_off, self.src_meta)
            self._build_wgrad_plan(model, joint=True)
            self.joint_bucket, self.joint_src = self.buckets[0], (self.src_off, self.src_meta)
            self.buckets, (self.src_off, self.src_meta) = heads_buckets, heads_src
        self.items = self._reduce_items(model)
        # ---- optimizer state ----
        n = model.num_params
        # target_kl (docs/ARCHITECTURE.md §22): gate = [stop, applied, trip_kl, last_kl], written by the
        # kl_gate launch that ends every step; the 8 loss sums sit behind the gradient in one allocation
        # so that a gated step's one collective sums both over the ranks.  Only with the flag on.
        self.gate: Optional[torch.Tensor] = None
        self._grad_sums: Optional[torch.Tensor] = None
        # lr_schedule (§23): lr is the host rate of the Adam launches (linear: the worker sets it once per
        # iteration, before begin_update()).  adaptive: the rate lives in lr_state = [lr, downs, ups,
        # reserved], read by the gated Adam launches and written by the kl_gate launch alone — the steps
        # take _gated_step whether or not target_kl is set.  Allocated only under adaptive.
        self.lr = float(params.lr)
        self.lr_state: Optional[torch.Tensor] = None
        self._rate_block: tuple = ()         # kl_gate's trailing operands
        if params.lr_schedule == "adaptive":
            self.lr_state = torch.tensor([self.lr, 0.0, 0.0, 0.0], **f32)
            self._rate_block = (self.lr_state, float(params.lr_kl_target), float(params.lr_adapt_factor),
                                float(params.lr_min), float(params.lr_max))
        self._gate_target = float(params.gate_target())
        if params.gated():
            self.gate = torch.zeros(4, **f32)
            self._grad_sums = torch.zeros(n + NPART_FIXED, **f32)
            self.grad_flat = self._grad_sums[:n]
        else:
            self.grad_flat = torch.zeros(n, **f32)
        self.adam_m = torch.zeros(n, **f32)
        self.adam_v = torch.zeros(n, **f32)
        self.adam_state = torch.zeros(4, **f32)
        self.adam_step = 0
        # per-block gradient sums of squares of whichever Adam path ran; the fused gather+Adam
        # launch uses one block per entry: A + 8 reduction blocks plus one per 256 elements
        # launch (one element per thread: a grid-stride second pass would double the load latency
        # chain of the blocks that take it) needs A + 8 reduction blocks plus one per 256 elements
        n_whole = min(4096, (n - self.A + 255) // 256 + self.A + 8)
        # (the fused gather + Adam launch takes one block per 32 reduce items first: with the fused
        # narrow / second-layer weight gradients there are tens of thousands of items)
        # (blocks of 32 items, csrc/kernels.h ITEM_IPB; blocks of 8 measured no faster, profiles/r6/ab_iter_phead_kb_vs_plain_ipb8_*.log)
        n_elem = min(4096, max(n_whole, -(-len(self.items.get("joint", self.items["legacy"])[0]) // 32) + (n + 255) // 256))
        # the streaming form (docs/ARCHITECTURE.md §26) takes one QUAD per thread behind the reduce blocks; n_elem
        # stays the per-element form's grid (ext.set_gather_stream(0), scripts/ab_iter.py arm "elem")
        fb = self.joint_bucket if self.heads else self.buckets[0]
        fused_items = self.items["joint" if self.heads else "legacy"][0]
        n_whole = min(4096, -(-len(fused_items) // 32) + (fb["nquads"] + 255) // 256) if self._tiles(fb) else n_elem
        self.norm_n_elem = n_elem
        # per-head regions (fixed: every head launch writes each block of its region): policy
        # [0, np_), value [np_, np_ + nv_)
        (plo, phi), (vlo, vhi) = self.head_range
        np_ = min(4096, self.A + 8 + (phi - self.A + 255) // 256)
        nv_ = min(4096, 8 + (vhi - vlo + 255) // 256)
        self.norm_regions = [(0, np_), (np_, np_ + nv_)]
        self.norm_part = torch.zeros(max(n_whole, n_elem, np_ + nv_), **f32)
        self.norm_n_whole = n_whole
        self._norm_n = n_whole       # entries the last Adam path wrote (metrics_pack sums them)
        # a value-head step not yet applied: ("work", all-reduce work, step, mean) on the
        # process-group chains, or ("side", None, step, mean) when it runs on the side stream
        self._pending_value = None
        self._side: Optional[torch.cuda.Stream] = None   # the side stream of the overlapped value step
        self.side_steps = 0          # value steps run on the side stream (bench / tests report it)
        self.pending_steps = 0       # value steps left pending on a process-group all-reduce
        # world-size-1 fast path: grad_gather + no-clip Adam in one launch (fused_apply=False: off)
        self.fused_apply = bool(params.fused_apply)
        mgn = params.max_grad_norm
        self.max_norm = float(mgn) if (mgn is not None and mgn > 0) else 0.0    # the global-norm clip (0.0: off)
        self.idx_dev = torch.zeros(self.ldT, dtype=torch.int32, **dev)
        self.key_action = rng.base_key(params.seed, rng.STREAM_ACTION, action_rank)
        self.std_var = 1 if params.std_convention == "var" else 0   # the policy launches' log_std flag
        self.empty = torch.empty(0, dtype=torch.int32, **dev)
        self.no_q = torch.empty(0, **f32)
        self._gate_arg = self.no_q if self.gate is None else self.gate    # the Adam bindings' gate (empty: ungated)
        self._lr_arg = self.no_q if self.lr_state is None else self.lr_state    # ... and lr_dev (empty: the host rate)
        self.no_u8 = torch.empty(0, dtype=torch.uint8, **dev)
        self._first_step = True
        self._loss_dev: Optional[torch.Tensor] = None
        self.local_stats: Optional[RunningObsStats] = None
        self.loss_sums = torch.zeros(NPART_FIXED, **f32) if self.gate is None else self._grad_sums[n:]
        # the iteration's metrics vector (pack_metrics), allocated once
        self.metrics_layout = MetricsLayout(params)
        self.metrics_buf = torch.zeros(self.metrics_layout.size, dtype=torch.float64, **dev)
        self.empty_x = torch.empty(0, dtype=self.sdtype, **dev)
        self.x_raw: Optional[torch.Tensor] = None   # compat Q8: raw bootstrap rows (values())
        # the rollout can emit the full-batch x^T operand when the update is one full-batch step
        # (Q8: the policy kernel writes the e4m3 x^T in the first full-batch step instead)
        self.xT_from_rollout = (self.mb == self.N and self.ldT == self.N and E % 16 == 0 and self.N % 32 == 0
                                and params.obs_norm_update == "rollout" and not self.q8
                                and not (self.phead and self.wg_x_full is not self.wg_x))
        self._xT_valid = False   # True once a rollout wrote x^T for the current buffer contents
        self.s12 = torch.zeros(2, O, dtype=torch.float64, **dev)
        stats.device_merge = self._device_merge
        # host-stepped env (--env-backend gym): no in-kernel dynamics; rollout() takes the host
        # path (_rollout_host) and the update runs on the HIP kernels as usual
        self.host_env = bool(getattr(env, "host_stepped", False))
        # a builtin (tensor) env of a kind the rollout / eval kernels do not run — a registered tensor
        # env (envs.register_tensor_env): rollout() and evaluate() step it on the device instead
        # (rollout_stepped: per step one act launch, the env's own torch ops, one env_advance launch)
        # params.env_fused: an env whose class has an in-kernel twin (VecEnv.kernel_kind: the cart-pole)
        # runs inside the rollout / eval kernels as that kind instead; an env without one is refused
        # here, not stepped quietly (kernel_kind_of raises, naming it).  rollout_stepped() keeps
        # working on such an env: it is the second reference of the fused cart-pole's tests.
        self.kernel_kind: Optional[int] = None      # the kind the kernels are launched with (None: none)
        if self.host_env:
            if bool(getattr(params, "env_fused", False)):
                raise ValueError("env_fused runs a builtin env inside the rollout kernel; a host-stepped (gym) env "
                                 "has no in-kernel dynamics")
        elif env.kind in (KIND_SYNTHETIC, KIND_PENDULUM):
            self.kernel_kind = int(env.kind)
        elif bool(getattr(params, "env_fused", False)):
            self.kernel_kind = kernel_kind_of(env)
        self.stepped_env = not self.host_env and self.kernel_kind is None
        # a discrete env whose class has a kernel kind (CartPole-v0): the fused kernels run it with the categorical
        # head (RolloutArgs / EvalArgs dist 1, docs/ARCHITECTURE.md §29); their check_env refuses what has no such form
        self.kernel_dist = 1 if self.discrete and not self.stepped_env else 0
        if self.kernel_dist and params.obs_norm_update == "step":
            raise ValueError(f"env {env.spec.name!r} with env_fused and obs_norm_update=step: the categorical head is "
                             "not built into the per-step observation filter's launch forms (the register-tight "
                             "4-wave forms of the rollout kernel); use obs_norm_update=rollout, or run it "
                             "device-stepped (without env_fused)")
        # bootstrap_time_limit: which steps ended by the step limit alone (trunc, like dones), the
        # normalised observation each reached before its reset (x_fin [K][E][d0] in x_buf's storage:
        # slot t // limit, an env's truncations being >= limit steps apart) and its value.  Transient:
        # rewritten by every rollout, never checkpointed.  Allocated only with the flag on.
        self.boot = bool(getattr(params, "bootstrap_time_limit", False))
        if self.boot:
            if self.host_env:
                raise ValueError("bootstrap_time_limit needs the final observation of a truncated step; a "
                                 "host-stepped (gym) env auto-resets on the host")
            self.fin_K = -(-T // int(env.limit))
            self.trunc = torch.zeros(self.N, **f32)
            self.x_fin = torch.zeros(self.fin_K * E, self.d0, dtype=self.sdtype, **dev)
            self.v_fin = torch.zeros(self.fin_K * E, **f32)
            self.boot_buf = torch.zeros(self.N, **f32)
            self._fin_rows = torch.zeros(E, self.d0, dtype=self.sdtype, **dev)   # rollout_stepped's scratch rows
            self._fin_slot = None
        # reward_norm: the carry of the discounted-return scan (per rank, checkpointed with the env),
        # the running statistics of the return (global; merged by csrc/obs.hip obs_merge with O = 1),
        # the scan's (S1, S2) and per-workgroup scratch (csrc/retnorm.hip).  Allocated only with the flag on.
        self.ret_stats: Optional[RunningReturnStats] = None
        self.ret_acc: Optional[torch.Tensor] = None
        if bool(getattr(params, "reward_norm", False)):
            self.ret_stats = RunningReturnStats(device)
            self.ret_stats.device_merge = self._ret_device_merge
            self.ret_acc = torch.zeros(E, **f32)
            self.ret_s12 = torch.zeros(2, dtype=torch.float64, **dev)
            self.ret_part = torch.zeros(2 * int(self.ext.ret_scan_nblk(T, E, 0)), dtype=torch.float64, **dev)
        # adv_norm_scope global | minibatch (docs/ARCHITECTURE.md §24): adv stays raw and the policy kernels apply
        # [mean, inv] at their advantage load.  adv_blocks = [the whole buffer's block (global: every rank's) | the
        # current step's (minibatch)], each fp32 [mean, inv, std, explained variance], written by csrc/advnorm.hip
        # on the compute stream; _adv_arg is the one the next update launch reads (_minibatch picks it; empty: off).
        # Allocated only with the flag on.
        self.adv_scope = params.adv_scope()
        self.adv_block: Optional[torch.Tensor] = None
        self._adv_arg = self.no_q
        if self.adv_scope:
            self.adv_blocks = torch.zeros(2, 4, **f32)
            self.adv_block, self.adv_block_mb = self.adv_blocks[0], self.adv_blocks[1]
            self._adv_arg = self.adv_block
            self.adv_sums_buf = torch.zeros(2, 4, dtype=torch.float64, **dev)     # likewise [buffer | step]
            self.adv_part = torch.zeros(4 * int(self.ext.adv_stats_nblk(self.N)), dtype=torch.float64, **dev)
        obs0 = env.reset()
        self._host_obs = obs0.to(device) if self.host_env else None
        self.params_changed()

    # ------------------------------------------------------------------------------------------
    def _build_wgrad_plan(self, model: ActorCritic, target_wgs: Optional[int] = None, joint: bool = False) -> None:
        """Task lists of the grouped split-K wgrad launches: (layer, output tile, batch chunk),
        output tiles from wgrad_tiles().

        One *bucket* = one wgrad launch + one gather launch over a contiguous flat range of the
        gradient.  Per-head kernels: bucket 0 = the policy layers p_fc1, p_fc2 (flat
        [A, v_fc1.weight)), bucket 1 = the value layers v_fc1, v_fc2 (flat [v_fc1.weight, n)),
        so each head's chain gathers (and all-reduces) its own range; ``joint`` (world size 1):
        those four layers in ONE bucket over [A, n).  The narrow output layers mu and v, log_std
        and the loss terms are the head kernels' reduce items (partial-row columns, _reduce_items),
        so their elements carry src_meta 0.  One-kernel path: every layer in one bucket.  Each
        bucket is chunked for ~target_wgs workgroups (default Params.wgrad_wgs, 0: one per CU)
        with its own fp32 partial slab."""
        if target_wgs is None:
            target_wgs = int(self.p.wgrad_wgs or WGRAD_TARGET_WGS)
        if target_wgs <= 0:
            target_wgs = (torch.cuda.get_device_properties(self.device).multi_processor_count
                          if self.device.type == "cuda" else 256)
        ls = self.L.layers
        names = [l.name for l in ls]
        # (the 32x32 policy head at bf16x3 sums p_fc2's weight gradient itself)
        pol = ("p_fc1",) if getattr(self, "phead_p2", False) else ("p_fc1", "p_fc2")
        val = ("v_fc1", "v_fc2")
        if self.heads and joint:
            groups = [[names.index(n) for n in pol + val]]
            ranges = [(self.A, model.num_params)]
            partials = [True]
        elif self.heads:
            groups = [[names.index(n) for n in pol], [names.index(n) for n in val]]
            (_, phi), (vlo, vhi) = self.head_range
            ranges = [(self.A, phi), (vlo, vhi)]
            partials = [True, False]
        else:
            groups = [list(range(len(ls)))]
            ranges = [(self.A, model.num_params)]
            partials = [True]
        src = torch.full((model.num_params,), -1, dtype=torch.int64)
        meta = torch.zeros(model.num_params, dtype=torch.int64)
        self.buckets = []
        max_chunks = max(1, self.ldT // 64)            # a task covers >= 64 batch rows
        # Batch chunks PER TILE, in proportion to the tile's operand stream ((nq + kq) * 64 rows
        # per k-step): every task then streams about the same bytes, and the task count is
        # ~target_wgs = one workgroup per CU (the kernel is bound by each CU's operand stream, so
        # every CU gets one equal share; largest-remainder rounding).  The chunk counts are
        # dealt over the tiles of ALL buckets together, so the per-head buckets and the joint one
        # split every tile identically: each weight-gradient element is the same fixed-order sum
        # on every path (the process-group chains == the in-stream joint path, bit for bit).
        # (two quadrants per wave at split-bf16 / bf16: Params.wgrad_wide)
        wide = bool(getattr(self, "wgrad_wide", False))
        all_tiles = []  # (layer, n0, k0, nq, kq)
        for li in sorted({li for layers in groups for li in layers}):
            l = ls[li]
            all_tiles += wgrad_tiles(li, l.fan_out, l.fan_in + 1, wide)
        costs = [t[3] + t[4] for t in all_tiles]
        raw = [target_wgs * c / sum(costs) for c in costs]
        nch_all = [max(1, int(r)) for r in raw]
        rest = sorted(range(len(all_tiles)), key=lambda t: raw[t] - int(raw[t]), reverse=True)
        for t in rest[:max(0, target_wgs - sum(nch_all))]:
            nch_all[t] += 1
        nch_of = {t: min(max_chunks, n) for t, n in zip(all_tiles, nch_all)}
        for bi, (layers, (lo, hi)) in enumerate(zip(groups, ranges)):
            tiles = [t for t in all_tiles if t[0] in layers]
            nch = [nch_of[t] for t in tiles]
            tasks, tile_off, base = [], {}, 0
            for t, n in zip(tiles, nch):
                size = t[3] * t[4] * 64 * 64
                # even number of 32-row k-steps per task (e4m3: a multiple of 4)
                mc = _r(-(-self.ldT // n), 128 if getattr(self, "q8", False) else 64)
                chunks = [(c0, min(c0 + mc, self.ldT)) for c0 in range(0, self.ldT, mc)]
                tile_off[t] = (base, len(chunks), size)
                for ci, (m0, m1) in enumerate(chunks):
                    tasks.append([t[0], t[1], t[2], m0, m1, base + ci * size, t[3], t[4]])
                base += len(chunks) * size
            # XCD-aware order: workgroups b, b+8, b+16, ... are dealt to the same XCD (observed
            # round-robin placement; speed only).  Tasks sorted by batch-row position are cut
            # into 8 runs, one per XCD, so the tasks that share operand rows (all tiles of one
            # row range) run on one XCD and share its L2.
            tasks.sort(key=lambda r: (r[3] + r[4], r[0], r[1], r[2]))
            per_xcd = [[] for _ in range(8)]
            for rank, r in enumerate(tasks):
                per_xcd[rank * 8 // len(tasks)].append(r)
            order = []
            j = 0
            while any(j < len(q) for q in per_xcd):
                for q in per_xcd:
                    if j < len(q):
                        order.append(q[j])
                j += 1
            tasks_host = torch.tensor(order, dtype=torch.int32).reshape(-1).contiguous()
            # flat index -> (offset of its element in its tile's chunk-0 slab, chunk count and
            # slab stride of that tile packed as nch * 32 + size / 4096)
            for li in layers:
                l = ls[li]
                woff, wn = model.offsets[f"{l.name}.weight"]
                nn_ = torch.arange(l.fan_out).repeat_interleave(l.fan_in)
                kk = torch.arange(l.fan_in).repeat(l.fan_out)
                src[woff:woff + wn], meta[woff:woff + wn] = self._slab_index(tile_off, li, nn_, kk)
                boff, bn = model.offsets[f"{l.name}.bias"]
                nb = torch.arange(l.fan_out)
                src[boff:boff + bn], meta[boff:boff + bn] = self._slab_index(tile_off, li, nb,
                                                                             torch.full_like(nb, l.fan_in))
            # every element this bucket gathers from its slab stays inside it (grad_gather relies
            # on it); the elements without a tile (src_meta 0) are reduce items
            so, sm = src[lo:hi], meta[lo:hi]
            has = sm > 0
            reach = so + ((sm >> 5) - 1).clamp(min=0) * ((sm & 31) << 12)
            assert bool((so[has] >= 0).all()) and int(reach[has].max()) < base, "wgrad gather plan exceeds its slab"
            # the same elements by tile, for the gathers' streaming form (csrc/kernels.h SlabTiles):
            # [base, nch, stride, n0, k0, kq, fan_in, fan_out, w_off, b_off, nq, quad0] per tile
            rows, quad0 = [], 0
            for t in tiles:
                l = ls[t[0]]
                tb, tn, size = tile_off[t]
                rows.append([tb, tn, size, t[1], t[2], t[4], l.fan_in, l.fan_out, model.offsets[f"{l.name}.weight"][0],
                             model.offsets[f"{l.name}.bias"][0], t[3], quad0])
                quad0 += min(t[3] * 64, l.fan_out - t[1]) * (-(-min(t[4] * 64, l.fan_in + 1 - t[2]) // 4))
            runs = self._slab_runs(sm, lo)
            HipEngine._check_tile_table(rows, src, meta, runs)   # (by class: the plan also runs on a CPU stand-in)
            self.buckets.append({
                "tasks_host": tasks_host, "tasks": tasks_host.to(self.device),
                "slab": torch.zeros(base, device=self.device, dtype=torch.float32),
                "lo": lo, "hi": hi, "partials": partials[bi], "runs": runs,
                "tile_rows": rows, "nquads": quad0, "tiles": {}})
        src[src < 0] = 0  # reduce items (log_std, and with the per-head kernels mu / v)
        self.src_off = src.to(torch.int32).to(self.device)
        self.src_meta = meta.to(torch.int32).to(self.device)

    def q8_maxima(self) -> torch.Tensor:
        """[3 slots][4 tensors] gradient maxima (g1p, g2p, g1v, g2v) of the amax ring (diagnostics)"""
        return self.q8_amax.view(3, 4, Q8_SUB, 32)[..., 0].view(torch.float32).amax(-1)

    def _wgrad_dt(self) -> int:
        return native.DT_CODE["fp8"] if self.q8 else self.dt

    def _q8_args(self) -> tuple:
        if self.q8:
            return (self.q8_amax, self._q8_step, [0, 1, -1, 2, 3, -1], [Q8_SX, Q8_SH, 1.0, Q8_SX, Q8_SH, 1.0])
        return (self.empty, 0, [-1] * 6, [1.0] * 6)

    def _wgrad(self, b: Dict, xmode: str) -> None:
        """one wgrad launch over bucket b's tasks (Q8: e4m3 operands, the step's scales); ``xmode``
        = where the minibatch's observation operand is (_minibatch: "fm" / "buf" / "mb")"""
        wg_x = self.wg_x_full if (self.phead and xmode == "buf") else self.wg_x
        rm = self.rm_xfm if (not self.phead or xmode == "fm") else self.rm
        self.ext.wgrad(self._wgrad_dt(), self.wg_g, wg_x, self.g_rows, self.x_rows, self.ldT, b["tasks"],
                       b["tasks_host"], b["slab"], *self._q8_args(), rm)

    def _w8(self):
        """fp8 mode: (e4m3 image, per-layer scales) for the value head's e4m3 fc1; else off"""
        return (self.wimg_fwd, self.qscale) if self.fp8 else (self.no_u8, self.no_q)

    def _f8(self, lo: int = 0, hi: Optional[int] = None):
        """fp8 mode: the Adam kernels' shadow e4m3 image (the update's fc1 reads it, csrc/mlp_head.hip
        F8) — (image, per-element layer id of the flat slice [lo, hi), per-layer scales); else off"""
        if not self.fp8:
            return (self.no_u8, self.empty, self.no_q)
        return (self.wimg_fwd, self.layer_id[lo:hi], self.qscale)

    @staticmethod
    def _slab_runs(meta_slice: torch.Tensor, lo: int) -> list:
        """the gathers' slab runs (csrc/kernels.h SlabRuns): the maximal index runs of a bucket's
        flat range [lo, hi) whose elements all have a slab source (src_meta > 0), flattened
        [lo0, hi0, ...] in absolute flat indices; the reduce items between them are not visited"""
        has = (meta_slice > 0).to(torch.int8).tolist()
        runs, start = [], None
        for k, h in enumerate(has + [0]):
            if h and start is None:
                start = k
            elif not h and start is not None:
                runs += [lo + start, lo + k]
                start = None
        assert 2 <= len(runs) <= 8, "a gather takes 1-4 slab runs"
        return runs

    @staticmethod
    def _check_tile_table(rows: list, src: torch.Tensor, meta: torch.Tensor, runs: list) -> None:
        """the tile table names exactly the runs' elements, each at the slab offset, chunk count and stride
        that src_off / src_meta give it (the streaming gathers index the slab and the flat vectors by it
        without a device check)"""
        idx = []
        for tb, tn, size, n0, k0, kq, fan_in, fan_out, woff, boff, nq, _ in rows:
            nr, nc = min(nq * 64, fan_out - n0), min(kq * 64, fan_in + 1 - k0)
            r = torch.arange(nr).repeat_interleave(nc)
            c = torch.arange(nc).repeat(nr)
            k = k0 + c
            i = torch.where(k < fan_in, woff + (n0 + r) * fan_in + k, boff + n0 + r)
            assert bool((src[i] == tb + r * (kq * 64) + c).all()) and bool((meta[i] == tn * 32 + size // 4096).all()), \
                "tile table disagrees with src_off / src_meta"
            idx.append(i)
        idx = torch.cat(idx).sort().values
        want = torch.cat([torch.arange(a, b) for a, b in zip(runs[0::2], runs[1::2])])
        assert torch.equal(idx, want), "tile table does not cover the slab runs exactly"

    def _tiles(self, b: Dict, lo: int = 0) -> tuple:
        """bucket b's tile table as the gathers' trailing operands (device, CPU mirror), its flat offsets
        relative to ``lo`` (a head's slice); (): the per-element form (more tiles than the kernels stage)"""
        if len(b["tile_rows"]) > 32:         # csrc/kernels.h SLAB_TILES_MAX
            return ()
        if lo not in b["tiles"]:
            host = torch.tensor([r[:8] + [r[8] - lo, r[9] - lo] + r[10:] for r in b["tile_rows"]],
                                dtype=torch.int32).reshape(-1).contiguous()
            b["tiles"][lo] = (host.to(self.device), host)
        return b["tiles"][lo]

    def _reduce_items(self, model: ActorCritic) -> Dict[str, tuple]:
        """Reduce items of the gather launches: (partial-row column, destination) pairs, the
        destination a flat index of the gathered range or -1 - q for the loss term q.  "legacy":
        the one-kernel update's [8 loss terms | A dlog_std] rows; "policy" / "value": one head's
        partial buffer (its loss columns, log_std, and mu / v from the fused dW blocks), the value
        destinations relative to its slice; "joint": both heads in the shared buffer."""
        A = self.A
        cols: Dict[str, list] = {k: [] for k in ("legacy", "policy", "value", "joint")}
        dsts: Dict[str, list] = {k: [] for k in cols}

        def add(kind, c, d):
            cols[kind].append(int(c))
            dsts[kind].append(int(d))
        for q in range(8):
            add("legacy", q, -1 - q)
        for j in range(A):
            add("legacy", 8 + j, j)
        vlo = self.head_range[1][0]

        def narrow(kind, layer, dw, base, stride=128):
            """the weight gradient of a layer summed in a head kernel, [out][stride] at partial column
            dw (rows j, k <= fan_in: k == fan_in is the bias)"""
            l = model.layer(layer)
            wo, bo = model.offsets[f"{layer}.weight"][0], model.offsets[f"{layer}.bias"][0]
            for j in range(l.fan_out):
                for k in range(l.fan_in):
                    add(kind, dw + j * stride + k, wo - base + j * l.fan_in + k)
                add(kind, dw + j * stride + l.fan_in, bo - base + j)
        # (the head kernels' dW_mu block holds 32 output rows: a wider action head — 40 logits of a categorical
        # policy — never takes them, and has no per-head items)
        for kind, dwp, dwv, vbase in (("policy", self.part_dw[0], None, None),
                                      ("value", None, self.part_dw[1], vlo),
                                      ("joint", self.part_dw_joint[0], self.part_dw_joint[1], 0)) if A <= 32 else ():
            if dwp is not None:
                for q in (0, 2, 3, 4, 5, 6, 7):
                    add(kind, q, -1 - q)
                for j in range(A):
                    add(kind, 8 + j, j)
                narrow(kind, "mu", dwp, 0)
                if self.phead_p2:
                    narrow(kind, "p_fc2", dwp + 32 * 128, 0)
            if dwv is not None:
                add(kind, 1, -2)
                narrow(kind, "v", dwv, vbase)
        out = {}
        for kind in cols:
            if not cols[kind]:
                continue
            c = torch.tensor(cols[kind], dtype=torch.int32)
            d = torch.tensor(dsts[kind], dtype=torch.int32)
            # the gather kernels index part rows and flat slices by these without a device check
            lim = {"legacy": self.npart, "policy": self.part_h[0].shape[1], "value": self.part_h[1].shape[1],
                   "joint": self.part_joint.shape[1]}[kind]
            assert int(c.min()) >= 0 and int(c.max()) < lim, kind
            assert len(set(d[d >= 0].tolist())) == int((d >= 0).sum()), kind   # one item per element
            out[kind] = (c.to(self.device), d.to(self.device))
        return out

    @staticmethod
    def _slab_index(tile_off, li, n, k):
        """dW[n][k] of layer li -> (slab offset in its tile's chunk-0 slab: tile base +
        (n - n0) * (kq * 64) + (k - k0); packed chunk count / stride of the tile)"""
        out = torch.full_like(n, -1)
        meta = torch.zeros_like(n)
        for (tl, n0, k0, nq, kq), (base, nch, size) in tile_off.items():
            if tl != li:
                continue
            m = (n >= n0) & (n < n0 + 64 * nq) & (k >= k0) & (k < k0 + 64 * kq)
            out[m] = base + (n[m] - n0) * (64 * kq) + (k[m] - k0)
            meta[m] = nch * 32 + size // 4096
        assert bool((out >= 0).all()), "wgrad tiles do not cover the layer"
        return out, meta

    # ------------------------------------------------------------------------------------------
    def sync_tile(self) -> None:
        """Row tile of the fused update kernel (64 rows when the layer set fits LDS, else 32;
        16 at fp32) and the partial-sum rows it produces; re-query after ext.set_mlp_rows."""
        xb = self.x_buf.numel() * self.x_buf.element_size()
        self.train_rows = int(self.ext.train_rows(self.dt, self.layout, self.A, xb))
        self.ntrain_blk = self.ldT // self.train_rows

    @property
    def adam_step(self) -> int:
        """Adam steps applied since the start of training.  Host-known without target_kl.  With it the
        device decides which steps are applied and kl_gate alone advances the counter, so the number is
        read from adam_state[0] (a host sync: checkpoints, params_changed — sync points already) and a
        host write (a resume) goes to the device counter too."""
        if self.gate is not None:
            return int(self.adam_state[0].item())
        return self._adam_step

    @adam_step.setter
    def adam_step(self, step: int) -> None:
        self._adam_step = int(step)
        if self.gate is not None:
            self.adam_state[0] = float(step)
            self.adam_state[1] = float(step)

    def params_changed(self) -> None:
        """re-pack the weight images from the fp32 master (after init / load / broadcast)."""
        self.ext.pack(self.model.flat.data, self.wimg, self.w_map, self.wt_map, self.dt, self.no_q)
        if self.gate is None:     # (target_kl: adam_state[0] IS the step number, nothing to mirror)
            self.adam_state[0] = float(self.adam_step)
        self.refresh_fwd_image()

    @torch.no_grad()
    def refresh_fwd_image(self) -> None:
        """fp8 only: per-layer amax scales + e4m3 image of the current weights, on the device in
        two launches (csrc/optim.hip fp8_amax_kernel + pack_fp8_kernel; no host sync).
        s_l = amax_l / 416 keeps every weight inside e4m3's finite range (448) with headroom;
        the kernels multiply each layer's accumulator by s_l."""
        if not self.fp8:
            return
        self.ext.fp8_refresh(self.model.flat.data, self.layer_id, self.qscale, self.fp8_part, self.wimg_fwd, self.w_map,
                             self.wt_map)

    def decode(self, t: torch.Tensor) -> torch.Tensor:
        """a storage-precision buffer of this engine (x_buf, an operand buffer) as fp32"""
        return storage.decode(t, self.dt)

    def encode(self, x: torch.Tensor) -> torch.Tensor:
        return storage.encode(x, self.dt)

    def current_obs(self) -> torch.Tensor:
        return self._host_obs if self.host_env else self.env.observe()

    def _device_merge(self, s1, s2, count, n_a, shift) -> None:
        """RunningObsStats merge on the device (csrc/obs.hip): one launch instead of ~15 ops."""
        st = self.stats
        if s1.data_ptr() == self.s12.data_ptr() and s2.data_ptr() == self.s12[1].data_ptr():
            s12 = self.s12
        else:
            s12 = torch.stack([s1.to(torch.float64), s2.to(torch.float64)]).contiguous()
        self.ext.obs_merge(s12, count, n_a, shift.contiguous(), st.mean, st.mean_diff, st.mean_f32,
                           st.inv_std_f32, 1e-2)

    def _ret_device_merge(self, s1, s2, count, n_a, shift) -> None:
        """RunningReturnStats merge on the device: obs_merge with O = 1 and the return floor (the
        shift is the statistics' own fp32 mean image, which the kernel reads before it writes)."""
        rs = self.ret_stats
        if s1.data_ptr() == self.ret_s12.data_ptr() and s2.data_ptr() == self.ret_s12[1:].data_ptr():
            s12 = self.ret_s12
        else:
            s12 = torch.cat([s1.reshape(1), s2.reshape(1)]).to(torch.float64)
        self.ext.obs_merge(s12, count, n_a, shift.contiguous(), rs.mean, rs.mean_diff, rs.mean_f32, rs.inv_std_f32,
                           RET_VAR_FLOOR)

    @torch.no_grad()
    def return_moments(self) -> torch.Tensor:
        """reward_norm, after a rollout: the discounted-return scan over the rollout's rewards / dones
        (csrc/retnorm.hip; ``ret_acc`` advanced in place) -> device fp64 [2] = (S1, S2) of its T*E
        samples about the statistics' shift.  No host sync; the worker sums it over ranks with the
        observation moments and hands it to ``merge_return_moments``."""
        T, E = self.T, self.E
        self.ext.ret_scan(self.rewards.view(T, E), self.dones.view(T, E), self.ret_acc, self.ret_stats.shift(),
                          self.ret_part, self.ret_s12, self.no_q, float(self.p.gamma), 0)
        return self.ret_s12

    def merge_return_moments(self, count: float, s12: torch.Tensor) -> None:
        rs = self.ret_stats
        rs.merge_moments(float(count), s12[0:1], s12[1:2], rs.shift())

    def env_state(self) -> Dict:
        d = self.env.state_dict()
        if self.ret_acc is not None:
            d = dict(d, ret_acc=self.ret_acc.detach().cpu().clone())
        return d

    def load_env_state(self, d: Dict) -> None:
        d = load_ret_acc(self, d)
        self.env.load_state_dict(d)
        if self.host_env:
            # the host envs were restored (and reset): the next rollout acts on their observation,
            # not on the one the constructor's reset left (TorchEngine.load_env_state does the same)
            self._host_obs = self.env.observe().to(self.device, torch.float32)

    # ------------------------------------------------------------------------------------------
    def _launch_rollout(self, T: int, t_base: int, t0: int, norm: RunningObsStats, shift: torch.Tensor,
                        xT: Optional[torch.Tensor] = None, mom: Optional[torch.Tensor] = None,
                        epstat: Optional[torch.Tensor] = None):
        head, tail = self._rollout_args(T, t_base, t0, shift, mom, epstat)
        args = (*head, norm.mean_f32, norm.inv_std_f32, *tail, self.empty_x if xT is None else xT, self.x_rows[0])
        if self.boot:
            self.ext.rollout_fin(*args, self.trunc, self.x_fin, self.fin_K)
        else:
            self.ext.rollout(*args)

    def _rollout_args(self, T: int, t_base: int, t0: int, shift: torch.Tensor, mom: Optional[torch.Tensor] = None,
                      epstat: Optional[torch.Tensor] = None):
        """The positional arguments every rollout binding shares, as (head, tail): ext.rollout /
        rollout_fin take (*head, mean_f32, inv_std_f32, *tail, xT, xT rows[, trunc, x_fin, fin_K]),
        ext.rollout_stepnorm (*head, *tail, its stats and granule buffers).
        ints = [env kind, E, O, A, state dim, steps T of this launch, its first buffer step t_base, the
        buffer's envs per step (E), step key t0 of its first step (32 bits), episode step limit, std_var,
        the policy head (0 Gaussian, 1 categorical)];
        keys = [env, terminal, reset, action]."""
        e = self.env
        kp = e.kernel_params()
        ints = [self._kind(), self.E, self.O, self.A, e.state_dim, T, t_base, self.E, t0 & 0xFFFFFFFF,
                kp["limit"], self.std_var, self.kernel_dist]
        keys = [kp["key_env"], kp["key_term"], kp["key_reset"], self.key_action]
        return ((self.dt_fwd, ROLL_ROWS, e.state, e.ep_len, e.ep_ret, self.wimg_fwd, self.layout, self.scales,
                 self.model.flat.data),
                (shift, self.x_buf, self.actions, self.logp, self.rewards, self.dones,
                 self.mom if mom is None else mom, self.epstat if epstat is None else epstat, ints, keys,
                 float(self.p.reward_clip), self.qscale))

    def _kind(self) -> int:
        """the in-kernel env kind of the rollout / eval launches; an env that has none never gets here
        through rollout() / evaluate() (``stepped_env``), so reaching this without one is a caller's error"""
        if self.kernel_kind is None:
            raise RuntimeError(f"env {self.env.spec.name!r} has no in-kernel dynamics selected (env_fused): the "
                               "rollout / evaluation kernels cannot run it")
        return self.kernel_kind

    def _stepnorm_fits(self) -> bool:
        """the per-step normalisation launch holds every env tile co-resident on this device"""
        if self._sn_cap is None:
            e = self.env
            self._sn_cap = int(self.ext.rollout_stepnorm_cap(self.dt_fwd, ROLL_ROWS, self.layout, self.O, self.A,
                                                              e.state_dim))
        return self.mom.shape[0] <= self._sn_cap

    def _launch_stepnorm(self, ls: RunningObsStats, shift: torch.Tensor) -> None:
        """obs_norm_update='step' as one cooperative rollout launch: every step merges its batch
        into ``ls`` (in place, fp64) before normalising it (csrc/rollout.hip sn_step)."""
        if self._sn_bufs is None:
            nroll = self.mom.shape[0]
            # (csrc/kernels.h sn_g1_elems: 4-feature x 4-workgroup line blocks)
            g1n = 2 * (-(-self.O // 4)) * (-(-nroll // 4)) * 16
            self._sn_bufs = (torch.zeros(g1n, dtype=torch.int64, device=self.device),
                             torch.zeros(2 * self.O, dtype=torch.int64, device=self.device),
                             torch.zeros(1, dtype=torch.int32, device=self.device),
                             torch.zeros(1, dtype=torch.int32, pin_memory=True))
        g1, g2, err, err_host = self._sn_bufs
        if int(err_host[0]) != 0:   # (staged after an earlier launch: no sync here)
            raise RuntimeError("per-step observation normalisation launch timed out waiting for a workgroup")
        head, tail = self._rollout_args(self.T, 0, self.env.t, shift)
        self.ext.rollout_stepnorm(*head, *tail, [ls.mean, ls.mean_diff, ls.mean_f32, ls.inv_std_f32], g1, g2, err,
                                  float(ls.n), self._sn_epoch, 1e-2)
        self._sn_epoch += self.T
        ls.n += float(self.N)
        err_host.copy_(err, non_blocking=True)

    def raise_if_failed(self, sync: bool = False) -> None:
        """A per-step normalisation launch that timed out waiting for a workgroup left its buffers
        partly written: raise before anything built on them is reported or saved.  The host copy
        of the timeout word is staged behind each launch; ``sync`` waits for it (checkpoints), the
        worker's metrics resolution calls it after the iteration's event has completed."""
        if self._sn_bufs is None:
            return
        if sync:
            torch.cuda.synchronize(self.device)
        if int(self._sn_bufs[3][0]) != 0:
            raise RuntimeError("per-step observation normalisation launch timed out waiting for a workgroup: "
                               "the iteration's rollout is incomplete")

    def _observe_step(self, norm: RunningObsStats, obs: torch.Tensor, shift: torch.Tensor) -> None:
        """norm.observes(obs) as three device launches (csrc/obs.hip obs_observe), moments about
        the iteration's shift snapshot."""
        if self._obs_scratch is None:
            self._obs_scratch = (torch.zeros(int(self.ext.obs_moments_nblk(self.E)), 2, self.O,
                                             dtype=torch.float32, device=self.device),
                                 torch.zeros(2, self.O, dtype=torch.float64, device=self.device))
        part, s12 = self._obs_scratch
        self.ext.obs_observe(obs.to(self.device, torch.float32).contiguous(), shift, norm.mean, norm.mean_diff,
                             norm.mean_f32, norm.inv_std_f32, float(norm.n), part, s12, 1e-2)
        norm.n += float(obs.shape[0])

    @torch.no_grad()
    def _rollout_host(self) -> Dict:
        """T steps of a host-stepped env (gym backend, train.py:82-106 vectorised): the env runs
        on the host, so the fused rollout kernel (which steps the builtin dynamics in-kernel)
        cannot; per step the E observations are normalised and the policy head evaluated as
        device tensor ops (E rows; ~126 small launches per step, ~0.8-1 ms: profiles/act/README.md), the action noise
        and log-prob use the same keyed RNG as the kernel, and the buffer rows are written in
        the storage precision.  The rollout-time x^T operand is not emitted (the update kernel
        transposes X itself).  Params.host_policy = "kernel" takes _rollout_host_kernel instead
        (one csrc/act.hip launch per step); this path stays the default and the reference of
        tests/test_gym_backend.py (profiles/act/README.md times both)."""
        from ..ops import oracle
        if self.p.host_policy == "kernel":
            return self._rollout_host_kernel()
        p, T, E, O = self.p, self.T, self.E, self.O
        norm, shift = self._rollout_begin()
        s1 = torch.zeros(O, dtype=torch.float64, device=self.device)
        s2 = torch.zeros_like(s1)
        ep = torch.zeros(2, dtype=torch.float64, device=self.device)
        log_std = self.model.view("log_std")
        log_sigma = log_std if p.std_convention == "std" else 0.5 * log_std
        sigma = torch.exp(log_sigma)
        eidx = torch.arange(E, device=self.device, dtype=torch.int64)
        dims = torch.arange(self.A, device=self.device, dtype=torch.int64)
        X = torch.zeros(T + 1, E, self.d0, device=self.device)
        X[..., O] = 1.0
        obs = self._host_obs
        for t in range(T):
            _, a1, a2 = RunningObsStats.moments(obs, shift)
            s1 += a1
            s2 += a2
            if p.obs_norm_update == "step":
                self._observe_step(norm, obs, shift)
            x = norm.normalize(obs)
            mu, _, _ = self.model(x)
            eps = rng.gauss(self.key_action, eidx[:, None], self.env.t, dims[None, :])
            a = mu + sigma * eps
            logp = (-0.5 * eps * eps - 0.5 * oracle.LOG_2PI - log_sigma).sum(-1)
            nobs, r, done, info = self.env.step(a)
            r = r.to(self.device)
            if p.reward_clip > 0:
                r = r.clamp(-p.reward_clip, p.reward_clip)
            X[t, :, :O] = x
            rows = slice(t * E, (t + 1) * E)
            self.actions[rows] = a
            self.logp[rows] = logp
            self.rewards[rows] = r
            self.dones[rows] = done.to(self.device, torch.float32)
            ep[0] += float(info["ep_return_sum"])
            ep[1] += float(info["ep_count"])
            obs = nobs.to(self.device, torch.float32)
        X[T, :, :O] = norm.normalize(obs)
        self._host_obs = obs
        self.x_buf.copy_(self.encode(X.view(-1, self.d0)))
        self._xT_valid = False
        return self._rollout_result(shift, (s1, s2), ep)

    def _rollout_begin(self, snapshot: bool = True):
        """(norm, shift) of a rollout: the stats that normalise its observations and the shift its
        moments are taken about.  obs_norm_update = "step": a fresh worker-local copy of the stats
        (``local_stats``), which every step's batch is merged into before it is normalised."""
        # a snapshot of the fp32 mean: always in step mode and on the host paths; the device-stepped
        # path in rollout mode passes the live mean itself, as the fused path does (no copy)
        shift = self.stats.shift().clone() if snapshot or self.p.obs_norm_update == "step" else self.stats.shift()
        if self.p.obs_norm_update != "step":
            return self.stats, shift
        self.local_stats = RunningObsStats(self.O, self.device)
        self.local_stats.copy_from(self.stats)
        return self.local_stats, shift

    def _rollout_result(self, shift: torch.Tensor, s12, ep: torch.Tensor) -> Dict:
        """what every rollout path returns: the moments (S1, S2) of its N observations about ``shift``
        and the fp64 [return sum, count] of the episodes it ended, all on the device"""
        return {"count": float(self.N), "s1": s12[0], "s2": s12[1], "shift": shift,
                "ep_return_sum": ep[0], "ep_count": ep[1], "ep2": ep}

    def _rollout_steps(self, obs: torch.Tensor, norm: RunningObsStats, shift: torch.Tensor, advance, host_sums=None):
        """The per-step loop of the stepped rollouts (_rollout_host_kernel, rollout_stepped).  Per env
        step, on the current stream and with no host sync of its own: in step mode the three
        obs_observe launches (_observe_step), then ONE csrc/act.hip launch that normalises ``obs``,
        evaluates the policy on MFMA, samples with the keyed RNG (step key ``env.t``, ``e_base`` 0,
        the engine's action key: the fused kernel's keys) and writes the step's ``actions`` / ``logp``
        / ``x_buf`` rows and the moments in ``self.mom``; then ``advance(t, rows, actions, key)``
        steps the env, fills the step's ``rewards`` / ``dones`` rows and returns the next observation
        (fp32, contiguous, on the device).  After the loop a rows-only launch writes the bootstrap
        rows and one obs_reduce turns the moments into ``self.s12`` (and ``epstat`` into ``ep_sum``).
        ``host_sums``: the host path's [return sum, count] list, which its ``advance`` adds to.
        Returns (the last observation, the rollout's result dict)."""
        T, E, env, none = self.T, self.E, self.env, self.no_q
        step = self.p.obs_norm_update == "step"
        for t in range(T):
            if step:
                self._observe_step(norm, obs, shift)
            rows = slice(t * E, (t + 1) * E)
            a = self.actions[rows]
            # step key: the host path's env.t as it is, the device path's 32 bits that its dynamics take too
            k = env.t if host_sums is not None else env.t & rng.MASK32
            self._launch_act(obs, k, False, 0, self.key_action, norm, shift, a, self.logp[rows], none,
                             self.x_buf[rows], self.mom, t == 0)
            obs = advance(t, rows, a, k)
        # episode sums: the host envs' in an fp64 tensor of their own (obs_reduce rewrites ep_sum from an
        # epstat that the host path never fills); the device paths' are env_advance's epstat, reduced into ep_sum
        ep = self.ep_sum if host_sums is None else torch.tensor(host_sums, dtype=torch.float64, device=self.device)
        # bootstrap rows [T*E, (T+1)*E): rows only, no MLP, no moments
        self._launch_act(obs, env.t, False, 0, self.key_action, norm, shift, none, none, none, self.x_buf[T * E:],
                         none, False)
        self._xT_valid = False
        self.ext.obs_reduce(self.mom, self.mom.shape[0], self.O, self.s12, self.epstat, self.ep_sum)
        return obs, self._rollout_result(shift, self.s12, ep)

    @torch.no_grad()
    def _rollout_host_kernel(self) -> Dict:
        """_rollout_host with Params.host_policy = "kernel": _rollout_steps' one act launch per env
        step in place of the torch ops, then the host env step.  No fp32 staging tensor, no encode
        copy, no per-step torch moments / normalise / model / RNG ops."""
        clip = self.p.reward_clip
        norm, shift = self._rollout_begin()
        sums = [0.0, 0.0]

        def advance(t, rows, a, k):
            nobs, r, done, info = self.env.step(a)
            # the env's outputs are host tensors: clip / convert there, so each reaches its buffer
            # rows as one upload and the act launch is the step's only kernel
            if clip > 0:
                r = r.clamp(-clip, clip)
            self.rewards[rows].copy_(r.to(torch.float32))
            self.dones[rows].copy_(done.to(torch.float32))
            sums[0] += float(info["ep_return_sum"])
            sums[1] += float(info["ep_count"])
            return nobs.to(torch.float32).to(self.device).contiguous()
        self._host_obs, ro = self._rollout_steps(self._host_obs.to(self.device, torch.float32).contiguous(), norm,
                                                 shift, advance, sums)
        return ro

    @torch.no_grad()
    def rollout_stepped(self) -> Dict:
        """T steps of a builtin tensor env stepped ON THE DEVICE by its own torch ops — the path of a
        registered tensor env (``stepped_env``), whose dynamics the rollout kernel does not know or
        was not asked to run (``env_fused`` off).  It also runs the envs rollout() takes in-kernel:
        kinds 0 / 1 and the fused cart-pole (the tests hold it against the fused kernel there).  Per step,
        all on the current stream and with no host sync:

          1. _rollout_steps' act launch (after the step-mode observe)
          2. ``env._dynamics`` and ``env._reset_state``: the env's torch ops
          3. one csrc/envstep.hip launch (``env_advance``): VecEnv.step's episode bookkeeping,
             straight into the ``rewards`` / ``dones`` rows, ``env.state`` / ``ep_len`` / ``ep_ret``
             (updated in place: they stay the env's live tensors, so ``env.state_dict()``
             checkpoints them as ever) and ``self.epstat``
          4. ``env.t += 1``, ``obs = env.observe()``

        The update runs on the usual kernels; the return dict is the other paths'.  With
        ``bootstrap_time_limit`` step 3 is preceded by ``observe()`` of the new state and a rows-only
        act launch into scratch rows, and ``env_advance_fin`` also writes the step's ``trunc`` row and
        copies the truncated envs' scratch rows into the slot ``x_fin[t // limit]``; still no host sync."""
        if self.host_env:
            raise RuntimeError("rollout_stepped() steps a builtin tensor env on the device; a host-stepped (gym) env "
                               "takes rollout()")
        if self.boot and self.p.obs_norm_update == "step":
            raise ValueError("bootstrap_time_limit is not built for obs_norm_update=step")
        self._flush_value()        # (fp8: the refresh reads every layer; and the reduce rewrites ep_sum)
        self.refresh_fwd_image()
        E, env, none, clip = self.E, self.env, self.no_q, float(self.p.reward_clip)
        norm, shift = self._rollout_begin(snapshot=False)
        if not env.state.is_contiguous():
            env.state = env.state.contiguous()

        def advance(t, rows, a, k):
            # (a discrete env: the index of the one-hot row, on the device)
            new_state, reward, terminal = env._dynamics(a.argmax(1) if self.discrete else a, k)
            reset_state = env._reset_state(k)
            # (.to / .contiguous: no-ops for an env that returns fp32 / bool contiguous tensors)
            adv_args = (reward.to(torch.float32).contiguous(), terminal.to(torch.bool).contiguous(),
                        new_state.to(torch.float32).contiguous(), reset_state.to(torch.float32).contiguous(),
                        env.state, env.ep_len, env.ep_ret, self.rewards[rows], self.dones[rows],
                        self.epstat, env.limit, clip, t == 0)
            if self.boot:
                # the observation of the stepped state (VecEnv.step's final_obs) as buffer rows: one
                # rows-only act launch into the scratch rows; env_advance copies the truncated envs'
                # rows into this step's x_fin slot.  The env's live state tensor is put back at once.
                live, env.state = env.state, adv_args[2]
                fobs = env.observe().to(torch.float32).contiguous()
                env.state = live
                self._launch_act(fobs, k, False, 0, self.key_action, norm, shift, none, none, none, self._fin_rows,
                                 none, False)
                slot = t // env.limit
                self.ext.env_advance_fin(*adv_args, self._fin_rows, self.x_fin[slot * E:(slot + 1) * E],
                                         self.trunc[rows])
            else:
                self.ext.env_advance(*adv_args)
            env.t += 1
            return env.observe().to(torch.float32).contiguous()
        return self._rollout_steps(env.observe().to(torch.float32).contiguous(), norm, shift, advance)[1]

    @torch.no_grad()
    def _evaluate_stepped(self, E: int, deterministic: bool):
        """evaluate() of a device-stepped env: the torch twin's loop (evaluator.evaluate_batch: fresh
        envs with the evaluator's keys, first-episode sums masked) with one csrc/act.hip launch as
        its policy step and no early exit — ``limit`` steps, no host sync.  Writes nothing but its
        own tensors (the envs are its own)."""
        from ..envs import make_vec_env
        from .evaluator import EVAL_ENV_SEED_OFFSET, eval_keys, evaluate_batch
        p = self.p
        env = make_vec_env(self.env.spec, E, seed=p.seed + EVAL_ENV_SEED_OFFSET, rank=0, device=self.device,
                           max_episode_length=p.max_episode_length)
        key_action = eval_keys(p.seed)["key_action"]
        a = self._eval_act_bufs.get(E)
        if a is None:
            a = self._eval_act_bufs[E] = torch.zeros(E, self.A, dtype=torch.float32, device=self.device)
        none = self.no_q

        def act_fn(obs, step_key):
            self._launch_act(obs.to(torch.float32).contiguous(), step_key, deterministic, 0, key_action, self.stats,
                             self.stats.shift(), a, none, none, self.empty_x, none, False)
            return a.argmax(1) if self.discrete else a
        return evaluate_batch(self.model, self.stats, env, E, p.seed, p.max_episode_length, p.std_convention,
                              deterministic, act_fn=act_fn, early_exit=False)

    @torch.no_grad()
    def rollout(self, stats_stream: Optional[torch.cuda.Stream] = None) -> Dict:
        """T env steps for every env.  ``stats_stream`` (rollout-mode obs stats only): the
        one-launch moment/episode-stat reduce runs there, ordered after the rollout kernel, so
        it (and the caller's merge, issued on the same stream) overlaps the value forward and
        the update; the caller orders its stream after that work before reading the stats."""
        if self.stepped_env:
            ro = self.rollout_stepped()
            if stats_stream is not None:
                # as the host path below: the caller merges on stats_stream, after this rollout's work
                stats_stream.wait_stream(torch.cuda.current_stream(self.device))
            return ro
        # fp8: the weights changed during the previous update (Adam rewrites only the bf16 image);
        # before either path, so values() / GAE of a host-env rollout see the current weights too.
        # The refresh reads every layer: a value step still running on the side stream
        # (--overlap-rollout) is joined first, so fp8 runs that step in order.
        if self.fp8 or self.host_env:
            self._flush_value()
        self.refresh_fwd_image()
        if self.host_env:
            ro = self._rollout_host()
            if stats_stream is not None:
                # the caller merges the moments on stats_stream: order it after the host rollout's
                # device work, which produced them (and reads the stats the merge overwrites)
                stats_stream.wait_stream(torch.cuda.current_stream(self.device))
            return ro
        p = self.p
        if p.obs_norm_update == "rollout":
            # the shift IS the fp32 mean, no snapshot copy: its readers are the rollout kernel
            # and obs_merge, which reads shift[d] before writing mean_f32[d] in the same thread
            shift = self.stats.shift()
            # full-batch update: the rollout also writes the fragment-major x^T wgrad operand once,
            # so the 10 epochs' fused kernels skip re-transposing X (xT_ready)
            self._launch_rollout(self.T, 0, self.env.t, self.stats, shift,
                                 self.xT if self.xT_from_rollout else None)
            self._xT_valid = self.xT_from_rollout
            self.env.t += self.T
            # --overlap-rollout: the previous iteration's last value-head step (side stream) ran
            # beside the rollout kernel just enqueued (which reads only the policy); join it here,
            # before the reduce rewrites the episode stats its metrics pack read
            self._flush_value()
            # one launch: moments [nblk][2][O] -> s12, episode stats [nblk][2] -> ep_sum
            if stats_stream is not None:
                stats_stream.wait_stream(torch.cuda.current_stream(self.device))
                shift.record_stream(stats_stream)
                with torch.cuda.stream(stats_stream):
                    self.ext.obs_reduce(self.mom, self.mom.shape[0], self.O, self.s12, self.epstat, self.ep_sum)
            else:
                self.ext.obs_reduce(self.mom, self.mom.shape[0], self.O, self.s12, self.epstat, self.ep_sum)
        else:
            # per-step obs-norm mode (the reference's filter updates with every observation before
            # normalising it, model.py:68 / train.py:84): step t's normalisation needs the stats of
            # step t's batch, a grid-wide dependency.  Default: ONE cooperative launch whose
            # workgroups exchange each step's moments and merged stats in-kernel
            # (csrc/rollout.hip sn_step), into the worker-local stats.  Fallback (the env tiles do
            # not fit co-resident): per step one observe (csrc/obs.hip: moments -> reduce -> merge)
            # + a one-step rollout launch, the steps' moments / episode stats in per-step slices
            # and ONE reduce after the loop.  No host sync either way.
            self._flush_value()
            ls, shift = self._rollout_begin()
            if self._stepnorm_fits():
                self._launch_stepnorm(ls, shift)
                self.env.t += self.T
                self.ext.obs_reduce(self.mom, self.mom.shape[0], self.O, self.s12, self.epstat, self.ep_sum)
                return self._rollout_result(shift, self.s12, self.ep_sum)
            T, nroll = self.T, self.mom.shape[0]
            if self._step_bufs is None or self._step_bufs[0].shape[0] != T:
                f32 = dict(dtype=torch.float32, device=self.device)
                self._step_bufs = (torch.zeros(T, nroll, 2, self.O, **f32), torch.zeros(T, nroll, 2, **f32))
            mom_t, ep_t = self._step_bufs
            for t in range(T):
                self._observe_step(ls, self.current_obs(), shift)
                self._launch_rollout(1, t, self.env.t, ls, shift, mom=mom_t[t], epstat=ep_t[t])
                self.env.t += 1
            self.ext.obs_reduce(mom_t, T * nroll, self.O, self.s12, ep_t, self.ep_sum)
        # everything stays on the device: no host sync inside the iteration
        return self._rollout_result(shift, self.s12, self.ep_sum)

    @torch.no_grad()
    def evaluate(self, num_envs: int, deterministic: bool = False):
        """Batched evaluation of the current policy (csrc/eval.hip): ``num_envs`` fresh evaluation
        envs (runtime/evaluator.py eval_keys: env seed + 7777, rank 0, the evaluator's action
        stream), each from its reset to the end of its first episode, under the current fp32
        images of ``self.stats``.  ONE launch on the current stream, no host sync; returns the
        device tensors ``(ret fp32 [E], len int32 [E])`` this engine owns (rewritten by the next
        call for the same ``num_envs``).  A device-stepped env (``stepped_env``) has no in-kernel
        dynamics: _evaluate_stepped runs the same evaluation as a device-stepped loop, still without
        a host sync.  Reads the policy image, log_std and the stats; writes
        nothing but its own outputs (no env state, buffers, stats, parameters or optimizer state)."""
        from .evaluator import eval_keys
        if self.host_env:
            raise RuntimeError("evaluate() runs the builtin envs in-kernel; a host-stepped (gym) env has no "
                               "device evaluation (use eval_mode='process')")
        E = int(num_envs)
        if E <= 0:
            raise ValueError(f"num_envs must be positive, got {num_envs}")
        # as rollout(): fp8's forward image follows the weights only through the refresh, which
        # reads every layer — a value step still pending / on the side stream is joined first
        if self.fp8:
            self._flush_value()
        self.refresh_fwd_image()
        if self.stepped_env:
            return self._evaluate_stepped(E, bool(deterministic))
        bufs = self._eval_bufs.get(E)
        if bufs is None:
            bufs = self._eval_bufs[E] = (torch.zeros(E, dtype=torch.float32, device=self.device),
                                         torch.zeros(E, dtype=torch.int32, device=self.device))
        ret, length = bufs
        e = self.env
        k = eval_keys(self.p.seed)
        limit = int(min(e.spec.time_limit, self.p.max_episode_length))
        ints = [self._kind(), E, self.O, self.A, e.state_dim, limit, self.std_var, 1 if deterministic else 0,
                self.kernel_dist]
        keys = [k["key_env"], k["key_term"], k["key_reset"], k["key_action"]]
        self.ext.eval_rollout(self.dt_fwd, self.wimg_fwd, self.layout, self.scales, self.model.flat.data,
                              self.stats.mean_f32, self.stats.inv_std_f32, ret, length, ints, keys, self.qscale)
        return ret, length

    def _launch_act(self, obs: torch.Tensor, step_key: int, deterministic: bool, e_base: int, key_action: int,
                    norm: RunningObsStats, shift: torch.Tensor, actions: torch.Tensor, logp: torch.Tensor,
                    mu: torch.Tensor, x_out: torch.Tensor, mom: torch.Tensor, mom_init: bool) -> None:
        """one csrc/act.hip launch on the current stream (an empty tensor skips that output)"""
        ints = [obs.shape[0], self.O, self.A, self.std_var, 1 if deterministic else 0, 1 if mom_init else 0,
                1 if self.discrete else 0]
        keys = [key_action & 0xFFFFFFFF, e_base & 0xFFFFFFFF, step_key & 0xFFFFFFFF]
        self.ext.policy_act(self.dt_fwd, self.wimg_fwd, self.layout, self.scales, self.model.flat.data, norm.mean_f32,
                            norm.inv_std_f32, shift, obs, actions, logp, mu, x_out, mom, ints, keys, self.qscale)

    @torch.no_grad()
    def act(self, obs: torch.Tensor, step_key: Optional[int] = None, deterministic: bool = False, e_base: int = 0, *,
            x_out: Optional[torch.Tensor] = None, mom: Optional[torch.Tensor] = None, mom_init: bool = False,
            key_action: Optional[int] = None):
        """One policy step for caller-supplied observations (csrc/act.hip): ``obs`` fp32 ``[E', O]``
        on the device, any ``E' >= 1`` (not tied to the engine's env count).  ONE launch on the
        current stream, no host sync; returns the device tensors ``(action [E',A], logp [E'],
        mu [E',A])`` (a discrete env: the one-hot rows, their log-probability, the logits) this engine owns (rewritten by the next call for the same ``E'``).  The noise
        of row r is keyed (``key_action``, ``e_base + r``, ``step_key``); ``step_key`` defaults to
        the env's step counter, ``key_action`` to the engine's action stream.  ``x_out``: ``E'``
        rows of ``d0`` in the buffer's storage precision (e.g. a slice of ``x_buf``) receive the
        normalised rows; ``mom`` ``[ceil(E'/16), 2, O]`` fp32 the per-tile moments about the current
        shift (overwritten with ``mom_init``, else added to).  Reads the policy image, log_std and
        the stats; writes nothing but its outputs (no env state, buffers, stats, parameters or
        optimizer state)."""
        if obs.dim() != 2 or obs.shape[1] != self.O or obs.shape[0] < 1:
            raise ValueError(f"obs must be [E, {self.O}], got {tuple(obs.shape)}")
        if obs.device != self.device or obs.dtype != torch.float32:
            raise ValueError("obs must be an fp32 tensor on the engine's device")
        # as evaluate(): fp8's forward image follows the weights only through the refresh
        if self.fp8:
            self._flush_value()
        self.refresh_fwd_image()
        E = int(obs.shape[0])
        bufs = self._act_bufs.get(E)
        if bufs is None:
            f32 = dict(dtype=torch.float32, device=self.device)
            bufs = self._act_bufs[E] = (torch.zeros(E, self.A, **f32), torch.zeros(E, **f32),
                                        torch.zeros(E, self.A, **f32))
        action, logp, mu = bufs
        self._launch_act(obs.contiguous(), self.env.t if step_key is None else int(step_key), deterministic,
                         int(e_base), self.key_action if key_action is None else int(key_action), self.stats,
                         self.stats.shift(), action, logp, mu, self.empty_x if x_out is None else x_out,
                         self.no_q if mom is None else mom, mom_init)
        return action, logp, mu

    @torch.no_grad()
    def _value_forward(self, x: torch.Tensor, M: int, out: torch.Tensor, head_f8: bool = True) -> None:
        """V of the first M rows of ``x`` (buffer storage precision) into ``out``: one csrc/mlp.hip launch"""
        if head_f8 and self.fp8 and self.heads:
            # fp8 mode on the per-head path: the value head's streaming forward with the e4m3 fc1
            # (fc2 / fc3 on the bf16 image; csrc/mlp_head.hip F8)
            dt, wimg, w8 = self.dt, self.wimg, self.wimg_fwd
        else:
            dt, wimg, w8 = self.dt_fwd, self.wimg_fwd, self.no_u8
        self.ext.mlp_value(dt, x, self.empty, 0, M, wimg, self.layout, self.scales, self.model.flat.data, self.A,
                           out, self.qscale, w8)

    @torch.no_grad()
    def values(self) -> None:
        self._flush_value()          # the value head must hold its last step
        self._value_forward(self.x_buf, (self.T + 1) * self.E, self.values_buf)
        if self.p.compat:
            # Q8 (train.py:109-112, ppo.py:119-122): the reference bootstraps R = V(s_T) from the
            # RAW, un-normalised last state.  Rows [T*E, (T+1)*E) of values_buf get V of the env's
            # current raw observation (the rollout left the env after its last step).
            raw = self.env.observe().to(self.device, torch.float32)
            xr = torch.zeros(self.E, self.d0, device=self.device)
            xr[:, :self.O] = raw
            xr[:, self.O] = 1.0
            if self.x_raw is None:
                self.x_raw = torch.empty(self.E, self.d0, dtype=self.sdtype, device=self.device)
            self.x_raw.copy_(self.encode(xr))
            # (the raw rows take the forward image on every layer, in fp8 mode on the per-head path too)
            self._value_forward(self.x_raw, self.E, self.values_buf[self.N:], head_f8=False)
        if self.boot:
            # V of the final rows: the same forward over x_fin's K * E rows (rows never written are
            # zero rows: a finite value that gae() masks)
            self._value_forward(self.x_fin, self.fin_K * self.E, self.v_fin)

    @torch.no_grad()
    def gae(self) -> None:
        T, E = self.T, self.E
        if self.boot:
            # boot[t, e] = trunc[t, e] ? v_fin[t // limit, e] : 0
            if self._fin_slot is None:
                self._fin_slot = torch.arange(T, device=self.device) // int(self.env.limit)
            torch.mul(self.trunc.view(T, E), self.v_fin.view(self.fin_K, E)[self._fin_slot], out=self.boot_buf.view(T, E))
        if self.ret_stats is not None:
            # reward_norm: the kernels scale the reward by the device-resident 1/std (boot is a value: not scaled)
            self.ext.gae_rn(self.rewards.view(T, E), self.values_buf.view(T + 1, E), self.dones.view(T, E),
                            self.boot_buf.view(T, E) if self.boot else self.no_q, self.ret_stats.scale,
                            float(self.p.reward_norm_clip), self.adv.view(T, E), self.ret.view(T, E),
                            float(self.p.gamma), float(self.p.gae_param), 0, self.p.gae_segment())
        elif self.boot:
            self.ext.gae_boot(self.rewards.view(T, E), self.values_buf.view(T + 1, E), self.dones.view(T, E),
                              self.boot_buf.view(T, E), self.adv.view(T, E), self.ret.view(T, E), float(self.p.gamma),
                              float(self.p.gae_param), 0, self.p.gae_segment())
        else:
            self.ext.gae(self.rewards.view(T, E), self.values_buf.view(T + 1, E), self.dones.view(T, E),
                         self.adv.view(T, E), self.ret.view(T, E), float(self.p.gamma), float(self.p.gae_param), 0,
                         self.p.gae_segment())
        if self.p.normalize_adv and not self.adv_scope:
            m, s = self.adv.mean(), self.adv.std()
            self.adv.sub_(m).div_(s + 1e-8)

    @torch.no_grad()
    def adv_sums(self, finish: bool = True) -> torch.Tensor:
        """adv_norm_scope global | minibatch, after gae(): device fp64 [sum a, sum a^2, sum r, sum r^2] of this
        rank's whole buffer (csrc/advnorm.hip: two launches, no host sync).  ``finish``: they are the iteration's
        (no other rank's join them) and the second launch also writes ``adv_block``; else the worker sums them over
        the ranks in stream order and hands them to ``set_adv_sums`` (one more launch)."""
        self.ext.adv_stats(self.adv, self.ret, self.empty, self.N, self.adv_part, self.adv_sums_buf[0], float(self.N),
                           self.adv_block if finish else self.no_q)
        return self.adv_sums_buf[0]

    def set_adv_sums(self, sums: torch.Tensor, n: float) -> None:
        self.ext.adv_block(sums, float(n), self.adv_block)

    def _keep_log_std(self) -> None:
        """train.py:164: log_std as this step's kernels read it, kept for the next step before Adam moves it (only the
        reference loss reads it)"""
        if self.p.loss == "dppo_ref":
            self.log_std_old.copy_(self.model.flat.data[:self.A])

    def begin_update(self) -> None:
        self._keep_log_std()
        self._first_step = True
        if self.gate is not None:
            self.gate.zero_()

    # ------------------------------------------------------------------------------------------
    def _minibatch(self, idx: Optional[torch.Tensor]):
        """(index tensor, first-step flag, x^T-ready flag, x-mode) of one minibatch call.

        x-mode: where the observation operand of p_fc1 / v_fc1's weight gradient is — "fm" the
        rollout's fragment-major x^T (full batch), "buf" x_buf's own rows (full batch under the
        32x32 policy head: no x^T written), "mb" the rows the policy kernel gathers into xT
        (minibatch).  Decided here, from the minibatch alone, and passed to both the head
        kernels and the wgrad (no engine state couples them)."""
        M = self.mb
        if idx is None:
            assert M == self.N, "full-batch call needs minibatch == buffer"
            idx_t = self.empty
        else:
            idx = idx.reshape(-1)
            if idx.numel() != M:
                raise ValueError(f"minibatch has {idx.numel()} rows, engine was planned for {M}")
            lo, hi = int(idx.min()), int(idx.max())
            if lo < 0 or hi >= self.N:   # host-side range check (the launch skips the device check)
                raise IndexError(f"minibatch indices out of range [0, {self.N}): {lo}..{hi}")
            self.idx_dev[:M].copy_(idx.to(torch.int32), non_blocking=True)
            idx_t = self.idx_dev
        if self.adv_scope:
            # minibatch scope: the block of this step's own rows (duplicates counted), two launches ahead of the
            # step's kernels; a full-batch step reads the whole buffer's block
            self._adv_arg = self.adv_block
            if self.adv_scope == "minibatch" and idx is not None:
                self.ext.adv_stats(self.adv, self.no_q, self.idx_dev, M, self.adv_part, self.adv_sums_buf[1], float(M),
                                   self.adv_block_mb)
                self._adv_arg = self.adv_block_mb
        first, xt_ready = bool(self._first_step), bool(idx is None and self._xT_valid)
        xmode = "fm"
        if self.phead:
            # (measured: the fragment-major x^T beside the row-major policy operands made the
            # wgrad slower than x_buf's rows — 4.378 vs 4.214 ms per bf16x3 iteration, profiles/r5 —
            # so x_buf's rows come first and the rollout writes no x^T when they can serve)
            full = idx is None
            if full and self.wg_x_full is not self.wg_x:
                xmode, xt_ready = "buf", True
            elif not (full and xt_ready):
                xmode, xt_ready = "mb", False
        self._x_mode = xmode      # (diagnostics / tests only)
        self._first_step = False
        self._q8_step, self._q8_next = self._q8_next, self._q8_next + 1
        self._loss_dev = self.loss_sums
        return idx_t, first, xt_ready, xmode

    def can_fuse_apply(self, extra_grad: float = 0.0) -> bool:
        """the one-kernel path's grad(idx, apply=True): one gradient range, no clipping (the Adam
        step needs no global norm first), eager launches (the host knows the step number), and
        no all-reduce between the gradient and the update (the caller checks: world size 1)."""
        return (self.fused_apply and not extra_grad and not self.max_norm
                and (self.heads or (len(self.buckets) == 1 and self.buckets[0]["partials"])))

    def step(self, idx: Optional[torch.Tensor], extra_grad: float = 0.0, allreduce=None,
             mean: bool = False, last: bool = False) -> bool:
        """ONE synchronous global step (train.py:133-175 + chief.py:13-20): the minibatch
        gradient, its sum (``mean``: average) over ranks, and the Adam step.  True: the host counts
        one applied update (gated: the device counts them, adam_state[0]).

        ``allreduce``: the worker's collective (parallel/dist.py grad_allreduce_fn), None at world
        size 1.  In-stream communicators (``allreduce.in_stream``: the native RCCL one — the
        default on an RCCL group — or the gloo adapter) reduce in stream order and do the mean
        themselves: joint kernels (one wgrad, one gather) → all-reduce → whole-vector Adam.
        With a side communicator, the value head's all-reduce + Adam go to a side stream instead:
        every epoch's under ``overlap_value_epochs`` (joined right before the next value kernel,
        so they overlap the policy Adam and the next policy kernel), and the iteration's last
        (``last``) under --overlap-rollout (overlapping the next rollout, which reads only the
        policy; joined in rollout()/values()).  Exact either way.

        Process-group collectives (``allreduce(t)`` returns an async work handle): per-head
        chains.  The policy range's all-reduce is issued as soon as it is gathered and runs while
        the value head's kernels compute; the value range's all-reduce runs while the policy Adam
        and the NEXT step's policy kernels compute — its Adam is applied just before the value
        kernel of the next step (or by finish_steps()).  Each head's Adam step e still precedes
        that head's kernel of step e+1, so the parameters are exactly the synchronous ones.
        Clipping (a global norm over both heads), the Q1 extra gradient and the one-kernel tile
        update take the whole-vector path."""
        if self.gate is not None:
            self._gated_step(idx, extra_grad, allreduce, mean)
            return False
        self._ungated_step(idx, extra_grad, allreduce, mean, last)
        return True

    def _ungated_step(self, idx: Optional[torch.Tensor], extra_grad: float, allreduce, mean: bool, last: bool) -> None:
        p = self.p
        if allreduce is None and self.can_fuse_apply(extra_grad):
            self.grad(idx, apply=True)          # world size 1: gather + Adam in one launch
            return
        if getattr(allreduce, "in_stream", False):
            if self.heads:
                # (a value step of the previous epoch still on the side stream is joined inside,
                # right before the value kernel: it ran beside this epoch's policy kernel)
                self._joint_grad(*self._minibatch(idx))
            else:
                self._flush_value()
                self.grad(idx)
            if (self.heads and getattr(allreduce, "side", False) and not self.max_norm and not extra_grad
                    and (p.overlap_value_epochs or (last and p.overlap_rollout))):
                self._split_step_side(allreduce)
                return
            self._flush_value()
            allreduce(self.grad_flat)           # sum / mean in stream order: no host-side scaling
            self.apply(extra_grad)
            return
        mbt = self._minibatch(idx)
        if not self.heads or self.max_norm or extra_grad:   # the whole-vector path
            self._flush_value()                 # (only the per-head chains leave a value step pending)
            self._grad_chain(*mbt)
            if allreduce is not None:
                self._reduce_wait(allreduce(self.grad_flat), self.grad_flat, mean)
            self.apply(extra_grad)
            return
        if allreduce is None:                   # (fused_apply=False: the two-launch chains, no collective)
            allreduce = lambda t: None          # noqa: E731
        step_no = self.adam_step + 1
        (plo, phi), (vlo, vhi) = self.head_range
        self._head_chain(0, *mbt)
        wp = allreduce(self.grad_flat[plo:phi])
        self._flush_value()
        self._head_chain(1, *mbt)
        self._pending_value = ("work", allreduce(self.grad_flat[vlo:vhi]), step_no, mean)
        self.pending_steps += 1
        self._reduce_wait(wp, self.grad_flat[plo:phi], mean)
        self._head_adam(0, step_no)
        self.adam_step += 1
        self._norm_n = self.norm_regions[1][1]

    def _gated_step(self, idx: Optional[torch.Tensor], extra_grad: float, allreduce, mean: bool) -> None:
        """step() under target_kl and / or lr_schedule=adaptive (docs/ARCHITECTURE.md §22, §23; adaptive: the
        Adam launch reads the rate lr_state[0] and kl_gate moves it): the gradient kernels always run; the Adam
        launch is the gated form (applied while gate[0] == 0, step number adam_state[0] + 1 read on the
        device); the kl_gate launch ends the step.  World size 1 with can_fuse_apply: the joint gather +
        Adam launch, gated.  Everything else: ONE gather of the whole gradient, ONE all-reduce of
        [gradient | loss sums] (so every rank gates on the same bits; under grad_reduce=mean both KL
        slots scale alike), ONE whole-vector Adam launch — the per-head Adam pairs and the side-stream
        split are never gated."""
        if allreduce is None and self.can_fuse_apply(extra_grad):
            self.grad(idx, apply=True)
        else:
            if self.heads:
                self._joint_grad(*self._minibatch(idx))
            else:
                self.grad(idx)
            if allreduce is not None:
                if getattr(allreduce, "in_stream", False):
                    allreduce(self._grad_sums)          # sum / mean in stream order
                else:
                    self._reduce_wait(allreduce(self._grad_sums), self._grad_sums, mean)
            self.apply(extra_grad)
        self.ext.kl_gate(self.loss_sums, self.gate, self.adam_state, self._gate_target, *self._rate_block)

    def _split_step_side(self, allreduce) -> None:
        """the joint gradient is gathered: the value range's all-reduce (the side communicator) +
        Adam are forked to the side stream right away, then the policy range's all-reduce + Adam
        run in stream order (the two collectives on two communicators may run concurrently).  The
        next value kernel (_joint_heads), rollout() / values() / finish_steps() join it
        (_flush_value): it overlaps the policy Adam and the next epoch's policy kernel, or the next
        rollout after the last epoch."""
        (plo, phi), (vlo, vhi) = self.head_range
        step_no = self.adam_step + 1
        if self._side is None:
            self._side = torch.cuda.Stream(device=self.device)
        side = self._side
        side.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(side):
            allreduce(self.grad_flat[vlo:vhi], stream=side)
            self._head_adam(1, step_no)
        allreduce(self.grad_flat[plo:phi])
        self._head_adam(0, step_no)
        self._pending_value = ("side", None, step_no, False)
        self.side_steps += 1
        self.adam_step += 1
        self._norm_n = self.norm_regions[1][1]

    def finish_steps(self) -> None:
        """apply a value-head step still waiting for its all-reduce (end of the epochs)"""
        self._flush_value()

    quiesce = finish_steps    # (nothing else is ever deferred here: the parameters are then the synchronous ones)

    def metrics_stream(self) -> Optional[torch.cuda.Stream]:
        """the stream the iteration's metrics are packed and staged on: the side stream while the
        last value step runs there (its Adam writes the value head's norm partials), else None"""
        pend = self._pending_value
        return self._side if (pend is not None and pend[0] == "side") else None

    def _flush_value(self) -> None:
        pend, self._pending_value = self._pending_value, None
        if pend is None:
            return
        kind, work, step_no, mean = pend
        if kind == "side":
            # everything enqueued on the side stream so far: the value step AND the metrics
            # pack / staging copy behind it (their buffers are rewritten after this point)
            torch.cuda.current_stream(self.device).wait_stream(self._side)
            return
        vlo, vhi = self.head_range[1]
        self._reduce_wait(work, self.grad_flat[vlo:vhi], mean)
        self._head_adam(1, step_no)

    def _reduce_wait(self, work, t: torch.Tensor, mean: bool) -> None:
        if work is not None:
            work.wait()          # orders the compute stream after RCCL's (no host block on GPU)
        if mean:
            t.mul_(1.0 / torch.distributed.get_world_size())

    def _grad_chain(self, idx_t, first: bool, xt_ready: bool, xmode: str) -> None:
        """the minibatch gradient into grad_flat: both per-head chains, or the tile kernel's one"""
        if self.heads:
            for h in (0, 1):
                self._head_chain(h, idx_t, first, xt_ready, xmode)
        else:
            self._launch_grad(idx_t, first, xt_ready)

    def _update_args(self, idx_t, first: bool, xt_ready: bool, part: torch.Tensor) -> tuple:
        """the positional block that leads ext.mlp_train, ext.mlp_head_train and ext.phead_train (csrc/bindings.cpp
        train_args): dt, A, the 11 operand buffers, the layout; x_buf, idx, row0, M; the weight image, scales, flat,
        log_std_old; actions, logp, adv, ret, values and mu_prev / v_prev; loss = [loss_kind, value_loss, std_var,
        first_step, clip, ent_coeff]; ldT; the partial rows and their width; xt_ready; the advantage block of
        adv_norm_scope global | minibatch (empty: off)"""
        p = self.p
        loss = [2.0 if self.discrete else float(p.loss != "ppo"), float(p.value_loss != "mse"), float(self.std_var), float(first),
                float(p.clip), float(p.ent_coeff)]
        return (self.dt, self.A, self.tbufs, self.layout, self.x_buf, idx_t, 0, self.mb, self.wimg, self.scales,
                self.model.flat.data, self.log_std_old, self.actions, self.logp, self.adv, self.ret, self.values_buf,
                self.mu_prev, self.v_prev, loss, self.ldT, part, part.shape[1], xt_ready, self._adv_arg)

    def _head_kernel(self, h: int, idx_t, first: bool, xt_ready: bool, part: torch.Tensor, part_dw: int) -> None:
        args = self._update_args(idx_t, first, xt_ready, part)
        if h == 0 and self.phead:
            # (the 32x32 policy kernel: xt_ready as _minibatch resolved it — it writes X rows into xT
            # only for x-mode "mb", a minibatch)
            self.ext.phead_train(*args, part_dw, self.phead_p2)
        else:
            # fp8: the value head's fc1 on the e4m3 image; the policy's GEMMs only with fp8_policy_gemms
            w8 = self._w8() if (h == 1 or self.p.fp8_policy_gemms) else (self.no_u8, self.no_q)
            amax = self.q8_amax if self.q8 else self.empty
            if self.q8 and not self._q8_cal[h]:
                # the first step of this engine: one pass as step -1 only to record the gradient maxima
                # the step-0 scales come from (its stores and partials are overwritten by the real one;
                # the reference loss's mu_prev / v_prev writes are idempotent)
                self.ext.mlp_head_train(*args, h, part_dw, *w8, amax, -1)
                self._q8_cal[h] = True
            self.ext.mlp_head_train(*args, h, part_dw, *w8, amax, self._q8_step)
        if h == 0 and idx_t is self.empty and not self.phead:
            self._xT_valid = True   # the policy kernel wrote x^T of this buffer (full batch)
        if h == 0:
            self._keep_log_std()

    def _joint_heads(self, idx_t, first: bool, xt_ready: bool, xmode: str) -> None:
        """both head kernels into the shared partial buffer (disjoint columns and operands), in
        stream order.  (Measured: the policy kernel on a side stream concurrent with the value
        kernel, joined before the wgrad: 4.57 vs 4.39 ms per iteration, same box — each kernel
        fills a CU's LDS, so they only time-slice the CUs and the stream hand-offs are extra.)"""
        for h in self.head_order:
            if h == 1:
                self._flush_value()   # the previous step's value Adam (side stream) lands first
            self._head_kernel(h, idx_t, first, xt_ready, self.part_joint, self.part_dw_joint[h])

    def _joint(self, gather, idx_t, first: bool, xt_ready: bool, xmode: str) -> None:
        """both head kernels (one shared partial buffer), ONE wgrad over both heads' layers, ONE ``gather`` launch
        over the whole flat vector"""
        self._joint_heads(idx_t, first, xt_ready, xmode)
        b = self.joint_bucket
        self._wgrad(b, xmode)
        gather(b, *self.joint_src, self.part_joint, self.nhead_blk, self.items["joint"])

    def _joint_grad(self, *mbt) -> None:
        """_joint ending in the gather of the whole gradient into grad_flat (no optimizer step)"""
        self._joint(self._gather, *mbt)

    def _joint_step(self, *mbt) -> None:
        """world size 1: _joint ending in the gather + Adam launch"""
        self._joint(self._gather_adam, *mbt)

    def _head_chain(self, h: int, idx_t, first: bool, xt_ready: bool, xmode: str) -> None:
        """head h's kernel -> its wgrad -> its gather into its flat range of grad_flat"""
        self._head_kernel(h, idx_t, first, xt_ready, self.part_h[h], self.part_dw[h])
        b = self.buckets[h]
        self._wgrad(b, xmode)
        self._gather(b, self.src_off, self.src_meta, self.part_h[h], self.nhead_blk,
                     self.items["policy" if h == 0 else "value"], *self.head_range[h])

    def _head_adam(self, h: int, step_no: int) -> None:
        """no-clip Adam over head h's flat range (after its all-reduce); its norm region"""
        lo, hi = self.head_range[h]
        r0, r1 = self.norm_regions[h]
        self._adam(lo, hi, self.norm_part[r0:r1], 0.0, step_no)

    def _next_step(self) -> int:
        """the host step number of the next optimizer launch; target_kl: 0, the gated form reads the number
        (and the stop flag) on the device"""
        return 0 if self.gate is not None else self.adam_step + 1

    def _stepped(self, norm_n: int) -> None:
        """books of a whole optimizer step just launched, which left norm_n norm partials"""
        if self.gate is None:       # (target_kl: kl_gate advances the device counter)
            self.adam_step += 1
        self._norm_n = norm_n

    def _adam(self, lo: int, hi: int, norm_part: torch.Tensor, max_norm: float, step_no: int) -> None:
        """the Adam launch over the flat range [lo, hi): one kernel without clipping when the step number is
        known (step_no >= 1, or gated), the sumsq + adam pair otherwise"""
        p = self.p
        b1, b2 = p.adam_betas
        self.ext.adam(self.model.flat.data[lo:hi], self.grad_flat[lo:hi], self.adam_m[lo:hi], self.adam_v[lo:hi],
                      float(self.lr), float(b1), float(b2), float(p.adam_eps), max_norm, self.adam_state, norm_part,
                      self.wimg, self.w_map[lo:hi], self.wt_map[lo:hi], self.dt, self.no_q, step_no,
                      *self._f8(lo, hi), self._gate_arg, self._lr_arg)

    def _gather(self, b: Dict, src_off: torch.Tensor, src_meta: torch.Tensor, part: torch.Tensor, npblk: int, items,
                lo: int = 0, hi: Optional[int] = None) -> None:
        """the gather launch of bucket b into grad_flat; [lo, hi): into one head's slice of the flat vectors"""
        grad, runs = self.grad_flat, b["runs"]
        if hi is not None:          # (red_dst indexes the slice: the runs and the tile table rebased to it)
            src_off, src_meta, grad, runs = src_off[lo:hi], src_meta[lo:hi], grad[lo:hi], [r - lo for r in runs]
        self.ext.grad_gather(b["slab"], src_off, src_meta, part, npblk, part.shape[1], *items, 1.0 / self.mb, grad,
                             self.loss_sums, runs, *self._tiles(b, lo if hi is not None else 0))

    def _gather_adam(self, b: Dict, src_off: torch.Tensor, src_meta: torch.Tensor, part: torch.Tensor, npblk: int,
                     items) -> None:
        """ONE whole optimizer step as the fused gather + no-clip Adam launch over bucket b (world size 1)"""
        p = self.p
        b1, b2 = p.adam_betas
        self.ext.gather_adam(b["slab"], src_off, src_meta, part, npblk, part.shape[1], *items, b["runs"],
                             1.0 / self.mb, self.loss_sums, self.grad_flat, self.model.flat.data, self.adam_m,
                             self.adam_v, float(self.lr), float(b1), float(b2), float(p.adam_eps), self._next_step(),
                             self.adam_state, self.norm_part[:self.norm_n_whole], self.wimg, self.w_map, self.wt_map,
                             self.dt, self.no_q, *self._f8(), self._gate_arg, self._lr_arg, *self._tiles(b))
        self._stepped(self.norm_n_whole)

    def grad(self, idx: Optional[torch.Tensor], apply: bool = False) -> None:
        """one minibatch gradient into grad_flat (no optimizer step; tests / the whole-vector
        path).  ``apply=True`` (one-kernel path, only when can_fuse_apply()): the gather and the
        Adam step run as ONE launch — the same update as grad() then apply()."""
        self._flush_value()                     # (only the per-head chains leave a value step pending)
        mbt = self._minibatch(idx)
        if not apply:
            self._grad_chain(*mbt)
            return None
        assert self.can_fuse_apply(), "fused gather + Adam is not available here"
        if self.heads:
            self._joint_step(*mbt)
        else:
            self._launch_grad(*mbt[:3], fused_apply=True)
        return None

    def _launch_grad(self, idx_t: torch.Tensor, first: bool, xt_ready: bool, fused_apply: bool = False) -> None:
        self.ext.mlp_train(*self._update_args(idx_t, first, xt_ready, self.part))
        b = self.buckets[0]
        self._wgrad(b, "fm")
        gather = (b, self.src_off, self.src_meta, self.part, self.ntrain_blk, self.items["legacy"])
        if fused_apply:
            self._keep_log_std()        # (before the fused Adam moves it)
            self._gather_adam(*gather)
        else:
            self._gather(*gather)
            self._keep_log_std()

    @torch.no_grad()
    def apply(self, extra_grad: float = 0.0) -> None:
        """whole-vector Adam (+ clip) after grad() [+ the all-reduce]"""
        self._flush_value()
        if extra_grad:
            self.grad_flat.add_(extra_grad)
        self._adam(0, self.grad_flat.numel(), self.norm_part[:self.norm_n_elem], self.max_norm, self._next_step())
        self._stepped(self.norm_n_elem)

    def pack_metrics(self, ep2: torch.Tensor, reduce=None) -> Optional[torch.Tensor]:
        """device f64[11] = [episode return sum, count | loss sums (8) | grad norm], written by ONE
        launch (csrc/optim.hip metrics_pack, 256 threads over the Adam partials) instead of ~6
        small torch ops per iteration, then the tails of ``self.metrics_layout``; the buffer is reused (stream
        order keeps the previous D2H copy ahead of the next pack).  ``reduce``: the worker's all-reduce
        for an ``ep2`` not yet summed over the ranks."""
        if self._loss_dev is None:
            return None
        if reduce is not None:
            ep2 = reduce(ep2)
        # every Adam path (fused no-clip, sumsq + clip, per head) leaves the per-block
        # sums of squares of the gradient it applied in norm_part[:_norm_n].  A value step left
        # pending on the process-group chains has not written its region yet: the norm is the
        # policy head's for that step.  One on the side stream: the pack runs there, after it.
        pend = self._pending_value
        n = self.norm_regions[0][1] if (pend is not None and pend[0] == "work") else self._norm_n
        side = self.metrics_stream()
        if side is not None:
            # everything the pack reads that the compute stream wrote after the value step was
            # forked (the side-stream obs-stat merge's episode sums are joined there at the end)
            side.wait_stream(torch.cuda.current_stream(self.device))
        with (torch.cuda.stream(side) if side is not None else contextlib.nullcontext()):
            self.ext.metrics_pack(ep2, self._loss_dev, self.norm_part[:n], self.metrics_buf)
            lay, buf = self.metrics_layout, self.metrics_buf
            if self.ret_stats is not None:      # return_std = sqrt(M2 / n)
                tail = buf[lay["return_std"]]
                torch.mul(self.ret_stats.mean_diff, 1.0 / max(self.ret_stats.n, 1.0), out=tail)
                tail.sqrt_()
            if self.gate is not None:           # [stop, applied, trip_kl | steps applied since the start]
                g = buf[lay["gate"]]
                g[:3].copy_(self.gate[:3])
                g[3:].copy_(self.adam_state[0:1])
            if self.lr_state is not None:       # [lr, downs, ups]
                buf[lay["lr"]].copy_(self.lr_state[:3])
            elif self.p.lr_schedule == "linear":            # the iteration's host rate
                buf[lay["lr"]].fill_(self.lr)
            if self.adv_scope:                  # [adv_mean, adv_std, explained_variance]
                a = buf[lay["adv"]]
                a[:1].copy_(self.adv_block[0:1])
                a[1:].copy_(self.adv_block[2:4])
        return self.metrics_buf

    def metrics_tails(self) -> Dict[str, torch.Tensor]:
        """the metrics vector's tails by field name, where pack_metrics does not run"""
        out = {}
        if self.ret_stats is not None:
            out["return_std"] = self.ret_stats.std()
        if self.gate is not None:
            out["gate"] = torch.cat([self.gate[:3], self.adam_state[0:1]])
        if self.p.lr_schedule != "constant":
            out["lr"] = self.lr_state[:3] if self.lr_state is not None else torch.tensor([self.lr], dtype=torch.float64)
        if self.adv_scope:
            out["adv"] = torch.cat([self.adv_block[0:1], self.adv_block[2:4]])
        return out

    def lr_state_dict(self) -> torch.Tensor:
        return self.lr_state.detach().cpu()

    def load_lr_state(self, t: torch.Tensor) -> None:
        self.lr_state.copy_(t.to(self.lr_state.device, torch.float32))

    def loss_vector(self) -> Optional[torch.Tensor]:
        """device [loss sums of the last minibatch (8) | grad norm of the last Adam step] — staged
        into host memory by the worker without a sync (``losses_from_vector`` decodes it)."""
        if self._loss_dev is None:
            return None
        if self.max_norm:
            gn = self.adam_state[2:3]              # the clip pass computed it
        else:                                      # no-clip Adam skips the norm: last step's gradient
            gn = torch.linalg.vector_norm(self.grad_flat).reshape(1)
        return torch.cat([self._loss_dev.reshape(-1), gn])

    @staticmethod
    def losses_from_vector(v) -> Dict[str, float]:
        n = max(v[_LS_COUNT], 1.0)
        out = {"loss_clip": v[_LS_CLIP] / n, "loss_value": v[_LS_VALUE] / n, "loss_ent": v[_LS_ENT] / n,
               "approx_kl": v[_LS_KL] / n, "clipfrac": v[_LS_CLIPFRAC] / n}
        out["loss"] = out["loss_clip"] + out["loss_value"] + out["loss_ent"]
        out["grad_norm"] = float(v[NPART_FIXED])
        return out

    def last_losses(self) -> Dict[str, float]:
        vec = self.loss_vector()
        return {} if vec is None else self.losses_from_vector(vec.tolist())

    def sync(self) -> None:
        torch.cuda.synchronize(self.device)
