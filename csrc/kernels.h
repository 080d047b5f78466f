// Host-visible launcher prototypes + argument structs (no torch headers: the .hip files
// compile fast and only bindings.cpp pulls in torch).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// The three-layer policy of the rollout / eval / act kernels (csrc/policy_step.h): the packed weight
// image in the storage precision and the Gaussian head's log_std.  bindings.cpp policy_net() fills
// and checks it for all three.
struct PolicyNet {
  const void* W;
  int off_w1, off_w2, off_w3;
  int d1, d2, d3;      // padded input widths of the 3 layers (P32(K+1))
  int n1, n2, n3;      // real output widths (H1, H2, A)
  float s1, s2, s3;    // dequant scales (fp8; 1 otherwise)
  const float* qscale; // optional device array of the 6 per-layer dequant scales (overrides s*)
  const float* log_std;  // [A] fp32 master
  int std_var;         // 1: exp(log_std) is the variance (reference DPPO), 0: it is sigma
};

struct RolloutArgs {
  // env (state lives in global memory between launches, in LDS during the launch)
  int kind;            // 0 synthetic, 1 pendulum, 2 cart-pole (csrc/env_core.h)
  int E, O, A, S;      // envs, obs dims, act dims, state dims
  int T;               // steps in this launch
  int t_base;          // buffer time index of the first step
  int buf_E;           // env stride of the [T+1][E] buffers (== E)
  uint32_t t0;         // global step counter of the first step (RNG key)
  int limit;           // episode step limit
  uint32_t key_env, key_term, key_reset, key_action;
  float* state;        // [E][S]
  int* ep_len;         // [E]
  float* ep_ret;       // [E]
  PolicyNet net;
  // observation normalisation
  const float* mean;
  const float* inv_std;
  const float* shift;
  float reward_clip;   // <= 0: off
  // outputs
  void* x_out;         // [(T+1)*E][d1] storage precision (row-major, update input)
  float* actions;      // [T][E][A]
  float* logp;         // [T][E]
  float* rewards;      // [T][E] (clipped)
  float* dones;        // [T][E]
  void* xT_out;        // optional FM [rows][ldT] transposed copy of x rows t*E+e (wgrad operand)
  int ldT;             // its row length (== T*E of the whole buffer)
  float* mom;          // [nblk][2][O]  sum(x-shift), sum((x-shift)^2)
  float* epstat;       // [nblk][2]     finished-episode return sum, count
  unsigned long long* tstamp;  // DIAGNOSTIC ONLY (null in real runs): [nblk][NW][8] phase cycles
  // Per-step observation normalisation INSIDE the launch (obs_norm_update = "step", the reference's
  // filter that absorbs every observation before normalising it, model.py:68 / train.py:84-85);
  // sn_g1 == null: off (mean / inv_std above are fixed for the launch).  Step t, all workgroups
  // co-resident (cooperative launch): each publishes its batch moments about `shift` as 8-byte
  // {tag, fp32} granules (sn_g1, sn_g1_index); workgroup b sums the 4-feature units b, b + nblk, ... over all
  // workgroups in a fixed order (fp64), Chan-merges them into the fp64 running stats (sn_mean,
  // sn_m2: each feature owned by ONE workgroup for the whole launch) and publishes the new fp32
  // (mean, 1/std) as granules (sn_g2[2O]); every workgroup gathers those and normalises.  Tags
  // are sn_epoch0 + t (the host never reuses one: no memset), spins are bounded (sn_err).
  double* sn_mean;           // [O] running mean (fp64, in place)
  double* sn_m2;             // [O] running sum of squared deviations (fp64, in place)
  float* sn_mean_f32;        // [O] fp32 images after the last step (host-visible)
  float* sn_inv_std;         // [O]
  unsigned long long* sn_g1; // sn_g1_elems(nblk, O) partial-moment granules (sn_g1_index)
  unsigned long long* sn_g2; // [2O] stats granules
  unsigned* sn_err;          // nonzero: a spin timed out (the launch gave up; the host raises)
  double sn_n0;              // running count before step 0 (each step adds E)
  unsigned sn_epoch0;        // tag of step 0's granules (>= 1)
  double sn_var_floor;
  // bootstrap_time_limit (both or neither; null: the kernel without them, sn_g1 must be null too).
  // An episode that ends by the step limit alone (done && !terminal) is "truncated": trunc gets
  // 1, and the normalised observation the env reached BEFORE its in-place reset is written, in
  // x_out's row format, to x_fin row ((t_base + step) / limit) * E + e.  An env's truncations are
  // >= limit steps apart, so that slot is its own: no counters, no atomics.
  float* trunc;        // [T][E] 0.f / 1.f, like dones
  void* x_fin;         // [fin_K][E][d1] storage precision (allocated zeroed by the host)
  int fin_K;           // >= ceil((t_base + T) / limit)
  // (last: every earlier member keeps its kernel-argument offset)
  // The policy head, as ActArgs::dist.  0: Gaussian.  1: categorical over A actions (policy_step.h categorical_row):
  // the Gumbel-max sample keyed (key_action, env, step, k), `actions` gets ONE-HOT rows, logp the log-softmax of the
  // chosen logit.  Cart-pole physics (kind 2) only, which is pushed +1 for index 1 and -1 for index 0; 16-row tiles,
  // not fp8, not the per-step filter (sn_g1 null).
  int dist;
};

// The per-step filter's partial-moment granules (RolloutArgs::sn_g1), line-blocked: a 128-byte
// line holds moment m of features 4 fu .. 4 fu + 3 of workgroups 4 wb .. 4 wb + 3 (granule
// 4 (w & 3) + (d & 3)); lines ordered [m][fu][wb].
inline __host__ __device__ size_t sn_g1_index(int m, int d, int w, int O, int nblk) {
  const int nfu = (O + 3) >> 2, nwb = (nblk + 3) >> 2;
  return ((size_t)(m * nfu + (d >> 2)) * nwb + (w >> 2)) * 16 + (size_t)(w & 3) * 4 + (d & 3);
}
inline __host__ __device__ size_t sn_g1_elems(int nblk, int O) {
  return (size_t)2 * ((O + 3) >> 2) * ((nblk + 3) >> 2) * 16;
}

// Batched policy evaluation (csrc/eval.hip): E fresh envs, each from its reset to the end of its
// first episode.  The env state lives in LDS only; the launch writes ret / len and nothing else.
struct EvalArgs {
  int kind;            // 0 synthetic, 1 pendulum, 2 cart-pole (csrc/env_core.h)
  int E, O, A, S;      // envs, obs dims, act dims, state dims
  int limit;           // episode step limit (the launch's loop bound)
  int deterministic;   // 1: a = mu, 0: a = mu + sigma * eps (eps keyed: action key, env, step)
  uint32_t key_env, key_term, key_reset, key_action;
  PolicyNet net;
  // fixed observation normalisation
  const float* mean;     // [O]
  const float* inv_std;  // [O]
  // outputs, frozen at an env's first done
  float* ret;          // [E] sum of the unclipped rewards, added in step order
  int* len;            // [E] steps
  // (last) the policy head as RolloutArgs::dist; 1 with deterministic: the arg-max of the logits
  int dist;
};

// One policy step for caller-supplied observations (csrc/act.hip): E rows of raw fp32 observations
// -> normalise -> policy MLP -> keyed Gaussian sample -> log-prob.  Every output is optional (null:
// skipped); with none of actions / logp / mu the launch writes x_out / mom only (no MLP).
struct ActArgs {
  int E, O, A;         // rows, obs dims, act dims
  int deterministic;   // 1: a = mu (eps = 0), 0: a = mu + sigma * eps
  uint32_t key_action; // eps keyed (key_action, e_base + row, step_key)
  uint32_t e_base, step_key;
  PolicyNet net;
  // fixed observation normalisation
  const float* mean;     // [O]
  const float* inv_std;  // [O]
  const float* shift;    // [O] the moments' shift (read only with mom)
  const float* obs;      // [E][O] raw observations
  // outputs
  float* actions;      // [E][A]
  float* logp;         // [E]
  float* mu;           // [E][A]
  void* x_out;         // [E][d1] buffer precision (XStore<DT>), row-major: e.g. a slice of x_buf
  float* mom;          // [nblk][2][O] sum(obs - shift), sum((obs - shift)^2) per 16-row workgroup (RolloutArgs::mom)
  int mom_init;        // != 0: mom is overwritten, 0: added to
  // (last: every earlier member keeps its kernel-argument offset)
  // 0: the Gaussian head above.  1: a categorical head over A actions (csrc/policy_step.h categorical_row) — the
  // network's outputs are logits z; actions [E][A] gets the ONE-HOT row of the chosen action, the lowest k
  // attaining max_k(z_k + g_k), g Gumbel noise keyed (key_action, e_base + row, step_key, k) (deterministic:
  // g = 0, the arg-max); logp its log-softmax; mu the logits.  log_std must still be a valid [A] array: the launch's
  // setup loads it into the sigma table, which the categorical step then never reads.
  int dist;
};

// Episode bookkeeping of ONE step of a device-stepped tensor env (csrc/envstep.hip): what
// VecEnv.step does after the env's own dynamics, straight into the rollout buffer rows.  Per env
// e < E: el = ep_len + 1, er = ep_ret + reward, done = terminal || el >= limit; on done the env's
// 16-env tile gets (er, 1) and el = er = 0; state = done ? reset_state : new_state.
constexpr int ENVSTEP_TILE = 16;   // envs per epstat entry: the rollout kernel's tile (RolloutArgs::epstat)
struct EnvStepArgs {
  int E, S;            // envs, state dims
  int limit;           // episode step limit
  float reward_clip;   // > 0: rewards_row = clamp(reward, +-reward_clip); ep_ret takes the unclipped reward
  int init;            // != 0: epstat is overwritten, 0: added to (as ActArgs::mom_init)
  const float* reward;              // [E] unclipped
  const unsigned char* terminal;    // [E] 0 / 1
  const float* new_state;           // [E][S]
  const float* reset_state;         // [E][S]
  // in / out
  float* state;        // [E][S] (written only)
  int* ep_len;         // [E]
  float* ep_ret;       // [E]
  // outputs
  float* rewards_row;  // [E]
  float* dones_row;    // [E] 0.f / 1.f
  float* epstat;       // [ceil(E/16)][2] (finished-episode return sum, count) per tile
  // bootstrap_time_limit (all three or none; null: the kernel without them): an env that ended by
  // the step limit alone (done && !terminal) gets trunc_row = 1 (else 0) and its row of fin_src
  // copied to fin_dst
  const void* fin_src; // [E][fin_row_bytes] the step's final observation rows (buffer precision)
  void* fin_dst;       // [E][fin_row_bytes] the x_fin slot of this step
  float* trunc_row;    // [E] 0.f / 1.f
  int fin_row_bytes;   // bytes of one row (a multiple of 16)
};

// fp8 mode's gradient-amax ring (csrc/common.h Q8): [3 slots][4 tensors][Q8_SUB sub-slots][Q8_LINE]
constexpr int Q8_SUB = 64, Q8_LINE = 32;
constexpr int Q8_SLOT = 4 * Q8_SUB * Q8_LINE;   // dwords per ring slot

// The loss row: the first LS_FIXED columns of a partial row (MlpArgs::part) and the loss sums the
// gather kernels make of them — sums over the rows of the policy loss, the value loss, the entropy
// bonus, the approximate KL and the clip flag, then the row count; the rest stay 0.  The same order
// by name: runtime/metrics_layout.py LOSS_SLOTS.
enum LossSlot { LS_CLIP = 0, LS_VALUE, LS_ENT, LS_KL, LS_CLIPFRAC, LS_COUNT, LS_FIXED = 8 };
static_assert(LS_COUNT + 2 == LS_FIXED - 1, "the kernels zero the two unused slots LS_COUNT + 1 and LS_FIXED - 1");

struct MlpArgs {
  // input rows: x_buf row-major [*][d1]; row m of this call reads x_buf[idx ? idx[m] : row0 + m]
  const void* x_buf;
  const int* idx;
  int row0;
  int M;               // rows in this call (multiple of ROWS handled by masking)
  // packed weights (storage precision) + offsets (elements) of Wp / Wpt per layer
  const void* W;
  const void* W8;        // fp8 mode: the e4m3 image (the value head's fc1, csrc/mlp_head.hip F8)
  int off_w[6];        // p1 p2 p3 v1 v2 v3 (forward images)
  int off_wt[6];       // transposed images (dgrad)
  int d_in[6];         // padded input width per layer
  int d_out[6];        // padded output width per layer
  int n_out[6];        // real output width per layer
  float scale[6];      // fp8 dequant scale per layer
  const float* qscale; // optional device array of the 6 per-layer scales (overrides scale[])
  int A;
  const float* log_std;  // [A]
  const float* log_std_old;  // [A] dppo_ref: log_std of the previous step
  // ---- training inputs (indexed by source row) ----
  const float* actions;   // [N][A]
  const float* logp_old;  // [N]
  const float* adv;       // [N]
  const float* ret;       // [N]
  const float* v_old;     // [N]
  float* mu_prev;         // [N][A] dppo_ref: params of the previous step (read, then overwritten)
  float* v_prev;          // [N]
  int loss_kind;          // 0 ppo, 1 dppo_ref, 2 ppo with a categorical head (the tile kernel only: actions
                          // holds one-hot rows, the policy's outputs are logits, dL/dlog_std = 0)
  int value_loss;         // 0 mse, 1 clipped_half
  int std_var;
  float clip, ent_coeff;
  int first_step;         // dppo_ref: 1 -> old == current
  // ---- outputs ----
  float* v_out;           // value-only mode: [M] (written at position m)
  // transposed (feature-major) operands for the wgrad GEMM, [rows][ldT] storage precision
  void* xT; void* h1pT; void* h2pT; void* h1vT; void* h2vT;
  void* g1pT; void* g2pT; void* g3pT; void* g1vT; void* g2vT; void* g3vT;
  int ldT;                // = M (row length of every transposed buffer)
  int xT_ready;           // 1: xT already holds this call's rows (full-batch: the rollout wrote it)
  int x_stream;           // 1: non-temporal observation-row loads (A/B knob; 0 default: cached)
  int64_t x_bytes;        // bytes of x_buf (kernels with 32-bit buffer offsets refuse >= 2 GiB)
  float* part;            // [nblk][NPART] per-workgroup partial sums (loss terms: LossSlot below, dlog_std)
  int npart;
  int part_dw;            // per-head kernels: column of the fused narrow-layer weight gradient in a
                          // partial row (policy: dW_mu [32][128], value: dW_v [128]; bias = column 100)
  // fp8 mode's e4m3 wgrad operands (csrc/common.h Q8): null = the operands in the update's
  // precision.  Slots of the gradient-amax ring (4 tensors g1p, g2p, g1v, g2v x Q8_SUB sub-slots,
  // fp32 bits): the scales of this step come from q8_rd, its |g| maxima go to q8_acc, q8_clr is
  // zeroed
  const unsigned* q8_rd;
  unsigned* q8_acc;
  unsigned* q8_clr;
  // DIAGNOSTIC ONLY (scripts/phase_timeline.py; null in every real run): per-wave s_memtime
  // stamps at the phase boundaries of every tstamp_every-th workgroup, [blk][NW][16]
  unsigned long long* tstamp;
  int tstamp_every;
  // (last: every earlier member keeps its kernel-argument offset)
  // adv_norm_scope global | minibatch: [mean, inv, ..] fp32 on the device (csrc/advnorm.hip); the policy loss
  // reads a' = fl32(fl32(adv - mean) * inv) (common.h adv_norm_apply), adv itself stays raw.  null: off.
  // The value head and the forward mode ignore it.
  const float* adv_norm;
};

// per-head streaming update (csrc/mlp_head.hip): head 0 = policy, 1 = value; 128 rows per workgroup
extern "C" int mlp_head_applies(const MlpArgs& a);
extern "C" int mlp_head_rows();
extern "C" int mlp_head_waves(int head);
extern "C" void launch_mlp_head(int dt, int head, const MlpArgs& a, hipStream_t s);   // dt: bf16x3 or bf16
extern "C" void launch_mlp_head_value(int dt, const MlpArgs& a, hipStream_t s);   // V(x) on the value head kernel
extern "C" void set_head_kernels(int enable);
extern "C" int head_kernels_enabled();
// policy head update on 32x32x16 MFMAs, transposed chain (csrc/phead.hip): 128 rows per workgroup
extern "C" int phead_applies(const MlpArgs& a);   // set_phead flag and shapes
extern "C" int phead_shape_ok(const MlpArgs& a);
extern "C" int phead_rows();
// p2: p_fc2's weight gradient summed in the kernel (else h1p / g2p stored row-major for the wgrad)
extern "C" void launch_phead_train(int dt, const MlpArgs& a, int p2, hipStream_t s);
extern "C" void set_phead(int enable);

// fp8 mode: the Adam kernels also refresh the e4m3 image the update's fc1 reads (csrc/mlp_head.hip
// F8), element i as p / qs[lid[i]] with the iteration's per-layer scales; img == nullptr: off
struct F8Shadow {
  uint8_t* img;
  const int* lid;
  const float* qs;
};

#define DEV_HOST_INLINE __host__ __device__ inline

// The slab elements of a gather: up to 4 runs [lo, hi) of flat indices, every element with a slab
// source (src_meta != 0); start[r] = elements before run r (start[n..3] = INT_MAX), total = all.
// The gathers iterate over them without a data-dependent branch, so every per-element load of a
// thread issues in one round trip before its slab-chunk loads.
struct SlabRuns {
  int n, total;
  int lo[4], start[4];
  DEV_HOST_INLINE int flat(int j) const {
    int i = lo[0] + j;
#pragma unroll
    for (int r = 1; r < 4; ++r)
      if (j >= start[r]) i = lo[r] + (j - start[r]);
    return i;
  }
};

// The same slab elements by tile (docs/ARCHITECTURE.md §26): record u of t is the SLAB_TILE_INTS ints
//   [base, nch, stride, n0, k0, kq, fan_in, fan_out, w_off, b_off, nq, quad0]
// of one wgrad output tile: chunk c of its row-major [nq * 64][kq * 64] fp32 tile starts at slab + base +
// c * stride; dW[n][k] of the layer is flat element w_off + n * fan_in + k, its bias column k == fan_in is
// b_off + n (offsets into the gathered slice).  A quad is four consecutive k of one (tile, n) — one
// aligned 16-byte load per chunk; the tile owns quads [quad0, quad0 + rows * ceil(cols / 4)), rows =
// min(nq * 64, fan_out - n0), cols = min(kq * 64, fan_in + 1 - k0): the padded rows and columns of a
// tile are not read.  t null: the per-element form (src_off / src_meta).
constexpr int SLAB_TILE_INTS = 12;
constexpr int SLAB_TILES_MAX = 32;
// chunks per batch of the streaming sum (common.h slab_sum4: two batches in flight, 2 x 6 x 4 VGPRs).  6 and
// not 8: the tests want tiles of exactly one batch and of one batch + 1 chunks, and at their 34 64-row
// blocks a tile has ceil(34 / k) chunks — 6 and 7 exist, 8 does not (tests/test_gather_stream.py)
constexpr int SLAB_SUM_BATCH = 6;
struct SlabTiles {
  const int* t;
  int n, nquads;
};
DEV_HOST_INLINE int slab_tile_rows(const int* e) { return e[10] * 64 < e[7] - e[3] ? e[10] * 64 : e[7] - e[3]; }
DEV_HOST_INLINE int slab_tile_cols(const int* e) { return e[5] * 64 < e[6] + 1 - e[4] ? e[5] * 64 : e[6] + 1 - e[4]; }

// reduce items per block of the gather kernels (common.h item_reduce)
constexpr int ITEM_IPB = 32;
inline __host__ __device__ int item_blocks(int nitems) { return (nitems + ITEM_IPB - 1) / ITEM_IPB; }

// A gradient gather (csrc/wgrad.hip grad_gather_kernel, csrc/optim.hip gather_adam_kernel): the
// slab elements of `runs` as split-K slab sums (src_off / src_meta, indexed by flat element) and
// the reduce items as column sums of the npblk x npart per-workgroup partial rows.  The flat
// vectors may be one head's slice (red_dst then indexes the slice).
struct GatherArgs {
  const float* slab;
  const int* src_off;
  const int* src_meta;
  const float* part;
  int npblk, npart;
  const int* red_col;   // [nitems] partial-row column of each reduce item
  const int* red_dst;   // [nitems] its flat gradient index, or -1 - q for loss_out[q]
  int nitems;
  SlabRuns runs;
  float scale;
  float* loss_out;      // [8]
  SlabTiles tiles;      // (last) the runs' elements by tile: the streaming form; t null: per element
};

// One optimizer step over a flat range of n parameters (csrc/optim.hip): Adam, the global-norm clip
// (max_norm > 0) and the refresh of the weight images.
struct AdamArgs {
  float* p;
  float* g;             // the gradient (read; the fused gather + Adam launch writes it)
  float* m;
  float* v;
  int n;
  float lr, b1, b2, eps;
  float max_norm;       // <= 0: no clipping (launch_gather_adam: unread)
  int host_step;        // >= 1: this update's step number (eager launches); 0: the device counter state[1]
  float* state;         // [4] step counter, staged counter, gradient norm of the clip pass
  float* norm_part;     // [nblk] per-block sums of squares of the gradient; nblk is the grid
  int nblk;
  void* wimg;           // packed weight image in storage precision dt
  const int* w_map;     // [n] image index of each parameter (-1: none)
  const int* wt_map;    // [n] index in the transposed image (-1: none)
  int dt;
  const float* img_scale;   // optional [n] multiplier of the image values
  F8Shadow f8;
  // target_kl (docs/ARCHITECTURE.md §22): null is the ungated launch; else the gated form — gate
  // f32[4] = [stop, applied, trip_kl, last_kl] is read only, the step number is state[0] + 1 read on
  // the device (host_step unread), and the launch writes neither state[0] nor state[1]: launch_kl_gate
  // is the only writer of gate and, in gated mode, of both.  A stopped launch (gate[0] != 0) still
  // writes the gradient, the loss sums, norm_part and state[2]; p, m, v and the images stay.
  const float* gate;
  // lr_schedule adaptive (docs/ARCHITECTURE.md §23): null is the host rate lr; else the rate is
  // lr_state[0], read on the device by the gated form (lr unread).  Needs gate.
  const float* lr_dev;
};

// lr_schedule adaptive: the rate block of launch_kl_gate.  lr_state f32[4] = [lr, downs, ups, reserved]
// (the counts cumulative); null lr_state: no adaptation, the rest unread.  After an applied step,
// kl > 2 * kl_target: lr = max(lr / factor, lr_min); kl < kl_target / 2: lr = min(lr * factor, lr_max).
struct LrAdapt {
  float* lr_state;
  float kl_target, factor, lr_min, lr_max;
};

struct WgradTask {
  int layer;      // 0..5
  int n0, k0;     // output tile origin
  int m0, m1;     // reduction (batch) range
  int slab;       // slab offset (floats) of this task's [nq*64][kq*64] tile
  int nq, kq;     // tile extent in 64x64 quadrants (one per wave): nq*kq <= 8, nq + kq <= 6
};

struct WgradArgs {
  const void* gT[6];   // dY^T per layer  [rows >= n tile][ld]
  const void* xT[6];   // X^T per layer   [rows >= k tile][ld]
  int ld;
  const WgradTask* tasks;
  int ntasks;
  float* slab;
  // e4m3 operands (dt fp8, csrc/common.h Q8): the product tile of layer l is multiplied by
  // 1 / (2^q8_exp(max of tensor q8_t[l]'s sub-slots in q8_rd) * q8_xs[l]) — the gradient
  // tensor's delayed scale (the slot the update read) times the activation side's fixed scale
  const unsigned* q8_rd;
  int q8_t[6];
  float q8_xs[6];
  // row-major operands: the row length in elements of layer l's dY (g_rm) / X (x_rm) operand
  // ([ld rows][features]: csrc/phead.hip, x_buf), 0 = fragment-major
  int g_rm[6], x_rm[6];
  int wide;   // some task runs two quadrants per wave (wgrad_task_ok): the launch takes the wider LDS ring
};

extern "C" {
// first launch / attribute error recorded since the last call (0 = none), message into msg;
// resets the record (csrc/common.h dppo_note_error)
int dppo_take_error(char* msg, int cap);
void launch_debug_invalid(double* out, hipStream_t s);   // test hook: a launch the runtime refuses
void launch_rollout(int dt, const RolloutArgs& a, int rows, hipStream_t s);
void set_rollout_waves(int nw);                 // 4 or 8 waves per rollout workgroup (A/B)
int rollout_stepnorm_cap(int dt, const RolloutArgs& a, int rows);   // co-resident grid of the SN launch
void launch_eval(int dt, const EvalArgs& a, hipStream_t s);   // 16 envs per workgroup (csrc/eval.hip)
void launch_act(int dt, const ActArgs& a, hipStream_t s);     // 16 rows per workgroup (csrc/act.hip)
void launch_env_advance(const EnvStepArgs& a, hipStream_t s);   // 256 envs per workgroup (csrc/envstep.hip)
void launch_mlp_value(int dt, const MlpArgs& a, hipStream_t s);
void launch_mlp_train(int dt, const MlpArgs& a, hipStream_t s);
size_t mlp_train_lds_bytes(int dt, const MlpArgs& a);
int mlp_train_rows(int dt, const MlpArgs& a);   // row tile the launcher will use (LDS-fit)
void set_mlp_rows_override(int rows);           // 0 auto; 16/32/64 force (A/B diagnostics)
void set_s3_train_waves(int nw);                // split-bf16 32-row tile: 4 or 8 waves (A/B)
void set_s3_value_waves(int nw);                // split-bf16 value forward: 4 or 8 waves (A/B)
int mlp_train_waves(int dt, const MlpArgs& a);  // workgroup waves the launcher will use
void launch_wgrad(int dt, const WgradArgs& a, hipStream_t s);
int wgrad_task_ok(int dt, int nq, int kq);   // the (nq, kq) quadrant tiles the wgrad kernel runs
// grad[i] = scale * (slab sum | item column sum) for the gather's elements, loss_out from its items
void launch_grad_gather(const GatherArgs& ga, float* grad, hipStream_t s);
// boot: optional [T][E] value of a truncated step's final observation (null: the kernels without it)
// scale: optional device scalar (reward_norm: r' = clamp(fl32(r * scale), +-rclip), rclip <= 0: no clamp;
// null: the kernels without the reward scaling)
void launch_gae_rn(const float* rewards, const float* values, const float* dones, const float* boot,
                   const float* scale, float rclip, float* adv, float* ret, int T, int E, float gamma, float lam,
                   int mode, int seg, hipStream_t s);
// csrc/retnorm.hip: forward scan of the discounted return over [T][E] rewards / dones (acc [E] in place),
// s12 = the samples' (S1, S2) about shift[0]; mode as launch_gae_rn; R_out optional [T][E] (null: skipped);
// part: ret_scan_blocks(T, E, mode) x 2 doubles of scratch
int ret_scan_blocks(int T, int E, int mode);
void launch_ret_scan(const float* rewards, const float* dones, float* acc, const float* shift, float* R_out,
                     double* part, double* s12, int T, int E, float gamma, int mode, hipStream_t s);
// csrc/advnorm.hip: sums fp64[4] = [sum a, sum a^2, sum r, sum r^2] over rows idx ? idx[i] : i, i < n, of adv / ret
// [nrows] (ret null: its sums are 0; idx null: n <= nrows), in a fixed order; part: adv_stats_blocks(n) x 4 doubles
// of scratch; block (optional) fp32[4] = [mean, inv, std, explained variance] finished from the sums with the count
// n_total in the same two launches.  launch_adv_block: the finish alone (an all-reduce of the sums in between).
int adv_stats_blocks(int n);
void launch_adv_stats(const float* adv, const float* ret, const int* idx, int n, int nrows, double* part, double* sums,
                      double n_total, float* block, hipStream_t s);
void launch_adv_block(const double* sums, double n_total, float* block, hipStream_t s);
void set_adam_fused(int on);
// one launch without clipping when the step number is known (host_step > 0 or gated), else sumsq + adam
void launch_adam(const AdamArgs& a, hipStream_t s);
// grad_gather + no-clip Adam in one launch: world size 1 only (no all-reduce between them); a.nblk
// must exceed item_blocks(ga.nitems), and ungated it needs a.host_step >= 1
void launch_gather_adam(const GatherArgs& ga, const AdamArgs& a, hipStream_t s);
void set_gather_stream(int on);   // A/B switch: 0 runs the per-element form even with a tile table
int gather_stream_on();
// target_kl: the gate after a step (AdamArgs::gate); ra: the adaptive rate's block (null lr_state: none)
void launch_kl_gate(const float* loss_sums, float* gate, float* state, float target_kl, const LrAdapt& ra,
                    hipStream_t s);
void launch_pack(const float* p, int n, void* wimg, const int* w_map, const int* wt_map, int dt,
                 const float* img_scale, hipStream_t s);
// fp8 forward image: qscale[6] = per-layer amax / 416 of p (lid: layer of each parameter, -1
// none; must be < 6), then the e4m3 image of p / qscale[lid] (two launches; part: 128 x 6
// floats of per-block maxima)
void launch_fp8_refresh(const float* p, const int* lid, int n, float* qscale, float* part, void* wimg,
                        const int* w_map, const int* wt_map, hipStream_t s);
// ep == nullptr: the moments only (epstat unread)
void launch_obs_reduce(const float* part, int nblk, int O, double* s12, const float* epstat, double* ep,
                       hipStream_t s);
// [E][O] observations -> [obs_moments_blocks(E)][2][O] fp32 partials about shift
int obs_moments_blocks(int E);
void launch_obs_moments(const float* obs, int E, int O, const float* shift, float* part, hipStream_t s);
void launch_obs_merge(const double* s12, int O, double count, double n_a, const float* shift, double* mean,
                      double* m2, float* mean_f32, float* inv_std, double var_floor, hipStream_t s);
// out f64[11] = [episode return sum, count | 8 loss sums | gradient L2 norm from the nblk
// per-block sums of squares the last Adam launch left in norm_part]
void launch_metrics_pack(const double* ep, const float* loss8, const float* norm_part, int nblk, double* out,
                         hipStream_t s);
// diagnostics: nblk workgroups of nthreads (lds bytes each) spinning `us` microseconds each
void launch_probe_spin(int nblk, int nthreads, int lds, double us, int* sink, hipStream_t s);
}

// operand buffers (feature-major) are padded to multiples of 128 rows
#define WGRAD_TILE 128
#define WGRAD_TASK_INTS 8
static_assert(sizeof(WgradTask) == WGRAD_TASK_INTS * sizeof(int), "WgradTask is an 8-int record");
