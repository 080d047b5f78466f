// Fused rollout kernel (SURVEY K1+K2/K3+K4+K6+K7+K8+K15): one launch collects T steps.
//
// Each workgroup owns ROWS envs for the whole launch.  Per step, entirely on-chip:
//   obs (from the env state in LDS) -> running-stat moments (K2) -> normalise + clamp (K3)
//   -> policy MLP on MFMA (K4; activations stay in LDS, weights stream from L2)
//   -> Gaussian sample + log-prob with in-kernel counter RNG (K6-K8)
//   -> env physics + reward clip + done/reset (K1, K15)
// and writes the update inputs (normalised obs in the MFMA storage precision, action, logp,
// clipped reward, done) to the HBM-resident [T][E] buffer.  The value head is NOT evaluated
// here: V(s_t) for GAE is computed afterwards by one big batched forward over all (T+1)*E
// rows (mlp.hip), which is far more MFMA-efficient than T small ones.
//
// The policy step (normalise, MLP chain, keyed sample, log-prob, row store) is csrc/policy_step.h
// and the env physics csrc/env_core.h, both shared with csrc/eval.hip (and act.hip); this file
// keeps what is the rollout's own: the moments, the x^T groups, the [T][E] buffer stores, the
// episode bookkeeping and the per-step normalisation hand-offs.
//
// Reference: train.py:82-106 (one env, batch 1, python loop) and model.py:68-80.
#include "env_core.h"
#include "policy_step.h"

namespace {

// ---- per-step observation normalisation inside the launch (RolloutArgs sn_*) ----
// 8-byte {tag, fp32 bits} granules, stored and loaded relaxed at agent scope (sc1 vector accesses:
// MI355X_MICROARCH.md "granule"): the data is its own flag, so a hand-off needs no fence and no
// separate flag word.  Every spin is bounded: on a timeout the launch gives up (sn_err) instead of
// leaving waves that never finish.
typedef unsigned long long u64;
constexpr unsigned SN_SPIN_MAX = 1u << 21;   // >= ~1 s of polling per hand-off
constexpr int SN_MAX_BLOCKS = 256;           // grid cap of the per-step normalisation launch
DEV void sn_put(u64* g, unsigned tag, float v) {
  __hip_atomic_store(g, ((u64)tag << 32) | (u64)__float_as_uint(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
DEV u64 sn_get(const u64* g) {
  return __hip_atomic_load(const_cast<u64*>(g), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
DEV float sn_val(u64 x) { return __uint_as_float((unsigned)x); }

// Workgroup `blk`: the step's Chan merge of the 4-feature units u = blk, blk + nblk, ...
// sn_g1 is line-blocked (kernels.h sn_g1_index): a 128-byte line holds one moment of 4 features x
// 4 workgroups, so a publisher writes 2 O / 4 partial lines and a unit is 2 nblk / 4 lines.
// (One reducer wave per feature over a workgroup-major layout polled one line per workgroup —
// 512 per feature, shared with 15 other features' reducers — and took 3-8 us per hand-off at 256
// workgroups; the idle cross-XCD hop is 0.41 us, scripts/probes/xcd_latency.hip.)  All NW waves
// poll a unit: wave w moment w & 1, line rows 4 ((w >> 1) RL + i) + (l >> 4), i < RL; lane
// l holds granule l & 15 (workgroup offset (l >> 2) & 3, feature fi = l & 3) and sums its rows
// in fp64 in order, then an xor butterfly over the lanes of one fi (the same bits in every lane:
// a fixed order) leaves the wave's partial in lanes 0-3; wave 0 adds the NW / 2 parts of each
// moment (fixed order), merges into the running (mean, M2) — csrc/obs.hip obs_merge's formulas —
// and publishes the (mean, 1/std) granules.  The values of a poll pass whose tags all match are
// the values.  (pf: the first unit's running (mean, M2), loaded by wave 0's lanes 0-3 at the
// start of the step — off the hand-off's critical path.)  Returns false on a timeout (after the
// workgroup's barriers).  Measured per rollout at 4,096 envs (profiles/r5/filter_probe_*): one
// reducer wave per feature 0.50 ms; one workgroup per 16-feature line block 0.60 ms (4 us per poll
// pass of 512 lines); 4x4 lines on waves 0-3 0.449 ms; on all 8 waves 0.415 ms; 2 features x 8
// workgroups per line 0.425 ms — the pass time follows each wave's outstanding line loads.
template <int NW>
DEV bool sn_reduce(const RolloutArgs& a, int nblk, int step, int wave, int lane, const float* shs,
                   double* red, double pmean, double pm2, unsigned& npoll) {
  const int O = a.O, nfu = (O + 3) >> 2, nwb = (nblk + 3) >> 2;
  const unsigned tag = a.sn_epoch0 + (unsigned)step;
  const int gp = lane & 15, fi = lane & 3, wi = (lane >> 2) & 3, lq = lane >> 4;
  constexpr int RL = SN_MAX_BLOCKS / 4 / 4 / (NW / 2);   // line rows per lane (64 rows in NW / 2 parts)
  const int m = wave & 1, part = wave >> 1;
  bool fail = false;
  for (int u = (int)blockIdx.x; u < nfu; u += nblk) {
    const int d = 4 * u + fi;
    {
      const u64* g = a.sn_g1 + (size_t)(m * nfu + u) * nwb * 16 + gp;
      float v[RL];
      for (unsigned spins = 0;; ++spins) {
        bool ok = true;
#pragma unroll
        for (int i = 0; i < RL; ++i) {
          const int wb = lq + 4 * (RL * part + i);
          v[i] = 0.f;
          if (wb < nwb && 4 * wb + wi < nblk && d < O) {
            const u64 x = sn_get(g + (size_t)wb * 16);
            ok &= (unsigned)(x >> 32) == tag;
            v[i] = sn_val(x);
          }
        }
        npoll = spins + 1;
        if (__all(ok)) break;
        if (spins > SN_SPIN_MAX) { fail = true; break; }
        if (spins > 8) __builtin_amdgcn_s_sleep(1);
      }
      double p = 0.0;
#pragma unroll
      for (int i = 0; i < RL; ++i) p += (double)v[i];
#pragma unroll
      for (int x = 4; x < 64; x <<= 1) p += __shfl_xor(p, x);
      if (lane < 4) red[4 * wave + lane] = p;
    }
    __syncthreads();
    if (wave == 0 && lane < 4 && d < O) {
      double p1 = 0.0, p2 = 0.0;
#pragma unroll
      for (int q = 0; q < NW / 2; ++q) {
        p1 += red[8 * q + lane];
        p2 += red[8 * q + 4 + lane];
      }
      const bool pf = u == (int)blockIdx.x;
      const double count = (double)a.E, n_a = a.sn_n0 + (double)step * count;
      const double bmean_d = p1 / count;
      const double bmean = (double)shs[d] + bmean_d;
      double bm2 = p2 - p1 * bmean_d;
      if (bm2 < 0.0) bm2 = 0.0;
      const double n = n_a + count;
      const double mean0 = pf ? pmean : a.sn_mean[d];
      const double delta = bmean - mean0;
      const double mu = mean0 + delta * (count / n);
      const double M2 = (pf ? pm2 : a.sn_m2[d]) + bm2 + delta * delta * (n_a * count / n);
      double var = M2 / n;
      if (var < a.sn_var_floor) var = a.sn_var_floor;
      const float muf = (float)mu, inv = (float)(1.0 / sqrt(var));
      a.sn_mean[d] = mu;
      a.sn_m2[d] = M2;
      a.sn_mean_f32[d] = muf;
      a.sn_inv_std[d] = inv;
      sn_put(a.sn_g2 + d, tag, muf);
      sn_put(a.sn_g2 + O + d, tag, inv);
    }
    if (u + nblk < nfu) __syncthreads();   // (red is reused by the next unit)
  }
  return !fail;
}

// Every wave: gather its share of the step's (mean, 1/std) granules into LDS (granules tid,
// tid + NTHR, ... of the 2 O; the values of the poll pass whose tags all match; O <= SN_MAX_O)
constexpr int SN_MAX_O = 384;
template <int NTHR>
DEV bool sn_gather(const RolloutArgs& a, int step, int tid, float* nm, float* ninv, unsigned& npoll) {
  constexpr int GU = (2 * SN_MAX_O + NTHR - 1) / NTHR;
  const int O = a.O;
  const unsigned tag = a.sn_epoch0 + (unsigned)step;
  float v[GU];
  for (unsigned spins = 0;; ++spins) {
    bool ok = true;
#pragma unroll
    for (int u = 0; u < GU; ++u) {
      const int i = tid + NTHR * u;
      if (i < 2 * O) {
        const u64 x = sn_get(a.sn_g2 + i);
        ok &= (unsigned)(x >> 32) == tag;
        v[u] = sn_val(x);
      }
    }
    npoll = spins + 1;
    if (__all(ok)) break;
    if (spins > SN_SPIN_MAX) return false;
    if (spins > 8) __builtin_amdgcn_s_sleep(1);
  }
#pragma unroll
  for (int u = 0; u < GU; ++u) {
    const int i = tid + NTHR * u;
    if (i < O) nm[i] = v[u];
    else if (i < 2 * O) ninv[i - O] = v[u];
  }
  return true;
}

// The launch's dynamic LDS: the kernel's pointers and the host's byte count (null smem: measuring)
// come from this one carve.  SN: the per-step normalisation's extra pieces.
template <int DT, int ROWS, bool SN>
struct RolloutLds {
  using XB = typename Prec<XStore<DT>::DTX>::T;   // buffer precision (bf16 when DT is fp8)
  LdsCarve cv;
  const int O, A, S;
  float* st = cv.take<float>(ROWS * S);           // env state
  PolicyTiles<DT> t;
  float* act = cv.take<float>(ROWS * A);          // the step's actions and their noise
  float* epsb = cv.take<float>(ROWS * A);
  float* s1 = cv.take<float>(O);                  // the launch's moments about the shift
  float* s2 = cv.take<float>(O);
  float* done_s = cv.take<float>(ROWS);
  int* eplen = cv.take<int>(ROWS);
  float* epret = cv.take<float>(ROWS);
  float* epacc = cv.take<float>(2 * ROWS);
  uint32_t* kes = cv.take<uint32_t>(3 * ROWS);    // per-env key prefixes of this step: action, env, reset
  float* wdrv = cv.take<float>(S);                // synthetic dynamics tables (env_core.h syn_tables)
  int* jdx = cv.take<int>(S);
  float* lsg = cv.take<float>(2 * A);             // [log sigma | sigma]
  // SN: the iteration shift and this step's (mean, 1/std) of every feature; the timeout flag;
  // the reduce's per-wave partials
  float* shs = SN ? cv.take<float>(O) : nullptr;
  float* nm = SN ? cv.take<float>(O) : nullptr;
  float* ninv = SN ? cv.take<float>(O) : nullptr;
  int* sn_fail = SN ? cv.take<int>(1) : nullptr;
  double* sn_red = SN ? cv.take<double>(32) : nullptr;
  XB* xsb;   // fp8: bf16 staging tile of the buffer rows (policy_step.h store_tile_rows)
  __host__ __device__ RolloutLds(char* smem, const RolloutArgs& a)
      : cv(smem), O(a.O), A(a.A), S(a.S), t(cv, a.net, ROWS, a.A),
        xsb(DT == DT_FP8 ? cv.take<XB>(ROWS * a.net.d1) : nullptr) {}
};

// NW waves per workgroup: a 16-env tile is one workgroup per CU at E = 4096, so the 8-wave
// form (2 waves per SIMD) doubles the threads of the VALU-heavy observe / sample / env phases
// and gives the SIMDs a second wave to hide latency with; the MFMA layers use the first waves.
// SN: per-step observation normalisation inside the launch (RolloutArgs sn_*; cooperative launch)
// FIN: bootstrap_time_limit (RolloutArgs trunc / x_fin): step (d) marks the rows that ended by the
// step limit alone, step (e) takes a cold branch for a tile that has one.  A template parameter so
// that the forms without it keep their instructions and registers; never together with SN.
// CAT: the categorical head (RolloutArgs::dist 1) on the cart-pole's physics — phases (c) and (d) are one
// per-env phase (policy_step.h categorical_row), one barrier per step fewer.  A template parameter for FIN's
// reason, and the env kind is then a constant: the forms with it hold no other env's code.  Never with SN.
template <int DT, int ROWS, int NW, bool SN, bool FIN, bool CAT = false>
__global__ __launch_bounds__(NW * 64) void rollout_kernel(RolloutArgs a) {
  using P = Prec<DT>;
  using T = typename P::T;
  constexpr int NTHR = 64 * NW;
  static_assert(ROWS % 4 == 0 && NTHR % ROWS == 0 && (NTHR / ROWS) <= 64, "rollout tiling");
  static_assert(!SN || NW >= 4, "the per-step filter's reduce polls with waves 0-3");
  static_assert(!(SN && FIN), "the final rows are normalised with the launch's fixed statistics");
  static_assert(!(SN && CAT), "the categorical head is not built into the per-step filter's forms");
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int e0 = blockIdx.x * ROWS;
  const int nvalid = min(ROWS, a.E - e0);
  const int O = a.O, A = a.A, S = a.S, d1 = a.net.d1;
  const int kind = CAT ? KIND_CARTPOLE : a.kind;

  extern __shared__ __attribute__((aligned(16))) char smem[];
  const RolloutLds<DT, ROWS, SN> L(smem, a);
  PolicyStep<DT, ROWS, NW> ps(a.net, L.t);
  const int ld1 = L.t.ld1;
  using PX = Prec<XStore<DT>::DTX>;
  constexpr bool STAGE = DT == DT_FP8;
  typename PX::T* xo = reinterpret_cast<typename PX::T*>(a.x_out);

  // ---- load state, zero the padded activation tiles (pad columns stay constant) ----
  for (int i = tid; i < ROWS * S; i += NTHR) {
    int r = i / S, d = i - r * S;
    L.st[i] = (r < nvalid) ? a.state[(size_t)(e0 + r) * S + d] : 0.f;
  }
  for (int d = tid; d < O; d += NTHR) { L.s1[d] = 0.f; L.s2[d] = 0.f; }
  if constexpr (SN) {
    for (int d = tid; d < O; d += NTHR) L.shs[d] = a.shift[d];
    if (tid == 0) *L.sn_fail = 0;
  }
  syn_tables(L.wdrv, L.jdx, S, A, tid, NTHR);
  ps.setup(L.lsg, tid);
  if (tid < ROWS) {
    int e = e0 + tid;
    L.eplen[tid] = (tid < nvalid) ? a.ep_len[e] : 0;
    L.epret[tid] = (tid < nvalid) ? a.ep_ret[e] : 0.f;
    L.epacc[2 * tid] = 0.f;
    L.epacc[2 * tid + 1] = 0.f;
  }
  __syncthreads();

  // normalisation constants of this thread's first feature: fixed for the whole launch, so
  // loaded once instead of once per step (the compiler cannot hoist them past the stores)
  float hm = 0.f, his = 1.f, hsh = 0.f;
  if (tid < O) { hm = a.mean[tid]; his = a.inv_std[tid]; hsh = a.shift[tid]; }
  constexpr bool SPLIT = IsSplit<DT>::value;
  // the buffer rows leave from the LDS tile (store_tile_rows) unless the tile's element type is
  // not the buffer's
  constexpr bool XO_FROM_LDS = std::is_same_v<T, typename PX::T> || SPLIT || STAGE;
  // the observe loop keeps this feature's ROWS values in the buffer type, or as fp32 for split
  // storage (split once, at the 32-byte x^T group store)
  using GT = std::conditional_t<SPLIT, float, typename PX::T>;
  // phase timeline (diagnostics, a.tstamp != null): per-wave shader-clock cycles summed over
  // the steps for each phase, written by lane 0 of every wave of every workgroup
  // (slots 7-10: the per-step filter's moments / reduce / gather / barrier, SN only)
  // (slots 11-14: absolute s_memrealtime of step 8's filter entry / moments published / reduce
  // done / gather done — the cross-workgroup skew of the hand-offs)
  // (slot 15: step 8's poll passes, gather << 32 | reduce)
  unsigned long long ph_acc[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  unsigned long long ph_t = a.tstamp ? __builtin_amdgcn_s_memtime() : 0ull;
#define PH(i)                                                     \
  do {                                                            \
    if (a.tstamp != nullptr) {                                    \
      const unsigned long long t_ = __builtin_amdgcn_s_memtime(); \
      ph_acc[i] += t_ - ph_t;                                     \
      ph_t = t_;                                                  \
    }                                                             \
  } while (0)
#define PH_ABS(i)                                                                  \
  do {                                                                             \
    if (a.tstamp != nullptr && step == 8) ph_acc[i] = __builtin_amdgcn_s_memrealtime(); \
  } while (0)
  for (int step = 0; step <= a.T; ++step) {
    const int tb = a.t_base + step;
    const bool last = (step == a.T);  // bootstrap observation only
    // ---- (a) observe, moments, normalise -> LDS tile + global buffer row ----
    auto observe = [&](auto kind_tag) {
      constexpr int KIND = decltype(kind_tag)::value;
      for (int d = tid; d < d1; d += NTHR) {
        float m = hm, is = his, sh = hsh;
        if constexpr (SN) {
          if (d < O) { m = L.nm[d]; is = L.ninv[d]; }
        } else {
          if (d != tid && d < O) { m = a.mean[d]; is = a.inv_std[d]; sh = a.shift[d]; }
        }
        float ls1 = 0.f, ls2 = 0.f;
        GT grp[ROWS];   // this feature's ROWS consecutive buffer rows (xT groups of 8)
#pragma unroll
        for (int r = 0; r < ROWS; ++r) {
          float xv;
          if (d < O) {
            float o = env_obs<KIND>(L.st, S, r, d);
            if (!SN && !last && r < nvalid) { float dd = o - sh; ls1 += dd; ls2 += dd * dd; }
            xv = norm_clamp(o, m, is);
          } else {
            xv = pad_col(d, O);
          }
          P::put(L.t.xs, r * ld1 + d, xv);
          if constexpr (SPLIT) grp[r] = xv;
          else grp[r] = PX::cvt(xv);
          if constexpr (STAGE) L.xsb[r * d1 + d] = grp[r];
        }
        if (!SN && d < O) { L.s1[d] += ls1; L.s2[d] += ls2; }
        // full-batch update operand: rows m = tb*E + e0 + r are contiguous 8-groups of the FM
        // layout (host guarantees E % 16 == 0), written once per rollout instead of per epoch
        if (a.xT_out != nullptr && !last) {
          typename PX::T* xT = reinterpret_cast<typename PX::T*>(a.xT_out);
          const int mrow = tb * a.buf_E + e0;
#pragma unroll
          for (int g = 0; g < ROWS / 8; ++g) {
            typename PX::T* o = xT + fm_index(d, mrow + 8 * g, a.ldT);
            if constexpr (SPLIT) {
              bf16x8 hv, lv;
#pragma unroll
              for (int j = 0; j < 8; ++j) {
                __bf16 h, l;
                Prec<DT_S3>::split(grp[8 * g + j], h, l);
                hv[j] = h;
                lv[j] = l;
              }
              uint4* o4 = reinterpret_cast<uint4*>(o);
              o4[0] = *reinterpret_cast<const uint4*>(&hv);
              o4[1] = *reinterpret_cast<const uint4*>(&lv);
            } else if constexpr (sizeof(typename PX::T) == 2) {
              *reinterpret_cast<uint4*>(o) = *reinterpret_cast<const uint4*>(&grp[8 * g]);
            } else {
              reinterpret_cast<uint4*>(o)[0] = reinterpret_cast<const uint4*>(&grp[8 * g])[0];
              reinterpret_cast<uint4*>(o)[1] = reinterpret_cast<const uint4*>(&grp[8 * g])[1];
            }
          }
        }
      }
    };
    if constexpr (SN) {
      if (!last) {
        // this step's batch moments about the iteration shift -> the iteration's moments (as in
        // rollout mode) and this workgroup's granules; its waves merge the features it owns
        // (sn_reduce), every wave gathers its share of the new stats of every feature (sn_gather)
        const unsigned tag = a.sn_epoch0 + (unsigned)step;
        auto moments = [&](auto kind_tag) {
          constexpr int KIND = decltype(kind_tag)::value;
          for (int d = tid; d < O; d += NTHR) {
            const float sh = L.shs[d];
            float ls1 = 0.f, ls2 = 0.f;
            // every row read unconditionally (st holds ROWS rows), the invalid ones masked: a
            // per-row branch kept the compiler from batching the LDS reads (one round trip each)
#pragma unroll
            for (int r = 0; r < ROWS; ++r) {
              const float o = env_obs<KIND>(L.st, S, r, d);
              const float dd = r < nvalid ? o - sh : 0.f;
              ls1 += dd;
              ls2 += dd * dd;
            }
            L.s1[d] += ls1;
            L.s2[d] += ls2;
            sn_put(a.sn_g1 + sn_g1_index(0, d, (int)blockIdx.x, O, (int)gridDim.x), tag, ls1);
            sn_put(a.sn_g1 + sn_g1_index(1, d, (int)blockIdx.x, O, (int)gridDim.x), tag, ls2);
          }
        };
        // the running (mean, M2) of this workgroup's first unit (4 features), loaded now:
        // consumed after the hand-off (wave 0, lanes 0-3)
        const int dfirst = 4 * (int)blockIdx.x + lane;
        double pmean = 0.0, pm2 = 0.0;
        if (wave == 0 && lane < 4 && dfirst < O) {
          pmean = a.sn_mean[dfirst];
          pm2 = a.sn_m2[dfirst];
        }
        PH_ABS(11);
        env_kind_switch(a.kind, moments);
        PH(7);
        PH_ABS(12);
        unsigned npr = 0, npg = 0;
        if (!sn_reduce<NW>(a, (int)gridDim.x, step, wave, lane, L.shs, L.sn_red, pmean, pm2, npr) && lane == 0)
          *L.sn_fail = 1;
        PH(8);
        PH_ABS(13);
        // the gather polls start once this workgroup's reducers are done: polling from the
        // other waves during the reduce queued ahead of the reducers' own loads on the CU
        __syncthreads();
        if (!sn_gather<NTHR>(a, step, tid, L.nm, L.ninv, npg) && lane == 0) *L.sn_fail = 1;
        PH(9);
        PH_ABS(14);
        if (a.tstamp != nullptr && step == 8) ph_acc[15] = ((unsigned long long)npg << 32) | npr;
        __syncthreads();
        PH(10);
        if (*L.sn_fail) {   // a peer never published: give up (the host raises)
          if (tid == 0) __hip_atomic_store(a.sn_err, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          return;
        }
      }
    }
    env_kind_switch(kind, observe);
    if (!last) ps.prefetch(wave, lane);
    __syncthreads();
    if constexpr (XO_FROM_LDS)
      store_tile_rows<DT, NTHR>(xo + ((size_t)tb * a.buf_E + e0) * d1, L.t, L.xsb, d1, nvalid, tid);
    if (last) break;
    // the key prefixes of the sample / env phases: hashed before fc1, so the layers' barriers
    // publish them and the sample phase needs no barrier of its own (the previous step's env
    // phase, their last reader, ended in a barrier)
    const uint32_t kstep = a.t0 + (uint32_t)step;
    key_prefixes<ROWS, NTHR>(L.kes, {a.key_action, a.key_env, a.key_reset}, (uint32_t)e0, kstep, tid);
    PH(0);   // (a) observe -> after its barrier
    // ---- (b) policy MLP: PH(1..3) = fc1, fc2, fc3 (each incl. barrier) ----
    ps.layers(wave, lane, [&](auto l) { PH(decltype(l)::value); });
    // ---- (c) sample a = mu + sigma * eps ----
    if constexpr (!CAT) {
      sample_loop<ROWS, NTHR>(L.kes, A, tid, true, [&](int r, int j, float eps) {
        const float av = L.t.mu[r * A + j] + L.lsg[A + j] * eps;
        L.act[r * A + j] = av;
        L.epsb[r * A + j] = eps;
        if (r < nvalid) a.actions[((size_t)tb * a.buf_E + e0 + r) * A + j] = av;
      });
      __syncthreads();
      PH(4);   // (c) sample
    }
    // ---- (d) per-env: logp, reward, termination, episode bookkeeping ----
    // LPE lanes per env (contiguous inside a wave) share the per-dim sums, then reduce by shuffles
    {
      constexpr int LPE = NTHR / ROWS;
      const int r = tid / LPE, l = tid - r * LPE;
      const int e = e0 + r;
      float lp = 0.f, err = 0.f;
      const int na = min(A, O);
      if constexpr (CAT) {
        // (c') + (d): mu holds the row's A logits, published by fc3's barrier like the key prefixes — no sample
        // loop, no noise tile, no barrier of its own.  Every lane of every wave is here (the row step shuffles).
        const CatRow c = categorical_row<LPE>(L.t.mu + r * A, A, l, L.kes[r], true);
        if (r < nvalid) {
          float* arow = a.actions + ((size_t)tb * a.buf_E + e) * A;
          for (int k = l; k < A; k += LPE) arow[k] = (k == c.a) ? 1.f : 0.f;   // the one-hot row
        }
        lp = c.logp;
        // the push CartPoleEnv._dynamics feeds its parent: 2 a - 1, exactly +-1 for the two actions.  This lane
        // is the slot's only reader (env_reward below; the cart-pole's transition reads no action).
        if (l == 0) L.act[r] = 2.f * (float)c.a - 1.f;
      } else {
        for (int j = l; j < A; j += LPE) {
          lp += logp_term(L.epsb[r * A + j], L.lsg[j]);
          if (a.kind == 0 && j < na) err += syn_err_term(L.act[r * A + j], L.st[r * S + j]);
        }
#pragma unroll
        for (int o = LPE / 2; o > 0; o >>= 1) {
          lp += __shfl_xor(lp, o, LPE);
          err += __shfl_xor(err, o, LPE);
        }
      }
      if (l == 0) {
        if constexpr (!CAT) lp -= logp_const(A);
        bool term;
        // (CAT: the push row [ROWS][1])
        const float rew = env_reward(kind, L.st, S, L.act, CAT ? 1 : A, r, err, na, a.key_term, (uint32_t)e, kstep, term);
        int el = L.eplen[r] + 1;
        float er_ = L.epret[r] + rew;
        bool done = term || (el >= a.limit);
        if (done) {
          if (r < nvalid) { L.epacc[2 * r] += er_; L.epacc[2 * r + 1] += 1.f; }
          el = 0;
          er_ = 0.f;
        }
        L.eplen[r] = el;
        L.epret[r] = er_;
        // FIN: done_s 2 marks a truncated row (terminal wins; the pad rows of the last tile never)
        const bool tr = FIN && done && !term && r < nvalid;
        L.done_s[r] = done ? (tr ? 2.f : 1.f) : 0.f;
        if (r < nvalid) {
          size_t o = (size_t)tb * a.buf_E + e;
          if constexpr (FIN) a.trunc[o] = tr ? 1.f : 0.f;
          float rc = rew;
          if (a.reward_clip > 0.f) rc = fminf(fmaxf(rc, -a.reward_clip), a.reward_clip);
          a.logp[o] = lp;
          a.rewards[o] = rc;
          a.dones[o] = done ? 1.f : 0.f;
        }
      }
    }
    __syncthreads();
    PH(5);   // (d) logp / reward
    // ---- (e) state transition (+ in-place reset on done) ----
    bool anyt = false;   // workgroup-uniform: every thread reads the same ROWS flags
    if constexpr (FIN) {
#pragma unroll
      for (int r = 0; r < ROWS; ++r) anyt |= L.done_s[r] > 1.5f;
    }
    // cold (anyt): some row of the tile is truncated.  Its final observation is of the state the
    // env reached, which the transition would replace by the reset: the truncated rows are stepped
    // as not done (flag -1), their normalised rows go to x_fin, then exactly those rows are reset.
    // The resets depend only on (reset key, env, step): st ends up the same bits either way, and
    // the transition is the one call for both paths.
    if (anyt) {
      __syncthreads();   // (every thread has read the flags)
      if (tid < ROWS && L.done_s[tid] > 1.5f) L.done_s[tid] = -1.f;
      __syncthreads();
    }
    env_transition<ROWS, NTHR>(kind, L.st, S, L.act, A, L.done_s, L.kes, L.wdrv, L.jdx, a.key_reset, e0, kstep, tid);
    if (anyt) {
      __syncthreads();
      // the rows as step (a) makes them, through the input tile (free until the next observe):
      // same norm_clamp / pad_col / storage conversion, so the 16-byte row stores are step (a)'s too
      auto final_rows = [&](auto kind_tag) {
        constexpr int KIND = decltype(kind_tag)::value;
        for (int i = tid; i < ROWS * d1; i += NTHR) {
          const int r = i / d1, d = i - r * d1;
          if (L.done_s[r] < -0.5f) {
            const float xv = d < O ? norm_clamp(env_obs<KIND>(L.st, S, r, d), a.mean[d], a.inv_std[d]) : pad_col(d, O);
            P::put(L.t.xs, r * ld1 + d, xv);
            if constexpr (STAGE) L.xsb[r * d1 + d] = PX::cvt(xv);
          }
        }
      };
      env_kind_switch(kind, final_rows);
      __syncthreads();
      const int slot = tb / a.limit;
      if (slot < a.fin_K) {
        typename PX::T* xf = reinterpret_cast<typename PX::T*>(a.x_fin) + ((size_t)slot * a.E + e0) * d1;
        constexpr int EPC = 16 / sizeof(typename PX::T);
        const int ch = d1 / EPC;
        for (int i = tid; i < nvalid * ch; i += NTHR) {
          const int r = i / ch, c = i - r * ch;
          if (L.done_s[r] < -0.5f) {
            const void* src = STAGE ? static_cast<const void*>(L.xsb + r * d1 + c * EPC)
                                    : static_cast<const void*>(L.t.xs + r * ld1 + c * EPC);
            *reinterpret_cast<uint4*>(xf + (size_t)r * d1 + c * EPC) = *reinterpret_cast<const uint4*>(src);
          }
        }
      }
      env_reset_rows<ROWS, NTHR>(kind, L.st, S, L.done_s, L.kes, a.key_reset, e0, kstep, tid);
    }
    __syncthreads();
    PH(6);   // (e) env transition
  }
  __syncthreads();
  if (a.tstamp != nullptr && lane == 0) {
#pragma unroll
    for (int i = 0; i < 16; ++i) a.tstamp[((size_t)blockIdx.x * NW + wave) * 16 + i] = ph_acc[i];
  }
#undef PH
#undef PH_ABS
  // ---- write back env state, episode trackers, partial moments / episode stats ----
  for (int i = tid; i < nvalid * S; i += NTHR) a.state[(size_t)e0 * S + i] = L.st[i];
  if (tid < nvalid) {
    a.ep_len[e0 + tid] = L.eplen[tid];
    a.ep_ret[e0 + tid] = L.epret[tid];
  }
  float* mom = a.mom + (size_t)blockIdx.x * 2 * O;
  for (int d = tid; d < O; d += NTHR) { mom[d] = L.s1[d]; mom[O + d] = L.s2[d]; }
  if (tid == 0) {
    float sr = 0.f, sc = 0.f;
    for (int r = 0; r < ROWS; ++r) { sr += L.epacc[2 * r]; sc += L.epacc[2 * r + 1]; }
    a.epstat[2 * blockIdx.x] = sr;
    a.epstat[2 * blockIdx.x + 1] = sc;
  }
}

int g_rollout_waves = 8;   // 4 or 8 (set_rollout_waves: A/B diagnostics)

// f(DT, ROWS, NW as integral_constants) for the form a launch takes.  16-row bf16x3 / bf16 / fp8
// tiles run 8 waves unless set_rollout_waves(4); the other forms exist with 4 waves only.
template <typename F>
auto dispatch_form(int dt, int rows, F&& f) {
  return dispatch_dt(dt, [&](auto d) {
    auto go = [&](auto r) {
      using W4 = std::integral_constant<int, 4>;
      if constexpr (POLICY_WAVES<decltype(d)::value, decltype(r)::value> == 8) {
        if (g_rollout_waves != 4) return f(d, r, std::integral_constant<int, 8>{});
      }
      return f(d, r, W4{});
    };
    return rows == 32 ? go(std::integral_constant<int, 32>{}) : go(std::integral_constant<int, 16>{});
  });
}

// the launch's dynamic-LDS bytes (and the kernel's attribute for them)
template <int DT, int ROWS, int NW, bool SN, bool FIN = false>
size_t launch_lds(const RolloutArgs& a) {
  const size_t lds = RolloutLds<DT, ROWS, SN>(nullptr, a).cv.off;
  if (lds > 65536) set_max_lds_once<rollout_kernel<DT, ROWS, NW, SN, FIN>>(lds);
  return lds;
}

// Per-step normalisation: every workgroup must be resident at once (the hand-offs wait on all
// of them), so the launch is cooperative (the runtime refuses a grid that cannot be co-resident)
// and its grid is also kept one workgroup per CU below the occupancy answer (MI355X_MICROARCH.md:
// the API can overstate residency by one per CU).  cap: the largest grid the launch accepts
// (0: none; the gather holds 2 O granules in registers).
template <int DT, int ROWS, int NW>
hipError_t stepnorm_cap(const RolloutArgs& a, size_t lds, int& cap) {
  int per_cu = 0, dev = 0, ncu = 0;
  hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(
      &per_cu, reinterpret_cast<const void*>(rollout_kernel<DT, ROWS, NW, true, false>), NW * 64, lds);
  if (e == hipSuccess) e = hipGetDevice(&dev);
  if (e == hipSuccess) e = hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev);
  cap = ncu * (per_cu > 1 ? per_cu - 1 : per_cu);
  if (cap > SN_MAX_BLOCKS) cap = SN_MAX_BLOCKS;
  if (e != hipSuccess || a.O > SN_MAX_O) cap = 0;
  return e;
}

template <int DT, int ROWS, int NW>
void launch(const RolloutArgs& a, hipStream_t s) {
  const int nblk = (a.E + ROWS - 1) / ROWS;
  if (a.sn_g1 == nullptr) {
    if (a.x_fin != nullptr) {
      const size_t lds = launch_lds<DT, ROWS, NW, false, true>(a);
      hipLaunchKernelGGL((rollout_kernel<DT, ROWS, NW, false, true>), dim3(nblk), dim3(NW * 64), lds, s, a);
    } else {
      const size_t lds = launch_lds<DT, ROWS, NW, false>(a);
      hipLaunchKernelGGL((rollout_kernel<DT, ROWS, NW, false, false>), dim3(nblk), dim3(NW * 64), lds, s, a);
    }
    HIP_CHECK_LAUNCH();
    return;
  }
  if (a.x_fin != nullptr) {   // (the binding refuses it first: the final rows take fixed statistics)
    dppo_note_error(hipErrorInvalidValue, __FILE__, __LINE__);
    return;
  }
  const size_t lds = launch_lds<DT, ROWS, NW, true>(a);
  int cap = 0;
  hipError_t e = stepnorm_cap<DT, ROWS, NW>(a, lds, cap);
  if (e == hipSuccess && nblk > cap) e = hipErrorCooperativeLaunchTooLarge;
  if (e != hipSuccess) {
    dppo_note_error(e, __FILE__, __LINE__);
    return;
  }
  RolloutArgs aa = a;
  void* args[] = {&aa};
  e = hipLaunchCooperativeKernel(reinterpret_cast<const void*>(rollout_kernel<DT, ROWS, NW, true, false>), dim3(nblk),
                                 dim3(NW * 64), args, (unsigned)lds, s);
  if (e != hipSuccess) dppo_note_error(e, __FILE__, __LINE__);
}

// RolloutArgs::dist 1: the categorical forms exist for 16-row tiles at fp32 / bf16x3 / bf16, in the
// precision's default wave count (set_rollout_waves is the Gaussian forms' A/B switch), with FIN on
// and off; anything else is the binding's to refuse, and an error here
void launch_categorical(int dt, const RolloutArgs& a, int rows, hipStream_t s) {
  if (rows != 16 || dt == DT_FP8 || a.sn_g1 != nullptr || a.kind != KIND_CARTPOLE) {
    dppo_note_error(hipErrorInvalidValue, __FILE__, __LINE__);
    return;
  }
  dispatch_dt(dt, [&](auto d) {
    constexpr int DT = decltype(d)::value, ROWS = 16, NW = POLICY_WAVES<DT, ROWS>;
    if constexpr (DT != DT_FP8) {
      const int nblk = (a.E + ROWS - 1) / ROWS;
      const size_t lds = RolloutLds<DT, ROWS, false>(nullptr, a).cv.off;
      auto go = [&](auto fin) {
        constexpr bool FIN = decltype(fin)::value;
        if (lds > 65536) set_max_lds_once<rollout_kernel<DT, ROWS, NW, false, FIN, true>>(lds);
        hipLaunchKernelGGL((rollout_kernel<DT, ROWS, NW, false, FIN, true>), dim3(nblk), dim3(NW * 64), lds, s, a);
      };
      if (a.x_fin != nullptr) go(std::true_type{});
      else go(std::false_type{});
      HIP_CHECK_LAUNCH();
    }
  });
}

}  // namespace

extern "C" void set_rollout_waves(int nw) { g_rollout_waves = nw; }

// workgroups the per-step normalisation launch can hold co-resident (its grid must not exceed it)
extern "C" int rollout_stepnorm_cap(int dt, const RolloutArgs& a, int rows) {
  return dispatch_form(dt, rows, [&](auto d, auto r, auto w) {
    constexpr int DT = decltype(d)::value, ROWS = decltype(r)::value, NW = decltype(w)::value;
    int cap = 0;
    (void)stepnorm_cap<DT, ROWS, NW>(a, launch_lds<DT, ROWS, NW, true>(a), cap);   // a failed query: cap 0
    return cap;
  });
}

extern "C" void launch_rollout(int dt, const RolloutArgs& a, int rows, hipStream_t s) {
  if (a.dist != 0) return launch_categorical(dt, a, rows, s);
  dispatch_form(dt, rows, [&](auto d, auto r, auto w) {
    launch<decltype(d)::value, decltype(r)::value, decltype(w)::value>(a, s);
  });
}
