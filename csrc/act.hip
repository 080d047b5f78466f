// Policy inference kernel: ONE policy step for E caller-supplied observations.
//
// The rollout kernel's per-step pipeline (csrc/policy_step.h, the code csrc/rollout.hip runs)
// without its env: the observations come from the caller (a host-stepped env, a served request
// batch), not from in-kernel physics.  Each workgroup owns ROWS rows; per row r < E:
//   (a) raw fp32 obs[r][0..O) from global memory -> x = clamp((obs - mean) * inv_std, -5, 5), the
//       constant 1 at column O, zeros up to d1 -> LDS tile (the rollout's observe phase); with `mom`
//       the workgroup's sum(obs - shift) / sum((obs - shift)^2) over its valid rows
//   (b) x_out: the tile's rows in the buffer precision (XStore<DT>), as 16-byte row chunks
//   (c) policy MLP on MFMA (the rollout's precisions and scales)
//   (d) a = mu + sigma * eps, eps keyed (action key, e_base + r, step_key), one Box-Muller pair per
//       two action dims; deterministic: a = mu, eps = 0
//   (e) logp = sum_j(-0.5 eps_j^2 - log sigma_j) - 0.5 A log(2 pi)
// ActArgs::dist 1 (a categorical head): (d), (e) are instead the Gumbel-max sample over the A logits, the one-hot
// action row and logp = z_a - logsumexp(z) (policy_step.h categorical_row); mu receives the logits.
// Every output is optional (null: skipped).  With none of actions / logp / mu the launch is
// ROWS-ONLY: (a), (b) and the moments, no MLP (a rollout's bootstrap row).  Rows >= E of the last
// tile are computed and never stored.  The kernel reads the policy image, log_std, the stats and
// obs; its only global stores are the outputs listed in ActArgs.  No atomics: a workgroup owns its
// rows and its moment slice (overwritten or added to, stream order), so a launch is deterministic.
#include "policy_step.h"

namespace {

// the launch's dynamic LDS: the kernel's pointers and the host's byte count from one carve
template <int DT, int ROWS>
struct ActLds {
  using XB = typename Prec<XStore<DT>::DTX>::T;
  LdsCarve cv;
  PolicyTiles<DT> t;
  float* epsb;     // [ROWS][A] the action noise
  float* lsg;      // [log sigma | sigma]
  uint32_t* kes;   // per-row (env, step) key prefix of the action noise
  XB* xsb;         // fp8: bf16 staging tile of the buffer rows (policy_step.h store_tile_rows)
  __host__ __device__ ActLds(char* smem, const ActArgs& a)
      : cv(smem), t(cv, a.net, ROWS, a.A), epsb(cv.take<float>(ROWS * a.A)), lsg(cv.take<float>(2 * a.A)),
        kes(cv.take<uint32_t>(ROWS)), xsb(DT == DT_FP8 ? cv.take<XB>(ROWS * a.net.d1) : nullptr) {}
};

template <int DT, int ROWS, int NW>
__global__ __launch_bounds__(NW * 64) void act_kernel(ActArgs a) {
  using P = Prec<DT>;
  using PX = Prec<XStore<DT>::DTX>;
  constexpr int NTHR = 64 * NW;
  static_assert(ROWS % 4 == 0 && NTHR % ROWS == 0 && (NTHR / ROWS) <= 64, "act tiling");
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int e0 = blockIdx.x * ROWS;
  const int nvalid = min(ROWS, a.E - e0);
  const int O = a.O, A = a.A, d1 = a.net.d1;
  const bool det = a.deterministic != 0;
  // (kernel arguments: every branch on them is workgroup-uniform)
  const bool mlp = a.actions != nullptr || a.logp != nullptr || a.mu != nullptr;

  extern __shared__ __attribute__((aligned(16))) char smem[];
  const ActLds<DT, ROWS> L(smem, a);
  PolicyStep<DT, ROWS, NW> ps(a.net, L.t);

  if (mlp) {
    ps.setup(L.lsg, tid);
    // hashed here, published by the observe phase's barrier
    key_prefixes<ROWS, NTHR>(L.kes, {a.key_action}, a.e_base + (uint32_t)e0, a.step_key, tid);
  }

  // ---- (a) observe, moments, normalise -> LDS tile: thread = feature (coalesced obs rows) ----
  for (int d = tid; d < d1; d += NTHR) {
    float m = 0.f, is = 1.f, sh = 0.f;
    if (d < O) {
      m = a.mean[d];
      is = a.inv_std[d];
      if (a.mom != nullptr) sh = a.shift[d];
    }
    float ls1 = 0.f, ls2 = 0.f;
#pragma unroll
    for (int r = 0; r < ROWS; ++r) {
      float xv;
      if (d < O) {
        // rows past E read nothing (their tile rows normalise a zero observation, never stored)
        const float o = r < nvalid ? a.obs[(size_t)(e0 + r) * O + d] : 0.f;
        const float dd = r < nvalid ? o - sh : 0.f;
        ls1 += dd;
        ls2 += dd * dd;
        xv = norm_clamp(o, m, is);
      } else {
        xv = pad_col(d, O);
      }
      P::put(L.t.xs, r * L.t.ld1 + d, xv);
      if constexpr (DT == DT_FP8) L.xsb[r * d1 + d] = PX::cvt(xv);
    }
    if (a.mom != nullptr && d < O) {
      // this workgroup's slice [2][O] of the RolloutArgs::mom layout, owned by thread d
      float* m1 = a.mom + (size_t)blockIdx.x * 2 * O + d;
      float* m2 = m1 + O;
      if (a.mom_init) {
        *m1 = ls1;
        *m2 = ls2;
      } else {
        *m1 += ls1;
        *m2 += ls2;
      }
    }
  }
  if (mlp) ps.prefetch(wave, lane);
  __syncthreads();
  // ---- (b) row-major buffer rows from the normalised LDS tile ----
  if (a.x_out != nullptr)
    store_tile_rows<DT, NTHR>(reinterpret_cast<typename PX::T*>(a.x_out) + (size_t)e0 * d1, L.t, L.xsb, d1, nvalid, tid);
  if (!mlp) return;
  // ---- (c) policy MLP ----
  ps.layers(wave, lane);
  if (a.dist == 1) {
    // ---- (d', e') categorical head: LPE lanes per row share its A logits (policy_step.h categorical_row) ----
    constexpr int LPE = NTHR / ROWS;
    const int r = tid / LPE, l = tid - r * LPE;
    const float* z = L.t.mu + r * A;
    const CatRow c = categorical_row<LPE>(z, A, l, L.kes[r], !det);
    if (r < nvalid) {
      const size_t o = (size_t)(e0 + r) * A;
      for (int k = l; k < A; k += LPE) {
        if (a.actions != nullptr) a.actions[o + k] = (k == c.a) ? 1.f : 0.f;   // the one-hot row
        if (a.mu != nullptr) a.mu[o + k] = z[k];
      }
      if (l == 0 && a.logp != nullptr) a.logp[e0 + r] = c.logp;
    }
    return;
  }
  // ---- (d) sample a = mu + sigma * eps ----
  sample_loop<ROWS, NTHR>(L.kes, A, tid, !det, [&](int r, int j, float eps) {
    const float mv = L.t.mu[r * A + j];
    const float av = det ? mv : mv + L.lsg[A + j] * eps;   // deterministic: the action IS mu
    L.epsb[r * A + j] = eps;
    if (r < nvalid) {
      const size_t o = (size_t)(e0 + r) * A + j;
      if (a.actions != nullptr) a.actions[o] = av;
      if (a.mu != nullptr) a.mu[o] = mv;
    }
  });
  if (a.logp == nullptr) return;
  __syncthreads();
  // ---- (e) logp: LPE lanes per row (contiguous inside a wave) share the dims, reduce by shuffles ----
  {
    constexpr int LPE = NTHR / ROWS;
    const int r = tid / LPE, l = tid - r * LPE;
    float lp = 0.f;
    for (int j = l; j < A; j += LPE) lp += logp_term(L.epsb[r * A + j], L.lsg[j]);
#pragma unroll
    for (int o = LPE / 2; o > 0; o >>= 1) lp += __shfl_xor(lp, o, LPE);
    if (l == 0 && r < nvalid) a.logp[e0 + r] = lp - logp_const(A);
  }
}

}  // namespace

// the rollout's launch forms (policy_step.h POLICY_WAVES), 16 rows per workgroup
extern "C" void launch_act(int dt, const ActArgs& a, hipStream_t s) {
  dispatch_dt(dt, [&](auto d) {
    constexpr int DT = decltype(d)::value, ROWS = 16, NW = POLICY_WAVES<DT, ROWS>;
    const size_t lds = ActLds<DT, ROWS>(nullptr, a).cv.off;
    if (lds > 65536) set_max_lds_once<act_kernel<DT, ROWS, NW>>(lds);
    hipLaunchKernelGGL((act_kernel<DT, ROWS, NW>), dim3((a.E + ROWS - 1) / ROWS), dim3(NW * 64), lds, s, a);
    HIP_CHECK_LAUNCH();
  });
}
