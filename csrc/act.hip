// Policy inference kernel: ONE policy step for E caller-supplied observations.
//
// The rollout kernel's per-step pipeline (csrc/rollout.hip) without its env: the observations come
// from the caller (a host-stepped env, a served request batch), not from in-kernel physics.  Each
// workgroup owns ROWS rows; per row r < E:
//   (a) raw fp32 obs[r][0..O) from global memory -> x = clamp((obs - mean) * inv_std, -5, 5), the
//       constant 1 at column O, zeros up to d1 -> LDS tile (the rollout's observe phase); with `mom`
//       the workgroup's sum(obs - shift) / sum((obs - shift)^2) over its valid rows
//   (b) x_out: the tile's rows in the buffer precision (XStore<DT>), as 16-byte row chunks
//   (c) policy MLP on MFMA (mlp_core.h layer_gemm, the rollout's precisions and scales)
//   (d) a = mu + sigma * eps, eps keyed (action key, e_base + r, step_key), one Box-Muller pair per
//       two action dims; deterministic: a = mu, eps = 0
//   (e) logp = sum_j(-0.5 eps_j^2 - log sigma_j) - 0.5 A log(2 pi)
// Every output is optional (null: skipped).  With none of actions / logp / mu the launch is
// ROWS-ONLY: (a), (b) and the moments, no MLP (a rollout's bootstrap row).  Rows >= E of the last
// tile are computed and never stored.  The kernel reads the policy image, log_std, the stats and
// obs; its only global stores are the outputs listed in ActArgs.  No atomics: a workgroup owns its
// rows and its moment slice (overwritten or added to, stream order), so a launch is deterministic.
#include <type_traits>

#include "kernels.h"
#include "mlp_core.h"

namespace {

constexpr float LOG_2PI_F = 1.8378770664093453f;

template <int DT, int ROWS, int NW>
__global__ __launch_bounds__(NW * 64) void act_kernel(ActArgs a) {
  using P = Prec<DT>;
  using T = typename P::T;
  constexpr int NTHR = 64 * NW;
  static_assert(ROWS % 4 == 0 && NTHR % ROWS == 0 && (NTHR / ROWS) <= 64, "act tiling");
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int e0 = blockIdx.x * ROWS;
  const int nvalid = min(ROWS, a.E - e0);
  const int O = a.O, A = a.A;
  const int ld1 = Lds<DT>::stride(a.d1), ld2 = Lds<DT>::stride(a.d2), ld3 = Lds<DT>::stride(a.d3);
  const bool det = a.deterministic != 0;
  // (kernel arguments: every branch on them is workgroup-uniform)
  const bool mlp = a.actions != nullptr || a.logp != nullptr || a.mu != nullptr;

  extern __shared__ __attribute__((aligned(16))) char smem[];
  LdsCarve cv(smem);
  T* xs = cv.take<T>(ROWS * ld1);
  T* h1 = cv.take<T>(ROWS * ld2);
  T* h2 = cv.take<T>(ROWS * ld3);
  float* mu = cv.take<float>(ROWS * A);
  float* epsb = cv.take<float>(ROWS * A);
  float* lsg = cv.take<float>(2 * A);             // per action dim: log sigma [0, A), sigma [A, 2A)
  uint32_t* kes = cv.take<uint32_t>(ROWS);        // per-row (env, step) key prefix of the action noise
  // fp8: the MFMA tile is e4m3 but the buffer rows are bf16 (csrc/rollout.hip: a bf16 staging tile
  // lets them leave as 16-byte row chunks)
  using PX = Prec<XStore<DT>::DTX>;
  using XB = typename PX::T;
  constexpr bool STAGE = DT == DT_FP8;
  XB* xsb = STAGE ? cv.take<XB>(ROWS * a.d1) : nullptr;

  const T* W = reinterpret_cast<const T*>(a.W);
  const T* W1 = W + a.off_w1;
  const T* W2 = W + a.off_w2;
  const T* W3 = W + a.off_w3;
  const float sc1 = a.qscale ? a.qscale[0] : a.s1;
  const float sc2 = a.qscale ? a.qscale[1] : a.s2;
  const float sc3 = a.qscale ? a.qscale[2] : a.s3;

  if (mlp) {
    preset_pad<DT>(h1, ld2, ROWS, a.n1, tid, NTHR);   // the layers' epilogues write columns < n
    preset_pad<DT>(h2, ld3, ROWS, a.n2, tid, NTHR);
    for (int j = tid; j < A; j += NTHR) {
      const float ls = a.log_std[j];
      const float lsig = a.std_var ? 0.5f * ls : ls;
      lsg[j] = lsig;
      lsg[A + j] = __expf(lsig);
    }
    // hashed here, published by the observe phase's barrier
    if (tid >= NTHR - ROWS) {
      const int r = tid - (NTHR - ROWS);
      kes[r] = key_es(a.key_action, a.e_base + (uint32_t)(e0 + r), a.step_key);
    }
  }

  // ---- (a) observe, moments, normalise -> LDS tile: thread = feature (coalesced obs rows) ----
  for (int d = tid; d < a.d1; d += NTHR) {
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
        xv = fminf(fmaxf((o - m) * is, -5.f), 5.f);
      } else {
        xv = (d == O) ? 1.f : 0.f;
      }
      P::put(xs, r * ld1 + d, xv);
      if constexpr (STAGE) xsb[r * a.d1 + d] = PX::cvt(xv);
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
  BPre<DT, ROWS / 16> pf;   // cross-barrier weight prefetch of each layer's first k-chunk
  if (mlp) layer_prefetch<DT, ROWS, NW>(pf, W1, a.d1, a.n1, wave, lane);
  __syncthreads();
  // ---- (b) row-major buffer rows from the normalised LDS tile: one 16-byte store per 16 bytes of
  // features (split-bf16: the LDS tile and the buffer share the 32-byte hi|lo group layout) ----
  if (a.x_out != nullptr) {
    XB* xo = reinterpret_cast<XB*>(a.x_out);
    constexpr int EPC = 16 / sizeof(XB);
    const int ch = a.d1 / EPC;
    for (int i = tid; i < nvalid * ch; i += NTHR) {
      const int r = i / ch, c = i - r * ch;
      const void* src = STAGE ? static_cast<const void*>(xsb + r * a.d1 + c * EPC)
                              : static_cast<const void*>(xs + r * ld1 + c * EPC);
      *reinterpret_cast<uint4*>(xo + (size_t)(e0 + r) * a.d1 + c * EPC) = *reinterpret_cast<const uint4*>(src);
    }
  }
  if (!mlp) return;
  // ---- (c) policy MLP ----
  layer_gemm<DT, ROWS, NW, EPI_TANH, true>(xs, ld1, a.d1, W1, a.n1, h1, ld2, sc1, wave, lane, nullptr, 0, 0, 0, &pf);
  layer_prefetch<DT, ROWS, NW>(pf, W2, a.d2, a.n2, wave, lane);
  __syncthreads();
  layer_gemm<DT, ROWS, NW, EPI_TANH, true>(h1, ld2, a.d2, W2, a.n2, h2, ld3, sc2, wave, lane, nullptr, 0, 0, 0, &pf);
  layer_prefetch<DT, ROWS, NW>(pf, W3, a.d3, a.n3, wave, lane);
  __syncthreads();
  layer_gemm<DT, ROWS, NW, EPI_LINEAR_F32, true>(h2, ld3, a.d3, W3, a.n3, mu, A, sc3, wave, lane, nullptr, 0, 0, 0,
                                                 &pf);
  __syncthreads();
  // ---- (d) sample a = mu + sigma * eps (one Box-Muller pair -> two action dims) ----
  const int npa = (A + 1) >> 1;
  for (int i = tid; i < ROWS * npa; i += NTHR) {
    const int r = i / npa, q = i - r * npa;
    float2 g = make_float2(0.f, 0.f);
    if (!det) g = gauss_pair(kes[r], (uint32_t)q);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int j = 2 * q + h;
      if (j < A) {
        const float eps = h ? g.y : g.x;
        const float mv = mu[r * A + j];
        const float av = det ? mv : mv + lsg[A + j] * eps;   // deterministic: the action IS mu
        epsb[r * A + j] = eps;
        if (r < nvalid) {
          const size_t o = (size_t)(e0 + r) * A + j;
          if (a.actions != nullptr) a.actions[o] = av;
          if (a.mu != nullptr) a.mu[o] = mv;
        }
      }
    }
  }
  if (a.logp == nullptr) return;
  __syncthreads();
  // ---- (e) logp: LPE lanes per row (contiguous inside a wave) share the dims, reduce by shuffles ----
  {
    constexpr int LPE = NTHR / ROWS;
    const int r = tid / LPE, l = tid - r * LPE;
    float lp = 0.f;
    for (int j = l; j < A; j += LPE) {
      const float ep = epsb[r * A + j];
      lp += -0.5f * ep * ep - lsg[j];
    }
#pragma unroll
    for (int o = LPE / 2; o > 0; o >>= 1) lp += __shfl_xor(lp, o, LPE);
    if (l == 0 && r < nvalid) a.logp[e0 + r] = lp - 0.5f * LOG_2PI_F * (float)A;
  }
}

template <int DT, int ROWS>
size_t act_lds(const ActArgs& a) {
  auto al = [](size_t b) { return (b + 15) & ~size_t(15); };
  using T = typename Prec<DT>::T;
  size_t b = 0;
  b += al(sizeof(T) * ROWS * Lds<DT>::stride(a.d1));
  b += al(sizeof(T) * ROWS * Lds<DT>::stride(a.d2));
  b += al(sizeof(T) * ROWS * Lds<DT>::stride(a.d3));
  b += 2 * al(sizeof(float) * ROWS * a.A);
  b += al(sizeof(float) * 2 * a.A);
  b += al(sizeof(uint32_t) * ROWS);
  if (DT == DT_FP8) b += al(sizeof(typename Prec<XStore<DT>::DTX>::T) * ROWS * a.d1);
  return b;
}

template <int DT, int ROWS, int NW>
void launch_nw(const ActArgs& a, hipStream_t s) {
  const size_t lds = act_lds<DT, ROWS>(a);
  const int nblk = (a.E + ROWS - 1) / ROWS;
  if (lds > 65536) set_max_lds_once<act_kernel<DT, ROWS, NW>>(lds);
  hipLaunchKernelGGL((act_kernel<DT, ROWS, NW>), dim3(nblk), dim3(NW * 64), lds, s, a);
  HIP_CHECK_LAUNCH();
}

}  // namespace

// the rollout's launch forms: 8 waves for bf16x3 / bf16 / fp8, 4 for fp32 (twice the fragment registers)
extern "C" void launch_act(int dt, const ActArgs& a, hipStream_t s) {
  if (dt == DT_F32) launch_nw<DT_F32, 16, 4>(a, s);
  else if (dt == DT_BF16) launch_nw<DT_BF16, 16, 8>(a, s);
  else if (dt == DT_S3) launch_nw<DT_S3, 16, 8>(a, s);
  else launch_nw<DT_FP8, 16, 8>(a, s);
}
