// Batched policy evaluation kernel (the reference's test.py, one env at batch 1
// on the CPU): one launch runs WHOLE episodes for a batch of fresh evaluation envs.
//
// Each workgroup owns ROWS envs from their reset to the end of their first episode.  Per step,
// entirely on-chip, the rollout kernel's pipeline (csrc/rollout.hip) without its outputs:
//   obs (env state in LDS) -> normalise with the FIXED (mean, 1/std) + clamp
//   -> policy MLP on MFMA (mlp_core.h layer_gemm, the rollout's precisions)
//   -> action: mu (deterministic) or mu + sigma * eps, eps keyed (action key, env, step)
//   -> env physics, unclipped reward, done / in-place reset
// The env state is created in-kernel (reset key step 0xFFFFFFFF, as VecEnv.reset()) and never
// leaves LDS: the kernel reads no env state from global memory and writes none.  The only global
// stores are ret[E] (sum of the unclipped rewards in step order) and len[E], frozen at an env's
// first done.  No [T][E] buffer rows, x^T, moments or episode stats: less LDS than the rollout and
// no stores on the step path.
//
// The env physics repeats csrc/rollout.hip's expressions (same helpers, same order), so both
// kernels are held to the same torch env (envs/vec_env.py); rollout.hip itself is untouched.
//
// Reference: test.py:24-65 (one env, batch 1, python loop).
#include <type_traits>

#include "kernels.h"
#include "mlp_core.h"

namespace {

constexpr float SYN_DECAY = 0.9f, SYN_DRIVE = 0.1f, SYN_NOISE = 0.05f, SYN_RESET = 0.1f;
constexpr float SYN_TERM_P = 0.002f;
constexpr uint32_t RESET_STEP_KEY = 0xFFFFFFFFu;   // VecEnv.reset()'s step key

// observation of env r, dim d (KIND a template parameter: see csrc/rollout.hip env_obs)
template <int KIND>
DEV float eval_obs(const float* st, int S, int r, int d) {
  if constexpr (KIND == 1) {  // pendulum: (cos th, sin th, thdot)
    const float th = st[r * S + 0];
    return d == 0 ? cosf(th) : (d == 1 ? sinf(th) : st[r * S + 1]);
  } else {
    return st[r * S + d];
  }
}

template <int DT, int ROWS, int NW>
__global__ __launch_bounds__(NW * 64) void eval_kernel(EvalArgs a) {
  using P = Prec<DT>;
  using T = typename P::T;
  constexpr int NTHR = 64 * NW;
  static_assert(ROWS % 4 == 0 && NTHR % ROWS == 0 && (NTHR / ROWS) <= 64, "eval tiling");
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int e0 = blockIdx.x * ROWS;
  const int nvalid = min(ROWS, a.E - e0);
  const int O = a.O, A = a.A, S = a.S;
  const int ld1 = Lds<DT>::stride(a.d1), ld2 = Lds<DT>::stride(a.d2), ld3 = Lds<DT>::stride(a.d3);
  const bool det = a.deterministic != 0;

  extern __shared__ __attribute__((aligned(16))) char smem[];
  LdsCarve cv(smem);
  float* st = cv.take<float>(ROWS * S);
  T* xs = cv.take<T>(ROWS * ld1);
  T* h1 = cv.take<T>(ROWS * ld2);
  T* h2 = cv.take<T>(ROWS * ld3);
  float* mu = cv.take<float>(ROWS * A);
  float* actb = cv.take<float>(ROWS * A);
  float* nm = cv.take<float>(O);                  // the fixed (mean, 1/std) of every feature
  float* ninv = cv.take<float>(O);
  float* done_s = cv.take<float>(ROWS);
  int* envlen = cv.take<int>(ROWS);               // the env's own step counter (auto-reset)
  int* eplen = cv.take<int>(ROWS);                // first-episode length / return, frozen at done
  float* epret = cv.take<float>(ROWS);
  int* fin = cv.take<int>(ROWS);                  // 1: the first episode has ended
  int* nfin = cv.take<int>(1);                    // finished valid envs of this workgroup
  uint32_t* kes = cv.take<uint32_t>(3 * ROWS);    // per-env key prefixes of this step: action, env, reset
  float* wdrv = cv.take<float>(S);                // synthetic dynamics: drive weight of state dim d
  int* jdx = cv.take<int>(S);                     //                     action index driving dim d
  float* sig = cv.take<float>(A);                 // sigma per action dim
  // deterministic: the action IS mu (no sample phase, no copy)
  const float* act = det ? mu : actb;

  const T* W = reinterpret_cast<const T*>(a.W);
  const T* W1 = W + a.off_w1;
  const T* W2 = W + a.off_w2;
  const T* W3 = W + a.off_w3;
  const float sc1 = a.qscale ? a.qscale[0] : a.s1;
  const float sc2 = a.qscale ? a.qscale[1] : a.s2;
  const float sc3 = a.qscale ? a.qscale[2] : a.s3;

  // ---- reset the envs in LDS (every row of the tile: rows past E are stepped but never read
  // out), zero the padded activation tiles ----
  if (a.kind == 1) {
    if (tid < ROWS) {
      const uint32_t e = (uint32_t)(e0 + tid);
      const float u0 = uniform01(keyed(a.key_reset, e, RESET_STEP_KEY, 0u));
      const float u1 = uniform01(keyed(a.key_reset, e, RESET_STEP_KEY, 1u));
      st[tid * S] = (2.f * u0 - 1.f) * 3.14159265358979f;
      st[tid * S + 1] = 2.f * u1 - 1.f;
    }
  } else {
    const int np = (S + 1) >> 1;
    for (int i = tid; i < ROWS * np; i += NTHR) {
      const int r = i / np, p = i - r * np;
      const float2 g = gauss_pair(key_es(a.key_reset, (uint32_t)(e0 + r), RESET_STEP_KEY), (uint32_t)p);
      st[r * S + 2 * p] = SYN_RESET * g.x;
      if (2 * p + 1 < S) st[r * S + 2 * p + 1] = SYN_RESET * g.y;
    }
  }
  preset_pad<DT>(h1, ld2, ROWS, a.n1, tid, NTHR);   // the layers' epilogues write columns < n
  preset_pad<DT>(h2, ld3, ROWS, a.n2, tid, NTHR);
  for (int d = tid; d < O; d += NTHR) { nm[d] = a.mean[d]; ninv[d] = a.inv_std[d]; }
  for (int d = tid; d < S; d += NTHR) {
    wdrv[d] = 0.5f + (float)(d % 7) / 7.0f;
    jdx[d] = d % A;
  }
  for (int j = tid; j < A; j += NTHR) {
    const float ls = a.log_std[j];
    sig[j] = __expf(a.std_var ? 0.5f * ls : ls);
  }
  if (tid < ROWS) {
    envlen[tid] = 0;
    eplen[tid] = 0;
    epret[tid] = 0.f;
    fin[tid] = 0;
  }
  if (tid == 0) *nfin = 0;
  __syncthreads();

  BPre<DT, ROWS / 16> pf;   // cross-barrier weight prefetch of each layer's first k-chunk
  // every env's first episode ends by step limit - 1 (done = terminal or length >= limit), so the
  // loop bound alone ends the launch
  for (int step = 0; step < a.limit; ++step) {
    // ---- (a) observe, normalise -> LDS tile ----
    auto observe = [&](auto kind_tag) {
      constexpr int KIND = decltype(kind_tag)::value;
      for (int d = tid; d < a.d1; d += NTHR) {
        float m = 0.f, is = 1.f;
        if (d < O) { m = nm[d]; is = ninv[d]; }
#pragma unroll
        for (int r = 0; r < ROWS; ++r) {
          float xv;
          if (d < O) {
            const float o = eval_obs<KIND>(st, S, r, d);
            xv = fminf(fmaxf((o - m) * is, -5.f), 5.f);
          } else {
            xv = (d == O) ? 1.f : 0.f;
          }
          P::put(xs, r * ld1 + d, xv);
        }
      }
    };
    if (a.kind == 1) observe(std::integral_constant<int, 1>{});
    else observe(std::integral_constant<int, 0>{});
    layer_prefetch<DT, ROWS, NW>(pf, W1, a.d1, a.n1, wave, lane);
    __syncthreads();
    // (env, step) key prefixes of the sample / env phases: hashed by the last wave's lanes before
    // fc1, so the layers' barriers publish them (the previous step's env phase, their last
    // reader, ended in a barrier)
    const uint32_t kstep = (uint32_t)step;   // a fresh env's global step counter starts at 0
    if (tid >= NTHR - ROWS) {
      const int r = tid - (NTHR - ROWS);
      const uint32_t e = (uint32_t)(e0 + r);
      kes[r] = key_es(a.key_action, e, kstep);
      kes[ROWS + r] = key_es(a.key_env, e, kstep);
      kes[2 * ROWS + r] = key_es(a.key_reset, e, kstep);
    }
    // ---- (b) policy MLP ----
    layer_gemm<DT, ROWS, NW, EPI_TANH, true>(xs, ld1, a.d1, W1, a.n1, h1, ld2, sc1, wave, lane, nullptr, 0, 0, 0, &pf);
    layer_prefetch<DT, ROWS, NW>(pf, W2, a.d2, a.n2, wave, lane);
    __syncthreads();
    layer_gemm<DT, ROWS, NW, EPI_TANH, true>(h1, ld2, a.d2, W2, a.n2, h2, ld3, sc2, wave, lane, nullptr, 0, 0, 0, &pf);
    layer_prefetch<DT, ROWS, NW>(pf, W3, a.d3, a.n3, wave, lane);
    __syncthreads();
    layer_gemm<DT, ROWS, NW, EPI_LINEAR_F32, true>(h2, ld3, a.d3, W3, a.n3, mu, A, sc3, wave, lane, nullptr, 0, 0, 0,
                                                   &pf);
    __syncthreads();
    // ---- (c) stochastic: a = mu + sigma * eps (one Box-Muller pair -> two action dims) ----
    if (!det) {   // (a kernel argument: the barrier below is workgroup-uniform)
      const int npa = (A + 1) >> 1;
      for (int i = tid; i < ROWS * npa; i += NTHR) {
        const int r = i / npa, q = i - r * npa;
        const float2 g = gauss_pair(kes[r], (uint32_t)q);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const int j = 2 * q + h;
          if (j < A) actb[r * A + j] = mu[r * A + j] + sig[j] * (h ? g.y : g.x);
        }
      }
      __syncthreads();
    }
    // ---- (d) per-env: reward, termination, first-episode bookkeeping ----
    {
      constexpr int LPE = NTHR / ROWS;
      const int r = tid / LPE, l = tid - r * LPE;
      const int e = e0 + r;
      float err = 0.f;
      const int na = min(A, O);
      if (a.kind != 1) {
        for (int j = l; j < na; j += LPE) {
          const float ac = fminf(fmaxf(act[r * A + j], -1.f), 1.f);
          const float d = ac - fast_tanh(st[r * S + j]);
          err += d * d;
        }
      }
#pragma unroll
      for (int o = LPE / 2; o > 0; o >>= 1) err += __shfl_xor(err, o, LPE);
      if (l == 0) {
        float rew;
        bool term = false;
        if (a.kind == 1) {
          float th = st[r * S], thd = st[r * S + 1];
          float u = fminf(fmaxf(act[r * A], -2.f), 2.f);
          float thn = fmodf(th + 3.14159265358979f, 6.28318530717959f);
          if (thn < 0.f) thn += 6.28318530717959f;
          thn -= 3.14159265358979f;
          rew = -(thn * thn + 0.1f * thd * thd + 0.001f * u * u);
        } else {
          rew = 1.f - err / (float)na;
          term = uniform01(keyed(a.key_term, (uint32_t)e, kstep, 0u)) < SYN_TERM_P;
        }
        const int el = envlen[r] + 1;
        const bool done = term || (el >= a.limit);
        envlen[r] = done ? 0 : el;
        done_s[r] = done ? 1.f : 0.f;
        if (!fin[r]) {   // finished envs keep stepping (lockstep keys) but leave the sums alone
          epret[r] += rew;
          eplen[r] += 1;
          if (done) {
            fin[r] = 1;
            if (r < nvalid) atomicAdd(nfin, 1);
          }
        }
      }
    }
    __syncthreads();
    // ---- (e) state transition (+ in-place reset on done) ----
    if (a.kind == 1) {
      if (tid < ROWS) {
        const int r = tid, e = e0 + r;
        if (done_s[r] > 0.5f) {
          float u0 = uniform01(keyed(a.key_reset, (uint32_t)e, kstep, 0u));
          float u1 = uniform01(keyed(a.key_reset, (uint32_t)e, kstep, 1u));
          st[r * S] = (2.f * u0 - 1.f) * 3.14159265358979f;
          st[r * S + 1] = 2.f * u1 - 1.f;
        } else {
          float th = st[r * S], thd = st[r * S + 1];
          float u = fminf(fmaxf(act[r * A], -2.f), 2.f);
          float nthd = thd + (-3.f * 10.f / 2.f * sinf(th + 3.14159265358979f) + 3.f * u) * 0.05f;
          float nth = th + nthd * 0.05f;
          nthd = fminf(fmaxf(nthd, -8.f), 8.f);
          st[r * S] = nth;
          st[r * S + 1] = nthd;
        }
      }
    } else {
      // item = (row r, dim pair p): one Box-Muller pair per item, every LDS read of an item before
      // its stores (items never share a state slot)
      const int np = (S + 1) >> 1;
      for (int i = tid; i < ROWS * np; i += NTHR) {
        const int r = i / np, p = i - r * np;
        const int d0 = 2 * p;
        const bool has1 = d0 + 1 < S;
        const int d1 = has1 ? d0 + 1 : d0;
        const bool done = done_s[r] > 0.5f;
        const uint32_t key = done ? kes[2 * ROWS + r] : kes[ROWS + r];
        const float st0 = st[r * S + d0], st1 = st[r * S + d1];
        const float a0 = fminf(fmaxf(act[r * A + jdx[d0]], -1.f), 1.f);
        const float a1 = fminf(fmaxf(act[r * A + jdx[d1]], -1.f), 1.f);
        const float w0 = wdrv[d0], w1 = wdrv[d1];
        const float2 g = gauss_pair(key, (uint32_t)p);
        float n0, n1;
        if (done) {
          n0 = SYN_RESET * g.x;
          n1 = SYN_RESET * g.y;
        } else {
          n0 = SYN_DECAY * st0 + SYN_DRIVE * fast_tanh(w0 * a0) + SYN_NOISE * g.x;
          n1 = SYN_DECAY * st1 + SYN_DRIVE * fast_tanh(w1 * a1) + SYN_NOISE * g.y;
        }
        st[r * S + d0] = n0;
        if (has1) st[r * S + d0 + 1] = n1;
      }
    }
    __syncthreads();
    // every valid env of the tile has finished: read after the step's closing barrier (nfin's next
    // writer is the next step's phase (d), barriers away), so the exit is workgroup-uniform
    if (*nfin >= nvalid) break;
  }
  if (tid < nvalid) {
    a.ret[e0 + tid] = epret[tid];
    a.len[e0 + tid] = eplen[tid];
  }
}

template <int DT, int ROWS>
size_t eval_lds(const EvalArgs& a) {
  auto al = [](size_t b) { return (b + 15) & ~size_t(15); };
  using T = typename Prec<DT>::T;
  size_t b = 0;
  b += al(sizeof(float) * ROWS * a.S);
  b += al(sizeof(T) * ROWS * Lds<DT>::stride(a.d1));
  b += al(sizeof(T) * ROWS * Lds<DT>::stride(a.d2));
  b += al(sizeof(T) * ROWS * Lds<DT>::stride(a.d3));
  b += 2 * al(sizeof(float) * ROWS * a.A);
  b += 2 * al(sizeof(float) * a.O);
  b += al(sizeof(float) * ROWS) + 2 * al(sizeof(int) * ROWS) + al(sizeof(float) * ROWS) + al(sizeof(int) * ROWS);
  b += al(sizeof(int));
  b += al(sizeof(uint32_t) * 3 * ROWS);
  b += al(sizeof(float) * a.S) + al(sizeof(int) * a.S);
  b += al(sizeof(float) * a.A);
  return b;
}

template <int DT, int ROWS, int NW>
void launch_nw(const EvalArgs& a, hipStream_t s) {
  const size_t lds = eval_lds<DT, ROWS>(a);
  const int nblk = (a.E + ROWS - 1) / ROWS;
  if (lds > 65536) set_max_lds_once<eval_kernel<DT, ROWS, NW>>(lds);
  hipLaunchKernelGGL((eval_kernel<DT, ROWS, NW>), dim3(nblk), dim3(NW * 64), lds, s, a);
  HIP_CHECK_LAUNCH();
}

}  // namespace

// the rollout's launch forms: 8 waves for bf16x3 / bf16 / fp8, 4 for fp32 (twice the fragment registers)
extern "C" void launch_eval(int dt, const EvalArgs& a, hipStream_t s) {
  if (dt == DT_F32) launch_nw<DT_F32, 16, 4>(a, s);
  else if (dt == DT_BF16) launch_nw<DT_BF16, 16, 8>(a, s);
  else if (dt == DT_S3) launch_nw<DT_S3, 16, 8>(a, s);
  else launch_nw<DT_FP8, 16, 8>(a, s);
}
