// One policy step on a ROWS-row tile, written once for the rollout, evaluation and inference
// kernels (csrc/rollout.hip, eval.hip, act.hip):
//   x = clamp((obs - mean) * inv_std, -5, 5) -> three-layer MLP on MFMA (activations stay in LDS,
//   each layer's first weight fragments prefetched across the previous barrier) -> mu
//   -> a = mu + sigma * eps, eps keyed (action key, env, step), one Box-Muller pair per two dims
//   -> logp = sum_j(-0.5 eps_j^2 - log sigma_j) - 0.5 A log(2 pi)
// A kernel keeps what is its own: where the observations come from, which outputs a sample
// writes, the deterministic rule, and what its per-env phase sums next to the log-prob.
#pragma once
#include <type_traits>

#include "kernels.h"
#include "mlp_core.h"

DEV float norm_clamp(float o, float mean, float inv_std) { return fminf(fmaxf((o - mean) * inv_std, -5.f), 5.f); }
// columns [O, d1) of the input tile: the constant 1 (fc1's bias input), then zeros
DEV float pad_col(int d, int O) { return (d == O) ? 1.f : 0.f; }

// The step's LDS tiles (consecutive in every kernel's carve): the input tile, the two hidden
// tiles in the MFMA storage precision with their padded row strides, and mu [rows][A] fp32.
template <int DT>
struct PolicyTiles {
  using T = typename Prec<DT>::T;
  int ld1, ld2, ld3;
  T *xs, *h1, *h2;
  float* mu;
  __host__ __device__ PolicyTiles(LdsCarve& cv, const PolicyNet& n, int rows, int A)
      : ld1(Lds<DT>::stride(n.d1)), ld2(Lds<DT>::stride(n.d2)), ld3(Lds<DT>::stride(n.d3)) {
    xs = cv.take<T>(rows * ld1);
    h1 = cv.take<T>(rows * ld2);
    h2 = cv.take<T>(rows * ld3);
    mu = cv.take<float>(rows * A);
  }
};

// Everything of one tile's policy that is fixed for the launch
template <int DT, int ROWS, int NW>
struct PolicyStep {
  using P = Prec<DT>;
  using T = typename P::T;
  static constexpr int NTHR = 64 * NW;
  // by value: a reference to the kernel arguments makes every use of a field a fresh argument
  // load at the use site instead of one at kernel entry (act fp8: 71 -> 79 VGPRs, an occupancy step)
  const PolicyNet n;
  const PolicyTiles<DT> t;
  const T *W1, *W2, *W3;
  float sc1, sc2, sc3;   // per-layer dequant scales: device array (fp8 images, refreshed on-device) or kernel args
  BPre<DT, ROWS / 16> pf;   // cross-barrier weight prefetch of each layer's first k-chunk

  DEV PolicyStep(const PolicyNet& net, const PolicyTiles<DT>& tiles) : n(net), t(tiles) {
    const T* W = reinterpret_cast<const T*>(n.W);
    W1 = W + n.off_w1;
    W2 = W + n.off_w2;
    W3 = W + n.off_w3;
    sc1 = n.qscale ? n.qscale[0] : n.s1;
    sc2 = n.qscale ? n.qscale[1] : n.s2;
    sc3 = n.qscale ? n.qscale[2] : n.s3;
  }
  // Once per launch, before the first barrier: the hidden tiles' pad columns (the layers'
  // epilogues write columns < n) and the sigma table lsg[2A] = [log sigma | sigma] (log_std is
  // fixed during a launch: no global load and exp per sampled dim and step)
  DEV void setup(float* lsg, int tid) const {
    preset_pad<DT>(t.h1, t.ld2, ROWS, n.n1, tid, NTHR);
    preset_pad<DT>(t.h2, t.ld3, ROWS, n.n2, tid, NTHR);
    const int A = n.n3;
    for (int j = tid; j < A; j += NTHR) {
      const float ls = n.log_std[j];
      const float lsig = n.std_var ? 0.5f * ls : ls;
      lsg[j] = lsig;
      lsg[A + j] = __expf(lsig);
    }
  }
  // fc1's first weight fragments: issued before the barrier that publishes the input tile
  DEV void prefetch(int wave, int lane) { layer_prefetch<DT, ROWS, NW>(pf, W1, n.d1, n.n1, wave, lane); }
  // xs -> mu.  after(integral_constant<int, l>) runs behind layer l's barrier, l = 1..3.
  template <typename F>
  DEV void layers(int wave, int lane, F&& after) {
    layer_gemm<DT, ROWS, NW, EPI_TANH, true>(t.xs, t.ld1, n.d1, W1, n.n1, t.h1, t.ld2, sc1, wave, lane, nullptr, 0, 0, 0, &pf);
    layer_prefetch<DT, ROWS, NW>(pf, W2, n.d2, n.n2, wave, lane);
    __syncthreads();
    after(std::integral_constant<int, 1>{});
    layer_gemm<DT, ROWS, NW, EPI_TANH, true>(t.h1, t.ld2, n.d2, W2, n.n2, t.h2, t.ld3, sc2, wave, lane, nullptr, 0, 0, 0, &pf);
    layer_prefetch<DT, ROWS, NW>(pf, W3, n.d3, n.n3, wave, lane);
    __syncthreads();
    after(std::integral_constant<int, 2>{});
    layer_gemm<DT, ROWS, NW, EPI_LINEAR_F32, true>(t.h2, t.ld3, n.d3, W3, n.n3, t.mu, n.n3, sc3, wave, lane, nullptr, 0, 0, 0,
                                                   &pf);
    __syncthreads();
    after(std::integral_constant<int, 3>{});
  }
  DEV void layers(int wave, int lane) { layers(wave, lane, [](auto) {}); }
};

// (env, step) key prefixes shared by every dim of the step: kes[k * ROWS + r] for base key k and
// tile row r (env env0 + r), hashed by the last ROWS threads (idle in the narrow policy layers).
// Written before a barrier the readers are behind.
template <int ROWS, int NTHR, int NK>
DEV void key_prefixes(uint32_t* kes, const uint32_t (&base)[NK], uint32_t env0, uint32_t step, int tid) {
  if (tid >= NTHR - ROWS) {
    const int r = tid - (NTHR - ROWS);
#pragma unroll
    for (int k = 0; k < NK; ++k) kes[k * ROWS + r] = key_es(base[k], env0 + (uint32_t)r, step);
  }
}

// Item = (row r, action pair q): body(r, j, eps) for the pair's dims j < A.  sample false: eps = 0.
template <int ROWS, int NTHR, typename F>
DEV void sample_loop(const uint32_t* kes, int A, int tid, bool sample, F&& body) {
  const int npa = (A + 1) >> 1;
  for (int i = tid; i < ROWS * npa; i += NTHR) {
    const int r = i / npa, q = i - r * npa;
    float2 g = make_float2(0.f, 0.f);
    if (sample) g = gauss_pair(kes[r], (uint32_t)q);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int j = 2 * q + h;
      if (j < A) body(r, j, h ? g.y : g.x);
    }
  }
}

// log-prob of a row: the sum of logp_term over its dims, minus logp_const
DEV float logp_term(float eps, float log_sigma) { return -0.5f * eps * eps - log_sigma; }
DEV float logp_const(int A) { return 0.5f * LOG_2PI_F * (float)A; }

// ---- categorical head (ActArgs::dist 1): the tile's mu [rows][K] holds the K logits z of each row ----
// Gumbel noise of action k: g = -log(-log u), u = uniform01(keyed(action key, env, step, k)) (utils/rng.py gumbel).
// The accurate logf, not the hardware log2: the arg-max below is a comparison of z + g against the torch twin's.
// The top bucket's u rounds to 1, so -log u is held at 2^-25 (g <= 17.33): finite for every hash.
DEV float gumbel(uint32_t kes, uint32_t k) {
  const float u = uniform01(hash_u32(kes ^ k));
  return -logf(fmaxf(-logf(u), 0x1p-25f));
}

struct CatRow {
  int a;        // the chosen action: the lowest k attaining max_k (z_k + g_k)
  float logp;   // z_a - lse
  float lse;    // m + log sum_k exp(z_k - m), m = max_k z_k
};

// One row's categorical step by its LPE lanes (consecutive in a wave, LPE a power of two <= 64; lane l takes
// the logits l, l + LPE, ..): the max, the sum of exponentials and the arg-max of z + g as a (value, index) pair
// that prefers the lower index on equal values, reduced by xor-shuffles; every lane gets the result.  A lane
// with no logit (K < LPE) contributes -inf to the max and the arg-max and 0 to the sum.  sample false: g = 0
// (the arg-max of the logits).  Every lane of the wave must call it (shuffles).
template <int LPE>
DEV CatRow categorical_row(const float* z, int K, int l, uint32_t kes, bool sample) {
  float m = -INFINITY, bv = -INFINITY;
  int bi = K;
  for (int k = l; k < K; k += LPE) {
    const float zk = z[k];
    m = fmaxf(m, zk);
    const float s = sample ? zk + gumbel(kes, (uint32_t)k) : zk;
    if (s > bv) {   // ascending k: an equal later value does not replace
      bv = s;
      bi = k;
    }
  }
#pragma unroll
  for (int o = LPE / 2; o > 0; o >>= 1) {
    m = fmaxf(m, __shfl_xor(m, o, LPE));
    const float ov = __shfl_xor(bv, o, LPE);
    const int oi = __shfl_xor(bi, o, LPE);
    if (ov > bv || (ov == bv && oi < bi)) {
      bv = ov;
      bi = oi;
    }
  }
  float se = 0.f;
  for (int k = l; k < K; k += LPE) se += __expf(z[k] - m);
#pragma unroll
  for (int o = LPE / 2; o > 0; o >>= 1) se += __shfl_xor(se, o, LPE);
  CatRow c;
  c.a = bi < K ? bi : 0;   // (no comparison held: NaN logits; stay inside the row)
  c.lse = m + __logf(se);
  c.logp = z[c.a] - c.lse;
  return c;
}

// Row-major buffer rows from the normalised LDS tile: one 16-byte store per 16 bytes of features
// instead of ROWS element stores per feature (fire-and-forget, overlaps the MFMA layers).  bf16 /
// fp32: the tile and the buffer share the element type; split-bf16: the 32-byte hi|lo group layout
// too; fp8: the tile is e4m3 but the buffer rows are bf16, so they leave from a bf16 staging tile
// xsb [ROWS][d1] (element stores strided by the row length were 2.6x the bf16 kernel's time).
// dst: the buffer row of tile row 0.
template <int DT, int NTHR>
DEV void store_tile_rows(typename Prec<XStore<DT>::DTX>::T* dst, const PolicyTiles<DT>& t,
                         const typename Prec<XStore<DT>::DTX>::T* xsb, int d1, int nvalid, int tid) {
  using XB = typename Prec<XStore<DT>::DTX>::T;
  constexpr int EPC = 16 / sizeof(XB);
  const int ch = d1 / EPC;
  for (int i = tid; i < nvalid * ch; i += NTHR) {
    const int r = i / ch, c = i - r * ch;
    const void* src = DT == DT_FP8 ? static_cast<const void*>(xsb + r * d1 + c * EPC)
                                   : static_cast<const void*>(t.xs + r * t.ld1 + c * EPC);
    *reinterpret_cast<uint4*>(dst + (size_t)r * d1 + c * EPC) = *reinterpret_cast<const uint4*>(src);
  }
}

// The kernels' launch form: 8 waves (2 per SIMD: twice the threads of the VALU-heavy observe /
// sample / env phases) for bf16x3 / bf16 / fp8 16-row tiles, 4 for fp32 operands and 32-row
// tiles (twice the fragment registers: the 8-wave form spills)
template <int DT, int ROWS> constexpr int POLICY_WAVES = (DT == DT_F32 || ROWS > 16) ? 4 : 8;
