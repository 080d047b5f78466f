// Advantage normalisation (Params.adv_norm_scope global | minibatch): the sums of the raw advantages
// (and returns) over a set of buffer rows, and the block of four fp32 scalars the update kernels and
// the metrics read,
//   block = [mean, inv, std, explained_variance],
//   mean = S1 / n,  var = max(S2 - S1 * mean, 0) / (n - 1),  std = sqrt(var),  inv = 1 / (std + 1e-8),
//   explained_variance = 1 - var(adv) / var(ret)   (NaN when var(ret) = 0),
// ops/oracle.adv_sums / adv_block's arithmetic: fp64 throughout, every operation rounded on its own
// (no FMA), the block rounded to fp32 once.  The sums S = [sum a, sum a^2, sum r, sum r^2] are fp64,
// taken in a fixed order (per thread in row order, a workgroup tree, then one workgroup over the
// per-workgroup partials): no atomics.  The update kernels apply the block at their one advantage
// load (MlpArgs::adv_norm, csrc/common.h adv_norm_apply); the adv buffer itself stays raw.
#include "kernels.h"
#include "common.h"

namespace {

constexpr int ADV_NT = 256;                  // threads per workgroup (a power of two)
constexpr int ADV_IPT = 4;                   // rows per thread
constexpr int ADV_ROWS = ADV_NT * ADV_IPT;   // rows per workgroup

// fixed-order sums of four values per thread over the workgroup (red [4][ADV_NT]), like
// csrc/retnorm.hip block_sum2
DEV void block_sum4(const double (&s)[4], double* red, double* __restrict__ out) {
  const int j = threadIdx.x;
#pragma unroll
  for (int q = 0; q < 4; ++q) red[q * ADV_NT + j] = s[q];
  __syncthreads();
  for (int w = ADV_NT / 2; w > 0; w >>= 1) {
    if (j < w) {
#pragma unroll
      for (int q = 0; q < 4; ++q) red[q * ADV_NT + j] += red[q * ADV_NT + j + w];
    }
    __syncthreads();
  }
  if (j < 4) out[j] = red[j * ADV_NT];
}

// sums fp64[4], n -> block fp32[4]; a product of two fp32 values is exact in fp64, so only the
// operations here need their own rounding
DEV void adv_finish(const double* __restrict__ sums, double n, float* __restrict__ block) {
#pragma clang fp contract(off)
  const double S1 = sums[0], S2 = sums[1], R1 = sums[2], R2 = sums[3];
  const double mean = S1 / n;
  const double m2 = S2 - S1 * mean;
  const double var = (m2 > 0.0 ? m2 : 0.0) / (n - 1.0);
  const double sd = sqrt(var);
  const double inv = 1.0 / (sd + 1e-8);
  const double rmean = R1 / n;
  const double r2 = R2 - R1 * rmean;
  const double rvar = (r2 > 0.0 ? r2 : 0.0) / (n - 1.0);
  const double ev = rvar > 0.0 ? 1.0 - var / rvar : (double)__builtin_nanf("");
  block[0] = (float)mean;
  block[1] = (float)inv;
  block[2] = (float)sd;
  block[3] = (float)ev;
}

// part [gridDim.x][4]: the workgroup's sums over rows idx ? idx[i] : i, i in its ADV_ROWS of [0, n).
// ret may be null (its two sums are then 0).  An index outside [0, nrows) is the caller's error (the
// engine checks its minibatch on the host); it is clamped here so that no read leaves the buffers.
__global__ __launch_bounds__(ADV_NT) void adv_stats_kernel(const float* __restrict__ adv,
                                                           const float* __restrict__ ret,
                                                           const int* __restrict__ idx, int n, int nrows,
                                                           double* __restrict__ part) {
  __shared__ double red[4 * ADV_NT];
  const long long base = (long long)blockIdx.x * ADV_ROWS;
  float av[ADV_IPT], rv[ADV_IPT];
#pragma unroll
  for (int k = 0; k < ADV_IPT; ++k) {
    const long long i = base + (long long)k * ADV_NT + threadIdx.x;
    const bool ok = i < n;
    int src = ok ? (idx != nullptr ? idx[i] : (int)i) : 0;
    src = min(max(src, 0), nrows - 1);
    av[k] = ok ? adv[src] : 0.f;
    rv[k] = (ok && ret != nullptr) ? ret[src] : 0.f;
  }
  double s[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int k = 0; k < ADV_IPT; ++k) {
    const double a = (double)av[k], r = (double)rv[k];
    s[0] += a;
    s[1] += a * a;
    s[2] += r;
    s[3] += r * r;
  }
  block_sum4(s, red, part + 4 * (size_t)blockIdx.x);
}

// sums[0..3] = the sums of part [nblk][4] in a fixed order; block != null: the finishing arithmetic
// in the same launch
__global__ __launch_bounds__(ADV_NT) void adv_moments_kernel(const double* __restrict__ part, int nblk,
                                                             double* __restrict__ sums, double n,
                                                             float* __restrict__ block) {
  __shared__ double red[4 * ADV_NT];
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  for (int b = threadIdx.x; b < nblk; b += ADV_NT) {
#pragma unroll
    for (int q = 0; q < 4; ++q) s[q] += part[4 * (size_t)b + q];
  }
  block_sum4(s, red, sums);
  if (block != nullptr && threadIdx.x == 0) {
    // (the tree's results, ordered before this read by its last barrier: the values sums[] got)
    const double t[4] = {red[0], red[ADV_NT], red[2 * ADV_NT], red[3 * ADV_NT]};
    adv_finish(t, n, block);
  }
}

// the finishing arithmetic alone: the path with an all-reduce of the sums in between
__global__ void adv_block_kernel(const double* __restrict__ sums, double n, float* __restrict__ block) {
  if (threadIdx.x == 0 && blockIdx.x == 0) adv_finish(sums, n, block);
}

}  // namespace

extern "C" int adv_stats_blocks(int n) { return (n + ADV_ROWS - 1) / ADV_ROWS; }

// adv / ret: [nrows] (ret null: no return sums); idx: optional [n] rows (null: rows 0 .. n - 1, n <= nrows);
// part: adv_stats_blocks(n) x 4 doubles of scratch; sums [4]; block: optional fp32 [4] finished from the
// sums with the count n_total (null: the sums only)
extern "C" void launch_adv_stats(const float* adv, const float* ret, const int* idx, int n, int nrows, double* part,
                                 double* sums, double n_total, float* block, hipStream_t s) {
  const int nblk = adv_stats_blocks(n);
  hipLaunchKernelGGL(adv_stats_kernel, dim3(nblk), dim3(ADV_NT), 0, s, adv, ret, idx, n, nrows, part);
  HIP_CHECK_LAUNCH();
  hipLaunchKernelGGL(adv_moments_kernel, dim3(1), dim3(ADV_NT), 0, s, part, nblk, sums, n_total, block);
  HIP_CHECK_LAUNCH();
}

extern "C" void launch_adv_block(const double* sums, double n_total, float* block, hipStream_t s) {
  hipLaunchKernelGGL(adv_block_kernel, dim3(1), dim3(64), 0, s, sums, n_total, block);
  HIP_CHECK_LAUNCH();
}
