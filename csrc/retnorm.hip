// Reward normalisation (Params.reward_norm): the forward scan of the discounted return over a
// rollout's [T][E] rewards / dones and the moments of its T*E samples about a shift,
//   R = fl32(fl32(gamma * R) + r_t);  the sample R joins (S1, S2);  R = 0 where done_t,
// ops/oracle.return_scan's arithmetic (two separately rounded fp32 operations, no FMA).  The carry
// ret_acc [E] is updated in place; S1 = sum(R - shift), S2 = sum((R - shift)^2) in fp64, summed in
// a fixed order (per thread in time order, a workgroup tree, then one workgroup over the
// per-workgroup partials): no atomics.  The merge into the running (n, mean, M2) is
// csrc/obs.hip's obs_merge with O = 1.
#include "kernels.h"
#include "common.h"

namespace {

DEV float ret_step(float gamma, float R, float r) {
#pragma clang fp contract(off)
  const float g = gamma * R;
  return g + r;
}

// fixed-order sum of one value per thread over the workgroup (NT threads, a power of two)
template <int NT>
DEV void block_sum2(double s1, double s2, double* red1, double* red2, double* __restrict__ out) {
  const int j = threadIdx.x;
  red1[j] = s1;
  red2[j] = s2;
  __syncthreads();
  for (int w = NT / 2; w > 0; w >>= 1) {
    if (j < w) {
      red1[j] += red1[j + w];
      red2[j] += red2[j + w];
    }
    __syncthreads();
  }
  if (j == 0) {
    out[0] = red1[0];
    out[1] = red2[0];
  }
}

// One lane per env, forward over T, shaped like gae_kernel (csrc/optim.hip): 64-thread workgroups,
// coalesced [T][E] reads, the loads of 8 steps issued before their part of the recurrence.
// part [gridDim.x][2]: the workgroup's (S1, S2).
__global__ __launch_bounds__(64) void ret_scan_lane_kernel(const float* __restrict__ rew,
                                                           const float* __restrict__ done,
                                                           float* __restrict__ acc, const float* __restrict__ shift,
                                                           float* __restrict__ R_out, double* __restrict__ part,
                                                           int T, int E, float gamma) {
  __shared__ double red1[64], red2[64];
  const int e = blockIdx.x * 64 + threadIdx.x;
  double s1 = 0.0, s2 = 0.0;
  if (e < E) {
    const double sh = (double)shift[0];
    float R = acc[e];
    auto step = [&](size_t o, float r, float d) {
      R = ret_step(gamma, R, r);
      if (R_out != nullptr) R_out[o] = R;
      const double x = (double)R - sh;
      s1 += x;
      s2 += x * x;
      if (d != 0.f) R = 0.f;
    };
    int t = 0;
    for (; t + 8 <= T; t += 8) {
      float r[8], d[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const size_t o = (size_t)(t + k) * E + e;
        r[k] = rew[o];
        d[k] = done[o];
      }
#pragma unroll
      for (int k = 0; k < 8; ++k) step((size_t)(t + k) * E + e, r[k], d[k]);
    }
    for (; t < T; ++t) {
      const size_t o = (size_t)t * E + e;
      step(o, rew[o], done[o]);
    }
    acc[e] = R;
  }
  block_sum2<64>(s1, s2, red1, red2, part + 2 * (size_t)blockIdx.x);
}

// Parallel-in-time form for few envs and long rollouts, shaped like gae_scan_kernel: one workgroup
// per env.  The carry x (R after the done reset) moves by the affine map x -> a_t x + b_t,
// a_t = gamma * (1 - d_t), b_t = r_t * (1 - d_t); composition is associative:
//   (a2, b2) o (a1, b1) = (a2 * a1, a2 * b1 + b2).
// Thread j composes the maps of its contiguous chunk of steps, an inclusive scan from the left over
// the 256 chunk maps (LDS, Hillis-Steele) gives each chunk its incoming carry, and every thread
// replays its chunk with the lane form's arithmetic.  Only the incoming carries differ from the lane
// form (the association of the products: fp32 rounding level); a chunk behind a done starts from
// the exact 0.  part [E][2].
__global__ __launch_bounds__(256) void ret_scan_time_kernel(const float* __restrict__ rew,
                                                            const float* __restrict__ done,
                                                            float* __restrict__ acc, const float* __restrict__ shift,
                                                            float* __restrict__ R_out, double* __restrict__ part,
                                                            int T, int E, float gamma) {
  __shared__ float sA[256], sB[256];
  __shared__ double red1[256], red2[256];
  const int e = blockIdx.x, j = threadIdx.x;
  const int chunk = (T + 255) / 256;
  const int t0 = min(T, j * chunk), t1 = min(T, t0 + chunk);
  float A = 1.f, B = 0.f;
  for (int t = t0; t < t1; ++t) {
    const size_t o = (size_t)t * E + e;
    const float nt = 1.f - done[o];
    const float a = gamma * nt, b = rew[o] * nt;
    B = a * B + b;
    A = a * A;
  }
  sA[j] = A;
  sB[j] = B;
  __syncthreads();
  // after it, (sA[j], sB[j]) = map_j o map_{j-1} o ... o map_0
  for (int off = 1; off < 256; off <<= 1) {
    float a1 = 1.f, b1 = 0.f;
    const bool has = j >= off;
    if (has) { a1 = sA[j - off]; b1 = sB[j - off]; }
    __syncthreads();
    if (has) {
      sB[j] = sA[j] * b1 + sB[j];
      sA[j] = sA[j] * a1;
    }
    __syncthreads();
  }
  const float x0 = acc[e];
  float R = j > 0 ? sA[j - 1] * x0 + sB[j - 1] : x0;
  const double sh = (double)shift[0];
  double s1 = 0.0, s2 = 0.0;
  for (int t = t0; t < t1; ++t) {
    const size_t o = (size_t)t * E + e;
    R = ret_step(gamma, R, rew[o]);
    if (R_out != nullptr) R_out[o] = R;
    const double x = (double)R - sh;
    s1 += x;
    s2 += x * x;
    if (done[o] != 0.f) R = 0.f;
  }
  // every thread read acc[e] before the barriers inside block_sum2; the last chunk's carry (an
  // empty chunk passes its incoming one on) is the env's
  block_sum2<256>(s1, s2, red1, red2, part + 2 * (size_t)e);
  if (j == 255) acc[e] = R;
}

// out[0..1] = the sums of part [nblk][2], in a fixed order
__global__ __launch_bounds__(256) void ret_moments_kernel(const double* __restrict__ part, int nblk,
                                                          double* __restrict__ out) {
  __shared__ double red1[256], red2[256];
  double s1 = 0.0, s2 = 0.0;
  for (int b = threadIdx.x; b < nblk; b += 256) {
    s1 += part[2 * (size_t)b];
    s2 += part[2 * (size_t)b + 1];
  }
  block_sum2<256>(s1, s2, red1, red2, out);
}

bool ret_scan_in_time(int T, int E, int mode) { return mode == 2 || (mode == 0 && E <= 64 && T >= 512); }

}  // namespace

extern "C" int ret_scan_blocks(int T, int E, int mode) { return ret_scan_in_time(T, E, mode) ? E : (E + 63) / 64; }

// mode: launch_gae_rn's (0 auto, 1 per-env lanes, 2 parallel in time); R_out: optional [T][E]
// (null: not written); part: ret_scan_blocks(T, E, mode) x 2 doubles of scratch; s12: [2]
extern "C" void launch_ret_scan(const float* rewards, const float* dones, float* acc, const float* shift,
                                float* R_out, double* part, double* s12, int T, int E, float gamma, int mode,
                                hipStream_t s) {
  const int nblk = ret_scan_blocks(T, E, mode);
  if (ret_scan_in_time(T, E, mode))
    hipLaunchKernelGGL(ret_scan_time_kernel, dim3(nblk), dim3(256), 0, s, rewards, dones, acc, shift, R_out, part, T,
                       E, gamma);
  else
    hipLaunchKernelGGL(ret_scan_lane_kernel, dim3(nblk), dim3(64), 0, s, rewards, dones, acc, shift, R_out, part, T,
                       E, gamma);
  HIP_CHECK_LAUNCH();
  hipLaunchKernelGGL(ret_moments_kernel, dim3(1), dim3(256), 0, s, part, nblk, s12);
  HIP_CHECK_LAUNCH();
}
