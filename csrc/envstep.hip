// Episode bookkeeping of one step of a device-stepped tensor env (runtime/engine_hip.py
// rollout_stepped): the part of VecEnv.step that follows the env's own dynamics, as ONE launch that
// writes the rollout buffer rows directly.
//
// The env's dynamics and reset draw are the user's torch ops (new_state, reward, terminal,
// reset_state); per env e < E this kernel does
//   el = ep_len + 1, er = ep_ret + reward (unclipped), done = terminal || el >= limit
//   rewards_row = reward clipped to +-reward_clip (reward_clip > 0), dones_row = done
//   done: the env's tile gets (er, 1), el = er = 0
//   state = done ? reset_state : new_state
// and per tile of ENVSTEP_TILE (16) envs the finished-episode (return sum, count) pair in the rollout
// kernel's epstat layout, so obs_reduce consumes it unchanged.
//
// A workgroup owns ES_ENVS consecutive envs (16 tiles): thread = env for the scalars, then the
// workgroup's [envs][S] state slab as one coalesced pass.  No atomics: every output element has one
// owner, and a tile's sum is added by one thread in env order, so a launch is deterministic.  The
// kernel's only global stores are the outputs listed in EnvStepArgs.
//
// bootstrap_time_limit (EnvStepArgs fin_*, trunc_row; null: none of this runs): an env that ended by
// the step limit alone also gets trunc_row = 1 and its final-observation row (fin_src: the rows one
// rows-only act launch made from observe(new_state)) copied into this step's x_fin slot (fin_dst),
// 16 bytes per thread and turn.
#include "kernels.h"
#include "common.h"

namespace {

constexpr int ES_ENVS = 256;
static_assert(ES_ENVS % ENVSTEP_TILE == 0, "a workgroup owns whole tiles");

__global__ __launch_bounds__(ES_ENVS) void env_advance_kernel(EnvStepArgs a) {
  __shared__ float fin_ret[ES_ENVS];
  __shared__ float fin_cnt[ES_ENVS];
  __shared__ unsigned char dn[ES_ENVS];
  const int tid = threadIdx.x;
  const int e0 = blockIdx.x * ES_ENVS;          // (E <= 2^30: the binding checks)
  const int e = e0 + tid;
  float fr = 0.f, fc = 0.f;
  unsigned char d = 0;
  if (e < a.E) {
    const float r = a.reward[e];
    int el = a.ep_len[e] + 1;
    float er = a.ep_ret[e] + r;
    const bool term = a.terminal[e] != 0;
    const bool done = term || el >= a.limit;
    if (done) {
      fr = er;
      fc = 1.f;
      el = 0;
      er = 0.f;
      d = term ? 1 : 2;   // 2: truncated (read by the final-row copy below)
    }
    if (a.trunc_row != nullptr) a.trunc_row[e] = d == 2 ? 1.f : 0.f;
    a.ep_len[e] = el;
    a.ep_ret[e] = er;
    const float c = a.reward_clip;
    // (comparisons, not fminf / fmaxf: a NaN reward stays NaN, as torch.clamp)
    a.rewards_row[e] = c > 0.f ? (r < -c ? -c : (r > c ? c : r)) : r;
    a.dones_row[e] = done ? 1.f : 0.f;
  }
  fin_ret[tid] = fr;
  fin_cnt[tid] = fc;
  dn[tid] = d;
  __syncthreads();
  // ---- per-tile episode stats: the tile's first thread adds its 16 envs in order (envs >= E: 0) ----
  if ((tid & (ENVSTEP_TILE - 1)) == 0 && e < a.E) {
    float sr = 0.f, sc = 0.f;
#pragma unroll
    for (int k = 0; k < ENVSTEP_TILE; ++k) {
      sr += fin_ret[tid + k];
      sc += fin_cnt[tid + k];
    }
    float* ep = a.epstat + (size_t)(e / ENVSTEP_TILE) * 2;
    if (a.init) {
      ep[0] = sr;
      ep[1] = sc;
    } else {
      ep[0] += sr;
      ep[1] += sc;
    }
  }
  // ---- state rows of this workgroup's envs: thread = element (coalesced), the env's done flag from LDS ----
  const int nenv = min(ES_ENVS, a.E - e0);
  const int S = a.S;
  const size_t base = (size_t)e0 * S;
  for (int i = tid; i < nenv * S; i += ES_ENVS) {   // (S < 2^20: nenv * S < 2^28)
    const int le = i / S;
    const float* src = dn[le] ? a.reset_state : a.new_state;
    a.state[base + i] = src[base + i];
  }
  if (a.fin_dst != nullptr) {
    const int ch = a.fin_row_bytes >> 4;   // 16-byte chunks per row (the binding checks the multiple)
    const uint4* src = static_cast<const uint4*>(a.fin_src) + (size_t)e0 * ch;
    uint4* dst = static_cast<uint4*>(a.fin_dst) + (size_t)e0 * ch;
    for (int i = tid; i < nenv * ch; i += ES_ENVS)   // (row bytes < 2^20: the binding checks)
      if (dn[i / ch] == 2) dst[i] = src[i];
  }
}

}  // namespace

extern "C" void launch_env_advance(const EnvStepArgs& a, hipStream_t s) {
  const int nblk = (a.E + ES_ENVS - 1) / ES_ENVS;
  hipLaunchKernelGGL(env_advance_kernel, dim3(nblk), dim3(ES_ENVS), 0, s, a);
  HIP_CHECK_LAUNCH();
}
