// Batched policy evaluation kernel (the reference's test.py, one env at batch 1
// on the CPU): one launch runs WHOLE episodes for a batch of fresh evaluation envs.
//
// Each workgroup owns ROWS envs from their reset to the end of their first episode.  Per step,
// entirely on-chip, the rollout kernel's pipeline without its outputs:
//   obs (env state in LDS) -> normalise with the FIXED (mean, 1/std) + clamp
//   -> policy MLP on MFMA (csrc/policy_step.h, the rollout's precisions)
//   -> action: mu (deterministic) or mu + sigma * eps, eps keyed (action key, env, step)
//   -> env physics (csrc/env_core.h), unclipped reward, done / in-place reset
// The env state is created in-kernel (reset key step 0xFFFFFFFF, as VecEnv.reset()) and never
// leaves LDS: the kernel reads no env state from global memory and writes none.  The only global
// stores are ret[E] (sum of the unclipped rewards in step order) and len[E], frozen at an env's
// first done.  No [T][E] buffer rows, x^T, moments or episode stats: less LDS than the rollout and
// no stores on the step path.
//
// The policy step and the env physics are the code the rollout kernel runs (the two headers), so
// an evaluation env and a rollout env with the same keys see the same trajectory bit for bit.
//
// Reference: test.py:24-65 (one env, batch 1, python loop).
#include "env_core.h"
#include "policy_step.h"

namespace {

// the launch's dynamic LDS: the kernel's pointers and the host's byte count from one carve
template <int DT, int ROWS>
struct EvalLds {
  LdsCarve cv;
  const int O, A, S;
  float* st = cv.take<float>(ROWS * S);           // env state
  PolicyTiles<DT> t;
  float* actb = cv.take<float>(ROWS * A);         // sampled actions (stochastic)
  float* nm = cv.take<float>(O);                  // the fixed (mean, 1/std) of every feature
  float* ninv = cv.take<float>(O);
  float* done_s = cv.take<float>(ROWS);
  int* envlen = cv.take<int>(ROWS);               // the env's own step counter (auto-reset)
  int* eplen = cv.take<int>(ROWS);                // first-episode length / return, frozen at done
  float* epret = cv.take<float>(ROWS);
  int* fin = cv.take<int>(ROWS);                  // 1: the first episode has ended
  int* nfin = cv.take<int>(1);                    // finished valid envs of this workgroup
  uint32_t* kes = cv.take<uint32_t>(3 * ROWS);    // per-env key prefixes of this step: action, env, reset
  float* wdrv = cv.take<float>(S);                // synthetic dynamics tables (env_core.h syn_tables)
  int* jdx = cv.take<int>(S);
  float* lsg = cv.take<float>(2 * A);             // [log sigma | sigma]
  __host__ __device__ EvalLds(char* smem, const EvalArgs& a)
      : cv(smem), O(a.O), A(a.A), S(a.S), t(cv, a.net, ROWS, a.A) {}
};

// CAT: the categorical head (EvalArgs::dist 1) on the cart-pole's physics, as the rollout kernel's: phases (c)
// and (d) are one per-env phase and the env kind a constant.  A template parameter so that the Gaussian forms
// keep their instructions.
template <int DT, int ROWS, int NW, bool CAT = false>
__global__ __launch_bounds__(NW * 64) void eval_kernel(EvalArgs a) {
  using P = Prec<DT>;
  constexpr int NTHR = 64 * NW;
  static_assert(ROWS % 4 == 0 && NTHR % ROWS == 0 && (NTHR / ROWS) <= 64, "eval tiling");
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int e0 = blockIdx.x * ROWS;
  const int nvalid = min(ROWS, a.E - e0);
  const int O = a.O, A = a.A, S = a.S;
  const bool det = a.deterministic != 0;
  const int kind = CAT ? KIND_CARTPOLE : a.kind;

  extern __shared__ __attribute__((aligned(16))) char smem[];
  const EvalLds<DT, ROWS> L(smem, a);
  PolicyStep<DT, ROWS, NW> ps(a.net, L.t);
  // deterministic: the action IS mu (no sample phase, no copy).  CAT: actb is the push row [ROWS][1]
  const float* act = (det && !CAT) ? L.t.mu : L.actb;
  const int actA = CAT ? 1 : A;

  // ---- reset the envs in LDS (every row of the tile: rows past E are stepped but never read
  // out), zero the padded activation tiles ----
  env_reset_fresh<ROWS, NTHR>(kind, L.st, S, a.key_reset, e0, tid);
  for (int d = tid; d < O; d += NTHR) { L.nm[d] = a.mean[d]; L.ninv[d] = a.inv_std[d]; }
  syn_tables(L.wdrv, L.jdx, S, A, tid, NTHR);
  ps.setup(L.lsg, tid);
  if (tid < ROWS) {
    L.envlen[tid] = 0;
    L.eplen[tid] = 0;
    L.epret[tid] = 0.f;
    L.fin[tid] = 0;
  }
  if (tid == 0) *L.nfin = 0;
  __syncthreads();

  // every env's first episode ends by step limit - 1 (done = terminal or length >= limit), so the
  // loop bound alone ends the launch
  for (int step = 0; step < a.limit; ++step) {
    // ---- (a) observe, normalise -> LDS tile ----
    env_kind_switch(kind, [&](auto kind_tag) {
      constexpr int KIND = decltype(kind_tag)::value;
      for (int d = tid; d < a.net.d1; d += NTHR) {
        float m = 0.f, is = 1.f;
        if (d < O) { m = L.nm[d]; is = L.ninv[d]; }
#pragma unroll
        for (int r = 0; r < ROWS; ++r) {
          float xv;
          if (d < O) xv = norm_clamp(env_obs<KIND>(L.st, S, r, d), m, is);
          else xv = pad_col(d, O);
          P::put(L.t.xs, r * L.t.ld1 + d, xv);
        }
      }
    });
    ps.prefetch(wave, lane);
    __syncthreads();
    // the key prefixes of the sample / env phases: hashed before fc1, so the layers' barriers
    // publish them (the previous step's env phase, their last reader, ended in a barrier)
    const uint32_t kstep = (uint32_t)step;   // a fresh env's global step counter starts at 0
    key_prefixes<ROWS, NTHR>(L.kes, {a.key_action, a.key_env, a.key_reset}, (uint32_t)e0, kstep, tid);
    // ---- (b) policy MLP ----
    ps.layers(wave, lane);
    // ---- (c) stochastic: a = mu + sigma * eps ----
    if (!CAT && !det) {   // (a kernel argument: the barrier below is workgroup-uniform)
      sample_loop<ROWS, NTHR>(L.kes, A, tid, true, [&](int r, int j, float eps) {
        L.actb[r * A + j] = L.t.mu[r * A + j] + L.lsg[A + j] * eps;
      });
      __syncthreads();
    }
    // ---- (d) per-env: reward, termination, first-episode bookkeeping ----
    {
      constexpr int LPE = NTHR / ROWS;
      const int r = tid / LPE, l = tid - r * LPE;
      float err = 0.f;
      const int na = min(A, O);
      if constexpr (CAT) {
        // mu holds the row's A logits (fc3's barrier published them and the key prefixes): the Gumbel-max sample,
        // or the arg-max of the logits, and the push 2 a - 1 the env takes (exactly +-1 for the two actions).
        // Every lane of every wave is here (the row step shuffles); lane 0 is the slot's only reader.
        const CatRow c = categorical_row<LPE>(L.t.mu + r * A, A, l, L.kes[r], !det);
        if (l == 0) L.actb[r] = 2.f * (float)c.a - 1.f;
      } else {
        if (a.kind == 0) {
          for (int j = l; j < na; j += LPE) err += syn_err_term(act[r * A + j], L.st[r * S + j]);
        }
#pragma unroll
        for (int o = LPE / 2; o > 0; o >>= 1) err += __shfl_xor(err, o, LPE);
      }
      if (l == 0) {
        bool term;
        const float rew = env_reward(kind, L.st, S, act, actA, r, err, na, a.key_term, (uint32_t)(e0 + r), kstep, term);
        const int el = L.envlen[r] + 1;
        const bool done = term || (el >= a.limit);
        L.envlen[r] = done ? 0 : el;
        L.done_s[r] = done ? 1.f : 0.f;
        if (!L.fin[r]) {   // finished envs keep stepping (lockstep keys) but leave the sums alone
          L.epret[r] += rew;
          L.eplen[r] += 1;
          if (done) {
            L.fin[r] = 1;
            if (r < nvalid) atomicAdd(L.nfin, 1);
          }
        }
      }
    }
    __syncthreads();
    // ---- (e) state transition (+ in-place reset on done) ----
    env_transition<ROWS, NTHR>(kind, L.st, S, act, actA, L.done_s, L.kes, L.wdrv, L.jdx, a.key_reset, e0, kstep, tid);
    __syncthreads();
    // every valid env of the tile has finished: read after the step's closing barrier (nfin's next
    // writer is the next step's phase (d), barriers away), so the exit is workgroup-uniform
    if (*L.nfin >= nvalid) break;
  }
  if (tid < nvalid) {
    a.ret[e0 + tid] = L.epret[tid];
    a.len[e0 + tid] = L.eplen[tid];
  }
}

}  // namespace

// the rollout's launch forms (policy_step.h POLICY_WAVES), 16 envs per workgroup
extern "C" void launch_eval(int dt, const EvalArgs& a, hipStream_t s) {
  dispatch_dt(dt, [&](auto d) {
    constexpr int DT = decltype(d)::value, ROWS = 16, NW = POLICY_WAVES<DT, ROWS>;
    const size_t lds = EvalLds<DT, ROWS>(nullptr, a).cv.off;
    if (a.dist != 0) {   // the categorical forms: the cart-pole, not fp8 (the binding refuses the rest first)
      if constexpr (DT != DT_FP8) {
        if (a.kind == KIND_CARTPOLE) {
          if (lds > 65536) set_max_lds_once<eval_kernel<DT, ROWS, NW, true>>(lds);
          hipLaunchKernelGGL((eval_kernel<DT, ROWS, NW, true>), dim3((a.E + ROWS - 1) / ROWS), dim3(NW * 64), lds, s, a);
          HIP_CHECK_LAUNCH();
          return;
        }
      }
      dppo_note_error(hipErrorInvalidValue, __FILE__, __LINE__);
      return;
    }
    if (lds > 65536) set_max_lds_once<eval_kernel<DT, ROWS, NW>>(lds);
    hipLaunchKernelGGL((eval_kernel<DT, ROWS, NW>), dim3((a.E + ROWS - 1) / ROWS), dim3(NW * 64), lds, s, a);
    HIP_CHECK_LAUNCH();
  });
}
