// The in-kernel envs' physics, written once: the rollout kernel (csrc/rollout.hip) and the
// evaluation kernel (csrc/eval.hip) both step their envs with these, so the two are bit-equal by
// construction and both are held to the same torch env (envs/vec_env.py).  kind 0: the synthetic
// S = O dim env; kind 1: the pendulum (state (th, thdot), obs (cos th, sin th, thdot)); kind 2: the
// continuous cart-pole (state = obs = (x, x_dot, th, th_dot), terminal on the NEW state).
// The env state is a [ROWS][S] fp32 tile in LDS; `act` the [ROWS][A] actions of the step.
#pragma once
#include <type_traits>

#include "kernels.h"
#include "mlp_core.h"

constexpr float SYN_DECAY = 0.9f, SYN_DRIVE = 0.1f, SYN_NOISE = 0.05f, SYN_RESET = 0.1f;
constexpr float SYN_TERM_P = 0.002f;
constexpr float ENV_PI = 3.14159265358979f, ENV_2PI = 6.28318530717959f;
constexpr uint32_t RESET_STEP_KEY = 0xFFFFFFFFu;   // VecEnv.reset()'s step key
constexpr int KIND_CARTPOLE = 2;
// CartPoleContinuousEnv's constants (envs/vec_env.py), each the fp32 rounding of the double the
// torch env multiplies its fp32 tensors with
constexpr float CP_GRAVITY = 9.8f, CP_HALF_LEN = 0.5f, CP_FORCE_MAG = 10.f, CP_DT = 0.02f;
constexpr float CP_MASS_POLE = 0.1f;
constexpr float CP_TOTAL_MASS = (float)(1.0 + 0.1);   // MASS_CART + MASS_POLE, summed in double
constexpr float CP_PML = (float)(0.1 * 0.5);          // MASS_POLE * HALF_LEN
constexpr float CP_FOUR_THIRDS = (float)(4.0 / 3.0);
constexpr float CP_X_LIMIT = 2.4f;
constexpr float CP_THETA_LIMIT = (float)(12.0 * 2.0 * 3.14159265358979323846 / 360.0);
constexpr float CP_RESET_RANGE = 0.05f;

// observation of env r, dim d.  KIND is a template parameter: with a runtime kind the
// pendulum's libm cosf/sinf (Payne-Hanek reduction, divergent per lane) was inlined into each
// of the ROWS unrolled iterations of the synthetic env's observe loop (~2,500 dead
// instructions per step and a 3x slower phase).
template <int KIND>
DEV float env_obs(const float* st, int S, int r, int d) {
  if constexpr (KIND == 1) {  // pendulum: (cos th, sin th, thdot)
    const float th = st[r * S + 0];
    return d == 0 ? cosf(th) : (d == 1 ? sinf(th) : st[r * S + 1]);
  } else {
    return st[r * S + d];
  }
}
// f(integral_constant<int, kind>): the caller's loop body compiled once per kind
template <typename F>
DEV void env_kind_switch(int kind, F&& f) {
  if (kind == 1) f(std::integral_constant<int, 1>{});
  else f(std::integral_constant<int, 0>{});
}

// synthetic dynamics, per state dim d: drive weight and driving action index (LDS tables filled
// once per launch: no per-step modulo)
DEV void syn_tables(float* wdrv, int* jdx, int S, int A, int tid, int nthr) {
  for (int d = tid; d < S; d += nthr) {
    wdrv[d] = 0.5f + (float)(d % 7) / 7.0f;
    jdx[d] = d % A;
  }
}

// synthetic reward: 1 - mean_j (clamp(a_j) - tanh(s_j))^2 over j < min(A, O); one term of the sum
DEV float syn_err_term(float av, float sv) {
  const float ac = fminf(fmaxf(av, -1.f), 1.f);
  const float d = ac - fast_tanh(sv);
  return d * d;
}
// The cart-pole: CartPoleContinuousEnv._dynamics (envs/vec_env.py) operation for operation, in
// its order, every operation rounded to fp32 on its own (no contraction into FMAs): it differs
// from the torch env's unfused ops only in the ulps of sinf / cosf (and of a division where the
// torch device multiplies by a scalar's reciprocal).
struct CartPoleState { float x, xd, th, thd; };
DEV CartPoleState cartpole_next(const float* s, float a0) {
#pragma clang fp contract(off)
  const float x = s[0], xd = s[1], th = s[2], thd = s[3];
  const float force = CP_FORCE_MAG * fminf(fmaxf(a0, -1.f), 1.f);
  const float c = cosf(th), sn = sinf(th);
  const float temp = (force + CP_PML * thd * thd * sn) / CP_TOTAL_MASS;
  const float thacc = (CP_GRAVITY * sn - c * temp) /
                      (CP_HALF_LEN * (CP_FOUR_THIRDS - CP_MASS_POLE * c * c / CP_TOTAL_MASS));
  const float xacc = temp - CP_PML * thacc * c / CP_TOTAL_MASS;
  CartPoleState n;
  n.x = x + CP_DT * xd;
  n.xd = xd + CP_DT * xacc;
  n.th = th + CP_DT * thd;
  n.thd = thd + CP_DT * thacc;
  return n;
}
DEV bool cartpole_terminal(const CartPoleState& n) {
  return fabsf(n.x) > CP_X_LIMIT || fabsf(n.th) > CP_THETA_LIMIT;
}
// reset of tile row r (env e) keyed (reset key, e, step): every dim uniform in +-CP_RESET_RANGE
DEV void cartpole_reset(float* st, int S, int r, uint32_t key_reset, uint32_t e, uint32_t step) {
#pragma clang fp contract(off)
#pragma unroll
  for (int d = 0; d < 4; ++d)
    st[r * S + d] = (2.f * uniform01(keyed(key_reset, e, step, (uint32_t)d)) - 1.f) * CP_RESET_RANGE;
}

// unclipped reward and termination of env e (tile row r) for this step's action; err: the
// synthetic env's sum of syn_err_term over its na dims (unused by the pendulum and the cart-pole).
// Kinds 0 / 1 only read st.  The cart-pole ADVANCES its row here: see below.
DEV float env_reward(int kind, float* st, int S, const float* act, int A, int r, float err, int na,
                     uint32_t key_term, uint32_t e, uint32_t kstep, bool& term) {
  term = false;
  if (kind == KIND_CARTPOLE) {
    // Terminal on the NEW state.  The step is computed once, here, and stashed in LDS for
    // env_transition, not recomputed there: two inlined copies of the step give the same bits only
    // as long as the compiler treats libm's sinf / cosf (whose operations carry their own
    // contraction flags) the same way in both, and no test can see a done flag and a stored state
    // that disagree by an ulp at a threshold.  One computation cannot disagree with itself, and it
    // is one sinf / cosf pair per env and step, not two.  The stash is the env's own state row:
    // in the kernels' phase (d) this lane is the row's only reader (the other lanes of the env
    // read st for the synthetic reward only) and nothing reads st between here and phase (e), so
    // the four floats the flag came from ARE the new state, env_transition only overwrites the
    // rows whose done flag is set, and the stash costs no LDS and no pointer (a separate
    // [ROWS][4] tile cost every instantiation of both kernels 2-3 VGPRs).
    float* row = st + r * S;
    const CartPoleState n = cartpole_next(row, act[r * A]);
    row[0] = n.x;
    row[1] = n.xd;
    row[2] = n.th;
    row[3] = n.thd;
    term = cartpole_terminal(n);
    return 1.f;
  }
  if (kind == 1) {
    float th = st[r * S], thd = st[r * S + 1];
    float u = fminf(fmaxf(act[r * A], -2.f), 2.f);
    float thn = fmodf(th + ENV_PI, ENV_2PI);
    if (thn < 0.f) thn += ENV_2PI;
    thn -= ENV_PI;
    return -(thn * thn + 0.1f * thd * thd + 0.001f * u * u);
  }
  term = uniform01(keyed(key_term, e, kstep, 0u)) < SYN_TERM_P;
  return 1.f - err / (float)na;
}

// pendulum reset of tile row r (env e) keyed (reset key, e, step)
DEV void pend_reset(float* st, int S, int r, uint32_t key_reset, uint32_t e, uint32_t step) {
  float u0 = uniform01(keyed(key_reset, e, step, 0u));
  float u1 = uniform01(keyed(key_reset, e, step, 1u));
  st[r * S] = (2.f * u0 - 1.f) * ENV_PI;
  st[r * S + 1] = 2.f * u1 - 1.f;
}
DEV void pend_step(float* st, int S, int r, float a0) {
  float th = st[r * S], thd = st[r * S + 1];
  float u = fminf(fmaxf(a0, -2.f), 2.f);
  float nthd = thd + (-3.f * 10.f / 2.f * sinf(th + ENV_PI) + 3.f * u) * 0.05f;
  float nth = th + nthd * 0.05f;
  nthd = fminf(fmaxf(nthd, -8.f), 8.f);
  st[r * S] = nth;
  st[r * S + 1] = nthd;
}

// synthetic item = (row, dim pair p): one Box-Muller pair gives the two dims' noise
struct SynItem {
  float st0, st1, a0, a1, w0, w1;
  uint32_t key;
  bool done, has1;
  int d0;
};
// done: the in-place reset (SYN_RESET * noise), else the transition
DEV void syn_item_next(const SynItem& q, int p, float& n0, float& n1) {
  const float2 g = gauss_pair(q.key, (uint32_t)p);
  if (q.done) {
    n0 = SYN_RESET * g.x;
    n1 = SYN_RESET * g.y;
  } else {
    const float a0 = fminf(fmaxf(q.a0, -1.f), 1.f);
    const float a1 = fminf(fmaxf(q.a1, -1.f), 1.f);
    n0 = SYN_DECAY * q.st0 + SYN_DRIVE * fast_tanh(q.w0 * a0) + SYN_NOISE * g.x;
    n1 = SYN_DECAY * q.st1 + SYN_DRIVE * fast_tanh(q.w1 * a1) + SYN_NOISE * g.y;
  }
}

// State transition of the whole tile, with the in-place reset of the rows whose done_s is set.
// kes: this step's per-row key prefixes [env | reset] at kes[ROWS + r] / kes[2 ROWS + r].  The
// caller's barriers separate it from the writers of act / done_s / kes and the readers of st.
template <int ROWS, int NTHR>
DEV void env_transition(int kind, float* st, int S, const float* act, int A, const float* done_s,
                        const uint32_t* kes, const float* wdrv, const int* jdx, uint32_t key_reset, int e0,
                        uint32_t kstep, int tid) {
  // the one-lane-per-env kinds share one branch (and one `tid < ROWS` region): a second top-level
  // branch for the cart-pole tipped two 4-wave per-step-filter forms of the rollout kernel, 3 and 4
  // VGPRs under 256, into AGPR spills
  if (kind != 0) {
    if (tid < ROWS) {
      const bool done = done_s[tid] > 0.5f;
      if (kind == 1) {
        if (done) pend_reset(st, S, tid, key_reset, (uint32_t)(e0 + tid), kstep);
        else pend_step(st, S, tid, act[tid * A]);
      } else if (done) {   // cart-pole: the rows already hold their new state (env_reward), only the resets are left
        cartpole_reset(st, S, tid, key_reset, (uint32_t)(e0 + tid), kstep);
      }
    }
    return;
  }
  // consecutive threads on consecutive pairs of one row: the ROWS x S/2 items spread evenly over
  // the threads and the per-dim constants come from the LDS tables.  Two items per turn with
  // every LDS read of both issued before any state store (items never share a state slot),
  // so the second item's loads, hashes and transcendentals overlap the first's instead of
  // waiting behind its stores; the reset / step choice is a select, not a branch.
  const int np = (S + 1) >> 1;
  int r = tid / np, p = tid - r * np;
  const int sr = NTHR / np, sp = NTHR - sr * np;
  auto load = [&](int rr, int pp) {
    SynItem q;
    q.d0 = 2 * pp;
    q.has1 = q.d0 + 1 < S;
    const int d1 = q.has1 ? q.d0 + 1 : q.d0;
    q.done = done_s[rr] > 0.5f;
    q.key = q.done ? kes[2 * ROWS + rr] : kes[ROWS + rr];
    q.st0 = st[rr * S + q.d0];
    q.st1 = st[rr * S + d1];
    q.a0 = act[rr * A + jdx[q.d0]];
    q.a1 = act[rr * A + jdx[d1]];
    q.w0 = wdrv[q.d0];
    q.w1 = wdrv[d1];
    return q;
  };
  while (r < ROWS) {
    int r2 = r + sr, p2 = p + sp;
    if (p2 >= np) { p2 -= np; ++r2; }
    const bool v2 = r2 < ROWS;
    const SynItem q1 = load(r, p);
    const SynItem q2 = load(v2 ? r2 : r, v2 ? p2 : p);   // past the end: re-read item 1 (unused)
    float n10, n11, n20, n21;
    syn_item_next(q1, p, n10, n11);
    syn_item_next(q2, v2 ? p2 : p, n20, n21);
    st[r * S + q1.d0] = n10;
    if (q1.has1) st[r * S + q1.d0 + 1] = n11;
    if (v2) {
      st[r2 * S + q2.d0] = n20;
      if (q2.has1) st[r2 * S + q2.d0 + 1] = n21;
    }
    r = r2 + sr;
    p = p2 + sp;
    if (p >= np) { p -= np; ++r; }
  }
}

// The in-place reset alone, of the rows whose flag is negative (the rollout kernel's truncated rows,
// stepped as not done first so that their final observation could be read): env_transition's reset
// expressions on the same keys, so the state is the bits its done branch would have left.
template <int ROWS, int NTHR>
DEV void env_reset_rows(int kind, float* st, int S, const float* flag_s, const uint32_t* kes, uint32_t key_reset,
                        int e0, uint32_t kstep, int tid) {
  if (kind != 0) {
    if (tid < ROWS && flag_s[tid] < -0.5f) {
      if (kind == 1) pend_reset(st, S, tid, key_reset, (uint32_t)(e0 + tid), kstep);
      else cartpole_reset(st, S, tid, key_reset, (uint32_t)(e0 + tid), kstep);
    }
    return;
  }
  const int np = (S + 1) >> 1;
  for (int i = tid; i < ROWS * np; i += NTHR) {
    const int r = i / np, p = i - r * np;
    if (flag_s[r] < -0.5f) {
      const float2 g = gauss_pair(kes[2 * ROWS + r], (uint32_t)p);
      st[r * S + 2 * p] = SYN_RESET * g.x;
      if (2 * p + 1 < S) st[r * S + 2 * p + 1] = SYN_RESET * g.y;
    }
  }
}

// Fresh envs for every row of the tile, as VecEnv.reset() (step key RESET_STEP_KEY)
template <int ROWS, int NTHR>
DEV void env_reset_fresh(int kind, float* st, int S, uint32_t key_reset, int e0, int tid) {
  if (kind != 0) {
    if (tid < ROWS) {
      if (kind == 1) pend_reset(st, S, tid, key_reset, (uint32_t)(e0 + tid), RESET_STEP_KEY);
      else cartpole_reset(st, S, tid, key_reset, (uint32_t)(e0 + tid), RESET_STEP_KEY);
    }
    return;
  }
  const int np = (S + 1) >> 1;
  for (int i = tid; i < ROWS * np; i += NTHR) {
    const int r = i / np, p = i - r * np;
    const float2 g = gauss_pair(key_es(key_reset, (uint32_t)(e0 + r), RESET_STEP_KEY), (uint32_t)p);
    st[r * S + 2 * p] = SYN_RESET * g.x;
    if (2 * p + 1 < S) st[r * S + 2 * p + 1] = SYN_RESET * g.y;
  }
}
