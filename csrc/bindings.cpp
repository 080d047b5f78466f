// PyTorch bindings for the DPPO HIP kernels.  Every entry point validates device, dtype,
// contiguity and the exact extents the kernel's grid/indexing assumes BEFORE launching, so
// a shape bug raises a Python exception instead of faulting the GPU.  Launches go to the
// current HIP stream (graph-capturable: no allocation, no sync in here).
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include <limits>
#include <vector>

#include "kernels.h"

namespace {

hipStream_t cur_stream() { return at::hip::getCurrentHIPStream().stream(); }

// Debug mode (DPPO_DEBUG_SYNC=1 / set_debug_sync, SURVEY §5.2 "HIP_LAUNCH_BLOCKING mode"): every
// binding synchronises its stream after its launch and raises on a launch or execution error,
// naming the binding — a kernel fault surfaces at the op that caused it, not at a later sync.
bool g_debug_sync = false;
void set_debug_sync(bool on) { g_debug_sync = on; }
// Always: a launch (or LDS attribute) error the launchers recorded raises here, naming the op.
void after_launch(const char* what) {
  char msg[192];
  const int code = dppo_take_error(msg, (int)sizeof(msg));
  TORCH_CHECK(code == 0, what, ": HIP launch failed: ", msg);
  if (!g_debug_sync) return;
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipStreamSynchronize(cur_stream());
  TORCH_CHECK(e == hipSuccess, "debug-sync: ", what, " failed: ", hipGetErrorString(e));
}

// diagnostics only: per-phase cycle sums of the rollout kernel (scripts/phase_timeline.py)
unsigned long long* g_roll_tstamp = nullptr;
int64_t g_roll_tstamp_numel = 0;
void set_rollout_tstamp(torch::Tensor buf) {
  if (!buf.defined() || buf.numel() == 0) { g_roll_tstamp = nullptr; return; }
  TORCH_CHECK(buf.scalar_type() == at::kLong && buf.is_cuda() && buf.is_contiguous(), "int64 device buffer");
  g_roll_tstamp = reinterpret_cast<unsigned long long*>(buf.data_ptr<int64_t>());
  g_roll_tstamp_numel = buf.numel();
}
// diagnostics only: phase-timeline stamps of mlp_train (scripts/phase_timeline.py)
unsigned long long* g_tstamp = nullptr;
int g_tstamp_every = 1;
int64_t g_tstamp_numel = 0;
void set_train_tstamp(torch::Tensor buf, int64_t every) {
  if (!buf.defined() || buf.numel() == 0) { g_tstamp = nullptr; return; }
  g_tstamp_numel = buf.numel();
  TORCH_CHECK(buf.scalar_type() == at::kLong && buf.is_cuda() && buf.is_contiguous(), "int64 device buffer");
  TORCH_CHECK(every >= 1, "every");
  g_tstamp = reinterpret_cast<unsigned long long*>(buf.data_ptr<int64_t>());
  g_tstamp_every = (int)every;
}
int g_x_stream = 0;     // A/B: non-temporal observation-row loads in the value / update kernels
void set_x_stream(int64_t on) { g_x_stream = on ? 1 : 0; }

// dt 3 (split-bf16): one 4-byte slot per logical element (hi | lo bf16 pairs in 32-byte groups,
// csrc/common.h Prec<DT_S3>), held in int32 tensors so numel counts logical elements
at::ScalarType storage_type(int dt) {
  return dt == 0 ? at::kFloat : (dt == 1 ? at::kBFloat16 : (dt == 3 ? at::kInt : at::kByte));
}

using CT = const torch::Tensor&;
using Ints = const std::vector<int64_t>&;

void check(CT t, const char* name, at::ScalarType st, int64_t min_numel) {
  TORCH_CHECK(t.is_cuda(), name, " must be a device tensor");
  TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
  TORCH_CHECK(t.scalar_type() == st, name, " has dtype ", t.scalar_type(), ", expected ", st);
  TORCH_CHECK(t.numel() >= min_numel, name, " has ", t.numel(), " elements, kernel needs >= ", min_numel);
}

float* fptr(CT t, const char* name, int64_t min_numel) {   // a checked fp32 device array
  check(t, name, at::kFloat, min_numel);
  return t.data_ptr<float>();
}

const float* opt_scales(const torch::Tensor& q) {
  if (!q.defined() || q.numel() == 0) return nullptr;
  check(q, "qscale", at::kFloat, 6);
  return q.data_ptr<float>();
}

struct Layout {
  int off_w[6], off_wt[6], d_in[6], d_out[6], n_out[6];
};

Layout parse_layout(const std::vector<int64_t>& v) {
  TORCH_CHECK(v.size() == 30, "layout must have 30 ints");
  Layout L;
  for (int i = 0; i < 6; ++i) {
    L.off_w[i] = (int)v[i];
    L.off_wt[i] = (int)v[6 + i];
    L.d_in[i] = (int)v[12 + i];
    L.d_out[i] = (int)v[18 + i];
    L.n_out[i] = (int)v[24 + i];
    TORCH_CHECK(L.d_in[i] % 32 == 0 && L.d_out[i] % 32 == 0, "padded dims must be multiples of 32");
    TORCH_CHECK(L.n_out[i] < L.d_out[i], "n_out must leave a pad column");
  }
  return L;
}

int64_t wimg_extent(const Layout& L) {
  int64_t mx = 0;
  for (int i = 0; i < 6; ++i) {
    mx = std::max<int64_t>(mx, (int64_t)L.off_w[i] + (int64_t)L.d_out[i] * L.d_in[i]);
    mx = std::max<int64_t>(mx, (int64_t)L.off_wt[i] + (int64_t)L.d_in[i] * L.d_out[i]);
  }
  return mx;
}

// The policy fields of RolloutArgs / EvalArgs / ActArgs, filled and checked in one place
PolicyNet policy_net(int64_t dt, const Layout& L, const torch::Tensor& wimg, const std::vector<double>& scales,
                     const torch::Tensor& flat, int64_t A, int64_t std_var, const torch::Tensor& qscale) {
  TORCH_CHECK(L.d_in[1] > L.n_out[0] && L.d_in[2] > L.n_out[1], "layout: hidden widths");
  check(wimg, "wimg", storage_type((int)dt), wimg_extent(L));
  check(flat, "flat", at::kFloat, A);
  PolicyNet n{};
  n.W = wimg.data_ptr();
  n.off_w1 = L.off_w[0]; n.off_w2 = L.off_w[1]; n.off_w3 = L.off_w[2];
  n.d1 = L.d_in[0]; n.d2 = L.d_in[1]; n.d3 = L.d_in[2];
  n.n1 = L.n_out[0]; n.n2 = L.n_out[1]; n.n3 = L.n_out[2];
  n.qscale = opt_scales(qscale);
  n.s1 = (float)scales.at(0); n.s2 = (float)scales.at(1); n.s3 = (float)scales.at(2);
  n.log_std = flat.data_ptr<float>();
  n.std_var = (int)std_var;
  return n;
}

// The env fields RolloutArgs and EvalArgs share (ints kind,E,O,A,S lead both bindings' lists): the env kind
// against its state / observation / action dims (O, A >= 1) and the layout, and the four stream keys.
// dist (the optional last int of both lists, default 0): the policy head.  1, the categorical head, exists on
// the cart-pole's physics alone (two pushes: A == 2), for 16-row tiles (rows: the rollout's tile; the
// evaluation's is 16) and not in fp8; the rollout's per-step filter refuses it too (rollout_stepnorm).
template <class Args> void check_env(const Args& a, const Layout& L, int64_t dt, int64_t rows) {
  TORCH_CHECK(a.kind >= 0 && a.kind <= 2, "kind must be 0 (synthetic), 1 (pendulum) or 2 (cart-pole), got ", a.kind);
  TORCH_CHECK(a.dist == 0 || a.dist == 1, "dist: 0 Gaussian, 1 categorical, got ", a.dist);
  TORCH_CHECK(a.dist == 0 || a.kind == 2, "dist 1 (the categorical head) runs on the cart-pole's physics (kind 2) only: "
              "the other in-kernel envs take continuous actions, got kind ", a.kind);
  TORCH_CHECK(a.O >= 1 && a.A >= 1, "O / A");
  TORCH_CHECK(a.kind == 0 ? a.S == a.O : a.kind == 1 ? (a.S == 2 && a.O == 3)
                                                      : (a.S == 4 && a.O == 4 && a.A == (a.dist == 1 ? 2 : 1)),
              "state dims");
  TORCH_CHECK(a.dist == 0 || dt != 2, "dist 1 (the categorical head) has no fp8 form: a categorical update runs on the "
              "tile kernel, which fp8 does not take");
  TORCH_CHECK(a.dist == 0 || rows == 16, "dist 1 (the categorical head) is built for 16-row tiles, got rows = ", rows);
  TORCH_CHECK(L.n_out[2] == a.A && L.d_in[0] == ((a.O + 1 + 31) / 32) * 32, "layout/env mismatch");
}
template <class Args> void env_keys(Args& a, Ints keys) {
  TORCH_CHECK(keys.size() == 4, "keys: env,term,reset,action");
  a.key_env = (uint32_t)keys[0]; a.key_term = (uint32_t)keys[1]; a.key_reset = (uint32_t)keys[2];
  a.key_action = (uint32_t)keys[3];
}

// ------------------------------------------------------------------------------------------
// RolloutArgs of a rollout launch, checked: the parameter list of ext.rollout, which rollout_fin extends
RolloutArgs rollout_args(int64_t dt, int64_t rows, CT state, CT ep_len, CT ep_ret, CT wimg, Ints layout,
                         const std::vector<double>& scales, CT flat, CT mean, CT inv_std, CT shift, CT x_out, CT actions,
                         CT logp, CT rewards, CT dones, CT mom, CT epstat, Ints ints, Ints keys, double reward_clip,
                         CT qscale, CT xT_out, int64_t xT_rows) {
  TORCH_CHECK(ints.size() == 11 || ints.size() == 12, "ints: kind,E,O,A,S,T,t_base,buf_E,t0,limit,std_var[,dist]");
  RolloutArgs a{};
  env_keys(a, keys);
  TORCH_CHECK(rows == 16 || rows == 32, "rows must be 16 or 32");
  Layout L = parse_layout(layout);
  a.kind = (int)ints[0]; a.E = (int)ints[1]; a.O = (int)ints[2]; a.A = (int)ints[3]; a.S = (int)ints[4];
  a.T = (int)ints[5]; a.t_base = (int)ints[6]; a.buf_E = (int)ints[7]; a.t0 = (uint32_t)ints[8];
  a.limit = (int)ints[9];
  a.dist = ints.size() == 12 ? (int)ints[11] : 0;
  TORCH_CHECK(a.E > 0 && a.T >= 1 && a.buf_E == a.E, "bad E/T");
  check_env(a, L, dt, rows);
  const int nblk = (a.E + (int)rows - 1) / (int)rows;
  check(state, "state", at::kFloat, (int64_t)a.E * a.S);
  check(ep_len, "ep_len", at::kInt, a.E);
  check(ep_ret, "ep_ret", at::kFloat, a.E);
  a.net = policy_net(dt, L, wimg, scales, flat, a.A, ints[10], qscale);
  check(mean, "mean", at::kFloat, a.O);
  check(inv_std, "inv_std", at::kFloat, a.O);
  check(shift, "shift", at::kFloat, a.O);
  const int64_t rows_needed = (int64_t)(a.t_base + a.T + 1) * a.E;
  check(x_out, "x_out", storage_type(dt == 2 ? 1 : (int)dt), rows_needed * L.d_in[0]);
  check(actions, "actions", at::kFloat, (int64_t)(a.t_base + a.T) * a.E * a.A);
  check(logp, "logp", at::kFloat, (int64_t)(a.t_base + a.T) * a.E);
  check(rewards, "rewards", at::kFloat, (int64_t)(a.t_base + a.T) * a.E);
  check(dones, "dones", at::kFloat, (int64_t)(a.t_base + a.T) * a.E);
  check(mom, "mom", at::kFloat, (int64_t)nblk * 2 * a.O);
  check(epstat, "epstat", at::kFloat, (int64_t)nblk * 2);
  a.state = state.data_ptr<float>();
  a.ep_len = ep_len.data_ptr<int>();
  a.ep_ret = ep_ret.data_ptr<float>();
  a.mean = mean.data_ptr<float>();
  a.inv_std = inv_std.data_ptr<float>();
  a.shift = shift.data_ptr<float>();
  a.reward_clip = (float)reward_clip;
  a.x_out = x_out.data_ptr();
  a.actions = actions.data_ptr<float>();
  a.logp = logp.data_ptr<float>();
  a.rewards = rewards.data_ptr<float>();
  a.dones = dones.data_ptr<float>();
  a.mom = mom.data_ptr<float>();
  a.xT_out = nullptr;
  a.ldT = 0;
  if (xT_out.defined() && xT_out.numel() > 0) {
    // FM transposed copy of the T*E training rows: the kernel writes 8-row groups per 16-env tile
    const int64_t ld = (int64_t)a.buf_E * (a.t_base + a.T);
    TORCH_CHECK(a.t_base == 0, "xT_out is written by a whole-rollout launch (t_base == 0)");
    TORCH_CHECK(a.E % 16 == 0 && ld % 32 == 0, "xT_out needs E % 16 == 0 and T*E % 32 == 0");
    TORCH_CHECK(xT_rows >= L.d_in[0] && xT_rows % 16 == 0, "xT_out rows must cover d_in and be a multiple of 16");
    check(xT_out, "xT_out", storage_type(dt == 2 ? 1 : (int)dt), xT_rows * ld);
    a.xT_out = xT_out.data_ptr();
    a.ldT = (int)ld;
  }
  a.epstat = epstat.data_ptr<float>();
  if (g_roll_tstamp != nullptr) {
    TORCH_CHECK(g_roll_tstamp_numel >= (int64_t)nblk * 8 * 16, "rollout tstamp buffer too small ([blk][8 waves][16])");
    a.tstamp = g_roll_tstamp;
  }
  return a;
}

// ext.rollout and ext.rollout_fin: rollout_args' parameters (the pack P, deduced from it) and one body.
// rollout_fin adds bootstrap_time_limit's outputs (csrc/rollout.hip FIN): trunc [t_base + T][E] fp32
// gets 1 where an episode ended by the step limit alone, and x_fin [fin_K][E][d1] (x_out's storage
// type, zeroed by the caller) the normalised observation such a step reached before its reset, at
// row ((t_base + step) / limit) * E + e.  Every extent the kernel indexes is checked here.
template <class F> struct RolloutBind;
template <class... P> struct RolloutBind<RolloutArgs (*)(int64_t, int64_t, P...)> {
  static void run(const char* who, bool fin, CT trunc, CT x_fin, int64_t fin_K, int64_t dt, int64_t rows, P... p) {
    RolloutArgs a = rollout_args(dt, rows, p...);
    if (fin) {
      TORCH_CHECK(a.limit >= 1, "limit must be >= 1, got ", a.limit);
      const int64_t steps = (int64_t)a.t_base + a.T;
      TORCH_CHECK(fin_K >= 1 && fin_K <= std::numeric_limits<int>::max() && fin_K >= (steps + a.limit - 1) / a.limit,
                  "fin_K = ", fin_K, " is below ceil(T / limit) = ", (steps + a.limit - 1) / a.limit);
      check(trunc, "trunc", at::kFloat, steps * a.E);
      check(x_fin, "x_fin", storage_type(dt == 2 ? 1 : (int)dt), fin_K * a.E * a.net.d1);
      a.trunc = trunc.data_ptr<float>();
      a.x_fin = x_fin.data_ptr();
      a.fin_K = (int)fin_K;
    }
    launch_rollout((int)dt, a, (int)rows, cur_stream());
    after_launch(who);
  }
  static void rollout(int64_t dt, int64_t rows, P... p) { run(__func__, false, {}, {}, 0, dt, rows, p...); }
  static void rollout_fin(int64_t dt, int64_t rows, P... p, torch::Tensor trunc, torch::Tensor x_fin, int64_t fin_K) {
    run(__func__, true, trunc, x_fin, fin_K, dt, rows, p...);
  }
};
using RolloutB = RolloutBind<decltype(&rollout_args)>;

// The per-step observation-normalisation rollout (obs_norm_update = "step") as ONE cooperative
// launch (csrc/rollout.hip sn_step): `sn` = [mean f64, m2 f64, mean_f32, inv_std] of the stats the
// steps absorb (updated in place), g1 / g2 the granule buffers (int64, zero-initialised once; tags
// never reused: epoch0 grows by T per launch), err an int32 timeout word.  The launch's own
// normalisation inputs (mean / inv_std) are ignored: every step takes the freshly merged stats.
void rollout_stepnorm(int64_t dt, int64_t rows, CT state, CT ep_len, CT ep_ret, CT wimg, Ints layout,
                      const std::vector<double>& scales, CT flat, CT shift, CT x_out, CT actions, CT logp, CT rewards,
                      CT dones, CT mom, CT epstat, Ints ints, Ints keys, double reward_clip, CT qscale,
                      const std::vector<torch::Tensor>& sn, CT g1, CT g2, CT err, double n0, int64_t epoch0,
                      double var_floor) {
  TORCH_CHECK(sn.size() == 4, "sn: mean f64, m2 f64, mean_f32, inv_std");
  RolloutArgs a = rollout_args(dt, rows, state, ep_len, ep_ret, wimg, layout, scales, flat, sn[2], sn[3], shift,
                               x_out, actions, logp, rewards, dones, mom, epstat, ints, keys, reward_clip, qscale,
                               torch::Tensor(), 0);
  TORCH_CHECK(a.dist == 0, "dist 1 (the categorical head) is not built into the per-step observation filter's launch "
              "forms (obs_norm_update = step): they are the register-tight 4-wave forms");
  TORCH_CHECK(a.t_base == 0, "the per-step normalisation launch covers the whole rollout");
  const int nblk = (a.E + (int)rows - 1) / (int)rows;
  check(sn[0], "sn mean", at::kDouble, a.O);
  check(sn[1], "sn m2", at::kDouble, a.O);
  TORCH_CHECK(sn[2].data_ptr() != shift.data_ptr(), "the shift must not alias the stats being merged into");
  check(g1, "g1", at::kLong, (int64_t)sn_g1_elems(nblk, a.O));
  check(g2, "g2", at::kLong, 2 * (int64_t)a.O);
  check(err, "err", at::kInt, 1);
  TORCH_CHECK(epoch0 >= 1 && epoch0 + a.T < (int64_t)UINT32_MAX, "epoch0");
  a.sn_mean = sn[0].data_ptr<double>();
  a.sn_m2 = sn[1].data_ptr<double>();
  a.sn_mean_f32 = sn[2].data_ptr<float>();
  a.sn_inv_std = sn[3].data_ptr<float>();
  a.sn_g1 = reinterpret_cast<unsigned long long*>(g1.data_ptr<int64_t>());
  a.sn_g2 = reinterpret_cast<unsigned long long*>(g2.data_ptr<int64_t>());
  a.sn_err = reinterpret_cast<unsigned*>(err.data_ptr<int>());
  a.sn_n0 = n0;
  a.sn_epoch0 = (unsigned)epoch0;
  a.sn_var_floor = var_floor;
  launch_rollout((int)dt, a, (int)rows, cur_stream());
  after_launch(__func__);
}

// Batched policy evaluation (csrc/eval.hip): E fresh envs run to the end of their first episode;
// writes ret [E] fp32 / len [E] int32 and nothing else.  ints: kind,E,O,A,S,limit,std_var,
// deterministic and optionally dist (check_env); keys: env,term,reset,action.
void eval_rollout(int64_t dt, torch::Tensor wimg, std::vector<int64_t> layout, std::vector<double> scales,
                  torch::Tensor flat, torch::Tensor mean, torch::Tensor inv_std, torch::Tensor ret, torch::Tensor len,
                  std::vector<int64_t> ints, std::vector<int64_t> keys, torch::Tensor qscale) {
  TORCH_CHECK(dt >= 0 && dt <= 3, "dt");
  TORCH_CHECK(ints.size() == 8 || ints.size() == 9, "ints: kind,E,O,A,S,limit,std_var,deterministic[,dist]");
  EvalArgs a{};
  env_keys(a, keys);
  TORCH_CHECK(scales.size() >= 3, "scales");
  Layout L = parse_layout(layout);
  TORCH_CHECK(ints[1] > 0 && ints[1] <= (int64_t)1 << 30, "E must be in [1, 2^30], got ", ints[1]);
  TORCH_CHECK(ints[5] >= 1 && ints[5] <= (int64_t)1 << 20, "limit must be in [1, 2^20], got ", ints[5]);
  a.kind = (int)ints[0]; a.E = (int)ints[1]; a.O = (int)ints[2]; a.A = (int)ints[3]; a.S = (int)ints[4];
  a.limit = (int)ints[5]; a.deterministic = ints[7] ? 1 : 0;
  a.dist = ints.size() == 9 ? (int)ints[8] : 0;
  check_env(a, L, dt, 16);
  a.net = policy_net(dt, L, wimg, scales, flat, a.A, ints[6] ? 1 : 0, qscale);
  check(mean, "mean", at::kFloat, a.O);
  check(inv_std, "inv_std", at::kFloat, a.O);
  check(ret, "ret", at::kFloat, a.E);
  check(len, "len", at::kInt, a.E);
  TORCH_CHECK(ret.numel() == a.E && len.numel() == a.E, "ret / len must have exactly E = ", a.E, " elements, got ",
              ret.numel(), " / ", len.numel());
  a.mean = mean.data_ptr<float>();
  a.inv_std = inv_std.data_ptr<float>();
  a.ret = ret.data_ptr<float>();
  a.len = len.data_ptr<int>();
  launch_eval((int)dt, a, cur_stream());
  after_launch(__func__);
}

// One policy step for caller-supplied observations (csrc/act.hip): obs [E][O] fp32 -> actions [E][A],
// logp [E], mu [E][A], x_out (E rows of d1 in the buffer precision, e.g. a slice of x_buf), mom
// [ceil(E/16)][2][O] (overwritten with mom_init, else added to).  Every output is optional: an
// empty tensor skips it; with none of actions / logp / mu the launch writes x_out / mom only.
// ints: E,O,A,std_var,deterministic,mom_init and optionally dist (0 Gaussian, the default; 1 categorical: actions gets
// one-hot rows, mu the logits); keys: action,e_base,step_key.
void policy_act(int64_t dt, torch::Tensor wimg, std::vector<int64_t> layout, std::vector<double> scales,
                torch::Tensor flat, torch::Tensor mean, torch::Tensor inv_std, torch::Tensor shift, torch::Tensor obs,
                torch::Tensor actions, torch::Tensor logp, torch::Tensor mu, torch::Tensor x_out, torch::Tensor mom,
                std::vector<int64_t> ints, std::vector<int64_t> keys, torch::Tensor qscale) {
  TORCH_CHECK(dt >= 0 && dt <= 3, "dt");
  TORCH_CHECK(ints.size() == 6 || ints.size() == 7, "ints: E,O,A,std_var,deterministic,mom_init[,dist]");
  TORCH_CHECK(keys.size() == 3, "keys: action,e_base,step_key");
  TORCH_CHECK(scales.size() >= 3, "scales");
  Layout L = parse_layout(layout);
  ActArgs a{};
  TORCH_CHECK(ints[0] > 0 && ints[0] <= (int64_t)1 << 30, "E must be in [1, 2^30], got ", ints[0]);
  TORCH_CHECK(ints[1] >= 1 && ints[1] < (int64_t)1 << 20 && ints[2] >= 1 && ints[2] < (int64_t)1 << 20, "O / A");
  a.E = (int)ints[0]; a.O = (int)ints[1]; a.A = (int)ints[2];
  a.deterministic = ints[4] ? 1 : 0; a.mom_init = ints[5] ? 1 : 0;
  a.dist = ints.size() == 7 ? (int)ints[6] : 0;
  TORCH_CHECK(a.dist == 0 || a.dist == 1, "dist: 0 Gaussian, 1 categorical, got ", a.dist);
  TORCH_CHECK(a.dist == 0 || a.A >= 2, "a categorical head has at least 2 actions, got ", a.A);
  TORCH_CHECK(L.n_out[2] == a.A && L.d_in[0] == ((a.O + 1 + 31) / 32) * 32, "layout / O / A mismatch");
  for (int i = 0; i < 3; ++i)
    TORCH_CHECK(keys[i] >= 0 && keys[i] <= (int64_t)UINT32_MAX, "keys must be 32-bit, got ", keys[i]);
  auto given = [](const torch::Tensor& t) { return t.defined() && t.numel() > 0; };
  const int nblk = (a.E + 15) / 16;
  a.net = policy_net(dt, L, wimg, scales, flat, a.A, ints[3] ? 1 : 0, qscale);
  check(mean, "mean", at::kFloat, a.O);
  check(inv_std, "inv_std", at::kFloat, a.O);
  check(obs, "obs", at::kFloat, (int64_t)a.E * a.O);
  TORCH_CHECK(obs.numel() == (int64_t)a.E * a.O, "obs must have exactly E*O = ", (int64_t)a.E * a.O, " elements, got ",
              obs.numel());
  if (given(actions)) { check(actions, "actions", at::kFloat, (int64_t)a.E * a.A); a.actions = actions.data_ptr<float>(); }
  if (given(logp)) { check(logp, "logp", at::kFloat, a.E); a.logp = logp.data_ptr<float>(); }
  if (given(mu)) { check(mu, "mu", at::kFloat, (int64_t)a.E * a.A); a.mu = mu.data_ptr<float>(); }
  if (given(x_out)) {
    check(x_out, "x_out", storage_type(dt == 2 ? 1 : (int)dt), (int64_t)a.E * L.d_in[0]);
    TORCH_CHECK(reinterpret_cast<uintptr_t>(x_out.data_ptr()) % 16 == 0, "x_out must be 16-byte aligned");
    a.x_out = x_out.data_ptr();
  }
  if (given(mom)) {
    check(mom, "mom", at::kFloat, (int64_t)nblk * 2 * a.O);
    check(shift, "shift", at::kFloat, a.O);
    a.mom = mom.data_ptr<float>();
    a.shift = shift.data_ptr<float>();
  }
  TORCH_CHECK(a.actions || a.logp || a.mu || a.x_out || a.mom, "policy_act: no output requested");
  a.key_action = (uint32_t)keys[0]; a.e_base = (uint32_t)keys[1]; a.step_key = (uint32_t)keys[2];
  a.mean = mean.data_ptr<float>();
  a.inv_std = inv_std.data_ptr<float>();
  a.obs = obs.data_ptr<float>();
  launch_act((int)dt, a, cur_stream());
  after_launch(__func__);
}

// Episode bookkeeping of one step of a device-stepped tensor env (csrc/envstep.hip): E and S come
// from state [E][S]; reward [E], terminal [E] (uint8 or bool), new_state / reset_state [E][S] are
// read; state, ep_len [E] int32, ep_ret [E] are updated in place; rewards_row / dones_row [E] and
// epstat [ceil(E/16)][2] (overwritten with init, else added to) are written.  Every extent is exact:
// the grid is sized from E alone.
// fin (bootstrap_time_limit, env_advance_fin): {fin_src, fin_dst, trunc_row} or empty.
void env_advance_impl(torch::Tensor reward, torch::Tensor terminal, torch::Tensor new_state, torch::Tensor reset_state,
                      torch::Tensor state, torch::Tensor ep_len, torch::Tensor ep_ret, torch::Tensor rewards_row,
                      torch::Tensor dones_row, torch::Tensor epstat, int64_t limit, double reward_clip, bool init,
                      const std::vector<torch::Tensor>& fin, const char* who) {
  TORCH_CHECK(state.dim() == 2 && state.size(0) >= 1 && state.size(1) >= 1, "state must be [E][S] with E, S >= 1");
  const int64_t E = state.size(0), S = state.size(1);
  TORCH_CHECK(E <= (int64_t)1 << 30 && S < (int64_t)1 << 20, "E must be <= 2^30 and S < 2^20, got ", E, " x ", S);
  TORCH_CHECK(limit >= 1 && limit <= std::numeric_limits<int>::max(), "limit must be a positive int32, got ", limit);
  const int64_t ntile = (E + ENVSTEP_TILE - 1) / ENVSTEP_TILE;
  auto exact = [](const torch::Tensor& t, const char* name, at::ScalarType st, int64_t n) {
    check(t, name, st, n);
    TORCH_CHECK(t.numel() == n, name, " must have exactly ", n, " elements, got ", t.numel());
  };
  exact(reward, "reward", at::kFloat, E);
  TORCH_CHECK(terminal.scalar_type() == at::kByte || terminal.scalar_type() == at::kBool,
              "terminal has dtype ", terminal.scalar_type(), ", expected uint8 or bool");
  exact(terminal, "terminal", terminal.scalar_type(), E);
  exact(new_state, "new_state", at::kFloat, E * S);
  exact(reset_state, "reset_state", at::kFloat, E * S);
  exact(state, "state", at::kFloat, E * S);
  exact(ep_len, "ep_len", at::kInt, E);
  exact(ep_ret, "ep_ret", at::kFloat, E);
  exact(rewards_row, "rewards_row", at::kFloat, E);
  exact(dones_row, "dones_row", at::kFloat, E);
  exact(epstat, "epstat", at::kFloat, ntile * 2);
  EnvStepArgs a{};
  a.E = (int)E; a.S = (int)S; a.limit = (int)limit;
  a.reward_clip = (float)reward_clip; a.init = init ? 1 : 0;
  a.reward = reward.data_ptr<float>();
  a.terminal = static_cast<const unsigned char*>(terminal.data_ptr());
  a.new_state = new_state.data_ptr<float>();
  a.reset_state = reset_state.data_ptr<float>();
  a.state = state.data_ptr<float>();
  a.ep_len = ep_len.data_ptr<int>();
  a.ep_ret = ep_ret.data_ptr<float>();
  a.rewards_row = rewards_row.data_ptr<float>();
  a.dones_row = dones_row.data_ptr<float>();
  a.epstat = epstat.data_ptr<float>();
  if (!fin.empty()) {
    const torch::Tensor &src = fin[0], &dst = fin[1], &tr = fin[2];
    TORCH_CHECK(src.dim() == 2 && src.size(0) == E && src.size(1) >= 1, "fin_src must be [E][d1]");
    const int64_t row_bytes = src.size(1) * src.element_size();
    TORCH_CHECK(row_bytes % 16 == 0 && row_bytes < ((int64_t)1 << 20), "final rows must be a multiple of 16 bytes, "
                "below 2^20, got ", row_bytes);
    TORCH_CHECK(dst.scalar_type() == src.scalar_type(), "fin_dst has dtype ", dst.scalar_type(), ", fin_src ",
                src.scalar_type());
    exact(src, "fin_src", src.scalar_type(), E * src.size(1));
    exact(dst, "fin_dst", src.scalar_type(), E * src.size(1));
    exact(tr, "trunc_row", at::kFloat, E);
    a.fin_src = src.data_ptr();
    a.fin_dst = dst.data_ptr();
    a.trunc_row = tr.data_ptr<float>();
    a.fin_row_bytes = (int)row_bytes;
  }
  launch_env_advance(a, cur_stream());
  after_launch(who);
}

void env_advance(torch::Tensor reward, torch::Tensor terminal, torch::Tensor new_state, torch::Tensor reset_state,
                 torch::Tensor state, torch::Tensor ep_len, torch::Tensor ep_ret, torch::Tensor rewards_row,
                 torch::Tensor dones_row, torch::Tensor epstat, int64_t limit, double reward_clip, bool init) {
  env_advance_impl(reward, terminal, new_state, reset_state, state, ep_len, ep_ret, rewards_row, dones_row, epstat,
                   limit, reward_clip, init, {}, __func__);
}

// env_advance with bootstrap_time_limit's outputs: trunc_row [E] gets 1 for an env that ended by the
// step limit alone, and such an env's row of fin_src [E][d1] (its final observation, normalised, in
// the buffer's storage type) is copied to fin_dst [E][d1], the caller's slice x_fin[t // limit].
void env_advance_fin(torch::Tensor reward, torch::Tensor terminal, torch::Tensor new_state, torch::Tensor reset_state,
                     torch::Tensor state, torch::Tensor ep_len, torch::Tensor ep_ret, torch::Tensor rewards_row,
                     torch::Tensor dones_row, torch::Tensor epstat, int64_t limit, double reward_clip, bool init,
                     torch::Tensor fin_src, torch::Tensor fin_dst, torch::Tensor trunc_row) {
  env_advance_impl(reward, terminal, new_state, reset_state, state, ep_len, ep_ret, rewards_row, dones_row, epstat,
                   limit, reward_clip, init, {fin_src, fin_dst, trunc_row}, __func__);
}

// the largest env-tile grid the per-step normalisation launch can run co-resident
int64_t rollout_stepnorm_cap_b(int64_t dt, int64_t rows, std::vector<int64_t> layout, int64_t O, int64_t A, int64_t S) {
  Layout L = parse_layout(layout);
  RolloutArgs a{};
  a.O = (int)O; a.A = (int)A; a.S = (int)S;
  a.net.d1 = L.d_in[0]; a.net.d2 = L.d_in[1]; a.net.d3 = L.d_in[2];
  a.sn_g1 = reinterpret_cast<unsigned long long*>(1);   // (only selects the LDS size of the SN kernel)
  return (int64_t)::rollout_stepnorm_cap((int)dt, a, (int)rows);
}

// The blank MlpArgs of a shape query: the layout's dims and the action width
MlpArgs shape_args(const Layout& L, int64_t A) {
  MlpArgs a{};
  for (int i = 0; i < 6; ++i) { a.d_in[i] = L.d_in[i]; a.d_out[i] = L.d_out[i]; a.n_out[i] = L.n_out[i]; }
  a.A = (int)A;
  return a;
}

// idx_limit: exclusive upper bound of the rows of an idx-less call (rows of x_buf and of every per-row array).  The
// index VALUES of a gathered call are range-checked by the caller on the host (HipEngine._minibatch): no sync here.
MlpArgs base_mlp(int dt, const Layout& L, const std::vector<double>& scales, CT x_buf, CT idx, int64_t row0, int64_t M,
                 CT wimg, CT flat, int64_t A, int64_t idx_limit) {
  MlpArgs a = shape_args(L, A);
  check(wimg, "wimg", storage_type(dt), wimg_extent(L));
  check(flat, "flat", at::kFloat, A);
  TORCH_CHECK(M > 0, "M must be > 0");
  TORCH_CHECK(L.d_in[0] == L.d_in[3], "both heads share the input width");
  const int64_t nrows_x = x_buf.numel() / L.d_in[0];
  check(x_buf, "x_buf", storage_type(dt == 2 ? 1 : dt), 1);  // fp8 kernels read a bf16 buffer
  TORCH_CHECK(x_buf.numel() % L.d_in[0] == 0, "x_buf rows must have d_in[0] elements");
  if (idx.defined() && idx.numel() > 0) {
    check(idx, "idx", at::kInt, M);
    a.idx = idx.data_ptr<int>();
  } else {
    TORCH_CHECK(row0 >= 0 && row0 + M <= std::min<int64_t>(idx_limit, nrows_x), "row range out of x_buf / per-row arrays");
  }
  a.x_buf = x_buf.data_ptr();
  a.x_bytes = (int64_t)x_buf.numel() * (int64_t)x_buf.element_size();
  a.row0 = (int)row0;
  a.M = (int)M;
  a.W = wimg.data_ptr();
  for (int i = 0; i < 6; ++i) { a.off_w[i] = L.off_w[i]; a.off_wt[i] = L.off_wt[i]; a.scale[i] = (float)scales.at(i); }
  a.log_std = flat.data_ptr<float>();
  a.x_stream = g_x_stream;
  return a;
}

// w8 (optional, fp8 mode with dt bf16): the e4m3 image the value head's fc1 reads with qscale
void set_w8(MlpArgs& a, CT w8, CT qscale, const Layout& L) {
  if (w8.defined() && w8.numel() > 0) {
    check(w8, "w8", at::kByte, wimg_extent(L));
    check(qscale, "qscale", at::kFloat, 6);
    a.W8 = w8.data_ptr();
    a.qscale = qscale.data_ptr<float>();
  }
}

void mlp_value(int64_t dt, CT x_buf, CT idx, int64_t row0, int64_t M, CT wimg, Ints layout,
               const std::vector<double>& scales, CT flat, int64_t A, CT v_out, CT qscale, CT w8) {
  const Layout L = parse_layout(layout);
  MlpArgs a = base_mlp((int)dt, L, scales, x_buf, idx, row0, M, wimg, flat, A, std::numeric_limits<int64_t>::max());
  a.v_out = fptr(v_out, "v_out", M);
  a.qscale = opt_scales(qscale);
  TORCH_CHECK(!(w8.defined() && w8.numel() > 0) || dt == 1, "w8: the fp8 mode's bf16 value forward only");
  set_w8(a, w8, qscale, L);
  launch_mlp_value((int)dt, a, cur_stream());
  after_launch(__func__);
}

// fp8 mode's gradient-amax ring (csrc/common.h Q8), checked: the slots of step `step` (-1: the calibration pass) —
// its |g| maxima go to acc, its scales come from rd (the step before's maxima), clr is zeroed for the step after
struct Q8Ring { unsigned *acc, *rd, *clr; };
Q8Ring q8_ring(CT q8_amax, int64_t step) {
  check(q8_amax, "q8_amax", at::kInt, 3 * Q8_SLOT);
  unsigned* base = reinterpret_cast<unsigned*>(q8_amax.data_ptr<int>());
  const int64_t e = ((step % 3) + 3) % 3;
  return {base + Q8_SLOT * e, base + Q8_SLOT * ((e + 2) % 3), base + Q8_SLOT * ((e + 1) % 3)};
}

int64_t train_lds_bytes(int64_t dt, std::vector<int64_t> layout, int64_t A) {
  return (int64_t)mlp_train_lds_bytes((int)dt, shape_args(parse_layout(layout), A));
}

// MlpArgs of one update launch, checked: what the tile kernel, the per-head kernels and the 32x32 policy head
// share.  A binding passes its kernel's row tile ROWS, workgroup waves nw (the timestamp hook's extent), the
// operand buffers' storage type and the parsed layout; the rest of this list leads its own.  tbufs: xT h1pT h2pT
// h1vT h2vT g1pT g2pT g3pT g1vT g2vT g3vT, rows of ldT elements; idx empty: rows row0 .. row0 + M of x_buf; loss:
// loss_kind (0 ppo, 1 dppo_ref, 2 ppo with a categorical head: mlp_train only), value_loss (0 mse, 1 clipped_half), std_var, first_step, clip, ent_coeff; part:
// [ceil(M / ROWS)][npart] per-workgroup partial rows; xT_ready: xT holds the rows already; adv_norm: the fp32
// [mean, inv, std, explained variance] block of csrc/advnorm.hip that the policy loss normalises adv by (empty: off).
using Tensors = const std::vector<torch::Tensor>&;
MlpArgs train_args(int ROWS, int64_t nw, at::ScalarType operand, const Layout& L, int64_t dt, int64_t A, Tensors tbufs,
                   CT x_buf, CT idx, int64_t row0, int64_t M, CT wimg, const std::vector<double>& scales, CT flat,
                   CT log_std_old, CT actions, CT logp_old, CT adv, CT ret, CT v_old, CT mu_prev, CT v_prev,
                   const std::vector<double>& loss, int64_t ldT, CT part, int64_t npart, bool xT_ready, CT adv_norm) {
  TORCH_CHECK(dt != 2, "the fp8 mode's update runs in bf16 (its e4m3 parts: the value fc1 image w8 and the wgrad operands q8_amax)");
  TORCH_CHECK(A > 0, "A");
  check(actions, "actions", at::kFloat, A);
  const int64_t nrows = actions.numel() / A;
  MlpArgs a = base_mlp((int)dt, L, scales, x_buf, idx, row0, M, wimg, flat, A, nrows);
  TORCH_CHECK(loss.size() == 6, "loss: loss_kind, value_loss, std_var, first_step, clip, ent_coeff");
  TORCH_CHECK(tbufs.size() == 11, "11 transposed buffers");
  a.actions = actions.data_ptr<float>();
  a.logp_old = fptr(logp_old, "logp_old", nrows);
  a.adv = fptr(adv, "adv", nrows);
  a.ret = fptr(ret, "ret", nrows);
  a.v_old = fptr(v_old, "v_old", nrows);
  a.mu_prev = fptr(mu_prev, "mu_prev", nrows * A);
  a.v_prev = fptr(v_prev, "v_prev", nrows);
  a.log_std_old = fptr(log_std_old, "log_std_old", A);
  const int64_t Mpad = ((M + ROWS - 1) / ROWS) * ROWS;
  TORCH_CHECK(ldT >= Mpad && ldT % 32 == 0, "ldT must cover M padded to the row tile and be a multiple of 32");
  // rows each transposed buffer must hold (writer side)
  const int64_t need[11] = {L.d_in[0], L.d_in[1], L.d_in[2], L.d_in[4], L.d_in[5],
                            L.n_out[0], L.n_out[1], L.n_out[2], L.n_out[3], L.n_out[4], L.n_out[5]};
  void** dst[11] = {&a.xT, &a.h1pT, &a.h2pT, &a.h1vT, &a.h2vT, &a.g1pT, &a.g2pT, &a.g3pT, &a.g1vT, &a.g2vT, &a.g3vT};
  for (int i = 0; i < 11; ++i) {
    check(tbufs[i], "transposed buffer", operand, need[i] * ldT);
    *dst[i] = tbufs[i].data_ptr();
  }
  a.ldT = (int)ldT;
  const int64_t nblk = Mpad / ROWS;
  a.part = fptr(part, "part", nblk * npart);
  a.npart = (int)npart;
  TORCH_CHECK(loss[0] == 0 || loss[0] == 1 || loss[0] == 2, "loss_kind: 0 ppo, 1 dppo_ref, 2 categorical ppo");
  a.loss_kind = (int)loss[0]; a.value_loss = (int)loss[1]; a.std_var = (int)loss[2]; a.first_step = (int)loss[3];
  a.clip = (float)loss[4]; a.ent_coeff = (float)loss[5];
  // a precomputed xT is only valid for the identity row order from row 0
  TORCH_CHECK(!xT_ready || (a.idx == nullptr && row0 == 0), "xT_ready needs a full-batch call");
  a.xT_ready = xT_ready ? 1 : 0;
  if (adv_norm.defined() && adv_norm.numel() > 0) a.adv_norm = fptr(adv_norm, "adv_norm", 4);
  if (g_tstamp != nullptr) {
    TORCH_CHECK(g_tstamp_numel >= ((nblk + g_tstamp_every - 1) / g_tstamp_every) * nw * 16, "tstamp buffer too small");
    a.tstamp = g_tstamp;
    a.tstamp_every = g_tstamp_every;
  }
  return a;
}

// The three update bindings: train_args' parameters (from dt on; the pack P, deduced from it), then each kernel's own
constexpr const char* HEADS_ONLY = "the per-head kernels cover split-bf16 / bf16 and the reference network only";
constexpr const char* CATEGORICAL_TILE_ONLY =
    "loss_kind 2 (a categorical head) runs on the tile kernel (mlp_train) only; the per-head and 32x32 policy kernels "
    "have the Gaussian head";
template <class F> struct TrainBind;
template <class... P>
struct TrainBind<MlpArgs (*)(int, int64_t, at::ScalarType, const Layout&, int64_t, int64_t, Tensors, P...)> {
  // The two-head tile kernel (csrc/mlp.hip)
  static void mlp_train(int64_t dt, int64_t A, Tensors tbufs, Ints layout, P... p) {
    const Layout L = parse_layout(layout);
    const MlpArgs s = shape_args(L, A);
    TORCH_CHECK(mlp_train_lds_bytes((int)dt, s) <= 160 * 1024, "mlp_train tile does not fit LDS");
    const MlpArgs a = train_args(mlp_train_rows((int)dt, s), mlp_train_waves((int)dt, s), storage_type((int)dt), L, dt,
                                 A, tbufs, p...);
    TORCH_CHECK(a.npart >= 8 + A, "npart too small");
    TORCH_CHECK(!a.xT_ready || a.ldT == a.M, "xT_ready needs a full-batch call");   // (xT: the whole buffer's rows)
    launch_mlp_train((int)dt, a, cur_stream());
    after_launch(__func__);
  }

  // One head's streaming kernel (csrc/mlp_head.hip; head 0 policy, 1 value) with its fused narrow-layer weight
  // gradient at partial column part_dw (policy dW_mu [32][128], value dW_v [128]).  fp8 mode (dt bf16), else empty
  // tensors: w8 / qscale, the e4m3 image the head's fc1 reads; q8_amax / q8_step, the gradient-amax ring — the
  // operand buffers then hold e4m3 bytes (csrc/common.h Q8).
  static void mlp_head_train(int64_t dt, int64_t A, Tensors tbufs, Ints layout, P... p, int64_t head, int64_t part_dw,
                             CT w8, CT qscale, CT q8_amax, int64_t q8_step) {
    const Layout L = parse_layout(layout);
    TORCH_CHECK(head == 0 || head == 1, "head: 0 policy, 1 value");
    TORCH_CHECK((dt == 3 || dt == 1) && mlp_head_applies(shape_args(L, A)), HEADS_ONLY);
    TORCH_CHECK(!(w8.defined() && w8.numel() > 0) || dt == 1, "w8: the fp8 mode's per-head bf16 update only");
    const bool q8 = q8_amax.defined() && q8_amax.numel() > 0;
    TORCH_CHECK(!q8 || dt == 1, "e4m3 wgrad operands: the fp8 mode's per-head bf16 update only");
    const Q8Ring ring = q8 ? q8_ring(q8_amax, q8_step) : Q8Ring{};
    MlpArgs a = train_args(mlp_head_rows(), mlp_head_waves((int)head), q8 ? at::kByte : storage_type((int)dt), L, dt, A,
                           tbufs, p...);
    TORCH_CHECK(a.loss_kind != 2, CATEGORICAL_TILE_ONLY);
    a.q8_acc = ring.acc; a.q8_rd = ring.rd; a.q8_clr = ring.clr;
    TORCH_CHECK(a.npart >= (head == 1 ? 8 : 8 + A), "npart too small");
    if (head == 0) TORCH_CHECK(part_dw >= 8 + A && part_dw + 32 * 128 <= a.npart, "part_dw: policy dW_mu block");
    if (head == 1) TORCH_CHECK(part_dw >= 8 && part_dw + 128 <= a.npart, "part_dw: value dW_v block");
    a.part_dw = (int)part_dw;
    TORCH_CHECK(!a.xT_ready || a.ldT == a.M, "xT_ready needs a full-batch call");
    set_w8(a, w8, qscale, L);
    launch_mlp_head((int)dt, (int)head, a, cur_stream());
    after_launch(__func__);
  }

  // The policy head's transposed-chain 32x32 kernel (csrc/phead.hip): h1p / g1p / g2p and, unless xT_ready, the
  // observation rows into xT, ROW-MAJOR (the engine's wgrad reads them so: its rm flags; under xT_ready x_buf itself
  // is the wgrad's X operand, so only the row order matters).  dW_mu is summed at partial column part_dw; p2 also
  // sums p_fc2's weight gradient behind it (no h1p / g2p stores).  (The value head's update stays on the 16x16
  // kernel: docs/ARCHITECTURE.md §13.)
  static void phead_train(int64_t dt, int64_t A, Tensors tbufs, Ints layout, P... p, int64_t part_dw, bool p2) {
    const Layout L = parse_layout(layout);
    const MlpArgs s = shape_args(L, A);
    TORCH_CHECK((dt == 3 || dt == 1) && mlp_head_applies(s), HEADS_ONLY);
    TORCH_CHECK(phead_shape_ok(s), "phead: the policy head at bf16x3 / bf16");
    MlpArgs a = train_args(mlp_head_rows(), mlp_head_waves(0), storage_type((int)dt), L, dt, A, tbufs, p...);
    TORCH_CHECK(a.loss_kind != 2, CATEGORICAL_TILE_ONLY);
    const int64_t ldT = a.ldT, npart = a.npart;
    TORCH_CHECK(npart >= 8 + A, "npart too small");
    TORCH_CHECK(part_dw >= 8 + A && part_dw + 32 * 128 <= npart, "part_dw: policy dW_mu block");
    TORCH_CHECK(part_dw + 32 * 128 + (p2 ? 128 * 128 : 0) <= npart,
                "phead: the dW_mu (and dW_p2) blocks must fit the partial row");
    a.part_dw = (int)part_dw;
    // the row-major operand rows the kernel writes are whole padded widths
    const int64_t pn = !p2 ? 128 : 0;   // h1p / g2p
    const int64_t wid[11] = {!a.xT_ready ? L.d_in[0] : 0, pn, 0, 0, 0, 128, pn, 0, 0, 0, 0};
    for (int i = 0; i < 11; ++i)
      TORCH_CHECK(tbufs[i].numel() >= wid[i] * ldT, "t32 head: row-major operand buffer ", i, " too small");
    const int64_t eb = dt == 3 ? 4 : 2, nblk = (a.M + mlp_head_rows() - 1) / mlp_head_rows();
    TORCH_CHECK(ldT * std::max<int64_t>(L.d_in[0], 128) * eb < (int64_t(1) << 31), "phead: row-major operands beyond 2 GiB");
    TORCH_CHECK(nblk * npart * 4 < (int64_t(1) << 31), "phead: partial buffer beyond 2 GiB");
    TORCH_CHECK(ldT % phead_rows() == 0 && (L.d_in[0] >> 4) / (dt == 3 ? 1 : 2) >= 3,
                "phead: ldT covers whole workgroups; fc1 has >= 3 stages");
    launch_phead_train((int)dt, a, p2 ? 1 : 0, cur_stream());
    after_launch(__func__);
  }
};
using TrainB = TrainBind<decltype(&train_args)>;

// the transposed-chain policy head covers this (dtype, network, action width)
bool phead_train_applies(int64_t dt, std::vector<int64_t> layout, int64_t A) {
  const MlpArgs a = shape_args(parse_layout(layout), A);
  return (dt == 3 || dt == 1) && phead_shape_ok(a) != 0 && (a.d_in[0] >> 4) / (dt == 3 ? 1 : 2) >= 3;
}

// the per-head kernels cover this (dtype, network); x_bytes is irrelevant to them (64-bit rows)
bool head_applies(int64_t dt, std::vector<int64_t> layout, int64_t A) {
  return (dt == 3 || dt == 1) && mlp_head_applies(shape_args(parse_layout(layout), A)) != 0;
}

int64_t train_rows(int64_t dt, std::vector<int64_t> layout, int64_t A, int64_t x_bytes) {
  MlpArgs a = shape_args(parse_layout(layout), A);
  a.x_bytes = x_bytes;
  return mlp_train_rows((int)dt, a);
}

int64_t train_waves(int64_t dt, std::vector<int64_t> layout, int64_t A) {
  return mlp_train_waves((int)dt, shape_args(parse_layout(layout), A));
}

void set_mlp_rows(int64_t rows) {
  TORCH_CHECK(rows == 0 || rows == 16 || rows == 32 || rows == 64, "rows: 0 (auto), 16, 32 or 64");
  set_mlp_rows_override((int)rows);
}

// dt 2 (fp8 mode): e4m3 operands; q8_amax / q8_step name the slot the update read its gradient
// scales from, q8_t the gradient tensor of each layer (-1: none), q8_xs the activation scales
WgradArgs wgrad_args(int64_t dt, std::vector<torch::Tensor> gT, std::vector<torch::Tensor> xT,
                     std::vector<int64_t> g_rows, std::vector<int64_t> x_rows, int64_t ld, torch::Tensor tasks,
                     torch::Tensor tasks_host, torch::Tensor slab, torch::Tensor q8_amax, int64_t q8_step,
                     std::vector<int64_t> q8_t, std::vector<double> q8_xs, std::vector<int64_t> rm) {
  TORCH_CHECK(gT.size() == 6 && xT.size() == 6 && g_rows.size() == 6 && x_rows.size() == 6, "6 layers");
  check(tasks, "tasks", at::kInt, WGRAD_TASK_INTS);
  TORCH_CHECK(tasks.numel() % WGRAD_TASK_INTS == 0, "tasks are 8-int records");
  TORCH_CHECK(!tasks_host.is_cuda() && tasks_host.numel() == tasks.numel(), "tasks_host must mirror tasks on CPU");
  const int ntasks = (int)(tasks.numel() / WGRAD_TASK_INTS);
  auto th = tasks_host.contiguous();
  const int* tp = th.data_ptr<int>();
  int64_t slab_need = 0;
  bool wide = false;
  for (int i = 0; i < ntasks; ++i) {
    const int* t = tp + WGRAD_TASK_INTS * i;
    TORCH_CHECK(t[0] >= 0 && t[0] < 6, "task layer");
    const int nq = t[6], kq = t[7];
    TORCH_CHECK(wgrad_task_ok((int)dt, nq, kq), "task quadrants beyond the workgroup (wgrad_task_ok)");
    wide = wide || nq * kq > 8;
    TORCH_CHECK(t[1] >= 0 && t[2] >= 0 && t[1] % 16 == 0 && t[2] % 16 == 0, "task tile origin");
    TORCH_CHECK(t[1] + 64 * nq <= g_rows[t[0]] && t[2] + 64 * kq <= x_rows[t[0]], "task tile beyond operand rows");
    // the kernel consumes 32-row k-steps in pairs (e4m3: in fours): every range is a positive
    // multiple of 64 (128) rows
    const int kq_rows = dt == 2 ? 128 : 64;
    TORCH_CHECK(t[3] >= 0 && t[4] <= ld && t[4] > t[3] && (t[4] - t[3]) % kq_rows == 0 && t[3] % 32 == 0,
                "task batch range (must be a positive multiple of 64 rows, 128 for e4m3)");
    TORCH_CHECK(t[5] >= 0, "task slab offset");
    slab_need = std::max<int64_t>(slab_need, (int64_t)t[5] + (int64_t)(64 * nq) * (64 * kq));
  }
  check(slab, "slab", at::kFloat, slab_need);
  WgradArgs a{};
  for (int i = 0; i < 6; ++i) {
    check(gT[i], "gT", storage_type((int)dt), g_rows[i] * ld);
    check(xT[i], "xT", storage_type((int)dt), x_rows[i] * ld);
    a.gT[i] = gT[i].data_ptr();
    a.xT[i] = xT[i].data_ptr();
  }
  a.ld = (int)ld;
  // rm: 12 flags (dY side of layers 0-5, then X side): 1 = row-major operands of row length g_rows /
  // x_rows (csrc/phead.hip, x_buf); split-bf16 / bf16 only, 64-feature quadrants inside the row
  TORCH_CHECK(rm.empty() || rm.size() == 12, "rm: 12 row-major flags");
  for (size_t i = 0; i < rm.size(); ++i) {
    if (!rm[i]) continue;
    TORCH_CHECK(dt == 1 || dt == 3, "row-major wgrad operands: split-bf16 / bf16 only");
    TORCH_CHECK(rm[i] == 1, "rm flag: 0 fragment-major, 1 row-major");
    const int64_t len = i < 6 ? g_rows[i] : x_rows[i - 6];
    TORCH_CHECK(len % 64 == 0 && ld * len * (dt == 3 ? 4 : 2) < (int64_t(1) << 40), "row-major operand rows");
    (i < 6 ? a.g_rm[i] : a.x_rm[i - 6]) = (int)len;
  }
  a.wide = wide ? 1 : 0;
  a.tasks = reinterpret_cast<const WgradTask*>(tasks.data_ptr<int>());
  a.ntasks = ntasks;
  a.slab = slab.data_ptr<float>();
  TORCH_CHECK(dt == 0 || dt == 1 || dt == 2 || dt == 3, "wgrad runs in fp32, bf16, e4m3 or bf16x3");
  if (dt == 2) {
    a.q8_rd = q8_ring(q8_amax, q8_step).rd;
    TORCH_CHECK(q8_t.size() == 6 && q8_xs.size() == 6, "q8_t / q8_xs: one per layer");
    for (int i = 0; i < ntasks; ++i) {
      const int l = tp[WGRAD_TASK_INTS * i];
      TORCH_CHECK(q8_t[l] >= 0 && q8_t[l] < 4 && q8_xs[l] > 0, "e4m3 wgrad task on a layer without operand scales");
    }
    for (int i = 0; i < 6; ++i) { a.q8_t[i] = (int)q8_t[i]; a.q8_xs[i] = (float)q8_xs[i]; }
  }
  return a;
}

void wgrad(int64_t dt, std::vector<torch::Tensor> gT, std::vector<torch::Tensor> xT, std::vector<int64_t> g_rows,
           std::vector<int64_t> x_rows, int64_t ld, torch::Tensor tasks, torch::Tensor tasks_host, torch::Tensor slab,
           torch::Tensor q8_amax, int64_t q8_step, std::vector<int64_t> q8_t, std::vector<double> q8_xs,
           std::vector<int64_t> rm) {
  const WgradArgs a = wgrad_args(dt, gT, xT, g_rows, x_rows, ld, tasks, tasks_host, slab, q8_amax, q8_step, q8_t, q8_xs, rm);
  launch_wgrad((int)dt, a, cur_stream());
  after_launch(__func__);
}

// The gradient of one flat range: slab elements [i_lo, i_hi) (src_meta != 0) as split-K slab
// sums, and the reduce items (red_col / red_dst: the partial-row column of each, and its flat
// index in `grad` or -1 - q for loss_out[q]) as column sums of the per-workgroup partial rows.
// grad / src_off / src_meta may be one head's slice of the flat vectors; red_dst then indexes
// the slice.  The item tables are validated on the host when the engine builds them
// (HipEngine._reduce_items): no per-epoch device sync here.
// the slab runs of a gather: flattened [lo0, hi0, lo1, hi1, ...] (<= 4, ascending, disjoint, inside
// [0, n)); every element of a run must have a slab source (src_meta != 0: the engine asserts it
// when it builds the plan, runtime/engine_hip.py _slab_runs)
SlabRuns make_runs(const std::vector<int64_t>& v, int64_t n) {
  TORCH_CHECK(v.size() % 2 == 0 && v.size() / 2 >= 1 && v.size() / 2 <= 4, "slab runs: 1-4 [lo, hi) pairs");
  SlabRuns r{};
  r.n = (int)(v.size() / 2);
  int64_t total = 0, prev = 0;
  for (int k = 0; k < 4; ++k) {
    if (k < r.n) {
      const int64_t lo = v[2 * k], hi = v[2 * k + 1];
      TORCH_CHECK(prev <= lo && lo <= hi && hi <= n, "slab runs must be ascending, disjoint and inside [0, n)");
      r.lo[k] = (int)lo;
      r.start[k] = (int)total;
      total += hi - lo;
      prev = hi;
    } else {
      r.lo[k] = 0;
      r.start[k] = INT32_MAX;
    }
  }
  r.total = (int)total;
  return r;
}

// The optional tile table of a gather (csrc/kernels.h SlabTiles): `tiles` on the device, `tiles_host` its CPU
// mirror (like wgrad's task list), checked here on every call — every quad's chunk loads stay inside the slab
// and every flat element inside [0, n).  Both absent (or empty): the per-element form.
using OptTensor = const std::optional<torch::Tensor>&;
SlabTiles slab_tiles(OptTensor tiles, OptTensor tiles_host, CT slab, const SlabRuns& runs, int64_t n) {
  SlabTiles st{};
  if (!tiles.has_value() || !tiles->defined() || tiles->numel() == 0) return st;
  TORCH_CHECK(tiles_host.has_value() && tiles_host->defined(), "a tile table needs its CPU mirror tiles_host");
  const int64_t nt = tiles->numel() / SLAB_TILE_INTS;
  check(*tiles, "tiles", at::kInt, 1);
  TORCH_CHECK(nt >= 1 && nt <= SLAB_TILES_MAX && tiles->numel() == nt * SLAB_TILE_INTS, "tiles: 1-", SLAB_TILES_MAX,
              " records of ", SLAB_TILE_INTS, " ints");
  TORCH_CHECK(!tiles_host->is_cuda() && tiles_host->scalar_type() == at::kInt && tiles_host->numel() == tiles->numel(),
              "tiles_host must mirror tiles on CPU");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(slab.data_ptr<float>()) % 16 == 0, "slab must be 16-byte aligned");
  auto th = tiles_host->contiguous();
  const int* t = th.data_ptr<int>();
  const int64_t slab_n = slab.numel();
  int64_t quads = 0, elems = 0;
  for (int64_t u = 0; u < nt; ++u) {
    const int* e = t + u * SLAB_TILE_INTS;
    const int64_t base = e[0], nch = e[1], stride = e[2], n0 = e[3], k0 = e[4], kq = e[5], fan_in = e[6],
                  fan_out = e[7], w_off = e[8], b_off = e[9], nq = e[10];
    TORCH_CHECK(nq >= 1 && kq >= 1 && nch >= 1 && fan_in >= 1 && n0 >= 0 && n0 < fan_out && k0 >= 0 && k0 <= fan_in,
                "tiles[", u, "]: bad tile shape");
    const int64_t size = nq * kq * 4096;
    TORCH_CHECK(base >= 0 && base % 4 == 0 && stride % 4 == 0 && stride >= size &&
                    base + (nch - 1) * stride + size <= slab_n,
                "tiles[", u, "] leaves the slab");
    TORCH_CHECK(w_off >= 0 && w_off + fan_out * fan_in <= n && b_off >= 0 && b_off + fan_out <= n,
                "tiles[", u, "] leaves the flat range");
    TORCH_CHECK(e[11] == quads, "tiles[", u, "]: quad0 must be the running quad count");
    quads += (int64_t)slab_tile_rows(e) * ((slab_tile_cols(e) + 3) / 4);
    elems += (int64_t)slab_tile_rows(e) * slab_tile_cols(e);
    TORCH_CHECK(quads < INT32_MAX, "too many quads");
  }
  TORCH_CHECK(elems == runs.total, "the tile table covers ", elems, " elements, the slab runs ", runs.total);
  st.t = tiles->data_ptr<int>();
  st.n = (int)nt;
  st.nquads = (int)quads;
  return st;
}

// GatherArgs (csrc/kernels.h) of a gather over a flat range of n elements, checked
GatherArgs gather_args(CT slab, CT src_off, CT src_meta, CT part, int64_t npblk, int64_t npart, CT red_col, CT red_dst,
                       const std::vector<int64_t>& runs, double scale, CT loss_out, int64_t n,
                       OptTensor tiles = std::nullopt, OptTensor tiles_host = std::nullopt) {
  check(src_off, "src_off", at::kInt, n);
  check(src_meta, "src_meta", at::kInt, n);
  check(slab, "slab", at::kFloat, 1);
  check(part, "part", at::kFloat, npblk * npart);
  check(loss_out, "loss_out", at::kFloat, 8);
  const int64_t nitems = red_col.numel();
  check(red_col, "red_col", at::kInt, nitems);
  check(red_dst, "red_dst", at::kInt, nitems);
  TORCH_CHECK(red_dst.numel() == nitems, "red_col / red_dst sizes");
  GatherArgs ga{};
  ga.slab = slab.data_ptr<float>();
  ga.src_off = src_off.data_ptr<int>();
  ga.src_meta = src_meta.data_ptr<int>();
  ga.part = part.data_ptr<float>();
  ga.npblk = (int)npblk;
  ga.npart = (int)npart;
  ga.red_col = red_col.data_ptr<int>();
  ga.red_dst = red_dst.data_ptr<int>();
  ga.nitems = (int)nitems;
  ga.runs = make_runs(runs, n);
  ga.scale = (float)scale;
  ga.loss_out = loss_out.data_ptr<float>();
  ga.tiles = slab_tiles(tiles, tiles_host, slab, ga.runs, n);
  return ga;
}

void grad_gather(torch::Tensor slab, torch::Tensor src_off, torch::Tensor src_meta, torch::Tensor part,
                 int64_t nblk, int64_t npart, torch::Tensor red_col, torch::Tensor red_dst, double scale,
                 torch::Tensor grad, torch::Tensor loss_out, std::vector<int64_t> runs, OptTensor tiles,
                 OptTensor tiles_host) {
  const int64_t n = grad.numel();
  check(grad, "grad", at::kFloat, n);
  const GatherArgs ga = gather_args(slab, src_off, src_meta, part, nblk, npart, red_col, red_dst, runs, scale,
                                    loss_out, n, tiles, tiles_host);
  launch_grad_gather(ga, grad.data_ptr<float>(), cur_stream());
  after_launch(__func__);
}

void obs_reduce(torch::Tensor part, int64_t nblk, int64_t O, torch::Tensor s12, torch::Tensor epstat,
                torch::Tensor ep) {
  check(part, "part", at::kFloat, nblk * 2 * O);
  check(s12, "s12", at::kDouble, 2 * O);
  check(epstat, "epstat", at::kFloat, nblk * 2);
  check(ep, "ep", at::kDouble, 2);
  launch_obs_reduce(part.data_ptr<float>(), (int)nblk, (int)O, s12.data_ptr<double>(), epstat.data_ptr<float>(),
                    ep.data_ptr<double>(), cur_stream());
  after_launch(__func__);
}

// the per-step obs-norm mode's observe (model.py:68 over one step's E observations): moments about
// shift -> fixed-order fp64 reduce -> Chan merge into (mean, m2) and the fp32 images; three
// launches, no host sync (n_a: the stats' count before this batch, tracked on the host)
void obs_observe(torch::Tensor obs, torch::Tensor shift, torch::Tensor mean, torch::Tensor m2, torch::Tensor mean_f32,
                 torch::Tensor inv_std, double n_a, torch::Tensor part, torch::Tensor s12, double var_floor) {
  const int64_t O = mean.numel();
  TORCH_CHECK(obs.dim() == 2 && obs.size(1) == O && obs.size(0) > 0, "obs must be [E][O]");
  const int E = (int)obs.size(0);
  const int nblk = obs_moments_blocks(E);
  check(obs, "obs", at::kFloat, (int64_t)E * O);
  check(shift, "shift", at::kFloat, O);
  check(part, "part", at::kFloat, (int64_t)nblk * 2 * O);
  check(s12, "s12", at::kDouble, 2 * O);
  check(mean, "mean", at::kDouble, O);
  check(m2, "m2", at::kDouble, O);
  check(mean_f32, "mean_f32", at::kFloat, O);
  check(inv_std, "inv_std", at::kFloat, O);
  TORCH_CHECK(shift.data_ptr() != mean_f32.data_ptr(), "shift must be a snapshot, not the stats' own mean image");
  const hipStream_t s = cur_stream();
  launch_obs_moments(obs.data_ptr<float>(), E, (int)O, shift.data_ptr<float>(), part.data_ptr<float>(), s);
  launch_obs_reduce(part.data_ptr<float>(), nblk, (int)O, s12.data_ptr<double>(), nullptr, nullptr, s);
  launch_obs_merge(s12.data_ptr<double>(), (int)O, (double)E, n_a, shift.data_ptr<float>(), mean.data_ptr<double>(),
                   m2.data_ptr<double>(), mean_f32.data_ptr<float>(), inv_std.data_ptr<float>(), var_floor, s);
  after_launch(__func__);
}

int64_t obs_moments_nblk(int64_t E) { return obs_moments_blocks((int)E); }

void obs_merge(torch::Tensor s12, double count, double n_a, torch::Tensor shift, torch::Tensor mean, torch::Tensor m2,
               torch::Tensor mean_f32, torch::Tensor inv_std, double var_floor) {
  const int64_t O = mean.numel();
  TORCH_CHECK(count > 0, "count must be positive");
  check(s12, "s12", at::kDouble, 2 * O);
  check(shift, "shift", at::kFloat, O);
  check(mean, "mean", at::kDouble, O);
  check(m2, "m2", at::kDouble, O);
  check(mean_f32, "mean_f32", at::kFloat, O);
  check(inv_std, "inv_std", at::kFloat, O);
  launch_obs_merge(s12.data_ptr<double>(), (int)O, count, n_a, shift.data_ptr<float>(), mean.data_ptr<double>(),
                   m2.data_ptr<double>(), mean_f32.data_ptr<float>(), inv_std.data_ptr<float>(), var_floor,
                   cur_stream());
  after_launch(__func__);
}

// The GAE scan over [T,E] buffers (csrc/optim.hip launch_gae_rn).  boot [T,E] (bootstrap_time_limit: V of a
// truncated step's final observation, 0 elsewhere): an empty tensor is the scan without it.  scale (reward_norm:
// the reward enters as r' = clamp(fl32(r * scale[0]), +-rclip), rclip <= 0: no clamp): a device scalar read by the
// kernel, null is the scan without it.
void gae_impl(const char* fn, CT rewards, CT values, CT dones, CT boot, const torch::Tensor* scale, double rclip,
              CT adv, CT ret, double gamma, double lam, int64_t mode, int64_t seg) {
  TORCH_CHECK(seg >= 0, "segment length must be >= 0 (0: no segment cut)");
  TORCH_CHECK(rewards.dim() == 2, "rewards [T,E]");
  TORCH_CHECK(mode >= 0 && mode <= 2, "gae mode: 0 auto, 1 per-env lanes, 2 parallel-in-time scan");
  const int64_t T = rewards.size(0), E = rewards.size(1);
  check(rewards, "rewards", at::kFloat, T * E);
  check(values, "values", at::kFloat, (T + 1) * E);
  check(dones, "dones", at::kFloat, T * E);
  if (scale != nullptr) check(*scale, "scale", at::kFloat, 1);
  check(adv, "adv", at::kFloat, T * E);
  check(ret, "ret", at::kFloat, T * E);
  const float* b = nullptr;
  if (boot.defined() && boot.numel() > 0) {
    check(boot, "boot", at::kFloat, T * E);
    b = boot.data_ptr<float>();
  }
  launch_gae_rn(rewards.data_ptr<float>(), values.data_ptr<float>(), dones.data_ptr<float>(), b,
                scale != nullptr ? scale->data_ptr<float>() : nullptr, (float)rclip, adv.data_ptr<float>(),
                ret.data_ptr<float>(), (int)T, (int)E, (float)gamma, (float)lam, (int)mode, (int)seg, cur_stream());
  after_launch(fn);
}

void gae(torch::Tensor rewards, torch::Tensor values, torch::Tensor dones, torch::Tensor adv, torch::Tensor ret,
         double gamma, double lam, int64_t mode, int64_t seg) {
  gae_impl(__func__, rewards, values, dones, torch::Tensor(), nullptr, 0.0, adv, ret, gamma, lam, mode, seg);
}

void gae_boot(torch::Tensor rewards, torch::Tensor values, torch::Tensor dones, torch::Tensor boot, torch::Tensor adv,
              torch::Tensor ret, double gamma, double lam, int64_t mode, int64_t seg) {
  gae_impl(__func__, rewards, values, dones, boot, nullptr, 0.0, adv, ret, gamma, lam, mode, seg);
}

void gae_rn(torch::Tensor rewards, torch::Tensor values, torch::Tensor dones, torch::Tensor boot, torch::Tensor scale,
            double rclip, torch::Tensor adv, torch::Tensor ret, double gamma, double lam, int64_t mode, int64_t seg) {
  gae_impl(__func__, rewards, values, dones, boot, &scale, rclip, adv, ret, gamma, lam, mode, seg);
}

// reward_norm: the discounted-return scan of a rollout (csrc/retnorm.hip).  ret_acc [E] is updated in place,
// s12 [2] fp64 = (S1, S2) of the T*E samples about shift[0]; R_out [T,E] is optional (an empty tensor: not
// written); part: fp64 scratch of ret_scan_nblk(T, E, mode) x 2
int64_t ret_scan_nblk(int64_t T, int64_t E, int64_t mode) { return ret_scan_blocks((int)T, (int)E, (int)mode); }

void ret_scan(torch::Tensor rewards, torch::Tensor dones, torch::Tensor ret_acc, torch::Tensor shift,
              torch::Tensor part, torch::Tensor s12, torch::Tensor R_out, double gamma, int64_t mode) {
  TORCH_CHECK(rewards.dim() == 2, "rewards [T,E]");
  TORCH_CHECK(mode >= 0 && mode <= 2, "ret_scan mode: 0 auto, 1 per-env lanes, 2 parallel-in-time scan");
  const int64_t T = rewards.size(0), E = rewards.size(1);
  TORCH_CHECK(T > 0 && E > 0, "rewards must not be empty");
  check(rewards, "rewards", at::kFloat, T * E);
  check(dones, "dones", at::kFloat, T * E);
  check(ret_acc, "ret_acc", at::kFloat, E);
  check(shift, "shift", at::kFloat, 1);
  check(part, "part", at::kDouble, 2 * ret_scan_nblk(T, E, mode));
  check(s12, "s12", at::kDouble, 2);
  float* ro = nullptr;
  if (R_out.defined() && R_out.numel() > 0) {
    check(R_out, "R_out", at::kFloat, T * E);
    ro = R_out.data_ptr<float>();
  }
  launch_ret_scan(rewards.data_ptr<float>(), dones.data_ptr<float>(), ret_acc.data_ptr<float>(),
                  shift.data_ptr<float>(), ro, part.data_ptr<double>(), s12.data_ptr<double>(), (int)T, (int)E,
                  (float)gamma, (int)mode, cur_stream());
  after_launch(__func__);
}

// adv_norm_scope global | minibatch (csrc/advnorm.hip): sums fp64[4] = [sum a, sum a^2, sum r, sum r^2] over the n rows
// idx ? idx[i] : i of adv / ret (idx empty: the first n rows; ret empty: its two sums are 0), in a fixed order; part:
// fp64 scratch of adv_stats_nblk(n) x 4; block (empty: the sums only): fp32[4] = [mean, inv, std, explained variance]
// finished from the sums with the count n_total in the same two launches.  adv_block: the finish alone, for sums that
// were all-reduced in between.  The indices are the caller's to range-check (the kernel clamps them to the buffer).
int64_t adv_stats_nblk(int64_t n) {
  TORCH_CHECK(n >= 1 && n < (int64_t(1) << 31), "adv_stats: n");
  return adv_stats_blocks((int)n);
}

void adv_stats(torch::Tensor adv, torch::Tensor ret, torch::Tensor idx, int64_t n, torch::Tensor part, torch::Tensor sums,
               double n_total, torch::Tensor block) {
  TORCH_CHECK(n >= 2 && n < (int64_t(1) << 31), "adv_stats: n >= 2 rows (the unbiased variance), got ", n);
  TORCH_CHECK(n_total >= 2.0, "adv_stats: n_total >= 2, got ", n_total);
  const bool has_idx = idx.defined() && idx.numel() > 0, has_ret = ret.defined() && ret.numel() > 0;
  check(adv, "adv", at::kFloat, has_idx ? 1 : n);
  TORCH_CHECK(adv.numel() < (int64_t(1) << 31), "adv_stats: 32-bit row indices");
  if (has_idx) check(idx, "idx", at::kInt, n);
  if (has_ret) {
    check(ret, "ret", at::kFloat, adv.numel());
    TORCH_CHECK(ret.numel() == adv.numel(), "adv_stats: ret must have adv's ", adv.numel(), " rows, got ", ret.numel());
  }
  check(part, "part", at::kDouble, 4 * adv_stats_nblk(n));
  check(sums, "sums", at::kDouble, 4);
  float* b = nullptr;
  if (block.defined() && block.numel() > 0) b = fptr(block, "block", 4);
  launch_adv_stats(adv.data_ptr<float>(), has_ret ? ret.data_ptr<float>() : nullptr,
                   has_idx ? idx.data_ptr<int>() : nullptr, (int)n, (int)adv.numel(), part.data_ptr<double>(),
                   sums.data_ptr<double>(), n_total, b, cur_stream());
  after_launch(__func__);
}

void adv_block(torch::Tensor sums, double n_total, torch::Tensor block) {
  TORCH_CHECK(n_total >= 2.0, "adv_block: n_total >= 2, got ", n_total);
  check(sums, "sums", at::kDouble, 4);
  launch_adv_block(sums.data_ptr<double>(), n_total, fptr(block, "block", 4), cur_stream());
  after_launch(__func__);
}

void metrics_pack(torch::Tensor ep, torch::Tensor loss8, torch::Tensor norm_part, torch::Tensor out) {
  check(ep, "ep", at::kDouble, 2);
  check(loss8, "loss8", at::kFloat, 8);
  check(norm_part, "norm_part", at::kFloat, 1);
  check(out, "out", at::kDouble, 11);
  launch_metrics_pack(ep.data_ptr<double>(), loss8.data_ptr<float>(), norm_part.data_ptr<float>(),
                      (int)norm_part.numel(), out.data_ptr<double>(), cur_stream());
  after_launch(__func__);
}

// diagnostics (scripts/probe_side_kernel.py): an RCCL-footprint stand-in on the current stream
void probe_spin(int64_t nblk, int64_t nthreads, int64_t lds, double us, torch::Tensor sink) {
  TORCH_CHECK(nblk >= 1 && nblk <= 4096 && nthreads >= 64 && nthreads <= 1024 && nthreads % 64 == 0 && lds >= 0 &&
                  lds <= 65536 && lds >= 4 * nthreads && us > 0 && us < 1e5,
              "probe_spin: 1-4096 blocks of 64-1024 threads, 4 * threads <= lds <= 64 KiB, 0 < us < 1e5");
  check(sink, "sink", at::kInt, nblk);
  launch_probe_spin((int)nblk, (int)nthreads, (int)lds, us, sink.data_ptr<int>(), cur_stream());
  after_launch(__func__);
}

// fp8 mode's shadow image (csrc/kernels.h F8Shadow): empty tensors = off
F8Shadow f8_shadow(torch::Tensor img, torch::Tensor lid, torch::Tensor qs, int64_t n) {
  F8Shadow f{nullptr, nullptr, nullptr};
  if (img.defined() && img.numel() > 0) {
    check(img, "f8_img", at::kByte, 1);
    check(lid, "f8_lid", at::kInt, n);
    check(qs, "f8_qscale", at::kFloat, 6);
    f.img = img.data_ptr<uint8_t>();
    f.lid = lid.data_ptr<int>();
    f.qs = qs.data_ptr<float>();
  }
  return f;
}

// target_kl's gate f32[4] = [stop, applied, trip_kl, last_kl] (csrc/optim.hip KlGate)
const float* gate_ptr(const torch::Tensor& gate) {
  check(gate, "gate", at::kFloat, 4);
  TORCH_CHECK(gate.numel() == 4, "gate is [stop, applied, trip_kl, last_kl]");
  return gate.data_ptr<float>();
}

// lr_schedule adaptive's lr_state f32[4] = [lr, downs, ups, reserved] (csrc/kernels.h LrAdapt)
float* lr_state_ptr(const torch::Tensor& t) {
  check(t, "lr_state", at::kFloat, 4);
  TORCH_CHECK(t.numel() == 4, "lr_state is [lr, downs, ups, reserved]");
  return t.data_ptr<float>();
}

// AdamArgs (csrc/kernels.h) of one optimizer launch over the flat range p, checked.  host_step >= 1: the step
// number of this update (eager launch: one fused kernel when there is no clipping); 0: read the device counter
// (graph replay).  gate: an empty tensor is the ungated launch; else target_kl's gated step — applied only while
// gate[0] == 0, the step number state[0] + 1 read on the device (host_step unused).  lr_dev: none or an empty tensor
// is the host rate lr; else lr_schedule adaptive's lr_state f32[4], whose slot 0 the gated form reads (lr unused).
using OptT = const std::optional<torch::Tensor>&;
AdamArgs adam_args(CT p, CT g, CT m, CT v, double lr, double b1, double b2, double eps, double max_norm,
                   int64_t host_step, CT state, CT norm_part, CT wimg, CT w_map, CT wt_map, int64_t dt, CT qmul,
                   CT f8_img, CT f8_lid, CT f8_qs, CT gate, OptT lr_dev) {
  const int64_t n = p.numel();
  check(p, "p", at::kFloat, n);
  check(g, "g", at::kFloat, n);
  check(m, "m", at::kFloat, n);
  check(v, "v", at::kFloat, n);
  check(state, "state", at::kFloat, 4);
  check(w_map, "w_map", at::kInt, n);
  check(wt_map, "wt_map", at::kInt, n);
  check(wimg, "wimg", storage_type((int)dt), 1);
  const int nblk = (int)norm_part.numel();
  check(norm_part, "norm_part", at::kFloat, nblk);
  TORCH_CHECK(nblk >= 1 && nblk <= 4096, "norm_part size");
  AdamArgs a{};
  a.p = p.data_ptr<float>();
  a.g = g.data_ptr<float>();
  a.m = m.data_ptr<float>();
  a.v = v.data_ptr<float>();
  a.n = (int)n;
  a.lr = (float)lr;
  a.b1 = (float)b1;
  a.b2 = (float)b2;
  a.eps = (float)eps;
  a.max_norm = (float)max_norm;
  a.state = state.data_ptr<float>();
  a.norm_part = norm_part.data_ptr<float>();
  a.nblk = nblk;
  a.wimg = wimg.data_ptr();
  a.w_map = w_map.data_ptr<int>();
  a.wt_map = wt_map.data_ptr<int>();
  a.dt = (int)dt;
  if (qmul.defined() && qmul.numel() > 0) { check(qmul, "qmul", at::kFloat, n); a.img_scale = qmul.data_ptr<float>(); }
  a.f8 = f8_shadow(f8_img, f8_lid, f8_qs, n);
  if (gate.defined() && gate.numel() > 0) a.gate = gate_ptr(gate);
  a.host_step = a.gate != nullptr ? 0 : (int)host_step;
  if (lr_dev.has_value() && lr_dev->defined() && lr_dev->numel() > 0) {
    TORCH_CHECK(a.gate != nullptr, "lr_dev needs a gate: only the gated launches read the rate on the device");
    a.lr_dev = lr_state_ptr(*lr_dev);
  }
  return a;
}

// Adam (+ clip) over a flat range: one launch without clipping when the step number is known (host_step >= 1, or
// gated), else the sumsq + adam pair
void adam(torch::Tensor p, torch::Tensor g, torch::Tensor m, torch::Tensor v, double lr, double b1, double b2,
          double eps, double max_norm, torch::Tensor state, torch::Tensor norm_part, torch::Tensor wimg,
          torch::Tensor w_map, torch::Tensor wt_map, int64_t dt, torch::Tensor qmul, int64_t host_step,
          torch::Tensor f8_img, torch::Tensor f8_lid, torch::Tensor f8_qs, torch::Tensor gate, OptT lr_dev) {
  launch_adam(adam_args(p, g, m, v, lr, b1, b2, eps, max_norm, host_step, state, norm_part, wimg, w_map, wt_map, dt,
                        qmul, f8_img, f8_lid, f8_qs, gate, lr_dev),
              cur_stream());
  after_launch(__func__);
}

// target_kl: the gate after a step (csrc/optim.hip kl_gate_kernel; ops/oracle.py kl_gate).  lr_state: none or an
// empty tensor is the gate alone (the other rate operands unread); else lr_schedule adaptive's rate block
// (ops/oracle.py lr_adapt)
void kl_gate(torch::Tensor loss_sums, torch::Tensor gate, torch::Tensor state, double target_kl, OptT lr_state,
             double kl_target, double factor, double lr_min, double lr_max) {
  check(loss_sums, "loss_sums", at::kFloat, 8);
  check(state, "state", at::kFloat, 4);
  TORCH_CHECK(target_kl > 0, "kl_gate needs target_kl > 0");
  LrAdapt ra{};
  if (lr_state.has_value() && lr_state->defined() && lr_state->numel() > 0) {
    ra.lr_state = lr_state_ptr(*lr_state);
    TORCH_CHECK(kl_target > 0 && std::isfinite(kl_target), "kl_gate's rate block needs a finite kl_target > 0");
    TORCH_CHECK(factor > 1 && std::isfinite(factor), "kl_gate's rate block needs a finite factor > 1");
    TORCH_CHECK(lr_min > 0 && lr_min <= lr_max && std::isfinite(lr_max), "kl_gate's rate block needs 0 < lr_min <= lr_max");
    ra.kl_target = (float)kl_target;
    ra.factor = (float)factor;
    ra.lr_min = (float)lr_min;
    ra.lr_max = (float)lr_max;
  }
  launch_kl_gate(loss_sums.data_ptr<float>(), const_cast<float*>(gate_ptr(gate)), state.data_ptr<float>(),
                 (float)target_kl, ra, cur_stream());
  after_launch(__func__);
}

// grad_gather (reduce items + slab elements of the runs) and the no-clip Adam step in one launch (world size 1:
// nothing runs between them).  Bit-identical parameters to grad_gather -> adam(host_step).  The flat tensors may be
// one head's slice (red_dst indexes the slice).  Gated (adam_args) it takes no host step number, and with gate[0]
// set it still writes g, loss_out and norm_part; p, m, v and the images stay.
void gather_adam(torch::Tensor slab, torch::Tensor src_off, torch::Tensor src_meta, torch::Tensor part,
                 int64_t npblk, int64_t npart, torch::Tensor red_col, torch::Tensor red_dst, std::vector<int64_t> runs,
                 double scale, torch::Tensor loss_out, torch::Tensor g, torch::Tensor p, torch::Tensor m,
                 torch::Tensor v, double lr, double b1, double b2, double eps, int64_t step, torch::Tensor state,
                 torch::Tensor norm_part, torch::Tensor wimg, torch::Tensor w_map, torch::Tensor wt_map, int64_t dt,
                 torch::Tensor qmul, torch::Tensor f8_img, torch::Tensor f8_lid, torch::Tensor f8_qs,
                 torch::Tensor gate, OptT lr_dev, OptTensor tiles, OptTensor tiles_host) {
  const AdamArgs a = adam_args(p, g, m, v, lr, b1, b2, eps, 0.0, step, state, norm_part, wimg, w_map, wt_map, dt, qmul,
                               f8_img, f8_lid, f8_qs, gate, lr_dev);
  const GatherArgs ga = gather_args(slab, src_off, src_meta, part, npblk, npart, red_col, red_dst, runs, scale,
                                    loss_out, p.numel(), tiles, tiles_host);
  TORCH_CHECK(a.gate != nullptr || step >= 1, "gather_adam needs the host step number (eager launches only)");
  TORCH_CHECK(a.nblk > item_blocks(ga.nitems), "norm_part must hold more blocks than the reduce blocks");
  launch_gather_adam(ga, a, cur_stream());
  after_launch(__func__);
}

void fp8_refresh(torch::Tensor p, torch::Tensor lid, torch::Tensor qscale, torch::Tensor part, torch::Tensor wimg,
                 torch::Tensor w_map, torch::Tensor wt_map) {
  check(part, "part", at::kFloat, 128 * 6);
  const int64_t n = p.numel();
  check(p, "p", at::kFloat, n);
  check(lid, "lid", at::kInt, n);
  check(qscale, "qscale", at::kFloat, 6);
  check(w_map, "w_map", at::kInt, n);
  check(wt_map, "wt_map", at::kInt, n);
  check(wimg, "wimg", at::kByte, 1);
  // lid must name a layer in [0, 6) for every parameter with an image entry (the kernel's scale
  // index): HipEngine validates the static map once at construction (no per-call device sync)
  launch_fp8_refresh(p.data_ptr<float>(), lid.data_ptr<int>(), (int)n, qscale.data_ptr<float>(), part.data_ptr<float>(),
                     wimg.data_ptr(), w_map.data_ptr<int>(), wt_map.data_ptr<int>(), cur_stream());
  after_launch(__func__);
}

void debug_invalid_launch() {
  launch_debug_invalid(nullptr, cur_stream());
  after_launch(__func__);
}

void pack(torch::Tensor p, torch::Tensor wimg, torch::Tensor w_map, torch::Tensor wt_map, int64_t dt, torch::Tensor qmul) {
  const int64_t n = p.numel();
  check(p, "p", at::kFloat, n);
  check(w_map, "w_map", at::kInt, n);
  check(wt_map, "wt_map", at::kInt, n);
  check(wimg, "wimg", storage_type((int)dt), 1);
  const float* q = nullptr;
  if (qmul.defined() && qmul.numel() > 0) { check(qmul, "qmul", at::kFloat, n); q = qmul.data_ptr<float>(); }
  launch_pack(p.data_ptr<float>(), (int)n, wimg.data_ptr(), w_map.data_ptr<int>(), wt_map.data_ptr<int>(), (int)dt, q,
              cur_stream());
  after_launch(__func__);
}

}  // namespace

void register_comm(pybind11::module& m);   // csrc/comm.cpp: native RCCL communicator

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.doc() = "MI355X-native DPPO kernels (gfx950 HIP)";
  register_comm(m);
  m.def("rollout", &RolloutB::rollout);
  m.def("rollout_fin", &RolloutB::rollout_fin);
  m.def("rollout_stepnorm", &rollout_stepnorm);
  m.def("eval_rollout", &eval_rollout);
  m.def("policy_act", &policy_act);
  m.def("env_advance", &env_advance);
  m.def("env_advance_fin", &env_advance_fin);
  m.def("rollout_stepnorm_cap", &rollout_stepnorm_cap_b);
  m.def("mlp_value", &mlp_value);
  m.def("mlp_train", &TrainB::mlp_train);
  m.def("mlp_head_train", &TrainB::mlp_head_train);
  m.def("phead_train", &TrainB::phead_train);
  m.def("head_applies", &head_applies);
  m.def("phead_train_applies", &phead_train_applies);
  m.def("set_phead", [](int64_t on) { set_phead((int)on); });
  m.def("head_rows", []() { return (int64_t)mlp_head_rows(); });
  m.def("head_waves", [](int64_t h) { return (int64_t)mlp_head_waves((int)h); });
  m.def("set_head_kernels", [](bool on) { set_head_kernels(on ? 1 : 0); });
  m.def("head_kernels_enabled", []() { return head_kernels_enabled() != 0; });
  m.def("train_lds_bytes", &train_lds_bytes);
  m.def("train_rows", &train_rows);
  m.def("train_waves", &train_waves);
  m.def("set_mlp_rows", &set_mlp_rows);
  m.def("set_s3_value_waves", [](int64_t nw) {
    TORCH_CHECK(nw == 4 || nw == 8, "split-bf16 value waves: 4 or 8");
    set_s3_value_waves((int)nw);
  });
  m.def("set_s3_train_waves", [](int64_t nw) {
    TORCH_CHECK(nw == 4 || nw == 8, "split-bf16 train waves: 4 or 8");
    set_s3_train_waves((int)nw);
  });
  m.def("set_debug_sync", &set_debug_sync);
  m.def("set_rollout_waves", [](int64_t nw) {
    TORCH_CHECK(nw == 4 || nw == 8, "rollout waves: 4 or 8");
    set_rollout_waves((int)nw);
  });
  m.def("set_train_tstamp", &set_train_tstamp);
  m.def("set_rollout_tstamp", &set_rollout_tstamp);
  m.def("wgrad", &wgrad);
  m.def("wgrad_task_ok", [](int64_t dt, int64_t nq, int64_t kq) { return wgrad_task_ok((int)dt, (int)nq, (int)kq) != 0; });
  m.def("grad_gather", &grad_gather, pybind11::arg("slab"), pybind11::arg("src_off"), pybind11::arg("src_meta"),
        pybind11::arg("part"), pybind11::arg("nblk"), pybind11::arg("npart"), pybind11::arg("red_col"),
        pybind11::arg("red_dst"), pybind11::arg("scale"), pybind11::arg("grad"), pybind11::arg("loss_out"),
        pybind11::arg("runs"), pybind11::arg("tiles") = pybind11::none(), pybind11::arg("tiles_host") = pybind11::none());
  m.attr("slab_sum_batch") = SLAB_SUM_BATCH;
  m.def("set_gather_stream", [](int64_t on) { set_gather_stream((int)on); });
  m.def("gae", &gae);
  m.def("gae_boot", &gae_boot);
  m.def("gae_rn", &gae_rn);
  m.def("ret_scan", &ret_scan);
  m.def("ret_scan_nblk", &ret_scan_nblk);
  m.def("adv_stats", &adv_stats);
  m.def("adv_block", &adv_block);
  m.def("adv_stats_nblk", &adv_stats_nblk);
  m.def("set_adam_fused", [](int64_t on) { set_adam_fused((int)on); });
  m.def("obs_reduce", &obs_reduce);
  m.def("obs_merge", &obs_merge);
  m.def("obs_observe", &obs_observe);
  m.def("obs_moments_nblk", &obs_moments_nblk);
  // (the trailing operands of lr_schedule adaptive have defaults: every earlier call keeps its argument list)
  namespace py = pybind11;
  m.def("adam", &adam, py::arg("p"), py::arg("g"), py::arg("m"), py::arg("v"), py::arg("lr"), py::arg("b1"),
        py::arg("b2"), py::arg("eps"), py::arg("max_norm"), py::arg("state"), py::arg("norm_part"), py::arg("wimg"),
        py::arg("w_map"), py::arg("wt_map"), py::arg("dt"), py::arg("qmul"), py::arg("host_step"), py::arg("f8_img"),
        py::arg("f8_lid"), py::arg("f8_qs"), py::arg("gate"), py::arg("lr_dev") = py::none());
  m.def("gather_adam", &gather_adam, py::arg("slab"), py::arg("src_off"), py::arg("src_meta"), py::arg("part"),
        py::arg("npblk"), py::arg("npart"), py::arg("red_col"), py::arg("red_dst"), py::arg("runs"), py::arg("scale"),
        py::arg("loss_out"), py::arg("g"), py::arg("p"), py::arg("m"), py::arg("v"), py::arg("lr"), py::arg("b1"),
        py::arg("b2"), py::arg("eps"), py::arg("step"), py::arg("state"), py::arg("norm_part"), py::arg("wimg"),
        py::arg("w_map"), py::arg("wt_map"), py::arg("dt"), py::arg("qmul"), py::arg("f8_img"), py::arg("f8_lid"),
        py::arg("f8_qs"), py::arg("gate"), py::arg("lr_dev") = py::none(), py::arg("tiles") = py::none(),
        py::arg("tiles_host") = py::none());
  m.def("kl_gate", &kl_gate, py::arg("loss_sums"), py::arg("gate"), py::arg("state"), py::arg("target_kl"),
        py::arg("lr_state") = py::none(), py::arg("kl_target") = 0.0, py::arg("factor") = 0.0,
        py::arg("lr_min") = 0.0, py::arg("lr_max") = 0.0);
  m.def("pack", &pack);
  m.def("debug_invalid_launch", &debug_invalid_launch);
  m.def("fp8_refresh", &fp8_refresh);
  m.def("set_x_stream", &set_x_stream);
  m.def("metrics_pack", &metrics_pack);
  m.def("probe_spin", &probe_spin);
  m.attr("arch") = "gfx950";
}
