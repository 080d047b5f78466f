// The loss arithmetic of the update step, shared by its three kernel families (csrc/mlp.hip the tile
// kernel, csrc/mlp_head.hip the 16x16 per-head kernels, csrc/phead.hip the 32x32 policy kernel): one
// definition, so every path rounds identically and a new loss is one function here plus a call per
// kernel.  Scalar fp32 in, a small struct or a float out.  A kernel keeps what is its own: where a
// dim's action, mu and log_std live, the order of the dims, the group sums, the `valid` masks and
// every store (dL/dmu, dL/dlog_std, mu_prev / v_prev, the loss row).
// A helper is optimised on its own before it is inlined, so where it is cut decides the kernels' code.
// The cuts below (what the caller forms and passes, what is a function of its own) are the ones that
// leave the kernels' registers and code size as they were: profiles/loss_core/README.md.
#pragma once
#include "kernels.h"
#include "common.h"

namespace {

// ---- clipped surrogate of corrected PPO (ppo.py:148-167) from the row's log-ratio ----
struct Surrogate {
  float loss;      // -min(ratio adv, clip(ratio) adv)
  float dlogp;     // d loss / d logp
  float kl;        // (ratio - 1) - log ratio
  float clipped;   // 1: |ratio - 1| > clip
};
DEV Surrogate ppo_surrogate(float lrat, float adv, float clip) {
  const float ratio = __expf(lrat);
  const float s1 = ratio * adv;
  const float s2 = fminf(fmaxf(ratio, 1.f - clip), 1.f + clip) * adv;
  Surrogate o;
  o.loss = -fminf(s1, s2);
  o.dlogp = (s1 <= s2) ? -adv * ratio : 0.f;
  o.kl = (ratio - 1.f) - lrat;
  o.clipped = (fabsf(ratio - 1.f) > clip) ? 1.f : 0.f;
  return o;
}

// ---- Gaussian head, one action dim: lsig = log sigma of the dim, and the caller forms
// isig = __expf(-lsig), z = (x - mu) * isig where its x and mu live ----
// the dim's term of the row's log-prob
DEV float gauss_logp_dim(float z, float lsig) { return -0.5f * z * z - 0.5f * LOG_2PI_F - lsig; }
// the dim's term of the entropy bonus -ent_coeff * H
DEV float gauss_ent_dim(float lsig, float ent_coeff) { return -ent_coeff * (0.5f + 0.5f * LOG_2PI_F + lsig); }
// dL/dmu and dL/dlog_std of the dim (log-prob term + entropy bonus; cvar: d lsig / d log_std)
struct GaussGrad { float dmu, dls; };
DEV GaussGrad gauss_grad_dim(float z, float isig, float dlogp, float ent_coeff, float cvar) {
  GaussGrad o;
  o.dmu = dlogp * z * isig;
  o.dls = (dlogp * (z * z - 1.f) - ent_coeff) * cvar;
  return o;
}

// ---- categorical head, one logit: dL/dz_k = dlogp (o_k - p_k) + ent_coeff p_k ((z_k - lse) + H) ----
// lz = z_k - lse and p = __expf(lz) (never log p_k: p_k may underflow to 0), o = the one-hot action's entry k
DEV float cat_grad_dim(float o, float p, float lz, float H, float dlogp, float ent_coeff) {
  return dlogp * (o - p) + ent_coeff * p * (lz + H);
}

// ---- reference DPPO loss (train.py:142-161), one action dim: per-dim pdf ratio, variance convention,
// entropy as p log(p + 1e-5); invA = 1 / A (the mean over the dims).  terms -> dL/dp -> (dL/dmu, dL/dlog_std),
// then the clip flag: dppo_ref_dim, dppo_ref_dp (once per dim), dppo_ref_dmu / _dls under the caller's `valid`,
// dppo_ref_cf. ----
struct RefDim {
  float lclip, lent;      // the row's running sums with the dim's terms added
  float p, lg, dps;       // carried to dppo_ref_dp: the pdf, log(p + 1e-5), the surrogate's share of dL/dp
  float ratio;            // carried to dppo_ref_cf
};
DEV RefDim dppo_ref_dim(float x, float mu, float var, float mu_o, float var_o, float adv, float clip, float ent_coeff,
                        float invA, float lclip, float lent) {
  RefDim o;
  o.p = __expf(-(x - mu) * (x - mu) / (2.f * var)) * rsqrtf(2.f * var * 3.14159265358979f);
  const float po = __expf(-(x - mu_o) * (x - mu_o) / (2.f * var_o)) * rsqrtf(2.f * var_o * 3.14159265358979f);
  o.ratio = o.p / (1e-10f + po);
  const float s1 = o.ratio * adv;
  const float s2 = fminf(fmaxf(o.ratio, 1.f - clip), 1.f + clip) * adv;
  o.lclip = lclip + -fminf(s1, s2) * invA;
  const float dratio = (s1 <= s2) ? -adv * invA : 0.f;
  o.dps = dratio / (1e-10f + po);
  o.lg = logf(o.p + 1e-5f);
  o.lent = lent + -ent_coeff * o.p * o.lg * invA;
  return o;
}
// dL/dp of the dim
DEV float dppo_ref_dp(const RefDim& t, float adv, float ent_coeff, float invA) {
  float dp = t.dps;
  dp += -ent_coeff * invA * (t.lg + t.p / (t.p + 1e-5f));
  return dp;
}
// dL/dmu and dL/dlog_std (log_std = log of the variance) from dL/dp
DEV float dppo_ref_dmu(float dp, float p, float x, float mu, float var) { return dp * p * (x - mu) / var; }
DEV float dppo_ref_dls(float dp, float p, float x, float mu, float var) {
  return dp * p * ((x - mu) * (x - mu) / (2.f * var) - 0.5f);
}
// the dim's contribution to the row's clip fraction
DEV float dppo_ref_cf(const RefDim& t, float clip, float invA) { return (fabsf(t.ratio - 1.f) > clip) ? invA : 0.f; }

// ---- value loss of one row, mse and clipped_half; the caller branches on MlpArgs::value_loss, chooses
// vold and forms d = v - ret ----
DEV void value_mse(float d, float& lv, float& dv) {
  lv = d * d;
  dv = 2.f * d;
}
DEV void value_clipped_half(float d1, float v, float ret, float vold, float clip, float& lv, float& dv) {
  const float dd = v - vold;
  const float vc = vold + fminf(fmaxf(dd, -clip), clip);
  const float d2 = vc - ret;
  const float f1 = d1 * d1, f2 = d2 * d2;
  const float inr = (dd >= -clip && dd <= clip) ? 1.f : 0.f;
  lv = 0.5f * fmaxf(f1, f2);
  // the gradient follows the larger term; a tie takes half of each
  if (f1 > f2) dv = d1;
  else if (f2 > f1) dv = d2 * inr;
  else dv = 0.5f * d1 + 0.5f * d2 * inr;
}

}  // namespace
