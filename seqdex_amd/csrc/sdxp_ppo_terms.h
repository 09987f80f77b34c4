// sdxp_ppo_terms.h — rl_games' PPO arithmetic of one minibatch, stated once: the loss terms per (row, action) and per row with
// their gradients, the step rules (clip_grad_norm_ scale, Adam bias corrections, legacy adaptive learning rate), the Adam element
// functions and the control block's bookkeeping.  Functions of scalars: no thread index, no LDS, no global memory; how a kernel
// spreads rows and actions over its lanes and reduces the summands is the kernel's own (sdxp_update.hip, sdxp_bigmb.hip).
// k_update_persistent (sdxp_persist.hip) restates the loss phase and the step rules in place: its schedule depends on the text.
#pragma once
#include "sdx_common.h"
#include "sdxp_types.h"

#define SDXP_LOG_2PI 1.8378770664093453f

// ------------------------------------------------------------------------------------------------ per (row, action)
// z = (action - mu) / sigma and the summands of the row's Gaussian neglogp (RC:2114-2126; the row adds 0.5 log(2 pi) act_dim:
// ppo_neglogp), of the KL to the stored mu / sigma (policy_kl), of the bound loss (soft bound 1.1) and of the entropy
__device__ __forceinline__ float ppo_z(float act, float mu, float sg) { return (act - mu) / sg; }
struct PpoActionTerms { float z, nlp, kl, bl, ent; };
__device__ __forceinline__ PpoActionTerms ppo_action_terms(float ls, float sg, float mu, float act, float omu, float osg) {
  PpoActionTerms t;
  t.z = ppo_z(act, mu, sg);
  t.nlp = 0.5f * t.z * t.z + ls;
  t.kl = logf(osg / sg + 1e-5f) + (sg * sg + (omu - mu) * (omu - mu)) / (2.0f * (osg * osg + 1e-5f)) - 0.5f;
  const float hi = fmaxf(mu - 1.1f, 0.0f), lo = fminf(mu + 1.1f, 0.0f);
  t.bl = hi * hi + lo * lo;
  t.ent = 0.5f + 0.5f * SDXP_LOG_2PI + ls;
  return t;
}
__device__ __forceinline__ float ppo_neglogp(float sum_nlp, int act_dim) { return sum_nlp + 0.5f * SDXP_LOG_2PI * (float)act_dim; }
// d loss / d mu of one (row, action), and the row's summand of d loss / d logstd; gnlp = d loss / d neglogp of the row (ppo_row_terms)
__device__ __forceinline__ float ppo_dlogstd_term(float gnlp, float z, float invM) { return gnlp * (1.0f - z * z) * invM; }
struct PpoActionGrad { float dmu, dls; };
__device__ __forceinline__ PpoActionGrad ppo_action_grad(float gnlp, float z, float sg, float mu, float bounds_coef, float invM) {
  const float hi = fmaxf(mu - 1.1f, 0.0f), lo = fminf(mu + 1.1f, 0.0f);
  PpoActionGrad g;
  g.dmu = gnlp * (-(z / sg)) * invM + bounds_coef * (2.0f * hi + 2.0f * lo) * invM;
  g.dls = ppo_dlogstd_term(gnlp, z, invM);
  return g;
}
// d loss / d logstd from the summed row terms: d(-coef * mean entropy) / d logstd = -coef; the gradient norm sees this value
__device__ __forceinline__ float ppo_dlogstd(float sum_dls, float entropy_coef) { return sum_dls - entropy_coef; }

// ------------------------------------------------------------------------------------------------ per row
// clipped surrogate (RC:1813) and the (clipped) value losses of the critic [0] and the central value [1] (RC:1818-1822) with their
// gradients: gnlp = d max(L1, L2) / d neglogp (L2 is constant outside the clip range), dv[j] = d loss / d v_j (outside the clip range
// v_clipped is constant); the critic's loss enters with 0.5 critic_coef (RC:2129-2132), the central value trains on its own
struct PpoRowTerms { float gnlp, a_loss, closs[2], dv[2]; };
__device__ __forceinline__ PpoRowTerms ppo_row_terms(const SdxpDev& D, float adv, float old_nlp, float nlp, float R, float vo, float v0,
                                                     float v1, float invM) {
  PpoRowTerms t;
  const float ratio = expf(old_nlp - nlp);
  const float L1 = -adv * ratio, L2 = -adv * clampf(ratio, 1.0f - D.e_clip, 1.0f + D.e_clip);
  const bool inr = ratio >= 1.0f - D.e_clip && ratio <= 1.0f + D.e_clip;
  t.gnlp = (L1 > L2 || inr) ? adv * ratio : 0.0f;
  t.a_loss = fmaxf(L1, L2);
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const float v = j == 0 ? v0 : v1;
    const float vc = vo + clampf(v - vo, -D.e_clip, D.e_clip);
    const float c1 = (v - R) * (v - R), c2 = (vc - R) * (vc - R);
    float d;
    if (D.clip_value) {
      t.closs[j] = fmaxf(c1, c2);
      const bool inv = fabsf(v - vo) <= D.e_clip;
      d = (c1 > c2 || inv) ? 2.0f * (v - R) : 0.0f;
    } else { t.closs[j] = c1; d = 2.0f * (v - R); }
    t.dv[j] = (j == 0 ? 0.5f * D.critic_coef : 1.0f) * d * invM;
  }
  return t;
}

// ------------------------------------------------------------------------------------------------ step rules
// clip_grad_norm_ (RC:1859-1877): the factor on the gradient, from its norm
__device__ __forceinline__ float ppo_clip_scale(const SdxpDev& D, float norm) {
  return D.truncate_grads ? fminf(1.0f, D.grad_norm / (norm + 1e-6f)) : 1.0f;
}
// Adam's bias corrections 1 - beta^t of step t (betas 0.9 / 0.999), and the two factors adam1 / adam1x take
struct PpoBias { float bc1, bc2; };
__device__ __forceinline__ PpoBias ppo_adam_bias(int t) { return {1.0f - powf(0.9f, (float)t), 1.0f - powf(0.999f, (float)t)}; }
struct PpoAdamScales { float lr_bc1, isq_bc2; };
__device__ __forceinline__ PpoAdamScales ppo_adam_scales(float lr, int t) {
  const PpoBias b = ppo_adam_bias(t);
  return {lr / b.bc1, 1.0f / sqrtf(b.bc2)};
}
// legacy adaptive schedule, after every minibatch, on the (rank-averaged) minibatch KL (PS:306-312)
__device__ __forceinline__ float ppo_adaptive_lr(float lr, float kl, float kl_threshold) {
  if (kl > 2.0f * kl_threshold) lr = fmaxf(lr / 1.5f, 1e-6f);
  if (kl < 0.5f * kl_threshold) lr = fminf(lr * 1.5f, 1e-2f);
  return lr;
}

// ------------------------------------------------------------------------------------------------ Adam element functions
// Adam step of one parameter (torch.optim.Adam, betas 0.9/0.999, eps 1e-8, bias corrections bc1/bc2 precomputed)
__device__ __forceinline__ float adam1(float w, float g, float& m, float& v, float lr_bc1, float isq_bc2) {
  m = 0.9f * m + 0.1f * g;
  v = 0.999f * v + 0.001f * g * g;
  return w - lr_bc1 * m / (sqrtf(v) * isq_bc2 + 1e-8f);
}
// adam1 with every rounding spelled out (no compiler-chosen contraction): k_adam3 and the one-launch apply (k_apply_factors_fused) inline it
// in different surroundings, where hipcc picked different fused multiply-adds for `0.9 m + 0.1 g` (first moments one ulp apart after one
// step); written this way the two forms of the apply are bit-identical (tests/test_gpu_fullsize_properties.py).
__device__ __forceinline__ float adam1x(float w, float g, float& m, float& v, float lr_bc1, float isq_bc2) {
#pragma clang fp contract(off)
  m = __builtin_fmaf(0.1f, g, 0.9f * m);
  v = __builtin_fmaf(0.001f * g, g, 0.999f * v);
  const float den = __builtin_fmaf(sqrtf(v), isq_bc2, 1e-8f);
  const float q = (lr_bc1 * m) / den;
  return w - q;
}

// ------------------------------------------------------------------------------------------------ control-block bookkeeping
// (on a reference: k_ctrl works on an LDS copy of the block, the other kernels on the one in HBM)
// end of a minibatch's loss: its sums over the rows, which the head kernels left in acc[1..6], into the epoch's statistics; returns
// the minibatch KL, which also goes to *kl_word where one is given (ac_g[g_tail]: it rides with the gradients)
__device__ __forceinline__ float ppo_account_minibatch(SdxpCtrl& c, float invM, float* kl_word) {
  const float kl = c.acc[4] * invM;
  c.sum_a_loss += c.acc[1] * invM; c.sum_c_loss += c.acc[2] * invM; c.sum_b_loss += c.acc[3] * invM;
  c.sum_kl += kl; c.sum_cv_loss += c.acc[5] * invM; c.sum_entropy += c.acc[6] * invM;
  c.n_mb += 1; c.last_kl = kl;
  if (kl_word) *kl_word = kl;
  return kl;
}
// the minibatch cursor: remembers the staged minibatch and, when one was just back-propagated, moves on to the next
__device__ __forceinline__ void ppo_advance_cursor(SdxpCtrl& c, int num_minibatches, bool stepped) {
  c.prev_mb = c.mb_index; c.prev_mini_epoch = c.mini_epoch;
  if (stepped) {
    int mbn = c.mb_index + 1;
    if (mbn >= num_minibatches) { mbn = 0; c.mini_epoch += 1; }
    c.mb_index = mbn;
    c.step += 1;
  }
}
// the explicit-gradient forms leave Adam to the apply kernels: nothing pending, squared norms start over
__device__ __forceinline__ void ppo_explicit_reset(SdxpCtrl& c) { c.gn2_ac = 0.0f; c.gn2_cv = 0.0f; c.ac_pending = 0; c.cv_pending = 0; }
// tail of an apply: Adam counter, running beta^t and reported gradient norm of one optimiser (which: 0 actor-critic, 1 central value)
__device__ __forceinline__ void ppo_adam_advance(SdxpCtrl& c, int which) {
  int32_t& t = which ? c.cv_t : c.ac_t;
  double &b1 = which ? c.cv_b1pow : c.ac_b1pow, &b2 = which ? c.cv_b2pow : c.ac_b2pow;
  t += 1; b1 *= 0.9; b2 *= 0.999;
  (which ? c.cv_gnorm : c.ac_gnorm) = sqrtf(which ? c.gn2_cv : c.gn2_ac);
}
// ... and the learning-rate rule on the rank-averaged KL
__device__ __forceinline__ void ppo_lr_advance(SdxpCtrl& c, const SdxpDev& D, float kl) {
  if (D.adaptive_lr) c.ac_lr = ppo_adaptive_lr(c.ac_lr, kl, D.kl_threshold);
}
