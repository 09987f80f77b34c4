// sdxp_persist_phase_d.h - private to the persistent PPO update (included by sdxp_persist.hip and sdxp_persist_checks.hip only): the pieces of phase D
// behind the head forward that stand on the step's dependent chain - the loss phase and the backward through the heads.  As the tails of
// sdxp_persist_tails.h, each asks LDS for its operands ahead of their use and keeps the arithmetic of the block it replaces, operand for operand
// (tests/test_gpu_persist_loss_phase.py, tests/test_gpu_persist_head_backward.py).
#pragma once
#include "sdxp_persist_adam.h"   // elu_g, rounded
#include "sdxp_persist_lds.h"
#include "sdxp_persist_sums.h"   // pair_sum, half_sum

namespace {
// ---- backward through the heads.  Lane (column k = c2n, row half c2c) forms its part of dX3[.][k] over head rows 13 c2c + j, j < 13, with wc[j]
// this lane's column of those rows; the two halves of a column are lanes l and l ^ 32 of one wave and meet in pair_sum; elu' of the three
// networks' x3 is applied in both lanes.  The upper half's j = 10, 11 are the two value heads (a1, a2) and S.dmu[.][23..25] are zeros, so its a0
// takes three exact zeros.  d2[net][s] = dY2[net][s][k].
// What the chains read is requested ahead of them: the S.dmu operands of samples 0..2 in one batch, the upper half's eight S.dv values as two
// 16-byte reads in ONE lane-conditional block in front of the first chain - the lower half's a1 / a2 are +0.0f - and sample 0's three S.x3 operands;
// behind chain s, through an index made opaque against its result so that the request cannot rise, the S.dmu operands of sample s + 3 and the S.x3
// operands of sample s + 1.  No wait in the block, and every wait of the chains is a partial count.  (The block the compiler made of
// `c2c ? S.dv[j][s] * wc[..] : 0.0f` per sample was eight branches with one read and one drained wait each, two in front of every chain.)
// The lane condition stays, and the S.dmu operands of the fourth sample are not requested up front, for registers: with the S.dv reads unconditional,
// or with all 52 + 8 + 12 operands in flight at once, the epoch instantiation spills (22 VGPRs, 76 B of scratch; 5..9 with fewer reads ahead).
// Per sample: a0 = fma(dmu[12], wc[12], ... fma(dmu[0], wc[0], 0)), a1 / a2 = the ROUNDED product dv * wc (it crosses lanes as bits, nothing can
// contract it) or +0.0f, d2 = rn(pair_sum(a) * elu').
__device__ __forceinline__ void head_backward(const PLds& S, const float (&wc)[13], int c2c, int c2n, float (&d2)[3][MB]) {
  constexpr int A = ACT, MA = 3;   // MA: samples whose S.dmu operands are requested up front
  const int jr = 13 * c2c;
  float dm[MB][13], dv[2][MB], x[3][MB];
#pragma unroll
  for (int s = 0; s < MA; ++s)
#pragma unroll
    for (int j = 0; j < 13; ++j) dm[s][j] = S.dmu[s][jr + j];
  if (c2c) {
#pragma unroll
    for (int s = 0; s < MB; ++s) { dv[0][s] = S.dv[0][s]; dv[1][s] = S.dv[1][s]; }
  } else {
#pragma unroll
    for (int s = 0; s < MB; ++s) { dv[0][s] = 0.0f; dv[1][s] = 0.0f; }
  }
#pragma unroll
  for (int net = 0; net < 3; ++net) x[net][0] = S.x3[net][0][c2n];
  asm volatile("" ::: "memory");   // every request above stands in front of the first fma (ordered_sum_ahead)
#pragma unroll
  for (int s = 0; s < MB; ++s) {
    float a0 = __builtin_fmaf(dm[s][0], wc[0], 0.0f);
#pragma unroll
    for (int j = 1; j < 13; ++j) a0 = __builtin_fmaf(dm[s][j], wc[j], a0);
    if (s + MA < MB) {
      const int o = opaque(jr, a0);
#pragma unroll
      for (int j = 0; j < 13; ++j) dm[s + MA][j] = S.dmu[s + MA][o + j];
    }
    if (s + 1 < MB) {
      const int o = opaque(c2n, a0);
#pragma unroll
      for (int net = 0; net < 3; ++net) x[net][s + 1] = S.x3[net][s + 1][o];
    }
    const float t1 = dv[0][s] * wc[A - 13], t2 = dv[1][s] * wc[A - 12];
    const float a1 = c2c ? t1 : 0.0f, a2 = c2c ? t2 : 0.0f;
    d2[0][s] = pair_sum(a0) * elu_g(x[0][s]);
    d2[1][s] = pair_sum(a1) * elu_g(x[1][s]);
    d2[2][s] = pair_sum(a2) * elu_g(x[2][s]);
  }
}
// ---- the loss phase: two LDS barriers between the head forward and the heads' backward.  In front of the first, thread (sample s, action a) <
// MB 32 of waves 0 and 1 forms z, the half-wave sum gives lane 31 the sample's -log p, and that lane forms the ratio, the clipped actor loss and
// S.gnlp[s]; behind it the same threads form dmu and lanes T_LS + a form dlogstd.  The step's chain is waves 0 and 1 - the other six stand at the
// barriers - so what they wait for is asked for early and what does not need the ratio is taken off them:
//   * the four LDS operands of the z chain are requested by loss_request, which the kernel calls in front of the column view's address
//     arithmetic and loads;
//   * the two value-head losses (closs, d, S.dv[j][s], S.stat[s][STAT_CRITIC / STAT_CV]) use no ratio: lane (j, s) = T_VLOSS + MB j + s of wave 3
//     forms one each, with its own S.val read, where the ratio lane ran both behind its expf, each behind a round trip of its own;
//   * the dmu thread holds z, sigma and mu in front of the first barrier: it forms q = z / sigma (the IEEE division) and the bounds term
//     bt = bounds_coef (2 hi + 2 lo) there, and behind the barrier only reads S.gnlp[s]: dmu = fma(bt, invM, -rn(rn(gnlp q) invM));
//   * the dlogstd lanes request gnlp[0..3] and their four z in one batch.
// The arithmetic is the block's these replace (sdxp_ppo_terms.h restated), with the contractions hipcc gave it written out.
struct LossCfg { float e_clip, critic_coef, bounds_coef; bool clip_value; };
struct ZOps { float act, mu, sg, ls; };
constexpr int T_VLOSS = 3 * 64;   // + MB j + s: the value-head loss of (head j, sample s)
// Every thread asks, for (s, a) = its index modulo MB 32: no lane-dependent branch stands around the reads - behind one, the compiler's counter model
// drains everything outstanding, the S.z store included, at the next write of a register a read was to fill.  Only threads (s, a) < MB 32 with a < ACT
// use what they get (the padding lanes' slots exist).
__device__ __forceinline__ void loss_request(const PLds& S, int tid, ZOps& o) {
  const int s = (tid / 32) % MB, a = tid % 32;
  o.act = S.act[s][a]; o.mu = S.mu[s][a]; o.sg = S.sgm[a]; o.ls = S.ls[a];
}
// one value head's loss for one sample: v the head's value, R the return, vo the old value; returns closs, d the derivative before the coefficient
__device__ __forceinline__ float value_loss(const LossCfg& c, float v, float R, float vo, float& d) {
  const float vc = vo + clampf(v - vo, -c.e_clip, c.e_clip);
  const float c1v = (v - R) * (v - R), c2v = (vc - R) * (vc - R);
  if (c.clip_value) {
    const bool inv = fabsf(v - vo) <= c.e_clip;
    d = (c1v > c2v || inv) ? 2.0f * (v - R) : 0.0f;
    return fmaxf(c1v, c2v);
  }
  d = 2.0f * (v - R);
  return c1v;
}
// in front of the first barrier.  pf_adv / pf_nlp: lanes (s, 31) of waves 0 and 1; pf_ret / pf_val: lanes T_VLOSS + MB j + s.  q, bt: the dmu thread's
// two values for loss_back
__device__ __forceinline__ void loss_front(PLds& S, const LossCfg& c, int tid, const ZOps& o, float pf_adv, float pf_nlp, float pf_ret, float pf_val, float invM,
                                           float& q, float& bt) {
  constexpr int A = ACT;
  float r_nlp = 0.0f, z_act = o.act, z_mu = o.mu, z_sg = o.sg, z_ls = o.ls;
  SDX_PIN4X(z_act, z_mu, z_sg, z_ls);   // (taken in straight-line code, in front of the lane-dependent branches: see loss_request)
  q = 0.0f; bt = 0.0f;
  if (tid < MB * 32) {
    const int s = tid / 32, a = tid % 32;
    float zz = 0.0f;
    if (a < A) {
      zz = (z_act - z_mu) / z_sg;
      r_nlp = __builtin_fmaf(zz, 0.5f * zz, z_ls);
      q = zz / z_sg;
      const float hi = fmaxf(z_mu - 1.1f, 0.0f), lo = fminf(z_mu + 1.1f, 0.0f);
      bt = c.bounds_coef * __builtin_fmaf(2.0f, hi, lo + lo);
    }
    S.z[s][a] = zz;
  }
  r_nlp = half_sum(r_nlp);
  if (tid < MB * 32 && (tid % 32) == 31) {
    const int s = tid / 32;
    const float nlp = r_nlp + 0.5f * 1.8378770664093453f * (float)A;
    const float adv = pf_adv;
    const float ratio = expf(pf_nlp - nlp);
    const float L1 = -adv * ratio, L2 = -adv * clampf(ratio, 1.0f - c.e_clip, 1.0f + c.e_clip);
    const bool inr = ratio >= 1.0f - c.e_clip && ratio <= 1.0f + c.e_clip;
    S.gnlp[s] = (L1 > L2 || inr) ? adv * ratio : 0.0f;
    S.stat[s][STAT_ACTOR] = fmaxf(L1, L2);
  }
  if (tid >= T_VLOSS && tid < T_VLOSS + 2 * MB) {
    const int j = (tid - T_VLOSS) / MB, s = (tid - T_VLOSS) % MB;
    float d;
    const float closs = value_loss(c, S.val[j][s], pf_ret, pf_val, d);
    S.dv[j][s] = (j == 0 ? 0.5f * c.critic_coef : 1.0f) * d * invM;   // (1.0f * d is d)
    S.stat[s][j == 0 ? STAT_CRITIC : STAT_CV] = closs;
  }
}
// between the two barriers
__device__ __forceinline__ void loss_back(PLds& S, int tid, float q, float bt, float invM) {
  constexpr int A = ACT;
  if (tid < MB * 32) {
    const int s = tid / 32, a = tid % 32;
    float dmu = 0.0f;
    if (a < A) {
      const float t = (S.gnlp[s] * q) * invM;
      dmu = __builtin_fmaf(bt, invM, -t);
    }
    S.dmu[s][a] = dmu;
  }
  if (tid >= T_LS && tid < T_LS + 32) {
    const int a = tid - T_LS;
    float dls = 0.0f;
    if (a < A) {
      float gn[MB], zs[MB];
#pragma unroll
      for (int s = 0; s < MB; ++s) { gn[s] = S.gnlp[s]; zs[s] = S.z[s][a]; }
      asm volatile("" ::: "memory");   // every read requested in front of the first product (ordered_sum_ahead)
#pragma unroll
      for (int s = 0; s < MB; ++s) dls = __builtin_fmaf(gn[s] * __builtin_fmaf(-zs[s], zs[s], 1.0f), invM, dls);
    }
    S.dls[a] = dls;
  }
}
}  // namespace
