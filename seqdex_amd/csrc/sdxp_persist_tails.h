// sdxp_persist_tails.h - private to the persistent PPO update (included by sdxp_persist.hip and sdxp_persist_checks.hip only): the short serial
// pieces that close a phase of k_update_persistent on one wave or one thread while the other waves stand at the phase's barrier - the publish
// tails of forward L0 / L1 / L2 and the statistics / learning-rate thread of the dY1 shadow.  Each asks LDS for everything it needs in ONE go
// and keeps the arithmetic of the form it replaces, operand for operand (tests/test_gpu_persist_forward_tails.py, _stats_thread.py).
#pragma once
#include "sdxp_device.h"   // elu
#include "sdxp_persist_lds.h"
#include "sdxp_persist_sums.h"   // dpp_mov

namespace {
// ---- publish tails of the forward phases.  The waves left their partial dot products in S.fpart[(net MB + s) NWV + wave]; one lane of wave 0
// per (network, sample, owned row) forms that output - partial sums in ascending wave order, bias, elu - and the three networks of a (sample,
// row) meet in the lane that stores the packed word.  L: the layer; lane map (net, s, r) = lane:
//   L = 0: 16 net + 4 s + r < 48  (row r < 4: waves 2 r, 2 r + 1)        the lane's partial sums are S.fpart[2 lane ..+2)
//   L = 1:  8 net + 2 s + r < 24  (row r < 2: waves 4 r .. 4 r + 3)                                  S.fpart[4 lane ..+4)
//   L = 2:  4 net + s       < 12  (one row: waves 0 .. 7)                                            S.fpart[8 lane ..+8)
template <int L> struct FwdTail;
template <> struct FwdTail<0> { static constexpr int LANES = 3 * MB * 4, STORING = MB * 4, TERMS = 2; };
template <> struct FwdTail<1> { static constexpr int LANES = 3 * MB * 2, STORING = MB * 2, TERMS = 4; };
template <> struct FwdTail<2> { static constexpr int LANES = 3 * MB, STORING = MB, TERMS = NWV; };
static_assert(MB == 4 && NWV == 8, "lane maps of the forward tails");
// the pre-activation of lane < FwdTail<L>::LANES, in the order the one-lane-per-sample tails had:
//   L = 0: (q[0] + q[1]) + bias    L = 1: (((q[0] + q[1]) + q[2]) + q[3]) + bias    L = 2: ((bias + q[0]) + q[1]) + ... + q[7]
template <int L>
__device__ __forceinline__ float fwd_tail_pre(const PLds& S, int lane) {
  constexpr int T = FwdTail<L>::TERMS;
  const int net = lane / (FwdTail<L>::LANES / 3), r = lane % (FwdTail<L>::STORING / MB);
  const float b = S.bias[L == 0 ? BIAS_L0 + net * 4 + r : L == 1 ? BIAS_L1 + net * 2 + r : BIAS_L2 + net];
  float q[T];
#pragma unroll
  for (int w = 0; w < T; ++w) q[w] = S.fpart[T * lane + w];
  asm volatile("" ::: "memory");   // every read requested in front of the first add (ordered_sum_ahead)
  if (L == 2) {
    float t = b;
#pragma unroll
    for (int w = 0; w < T; ++w) t += q[w];
    return t;
  }
  float t = q[0];
#pragma unroll
  for (int w = 1; w < T; ++w) t += q[w];
  return t + b;
}
// The whole of wave 0 calls this (the cross-lane moves run with every lane active).  Lanes < FwdTail<L>::STORING = (sample, row) return with
// y[net] = the three networks' outputs of their word; the other lanes' y is of no use.
//   L = 0: networks 1, 2 sit 16 / 32 lanes up: v_permlane16_swap (rows 1, 3 -> rows 0, 2), v_permlane32_swap (upper half -> lower half)
//   L = 1: 8 / 16 lanes up: row_shl:8 inside the DPP row, v_permlane16_swap
//   L = 2: 4 / 8 lanes up: row_shl:4, row_shl:8
template <int L>
__device__ __forceinline__ void fwd_tail(const PLds& S, int lane, float (&y)[3]) {
  float v = 0.0f;
  if (lane < FwdTail<L>::LANES) v = elu(fwd_tail_pre<L>(S, lane));
  const unsigned u = __builtin_bit_cast(unsigned, v);
  y[0] = v;
  if (L == 0) {
    const auto r16 = __builtin_amdgcn_permlane16_swap(u, u, false, false);   // r16[1]: rows 1, 1, 3, 3 - lane l + 16 for l < 16
    const auto r32 = __builtin_amdgcn_permlane32_swap(u, u, false, false);   // r32[1]: the upper half in both halves - lane l + 32 for l < 32
    y[1] = __builtin_bit_cast(float, (unsigned)r16[1]); y[2] = __builtin_bit_cast(float, (unsigned)r32[1]);
  } else if (L == 1) {
    y[1] = dpp_mov<0x108, 0xF>(0.0f, v);                                    // row_shl:8: lane l + 8
    const auto r16 = __builtin_amdgcn_permlane16_swap(u, u, false, false);
    y[2] = __builtin_bit_cast(float, (unsigned)r16[1]);
  } else {
    y[1] = dpp_mov<0x104, 0xF>(0.0f, v);                                    // row_shl:4: lane l + 4
    y[2] = dpp_mov<0x108, 0xF>(0.0f, v);                                    // row_shl:8: lane l + 8
  }
}
// ---- the statistics / learning-rate thread of the dY1 shadow (thread T_STATS; every wave of the CU waits for it at the shadow's closing barrier).
// The 24 per-sample statistics (S.stat[s][STAT_ACTOR .. STAT_ENTROPY]), the six running sums and ac_lr are requested in ONE go; then the
// arithmetic of the loop it replaces: six 4-term sums from 0.0f in ascending s, each folded into its running sum as fma(t, invM, sum) - the
// contraction hipcc gave `sum += t * invM`, all six - the rounded kl = t * invM for the rule, and the legacy adaptive rule (PS:306-312) with its
// IEEE division.  The second comparison sees the learning rate the first one left, as it did through LDS.
__device__ __forceinline__ void stats_lr_once(PLds& S, float invM, bool adaptive, float klt) {
  PLds::Ctl& C = S.ctl;
  constexpr int NS = STAT_ENTROPY - STAT_ACTOR + 1;
  static_assert(NS == 6 && STAT_CRITIC == STAT_ACTOR + 1 && STAT_BOUNDS == STAT_ACTOR + 2 && STAT_KL == STAT_ACTOR + 3 && STAT_CV == STAT_ACTOR + 4, "statistics columns");
  float st[MB][NS], sum[NS], lr;
#pragma unroll
  for (int s = 0; s < MB; ++s)
#pragma unroll
    for (int j = 0; j < NS; ++j) st[s][j] = S.stat[s][STAT_ACTOR + j];
  sum[0] = C.sum_a; sum[1] = C.sum_c; sum[2] = C.sum_b; sum[3] = C.sum_kl; sum[4] = C.sum_cv; sum[5] = C.sum_ent; lr = C.ac_lr;
  asm volatile("" ::: "memory");   // every read requested in front of the first add
  float t[NS];
#pragma unroll
  for (int j = 0; j < NS; ++j) {
    t[j] = 0.0f;
#pragma unroll
    for (int s = 0; s < MB; ++s) t[j] += st[s][j];
  }
  float kl = t[STAT_KL - STAT_ACTOR] * invM;
  asm volatile("" : "+v"(kl));     // (the rounded product: the rule compares it, last_kl keeps it)
#pragma unroll
  for (int j = 0; j < NS; ++j) sum[j] = __builtin_fmaf(t[j], invM, sum[j]);
  C.sum_a = sum[0]; C.sum_c = sum[1]; C.sum_b = sum[2]; C.sum_kl = sum[3]; C.sum_cv = sum[4]; C.sum_ent = sum[5];
  C.last_kl = kl;
  if (adaptive) {
    // (the two thresholds are formed HERE from an opaque copy: hoisted out of the step loop they cost two registers for the whole launch)
    asm volatile("" : "+v"(klt));
    if (kl > 2.0f * klt) lr = fmaxf(lr / 1.5f, 1e-6f);
    if (kl < 0.5f * klt) lr = fminf(lr * 1.5f, 1e-2f);
    C.ac_lr = lr;
  }
}
// ---- head forward, wave per row: rows wave, wave + 8, wave + 16 (< 23: actor rows, except row 23 = the critic's value on wave 7) and wave + 24
// (only wave 0: row 24, the central value).  wh[j][e]: columns lane + 64 e of row wave + 8 j.  The actor rows of a wave share ONE set of x3
// operands; the value row's sixteen (S.x3[1] on wave 7, S.x3[2] on wave 0) and the biases of the wave's rows (row index clamped to the last
// row, loads unconditional) are requested with them, in front of the first fma - one LDS round trip where the value rows had eight dependent
// ones and the bias tail four.  Per (row, sample): fma(w, x, 0), then three fmas in ascending e; wave_sums over lanes; lane s < MB adds the bias
// and stores S.mu[s][row] / S.val[row - ACT][s].
__device__ __forceinline__ void head_forward(PLds& S, const float (&wh)[HR][4], int wave, int lane) {
  constexpr int A = ACT;
  float q[HR * MB], u[HR], xa[MB][4], xv[MB][4], hb[HR];   // value MB j + s: lane s < 4 ends with sample s of the wave's rows; xv: waves 0 and 7 only
  const bool vrow = wave == 0 || wave == NWV - 1;            // (wave-uniform)
#pragma unroll
  for (int s = 0; s < MB; ++s)
#pragma unroll
    for (int e = 0; e < 4; ++e) xa[s][e] = S.x3[0][s][lane + 64 * e];
  if (vrow) {
    const float* xr = &S.x3[wave == 0 ? 2 : 1][0][0];
#pragma unroll
    for (int s = 0; s < MB; ++s)
#pragma unroll
      for (int e = 0; e < 4; ++e) xv[s][e] = xr[s * U2 + lane + 64 * e];
  }
#pragma unroll
  for (int j = 0; j < HR; ++j) hb[j] = S.bias[BIAS_HEAD + min(wave + 8 * j, A + 1)];
  asm volatile("" ::: "memory");   // every read requested in front of the first fma (ordered_sum_ahead)
  auto dot = [](const float (&w)[4], const float (&x)[4]) -> float {
    float t = __builtin_fmaf(w[0], x[0], 0.0f);
#pragma unroll
    for (int e = 1; e < 4; ++e) t = __builtin_fmaf(w[e], x[e], t);
    return t;
  };
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int s = 0; s < MB; ++s) q[MB * j + s] = dot(wh[j], xa[s]);
  if (wave == NWV - 1) {          // row 23: critic value (net 1)
#pragma unroll
    for (int s = 0; s < MB; ++s) { SDX_PIN4(xv[s]); q[MB * 2 + s] = dot(wh[2], xv[s]); }   // (pinned: this side keeps its own sixteen fmas - no operand selects on the other waves)
  } else {
#pragma unroll
    for (int s = 0; s < MB; ++s) q[MB * 2 + s] = dot(wh[2], xa[s]);
  }
  if (wave == 0) {                // row 24: central value (net 2), the fourth quad of a 16-wide butterfly on this wave only
#pragma unroll
    for (int s = 0; s < MB; ++s) q[MB * 3 + s] = dot(wh[3], xv[s]);
    wave_sums<HR * MB>(q, u, lane);
  } else {
    float q3[3 * MB], u3[3];
#pragma unroll
    for (int i = 0; i < 3 * MB; ++i) q3[i] = q[i];
    wave_sums<3 * MB>(q3, u3, lane);
#pragma unroll
    for (int j = 0; j < 3; ++j) u[j] = u3[j];
    u[3] = 0.0f;
  }
  if (lane < MB) {                // sample s = lane: one bias per row
#pragma unroll
    for (int j = 0; j < HR; ++j) {
      const int row = wave + 8 * j;
      if (row < A + 2) { const float y = u[j] + hb[j]; if (row < A) S.mu[lane][row] = y; else S.val[row - A][lane] = y; }
    }
  }
}
}  // namespace
