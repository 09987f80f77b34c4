// sdxp_persist_adam.h - private to sdxp_persist.hip (included by it and by the test entries of sdxp_persist_checks.hip): the per-element Adam updates of k_update_persistent and the opaque
// copies / register pins that keep its schedule and register allocation where they are
#pragma once
#include "sdxp_persist_lds.h"

namespace {
__device__ __forceinline__ float elu_g(float h) { return h > 0.0f ? 1.0f : h + 1.0f; }
// Opaque copy of an index.  volatile asm statements keep their program order relative to each other and to sched_barrier,
// and an LDS load whose address depends on the result cannot be floated above it: this is what keeps the operand loads of
// Adam element i+1 below the arithmetic of element i.
// Passing the weight updated by element i as a (fake) input orders element i+1's loads after element i's arithmetic too.
__device__ __forceinline__ int opaque(int x, float after) { asm volatile("" : "+v"(x) : "v"(after)); return x; }
__device__ __forceinline__ void adam1(float& w, float g, float& m, float& v, float lr_bc1, float isq_bc2) {
  m = 0.9f * m + 0.1f * g;
  v = 0.999f * v + 0.001f * g * g;
  // v_sqrt_f32 / v_rcp_f32 (1 ulp each) instead of the IEEE sequences: the Adam arithmetic of ~45 elements per lane is VALU bound
  w -= lr_bc1 * m * __builtin_amdgcn_rcpf(__builtin_amdgcn_sqrtf(v) * isq_bc2 + 1e-8f);
  // one element at a time: without this the scheduler forms all ~45 gradients of the lane first and holds them (and the
  // half-updated moments) in registers while it interleaves the long sqrt/div chains
  __builtin_amdgcn_sched_barrier(0);
}
// layer 0 (the only Adam on the step's dependent chain): the moments arrive PRE-SCALED by 0.9 / 0.999 - done in the dY0 shadow, where the
// element's gradient is formed - so that behind the clip scale an element is 7 VALU + sqrt + rcp instead of 11 (round 6)
__device__ __forceinline__ void adam1p(float& w, float g, float& m9, float& v999, float lr_bc1, float isq_bc2) {
  m9 = __builtin_fmaf(0.1f, g, m9);
  v999 = __builtin_fmaf(0.001f * g, g, v999);
  w -= lr_bc1 * m9 * __builtin_amdgcn_rcpf(__builtin_amdgcn_sqrtf(v999) * isq_bc2 + 1e-8f);
  __builtin_amdgcn_sched_barrier(0);
}
// the optimiser step's scalars (PLds::scal, SC_*) and the selection per network: the actor and the critic share one optimiser, the central
// value (net 2) has its own
struct StepScal {
  float gs_ac, gs_cv, ac_lr_bc1, ac_isq, cv_lr_bc1, cv_isq;
  __device__ __forceinline__ float gs(int net) const { return net == 2 ? gs_cv : gs_ac; }
  __device__ __forceinline__ float lrb(int net) const { return net == 2 ? cv_lr_bc1 : ac_lr_bc1; }
  __device__ __forceinline__ float isq(int net) const { return net == 2 ? cv_isq : ac_isq; }
};
__device__ __forceinline__ StepScal step_scal(const PLds& S) {
  return {S.scal[SC_AC_GSCALE], S.scal[SC_CV_GSCALE], S.scal[SC_AC_LR_BC1], S.scal[SC_AC_ISQ], S.scal[SC_CV_LR_BC1], S.scal[SC_CV_ISQ]};
}
// Adam of the bias in `slot` (BIAS_*) of network `net`, run by the slot's thread; gg: sum_s dY_s[row], before the clip scale
__device__ __forceinline__ void adam_bias(PLds& S, const StepScal& sc, int slot, int net, float gg) {
  float b = S.bias[slot], bm = S.bias_m[slot], bv = S.bias_v[slot];
  adam1(b, gg * sc.gs(net), bm, bv, sc.lrb(net), sc.isq(net));
  S.bias[slot] = b; S.bias_m[slot] = bm; S.bias_v[slot] = bv;
}
#define SDX_PIN4X(a, b, c, d) asm volatile("" : "+v"(a), "+v"(b), "+v"(c), "+v"(d))
#define SDX_PIN3X(a, b, c) asm volatile("" : "+v"(a), "+v"(b), "+v"(c))

// ---- Adam with the operands of the next elements in flight (the x1 shadow), two elements at a time
// adam1 with every rounding written out: the three products a contraction could take either way go through an opaque copy, the fmas are
// explicit.  These are the forms hipcc gives adam1 inside the serial loops (tests/test_gpu_persist_adam_ahead.py holds the two to each other):
//   m = fma(0.1, g, rn(0.9 m)), v = fma(g, rn(0.001 g), rn(0.999 v)), w = fma(-rn(lrb m), rcp(fma(isq, sqrt(v), 1e-8)), w)
// adam2x takes TWO elements through these forms as packed f32 (v_pk_mul_f32 / v_pk_fma_f32: two independent IEEE operations per lane and
// instruction, each component rounded as the plain instruction rounds it, so a pair ends with the bits of its two elements run one after the
// other; the one-element form adam1x is kept as the reference in sdxp_persist_checks.hip).  Only operations whose operands are pairs already -
// or one splat built once for several uses - are paired: v_sqrt_f32 / v_rcp_f32 have no packed form and stay per component.
typedef float f32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ f32x2 rounded2(f32x2 x) { asm volatile("" : "+v"(x)); return x; }
__device__ __forceinline__ f32x2 splat2(float x) { return f32x2{x, x}; }
__device__ __forceinline__ f32x2 fma2(f32x2 a, f32x2 b, f32x2 c) { return __builtin_elementwise_fma(a, b, c); }
__device__ __forceinline__ void adam2x(f32x2& w, f32x2 g, f32x2& m, f32x2& v, float lr_bc1, float isq_bc2) {
  const f32x2 m9 = rounded2(splat2(0.9f) * m), v999 = rounded2(splat2(0.999f) * v), t = rounded2(splat2(0.001f) * g);
  m = fma2(splat2(0.1f), g, m9);
  v = fma2(g, t, v999);
  const f32x2 lm = rounded2(splat2(lr_bc1) * m);
  const f32x2 sq = {__builtin_amdgcn_sqrtf(v.x), __builtin_amdgcn_sqrtf(v.y)};
  const f32x2 dn = fma2(splat2(isq_bc2), sq, splat2(1e-8f));
  const f32x2 rc = {__builtin_amdgcn_rcpf(dn.x), __builtin_amdgcn_rcpf(dn.y)};
  w = fma2(-lm, rc, w);
  __builtin_amdgcn_sched_barrier(0);
}
// the gradient elements sum_s d_s x_s of two elements that share the factors d_s (splats), from 0 in ascending order of s, one fma per sample
__device__ __forceinline__ f32x2 grad4x2(const f32x2 (&d)[MB], const f32x2 (&x)[MB]) {
  static_assert(MB == 4, "four samples");
  return fma2(d[3], x[3], fma2(d[2], x[2], fma2(d[1], x[1], fma2(d[0], x[0], splat2(0.0f)))));
}
// Adam of layer 1 as ONE loop over the lane's 24 elements, taken two at a time: per network the row elements (0, 1), (2, 3) (columns kr + 64 i of
// S.x1, factors S.dyown[net][.][DY_L1 + o_row]), then the column elements (0, 1), (2, 3) (columns kc + c, factors S.dy1[net][.][o_thr]) - the
// serial loops' order.  The two elements of a pair share their factors and their scalars; their weights, moments and S.x1 operands are pairs.
// The eight operands of pair p are pinned together (one wait), then the eight S.x1 operands of pair p + 1 are requested - through an
// index made opaque against the weight pair p - 1 wrote, so the request can rise no further, and with a sched_barrier behind it, so it
// cannot sink into the arithmetic of pair p - and fly under that arithmetic.  The pin stands IN FRONT of the request on purpose: every wait
// hipcc places in this region is lgkmcnt(0), never a partial count, so a wait behind the request would drain the reads just issued; in front of
// it, it finds reads that were requested a whole pair ago.  The factors are requested a network ahead, into the registers their
// predecessors left: the row factors under the first column pair of the network in front, the column factors under the first row pair; each is
// scaled by the clip factor (plain products, as before) and splatted where it is first used.
// sink(net, j, gg): the gradient element, for the test entries; the kernel passes an empty one.
template <class Sink>
__device__ __forceinline__ void adam_l1_ahead(const PLds& S, const StepScal& sc, int kr, int kc, int o_row, int o_thr, float (&w1)[3][4],
                                              float (&m1)[3][4], float (&v1)[3][4], float (&c1)[3][4], float (&cm1)[3][4], float (&cv1)[3][4],
                                              Sink&& sink) {
  float dr[MB], dn[MB], dep = 0.0f;
  f32x2 x[2][MB], d2[MB];   // x[p & 1]: the operands of pair p; d2: the factors of the pair's kind, scaled and splatted
  {
    const int o_r = opaque(o_row, dep), o_t = opaque(o_thr, dep), k = opaque(kr, dep);
#pragma unroll
    for (int s = 0; s < MB; ++s) { dr[s] = S.dyown[0][s][DY_L1 + o_r]; dn[s] = S.dy1[0][s][o_t]; x[0][s] = f32x2{S.x1[0][s][k], S.x1[0][s][k + 64]}; }
  }
#pragma unroll
  for (int p = 0; p < 12; ++p) {
    const int net = p / 4, jp = p % 4, j = 2 * jp;   // elements j, j + 1 of the network: j < 4 rows, else columns j - 4, j - 3
    f32x2 (&xc)[MB] = x[p & 1], (&xn)[MB] = x[(p + 1) & 1];
    SDX_PIN4X(xc[0], xc[1], xc[2], xc[3]);
    if (p + 1 < 12) {
      const int n1 = (p + 1) / 4, j1 = 2 * ((p + 1) % 4);
      const int k = opaque(j1 < 4 ? kr + 64 * j1 : kc + (j1 - 4), dep);
#pragma unroll
      for (int s = 0; s < MB; ++s) xn[s] = f32x2{S.x1[n1][s][k], S.x1[n1][s][k + (j1 < 4 ? 64 : 1)]};
    }
    if (jp == 2 && net < 2) {
      const int o_r = opaque(o_row, dep);
#pragma unroll
      for (int s = 0; s < MB; ++s) dr[s] = S.dyown[net + 1][s][DY_L1 + o_r];
    }
    if (jp == 0 && net > 0) {
      const int o_t = opaque(o_thr, dep);
#pragma unroll
      for (int s = 0; s < MB; ++s) dn[s] = S.dy1[net][s][o_t];
    }
    __builtin_amdgcn_sched_barrier(0);
    if (jp == 0) {
#pragma unroll
      for (int s = 0; s < MB; ++s) d2[s] = splat2(dr[s] * sc.gs(net));
    }
    if (jp == 2) {
#pragma unroll
      for (int s = 0; s < MB; ++s) d2[s] = splat2(dn[s] * sc.gs(net));
    }
    const f32x2 gg = grad4x2(d2, xc);
    sink(net, j, gg.x); sink(net, j + 1, gg.y);
    float (&wa)[4] = j < 4 ? w1[net] : c1[net], (&ma)[4] = j < 4 ? m1[net] : cm1[net], (&va)[4] = j < 4 ? v1[net] : cv1[net];
    const int i = j & 3;
    f32x2 w = {wa[i], wa[i + 1]}, m = {ma[i], ma[i + 1]}, v = {va[i], va[i + 1]};
    adam2x(w, gg, m, v, sc.lrb(net), sc.isq(net));
    wa[i] = w.x; wa[i + 1] = w.y; ma[i] = m.x; ma[i + 1] = m.y; va[i] = v.x; va[i + 1] = v.y;
    dep = w.y;
  }
}
}  // namespace
