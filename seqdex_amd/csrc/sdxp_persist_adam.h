// sdxp_persist_adam.h - private to sdxp_persist.hip (included by it only): the per-element Adam updates of k_update_persistent and the opaque
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
}  // namespace
