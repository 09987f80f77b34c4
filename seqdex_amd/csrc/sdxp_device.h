// sdxp_device.h — device helpers shared by the PPO units (sdxp_rollout.hip, sdxp_update.hip, sdxp_multirank.hip, sdxp_persist.hip): ELU, the DPP wave sum
// and the accessors of the rank-MB factor buffers of SdxpDev.
#pragma once
#include "sdx_common.h"
#include "sdxp_types.h"
__device__ __forceinline__ float elu(float x) { return x > 0.0f ? x : expm1f(x); }
// wave64 sum with DPP cross-lane moves (VALU rate) instead of ds_bpermute-based __shfl_xor butterflies: quad_perm xor 1,
// xor 2, row_half_mirror, row_mirror give every lane its 16-lane row sum; row_bcast15 / row_bcast31 fold the four rows
// into lane 63, which is broadcast with v_readlane.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ float dpp_add(float v) {
  const int r = __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, ROW_MASK, 0xF, false);
  return v + __builtin_bit_cast(float, r);
}
__device__ __forceinline__ float wave_sum(float v) {
  v = dpp_add<0xB1, 0xF>(v);    // quad_perm [1,0,3,2]
  v = dpp_add<0x4E, 0xF>(v);    // quad_perm [2,3,0,1]
  v = dpp_add<0x141, 0xF>(v);   // row_half_mirror
  v = dpp_add<0x140, 0xF>(v);   // row_mirror
  v = dpp_add<0x142, 0xA>(v);   // row_bcast15 into rows 1 and 3
  v = dpp_add<0x143, 0xC>(v);   // row_bcast31 into rows 2 and 3
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 63));
}
__device__ __forceinline__ float lane0(float v) { return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, v))); }

// ---- small-minibatch (rank-MB) update: network ids 0 actor trunk, 1 critic trunk, 2 central-value trunk.
//   x[net][l] (l=1..3)   [2][MB][units[l-1]]  ELU output of trunk layer l-1 == input of layer l (l=3: head input),
//                        double buffered by optimiser-step parity.  Layer-0 inputs are read straight from the dataset
//                        (obs rows; pre-normalised central-value rows, see k_cv_prenorm).
//   dy2[net]             [2][MB][units[2]]    dLoss/d(pre-activation) of trunk layer 2 (written by the HEAD kernel)
//   dxacc[net][l] l=0,1  [2][MB][units[l]]    dLoss/d(OUTPUT) of trunk layer l, accumulated with atomics by the B kernels;
//                        consumers multiply by elu'(output) on the fly: dY_l = dxacc_l * elu'(x[l+1]).
__device__ __forceinline__ float elu_grad_from_out(float h) { return h > 0.0f ? 1.0f : h + 1.0f; }

template <int MB>
__device__ __forceinline__ const float* layer_input(const SdxpDev& D, const SdxpCtrl* ctl, int net, int l, bool cur) {
  const int par = ctl->step & 1;
  if (l > 0) return D.x[net][l] + (size_t)(cur ? par : par ^ 1) * MB * D.units[l - 1];
  const int mb = cur ? ctl->mb_index : ctl->prev_mb;
  const int me = cur ? ctl->mini_epoch : ctl->prev_mini_epoch;
  if (net == 2) return (me == 0 ? D.cvx0 : D.cvx1) + (size_t)mb * MB * D.state_dim;
  return D.mb_obs + (size_t)mb * MB * D.obs_dim;
}
// dLoss/d(pre-activation) of trunk layer l, sample s, neuron n, for step parity `par`
template <int MB>
__device__ __forceinline__ float dy_at(const SdxpDev& D, int net, int l, int par, int s, int n) {
  const int Nl = D.units[l];
  if (l == 2) return D.dy2[net][(size_t)par * MB * Nl + s * Nl + n];
  return D.dxacc[net][l][(size_t)par * MB * Nl + s * Nl + n] * elu_grad_from_out(D.x[net][l + 1][(size_t)par * MB * Nl + s * Nl + n]);
}
