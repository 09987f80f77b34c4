// sdxp_device.h — device helpers shared by the PPO units (sdxp_rollout.hip, sdxp_update.hip, sdxp_multirank.hip, sdxp_persist.hip): ELU, the DPP wave sum
// the accessors of the rank-MB factor buffers of SdxpDev, and the parameter map of the rank-MB kernels (trunk_slot, head_row, trunk_kmax).
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

// ---- the parameter map of the rank-MB kernels, stated once.  Actor and critic share the actor-critic buffers (ac, ac_m, ac_v, ac_g; offsets
// SdxpDev::off), the central value has its own (cv, ...; SdxpDev::coff).
// Trunk layer l of network net: weight [N][K] at woff, bias [N] at boff of the network's parameter / moment / gradient buffers
struct TrunkSlot { int K, N; size_t woff, boff; float *P, *M, *V, *G; };
__device__ __forceinline__ TrunkSlot trunk_slot(const SdxpDev& D, int net, int l) {
  // (the eight pointers are read, then chosen among: written as net == 2 ? D.cv : D.ac the compiler chooses the address first and the
  // kernels' scalar preambles become chains of dependent loads)
  float *const ac = D.ac, *const ac_m = D.ac_m, *const ac_v = D.ac_v, *const ac_g = D.ac_g, *const cv = D.cv, *const cv_m = D.cv_m, *const cv_v = D.cv_v, *const cv_g = D.cv_g;
  return {(l == 0) ? (net == 2 ? D.state_dim : D.obs_dim) : D.units[l - 1], D.units[l],
          net == 0 ? D.off.a_w[l] : net == 1 ? D.off.c_w[l] : D.coff.w[l], net == 0 ? D.off.a_b[l] : net == 1 ? D.off.c_b[l] : D.coff.b[l],
          net == 2 ? cv : ac, net == 2 ? cv_m : ac_m, net == 2 ? cv_v : ac_v, net == 2 ? cv_g : ac_g};
}
// Head row `row`: rows 0 .. A-1 are mu, row A the critic's value, row A+1 the central value.  net: whose trunk feeds it; buf: 0 the
// actor-critic buffers, 1 the central value's; weight [units[2]] at woff, bias at boff; col: the row's column of dhead [MB][34]
struct HeadRow { int net, buf, col; size_t woff, boff; };
__device__ __forceinline__ HeadRow head_row(const SdxpDev& D, int row) {
  const int A = D.act_dim;
  return {row < A ? 0 : (row == A ? 1 : 2), row <= A ? 0 : 1, row < A ? row : 32 + (row - A),
          row < A ? D.off.mu_w + (size_t)row * D.units[2] : (row == A ? D.off.v_w : D.coff.v_w), row < A ? D.off.mu_b + row : (row == A ? D.off.v_b : D.coff.v_b)};
}
// launch shapes of the kernels that give a wave one weight row of trunk layer l (k_grad_layer, k_grad_layer_w, the trunk blocks of the
// apply grid): the longest row among the three networks (the LDS image of the layer's input is sized by it), and the workgroups of four rows
inline int trunk_kmax(const SdxpDev* D, int l) { return l == 0 ? (D->state_dim > D->obs_dim ? D->state_dim : D->obs_dim) : D->units[l - 1]; }
__host__ __device__ inline int trunk_row_blocks(const SdxpDev& D, int l) { return 3 * ((D.units[l] + 3) / 4); }
