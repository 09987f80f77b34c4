// sdx_mfma.h — what every kernel built on the 32 x 32 v_mfma blocks shares (k_gemm of sdx_gemm.h, k_gemm_nt / k_gemm_tt of sdx_gemm_nt.h,
// k_linear_mfma / k_linear_glds of sdxp_rollout.hip): the accumulator type, its zeroing and the C/D register layout.  gfx950 only.
// (Not in sdx_common.h: the emulator builds of the simulator compile that header with g++, which has no ext_vector_type.)
#pragma once
#include <hip/hip_runtime.h>

typedef float f32x16 __attribute__((ext_vector_type(16)));   // the accumulator of one 32 x 32 block: 16 registers per lane

// C/D layout of v_mfma_f32_32x32x*: lane l holds column (l & 31) of the block, and its register r = 0..15 belongs to this row of the
// matrix, row0 being the block's first
__device__ __forceinline__ int mfma_cd_row(int row0, int r, int lane) { return row0 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5); }

// an accumulator, or an array of them of any rank, set to zero.  (k_linear_mfma / k_linear_glds keep loops of their own: through this
// function the compiler schedules their prologues differently, and the rollout kernels are held to the instructions they had.)
__device__ __forceinline__ void mfma_zero(f32x16& acc) {
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = 0.0f;
}
template <class T, int N>
__device__ __forceinline__ void mfma_zero(T (&acc)[N]) {
#pragma unroll
  for (int u = 0; u < N; ++u) mfma_zero(acc[u]);
}
