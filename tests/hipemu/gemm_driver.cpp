// TEST INFRASTRUCTURE ONLY: seqdex_amd/csrc/sdx_gemm_nt.h (the product's kernel source) on the SIMT emulator, so that the swizzle, the
// fragment / accumulator layouts, the epilogues and the staging kernel are checked against numpy in the CPU suite.  The products go
// through the header's own launchers, which pick the grid and the dynamic LDS of a tile.
#include <hipemu_mfma.h>

#include "sdx_common.h"
#include "sdx_gemm_nt.h"

// `count` (1..3) products of one launch: operands in the element type (fp32, or bf16 bit patterns as uint16), K a multiple of the chunk;
// tile: 0 = the launcher's choice, 1 = 128 x 64, 2 = 128 x 128
extern "C" int emu_gemm_nt(int bf, int epi, const NtArgs* gs, int count, int splits, int tile) {
  if (bf) {
    if (epi == EPI_FWD) gemm_nt<1, EPI_FWD>(gs, count, splits, nullptr, tile);
    else if (epi == EPI_NN) gemm_nt<1, EPI_NN>(gs, count, splits, nullptr, tile);
    else gemm_nt<1, EPI_TN>(gs, count, splits, nullptr, tile);
  } else {
    if (epi == EPI_FWD) gemm_nt<0, EPI_FWD>(gs, count, splits, nullptr, tile);
    else if (epi == EPI_NN) gemm_nt<0, EPI_NN>(gs, count, splits, nullptr, tile);
    else gemm_nt<0, EPI_TN>(gs, count, splits, nullptr, tile);
  }
  return 0;
}
// fp32 weight gradients from [row][feature] operands (k_gemm_tt): G[n][k] = sum_r A[r][n] B[r][k] in `splits` row ranges of kchunk rows
extern "C" int emu_gemm_tt(const NtArgs* gs, int count, int splits, int tile) {
  static float zeros[64] = {0};
  gemm_tt(gs, count, splits, zeros, nullptr, tile);
  return 0;
}
extern "C" int emu_stage(int bf, const float* src, int lds, int R, int K, int Kp, void* dn, int ldn, void* dt, int ldt) {
  StageBatch sb;
  StageArgs a = {src, lds, R, K, Kp, dn, ldn, dt, ldt};
  for (int q = 0; q < 9; ++q) sb.a[q] = a;
  dim3 grid((Kp + 63) / 64, (R + 63) / 64, 1);
  if (bf) hipLaunchKernelGGL((k_stage<1>), grid, dim3(256), 0, nullptr, sb);
  else hipLaunchKernelGGL((k_stage<0>), grid, dim3(256), 0, nullptr, sb);
  return 0;
}
