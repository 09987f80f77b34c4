// sdxp_persist_checks.hip — test entries for the sum machinery of the persistent PPO update (sdxp_persist_sums.h): each runs the helper
// k_update_persistent uses beside the trees it stands for, in one workgroup, and hands both results back.  Built with the flags of
// sdxp_persist.hip (Makefile), so that the helpers are compiled here as they are inside the kernel.
#include "sdx_common.h"
#include "sdxp_launch.h"
#include "sdxp_persist_sums.h"

// Test entry (tests/test_gpu_wave_sums.py): one workgroup of NTH threads, in / ref / got are [N][NTH].  ref[i][t] = wave_sum of value i in t's
// wave, on every lane; got[i][t] = what wave_sums<N> left in lane t for value i - written by the lanes with (t & 3) == (i & 3), the others'
// slots are not touched.
template <int N>
__global__ __launch_bounds__(NTH) void k_wave_sums_check(const float* in, float* ref, float* got) {
  const int tid = threadIdx.x, lane = tid & 63;
  float v[N], u[(N + 3) / 4];
#pragma unroll
  for (int i = 0; i < N; ++i) v[i] = in[i * NTH + tid];
#pragma unroll
  for (int i = 0; i < N; ++i) ref[i * NTH + tid] = wave_sum(v[i]);
  wave_sums<N>(v, u, lane);
#pragma unroll
  for (int j = 0; j < (N + 3) / 4; ++j) got[(4 * j + (lane & 3)) * NTH + tid] = u[j];
}
extern "C" int sdxpk_wave_sums_check(const float* in, float* ref, float* got, int n, hipStream_t st) {
  if (n == 12) hipLaunchKernelGGL(k_wave_sums_check<12>, dim3(1), dim3(NTH), 0, st, in, ref, got);
  else if (n == 16) hipLaunchKernelGGL(k_wave_sums_check<16>, dim3(1), dim3(NTH), 0, st, in, ref, got);
  else return -1;
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
// Test entry (tests/test_gpu_fwd2_sums.py): one workgroup of NTH threads, w is [3][NTH], x [3][MB][NTH], ref / got [3 MB][NTH], value
// net MB + s.  ref[i][t] = the tree forward L2 used to run for value i in t's wave, written serially: the explicit fma first level, the
// five dpp_add levels of wave_sum, lane 63.  got[i][t] = what fwd2_sums left in lane t for value i - written by the 32 lanes of a wave that hold
// sample i % MB (fwd2_sample, the eight useful lanes of every DPP row), the others' slots are not touched.
__global__ __launch_bounds__(NTH) void k_fwd2_sums_check(const float* w, const float* x, float* ref, float* got) {
  const int tid = threadIdx.x, lane = tid & 63;
  float wv[3], xv[3][MB], u[3];
#pragma unroll
  for (int net = 0; net < 3; ++net) {
    wv[net] = w[net * NTH + tid];
#pragma unroll
    for (int s = 0; s < MB; ++s) xv[net][s] = x[(net * MB + s) * NTH + tid];
  }
#pragma unroll
  for (int net = 0; net < 3; ++net)
#pragma unroll
    for (int s = 0; s < MB; ++s) {
      float t = wv[net] * xv[net][s];
      asm volatile("" : "+v"(t));
      float v = __builtin_fmaf(wv[net], xv[net][s], dpp_mov<0xB1, 0xF>(0.0f, t));
      v = dpp_add<0x4E, 0xF>(v); v = dpp_add<0x141, 0xF>(v); v = dpp_add<0x140, 0xF>(v); v = dpp_add<0x142, 0xA>(v); v = dpp_add<0x143, 0xC>(v);
      ref[(net * MB + s) * NTH + tid] = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 63));
    }
  fwd2_sums(wv, xv, u, lane);
  if ((0xA5A5 >> (lane & 15)) & 1) {
    const int s = fwd2_sample(lane);
#pragma unroll
    for (int net = 0; net < 3; ++net) got[(net * MB + s) * NTH + tid] = u[net];
  }
}
extern "C" int sdxpk_fwd2_sums_check(const float* w, const float* x, float* ref, float* got, hipStream_t st) {
  hipLaunchKernelGGL(k_fwd2_sums_check, dim3(1), dim3(NTH), 0, st, w, x, ref, got);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
// Test entry (tests/test_gpu_persist_input_grams.py): the Grams of the layer-0 inputs in the form the epoch kernel gave them while it formed
// them itself, in the shadow of its x1 edge - the reference that the per-epoch table (k_input_grams, sdxp_persist.hip) is held to, bit for bit.
// One workgroup per minibatch; the rows go into the S.obs / S.cvx images (columns of S.obs past obs_dim zero), then gram_acc10 per thread, the
// 22-value block_sum (row_butterfly over the DPP rows, the 32 row sums added from 0.0f in ascending order) and the 16-entry expansion.
// obs [4 n_mb][obs_dim], cvx [4 n_mb][ST] -> out [n_mb][2][16]: the observations' Gram, the central value's.
__global__ __launch_bounds__(NTH) void k_input_grams_reference(const float* obs, int obs_dim, const float* cvx, float* out) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  PLds& S = *reinterpret_cast<PLds*>(smem_raw);
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const size_t mb = blockIdx.x;
  for (int i = tid; i < MB * OBS; i += NTH) { const int s = i / OBS, k = i % OBS; S.obs[s][k] = k < obs_dim ? obs[(mb * MB + s) * obs_dim + k] : 0.0f; }
  for (int i = tid; i < MB * ST; i += NTH) (&S.cvx[0][0])[i] = cvx[mb * MB * ST + i];
  __syncthreads();
  float p[22];
#pragma unroll
  for (int i = 0; i < 22; ++i) p[i] = 0.0f;
  if (tid < OBS) gram_acc10(&p[0], S.obs[0][tid], S.obs[1][tid], S.obs[2][tid], S.obs[3][tid]);
  gram_acc10(&p[11], S.cvx[0][tid], S.cvx[1][tid], S.cvx[2][tid], S.cvx[3][tid]);
  if (tid + NTH < ST) gram_acc10(&p[11], S.cvx[0][tid + NTH], S.cvx[1][tid + NTH], S.cvx[2][tid + NTH], S.cvx[3][tid + NTH]);
  block_sum<22>(S, p, S.part, tid, wave, lane);
  if (tid < 16) out[mb * 32 + tid] = S.part[tri16(tid)];
  else if (tid >= 64 && tid < 80) out[mb * 32 + 16 + tid - 64] = S.part[11 + tri16(tid - 64)];
}
extern "C" int sdxpk_input_grams_reference(const float* obs, int obs_dim, const float* cvx, int n_mb, float* out, hipStream_t st) {
  if (obs_dim < 1 || obs_dim > OBS || n_mb < 1) return -1;
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(k_input_grams_reference), hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(PLds)) != hipSuccess) return -1;
  hipLaunchKernelGGL(k_input_grams_reference, dim3(n_mb), dim3(NTH), sizeof(PLds), st, obs, obs_dim, cvx, out);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
