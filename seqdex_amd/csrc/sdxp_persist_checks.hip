// sdxp_persist_checks.hip — test entries for the machinery of the persistent PPO update (sdxp_persist_sums.h, sdxp_persist_adam.h, sdxp_persist_tails.h, sdxp_persist_phase_d.h,
// the head_* helpers of sdxp_persist_exchange.h): each runs the
// helper k_update_persistent uses beside the form it stands for, in one workgroup, and hands both results back.  Built with the flags of
// sdxp_persist.hip (Makefile), so that the helpers are compiled here as they are inside the kernel.
#include "sdx_common.h"
#include "sdxp_launch.h"
#include "sdxp_persist_exchange.h"
#include "sdxp_persist_sums.h"
#include "sdxp_persist_adam.h"
#include "sdxp_persist_tails.h"
#include "sdxp_persist_phase_d.h"

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
// Test entry (tests/test_gpu_persist_adam_ahead.py): Adam of layer 1 in the x1 shadow, one workgroup of NTH threads standing for CU g.  x1 [3][MB][U0]
// goes into the S.x1 image, dy1 [3][MB][U1] into S.dy1 (the column factors, one per lane), dyr [3][MB][2] into S.dyown[.][.][DY_L1 + row] (the
// row factors of the workgroup's two rows), scal [6] into S.scal (SC_*).  state [3][24][NTH]: (w, m, v) of the lane's elements, element
// net 8 + j: j < 4 the row element of column (wave & 3) 256 + lane + 64 j, j >= 4 the column element of column 4 g + j - 4.
// out [2][4][24][NTH]: (gg, m, v, w) of [0] the serial loops the epoch kernel ran before adam_l1_ahead - every operand read behind the
// arithmetic of the element in front, adam1 - kept here as the reference, and of [1] adam_l1_ahead on the same inputs.
__global__ __launch_bounds__(NTH) void k_adam_ahead_check(const float* x1, const float* dy1, const float* dyr, const float* scal, int g, const float* state, float* out) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  PLds& S = *reinterpret_cast<PLds*>(smem_raw);
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r1w = wave >> 2, q1 = wave & 3;
  for (int i = tid; i < 3 * MB * U0; i += NTH) (&S.x1[0][0][0])[i] = x1[i];
  for (int i = tid; i < 3 * MB * U1; i += NTH) (&S.dy1[0][0][0])[i] = dy1[i];
  if (tid < 3 * MB * 2) S.dyown[tid / (2 * MB)][(tid / 2) % MB][DY_L1 + tid % 2] = dyr[tid];
  if (tid < 6) S.scal[tid] = scal[tid];
  __syncthreads();
  const StepScal sc = step_scal(S);
  float w1[3][4], m1[3][4], v1[3][4], c1[3][4], cm1[3][4], cv1[3][4];
  auto load = [&]() {
#pragma unroll
    for (int net = 0; net < 3; ++net)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int r = (net * 8 + j) * NTH + tid, c = (net * 8 + 4 + j) * NTH + tid;
        w1[net][j] = state[r]; m1[net][j] = state[24 * NTH + r]; v1[net][j] = state[48 * NTH + r];
        c1[net][j] = state[c]; cm1[net][j] = state[24 * NTH + c]; cv1[net][j] = state[48 * NTH + c];
      }
  };
  auto store = [&](float* o) {   // o: [4][24][NTH], the gradient elements are already there
#pragma unroll
    for (int net = 0; net < 3; ++net)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int r = (net * 8 + j) * NTH + tid, c = (net * 8 + 4 + j) * NTH + tid;
        o[24 * NTH + r] = m1[net][j]; o[48 * NTH + r] = v1[net][j]; o[72 * NTH + r] = w1[net][j];
        o[24 * NTH + c] = cm1[net][j]; o[48 * NTH + c] = cv1[net][j]; o[72 * NTH + c] = c1[net][j];
      }
  };
  load();
  {
    float dep = 0.0f;
#pragma unroll
    for (int net = 0; net < 3; ++net) {
      const float gs = sc.gs(net), lrb = sc.lrb(net), isq = sc.isq(net);
      float d1r[MB], dn1[MB];
      const int o_r = opaque(r1w, dep), o_t = opaque(tid, dep);
#pragma unroll
      for (int s = 0; s < MB; ++s) { d1r[s] = S.dyown[net][s][DY_L1 + o_r] * gs; dn1[s] = S.dy1[net][s][o_t] * gs; }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int k = opaque(q1 * 256 + lane + 64 * i, dep);
        float gg = 0.0f;
#pragma unroll
        for (int s = 0; s < MB; ++s) gg += d1r[s] * S.x1[net][s][k];
        out[(net * 8 + i) * NTH + tid] = gg;
        adam1(w1[net][i], gg, m1[net][i], v1[net][i], lrb, isq); dep = w1[net][i];
      }
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int k = opaque(4 * g + c, dep);
        float gg = 0.0f;
#pragma unroll
        for (int s = 0; s < MB; ++s) gg += dn1[s] * S.x1[net][s][k];
        out[(net * 8 + 4 + c) * NTH + tid] = gg;
        adam1(c1[net][c], gg, cm1[net][c], cv1[net][c], lrb, isq); dep = c1[net][c];
      }
    }
  }
  store(out);
  load();
  float* got = out + 4 * 24 * NTH;
  adam_l1_ahead(S, sc, q1 * 256 + lane, 4 * g, r1w, tid, w1, m1, v1, c1, cm1, cv1, [&](int net, int j, float gg) { got[(net * 8 + j) * NTH + tid] = gg; });
  store(got);
}
extern "C" int sdxpk_adam_ahead_check(const float* x1, const float* dy1, const float* dyr, const float* scal, int g, const float* state, float* out, hipStream_t st) {
  if (g < 0 || g >= NWG) return -1;
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(k_adam_ahead_check), hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(PLds)) != hipSuccess) return -1;
  hipLaunchKernelGGL(k_adam_ahead_check, dim3(1), dim3(NTH), sizeof(PLds), st, x1, dy1, dyr, scal, g, state, out);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
// Test entry (tests/test_gpu_persist_packed_adam.py): adam_l1_ahead takes the lane's 24 layer-1 elements two at a time as packed f32 (adam2x, grad4x2).
// The reference is the one-element form it replaced - adam1x, grad4 and the loop over 24 elements, kept here verbatim but for the loop's name.
// Inputs and layout as sdxpk_adam_ahead_check; out [2][4][24][NTH]: (gg, m, v, w) of [0] the one-element form, [1] adam_l1_ahead.
namespace {
__device__ __forceinline__ float rounded(float x) { asm volatile("" : "+v"(x)); return x; }
__device__ __forceinline__ void adam1x(float& w, float g, float& m, float& v, float lr_bc1, float isq_bc2) {
  const float m9 = rounded(0.9f * m), v999 = rounded(0.999f * v), t = rounded(0.001f * g);
  m = __builtin_fmaf(0.1f, g, m9);
  v = __builtin_fmaf(g, t, v999);
  const float lm = rounded(lr_bc1 * m);
  w = __builtin_fmaf(-lm, __builtin_amdgcn_rcpf(__builtin_fmaf(isq_bc2, __builtin_amdgcn_sqrtf(v), 1e-8f)), w);
  __builtin_amdgcn_sched_barrier(0);
}
// the gradient element sum_s d_s x_s, from 0 in ascending order of s, one fma per sample
__device__ __forceinline__ float grad4(const float (&d)[MB], const float (&x)[MB]) {
  static_assert(MB == 4, "four samples");
  return __builtin_fmaf(d[3], x[3], __builtin_fmaf(d[2], x[2], __builtin_fmaf(d[1], x[1], __builtin_fmaf(d[0], x[0], 0.0f))));
}
// (the parent form of adam_l1_ahead) Adam of layer 1 as ONE loop over the lane's 24 elements: per network the row elements 0..3 (columns kr + 64 i of S.x1, factors
// S.dyown[net][.][DY_L1 + o_row]), then the column elements 0..3 (columns kc + c, factors S.dy1[net][.][o_thr]) - the serial loops' order.
// The four operands of element e are pinned together (one wait), then the four S.x1 operands of element e + 1 are requested - through an
// index made opaque against the weight element e - 1 wrote, so the request can rise no further, and with a sched_barrier behind it, so it
// cannot sink into the arithmetic of element e - and fly under that arithmetic.  The pin stands IN FRONT of the request on purpose: every wait
// hipcc places in this region is lgkmcnt(0), never a partial count, so a wait behind the request would drain the reads just issued; in front of
// it, it finds reads that were requested a whole element ago.  The factors are requested a network ahead, into the registers their
// predecessors left: the row factors under column element 1 of the network in front, the column factors under row element 1; each is scaled
// by the clip factor where it is first used.
// sink(net, j, gg): the gradient element, for the test entry; the kernel passes an empty one.
template <class Sink>
__device__ __forceinline__ void adam_l1_ahead_scalar(const PLds& S, const StepScal& sc, int kr, int kc, int o_row, int o_thr, float (&w1)[3][4],
                                              float (&m1)[3][4], float (&v1)[3][4], float (&c1)[3][4], float (&cm1)[3][4], float (&cv1)[3][4],
                                              Sink&& sink) {
  float dr[MB], dn[MB], x[2][MB], dep = 0.0f;   // x[e & 1]: the operands of element e
  {
    const int o_r = opaque(o_row, dep), o_t = opaque(o_thr, dep), k = opaque(kr, dep);
#pragma unroll
    for (int s = 0; s < MB; ++s) { dr[s] = S.dyown[0][s][DY_L1 + o_r]; dn[s] = S.dy1[0][s][o_t]; x[0][s] = S.x1[0][s][k]; }
  }
#pragma unroll
  for (int e = 0; e < 24; ++e) {
    const int net = e / 8, j = e % 8;
    float (&xc)[MB] = x[e & 1], (&xn)[MB] = x[(e + 1) & 1];
    SDX_PIN4X(xc[0], xc[1], xc[2], xc[3]);
    if (e + 1 < 24) {
      const int n1 = (e + 1) / 8, j1 = (e + 1) % 8;
      const int k = opaque(j1 < 4 ? kr + 64 * j1 : kc + (j1 - 4), dep);
#pragma unroll
      for (int s = 0; s < MB; ++s) xn[s] = S.x1[n1][s][k];
    }
    if (j == 5 && net < 2) {
      const int o_r = opaque(o_row, dep);
#pragma unroll
      for (int s = 0; s < MB; ++s) dr[s] = S.dyown[net + 1][s][DY_L1 + o_r];
    }
    if (j == 1 && net > 0) {
      const int o_t = opaque(o_thr, dep);
#pragma unroll
      for (int s = 0; s < MB; ++s) dn[s] = S.dy1[net][s][o_t];
    }
    __builtin_amdgcn_sched_barrier(0);
    if (j == 0) {
#pragma unroll
      for (int s = 0; s < MB; ++s) dr[s] *= sc.gs(net);
    }
    if (j == 4) {
#pragma unroll
      for (int s = 0; s < MB; ++s) dn[s] *= sc.gs(net);
    }
    const float gg = grad4(j < 4 ? dr : dn, xc);
    sink(net, j, gg);
    float& w = j < 4 ? w1[net][j] : c1[net][j - 4];
    adam1x(w, gg, j < 4 ? m1[net][j] : cm1[net][j - 4], j < 4 ? v1[net][j] : cv1[net][j - 4], sc.lrb(net), sc.isq(net));
    dep = w;
  }
}
}  // namespace
__global__ __launch_bounds__(NTH) void k_packed_adam_check(const float* x1, const float* dy1, const float* dyr, const float* scal, int g, const float* state, float* out) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  PLds& S = *reinterpret_cast<PLds*>(smem_raw);
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r1w = wave >> 2, q1 = wave & 3;
  for (int i = tid; i < 3 * MB * U0; i += NTH) (&S.x1[0][0][0])[i] = x1[i];
  for (int i = tid; i < 3 * MB * U1; i += NTH) (&S.dy1[0][0][0])[i] = dy1[i];
  if (tid < 3 * MB * 2) S.dyown[tid / (2 * MB)][(tid / 2) % MB][DY_L1 + tid % 2] = dyr[tid];
  if (tid < 6) S.scal[tid] = scal[tid];
  __syncthreads();
  const StepScal sc = step_scal(S);
  float w1[3][4], m1[3][4], v1[3][4], c1[3][4], cm1[3][4], cv1[3][4];
  auto load = [&]() {
#pragma unroll
    for (int net = 0; net < 3; ++net)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int r = (net * 8 + j) * NTH + tid, c = (net * 8 + 4 + j) * NTH + tid;
        w1[net][j] = state[r]; m1[net][j] = state[24 * NTH + r]; v1[net][j] = state[48 * NTH + r];
        c1[net][j] = state[c]; cm1[net][j] = state[24 * NTH + c]; cv1[net][j] = state[48 * NTH + c];
      }
  };
  auto store = [&](float* o) {   // o: [4][24][NTH], the gradient elements are already there
#pragma unroll
    for (int net = 0; net < 3; ++net)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int r = (net * 8 + j) * NTH + tid, c = (net * 8 + 4 + j) * NTH + tid;
        o[24 * NTH + r] = m1[net][j]; o[48 * NTH + r] = v1[net][j]; o[72 * NTH + r] = w1[net][j];
        o[24 * NTH + c] = cm1[net][j]; o[48 * NTH + c] = cv1[net][j]; o[72 * NTH + c] = c1[net][j];
      }
  };
  load();
  adam_l1_ahead_scalar(S, sc, q1 * 256 + lane, 4 * g, r1w, tid, w1, m1, v1, c1, cm1, cv1, [&](int net, int j, float gg) { out[(net * 8 + j) * NTH + tid] = gg; });
  store(out);
  load();
  float* got = out + 4 * 24 * NTH;
  adam_l1_ahead(S, sc, q1 * 256 + lane, 4 * g, r1w, tid, w1, m1, v1, c1, cm1, cv1, [&](int net, int j, float gg) { got[(net * 8 + j) * NTH + tid] = gg; });
  store(got);
}
extern "C" int sdxpk_packed_adam_check(const float* x1, const float* dy1, const float* dyr, const float* scal, int g, const float* state, float* out, hipStream_t st) {
  if (g < 0 || g >= NWG) return -1;
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(k_packed_adam_check), hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(PLds)) != hipSuccess) return -1;
  hipLaunchKernelGGL(k_packed_adam_check, dim3(1), dim3(NTH), sizeof(PLds), st, x1, dy1, dyr, scal, g, state, out);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
// Test entry (tests/test_gpu_persist_gram_x.py): the Grams of x2 and x1 as the epoch kernel forms them in the shadow of its x3 edge, one
// workgroup of NTH threads.  x1 [3][MB][U0] and x2 [3][MB][U1] go into the S.x1 / S.x2 images; the block below is the kernel's, verbatim - two
// butterflies, ONE reduction of 64 columns, the first column's products of x1 kept rounded by an opaque copy - but for the stores of terms.
// terms [2][30][NTH] (Gram: 0 = x2, 1 = x1): what every thread holds in front of its butterfly, value net 10 + e; entries [2][48]: the finished
// 16-entry matrices of the three networks (S.gx[net][2], S.gx[net][1]).
__global__ __launch_bounds__(NTH) void k_gram_x_check(const float* x1, const float* x2, float* terms, float* entries) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  PLds& S = *reinterpret_cast<PLds*>(smem_raw);
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  for (int i = tid; i < 3 * MB * U0; i += NTH) (&S.x1[0][0][0])[i] = x1[i];
  for (int i = tid; i < 3 * MB * U1; i += NTH) (&S.x2[0][0][0])[i] = x2[i];
  __syncthreads();
  {
    float ua[8], ub[8];
    {
      float p[30];
#pragma unroll
      for (int i = 0; i < 30; ++i) p[i] = 0.0f;
#pragma unroll
      for (int net = 0; net < 3; ++net) gram_acc10(&p[net * 10], S.x2[net][0][tid], S.x2[net][1][tid], S.x2[net][2][tid], S.x2[net][3][tid]);
#pragma unroll
      for (int i = 0; i < 30; ++i) terms[i * NTH + tid] = p[i];
      row_butterfly<30>(p, ua, lane);
    }
    rows_store<8>(S, ua, 0, wave, lane);
    {
      float p[30];
#pragma unroll
      for (int i = 0; i < 30; ++i) p[i] = 0.0f;
#pragma unroll
      for (int h = 0; h < U0 / NTH; ++h) {
#pragma unroll
        for (int net = 0; net < 3; ++net) { const int k = tid + NTH * h; gram_acc10(&p[net * 10], S.x1[net][0][k], S.x1[net][1][k], S.x1[net][2][k], S.x1[net][3][k]); }
        if (h == 0) {
#pragma unroll
          for (int i = 0; i < 30; ++i) asm("" : "+v"(p[i]));
        }
      }
#pragma unroll
      for (int i = 0; i < 30; ++i) terms[(30 + i) * NTH + tid] = p[i];
      row_butterfly<30>(p, ub, lane);
    }
    rows_store<8>(S, ub, 32, wave, lane);
    rows_reduce(S, 64, S.part, tid);
    if (tid < 48) S.gx[tid >> 4][2][tid & 15] = S.part[(tid >> 4) * 10 + tri16(tid & 15)];
    else if (tid >= 64 && tid < 64 + 48) { const int t = tid - 64; S.gx[t >> 4][1][t & 15] = S.part[32 + (t >> 4) * 10 + tri16(t & 15)]; }
  }
  __syncthreads();
  if (tid < 48) { entries[tid] = S.gx[tid >> 4][2][tid & 15]; entries[48 + tid] = S.gx[tid >> 4][1][tid & 15]; }
}
extern "C" int sdxpk_gram_x_check(const float* x1, const float* x2, float* terms, float* entries, hipStream_t st) {
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(k_gram_x_check), hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(PLds)) != hipSuccess) return -1;
  hipLaunchKernelGGL(k_gram_x_check, dim3(1), dim3(NTH), sizeof(PLds), st, x1, x2, terms, entries);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
// Test entry (tests/test_gpu_row_butterfly.py): one workgroup of NTH threads, in / ref / got are [N][NTH].  ref[i][t] = the sum of value i over
// t's 16-lane DPP row as ONE plain tree per value - partners lane ^ 1, ^ 2, ^ 4, ^ 8, fetched with __shfl_xor (ds_bpermute: no DPP) - on
// every lane; got[i][t] = what row_butterfly<N> left in lane t for value i - written by the lanes with (t & 3) == (i & 3), the others' slots
// are not touched.
template <int N>
__global__ __launch_bounds__(NTH) void k_row_butterfly_check(const float* in, float* ref, float* got) {
  const int tid = threadIdx.x, lane = tid & 63;
  float v[N], u[(N + 3) / 4];
#pragma unroll
  for (int i = 0; i < N; ++i) v[i] = in[i * NTH + tid];
#pragma unroll
  for (int i = 0; i < N; ++i) {
    float s = v[i];
#pragma unroll
    for (int m = 1; m < 16; m <<= 1) { float o = __shfl_xor(s, m, 64); asm volatile("" : "+v"(o)); s = s + o; }
    ref[i * NTH + tid] = s;
  }
  row_butterfly<N>(v, u, lane);
#pragma unroll
  for (int j = 0; j < (N + 3) / 4; ++j)
    if (4 * j + (lane & 3) < N) got[(4 * j + (lane & 3)) * NTH + tid] = u[j];
}
extern "C" int sdxpk_row_butterfly_check(const float* in, float* ref, float* got, int n, hipStream_t st) {
  if (n == 12) hipLaunchKernelGGL(k_row_butterfly_check<12>, dim3(1), dim3(NTH), 0, st, in, ref, got);
  else if (n == 30) hipLaunchKernelGGL(k_row_butterfly_check<30>, dim3(1), dim3(NTH), 0, st, in, ref, got);
  else if (n == 48) hipLaunchKernelGGL(k_row_butterfly_check<48>, dim3(1), dim3(NTH), 0, st, in, ref, got);
  else return -1;
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
// Test entry (tests/test_gpu_persist_ordered_sum.py): one workgroup of NTH threads, rows [4 NWV][64] go into S.red.  ref[n][c] (n = 0: 16 rows,
// 1: 32 rows; c < 64): the plain serial loop, every row read through a volatile pointer so that each add waits for its own read - the form the
// reductions of k_update_persistent had; got[n][c]: ordered_sum_ahead on the same rows.
__global__ __launch_bounds__(NTH) void k_ordered_sum_check(const float* rows, float* ref, float* got) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  PLds& S = *reinterpret_cast<PLds*>(smem_raw);
  const int tid = threadIdx.x;
  for (int i = tid; i < 4 * NWV * 64; i += NTH) (&S.red[0][0])[i] = rows[i];
  __syncthreads();
  if (tid < 64) {
    const volatile float* col = &S.red[0][tid];
    float t = 0.0f;
    for (int w = 0; w < 2 * NWV; ++w) t += col[w * 64];
    ref[tid] = t;
    for (int w = 2 * NWV; w < 4 * NWV; ++w) t += col[w * 64];
    ref[64 + tid] = t;
    got[tid] = ordered_sum_ahead<2 * NWV, 64>(&S.red[0][tid]);
    got[64 + tid] = ordered_sum_ahead<4 * NWV, 64>(&S.red[0][tid]);
  }
}
extern "C" int sdxpk_ordered_sum_check(const float* rows, float* ref, float* got, hipStream_t st) {
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(k_ordered_sum_check), hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(PLds)) != hipSuccess) return -1;
  hipLaunchKernelGGL(k_ordered_sum_check, dim3(1), dim3(NTH), sizeof(PLds), st, rows, ref, got);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
// Test entry (tests/test_gpu_persist_forward_tails.py): the publish tails of forward L0 / L1 / L2, one workgroup of NTH threads per case.  fpart
// [n][3 MB NWV] goes into S.fpart, bias [n][64] into S.bias.  ref [n][16][3]: the three networks' outputs the storing lanes (tid < 16 / 8 / 4) would
// publish, in the form the epoch kernel had before fwd_tail - one lane per (sample, row) forms the three networks one after the other - kept here
// verbatim as the reference; got [n][16][3]: fwd_tail on the same LDS image (slots of lanes that do not store are not touched); pre [n][48]: the
// pre-activation of lane (net, sample, row) < 48 / 24 / 12 (fwd_tail_pre).
template <int L>
__global__ __launch_bounds__(NTH) void k_forward_tail_check(const float* fpart, const float* bias, float* ref, float* got, float* pre) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  PLds& S = *reinterpret_cast<PLds*>(smem_raw);
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const size_t c = blockIdx.x;
  if (tid < 3 * MB * NWV) S.fpart[tid] = fpart[c * 3 * MB * NWV + tid];
  if (tid < 64) S.bias[tid] = bias[c * 64 + tid];
  __syncthreads();
  float* rc = ref + c * 48;
  if constexpr (L == 0) {
    if (tid < MB * 4) {   // (sample s, owned row r): the three networks' outputs in one packed word
      const int s = tid / 4, r = tid % 4;
      float y[3];
#pragma unroll
      for (int net = 0; net < 3; ++net)
        y[net] = elu(S.fpart[(net * MB + s) * NWV + 2 * r] + S.fpart[(net * MB + s) * NWV + 2 * r + 1] + S.bias[BIAS_L0 + net * 4 + r]);
      rc[tid * 3] = y[0]; rc[tid * 3 + 1] = y[1]; rc[tid * 3 + 2] = y[2];
    }
  } else if constexpr (L == 1) {
    if (tid < MB * 2) {
      const int s = tid / 2, r = tid % 2;
      float y[3];
#pragma unroll
      for (int net = 0; net < 3; ++net) {
        const float* q = &S.fpart[(net * MB + s) * NWV + 4 * r];
        y[net] = elu(q[0] + q[1] + q[2] + q[3] + S.bias[BIAS_L1 + net * 2 + r]);
      }
      rc[tid * 3] = y[0]; rc[tid * 3 + 1] = y[1]; rc[tid * 3 + 2] = y[2];
    }
  } else {
    if (tid < MB) {
      const int s = tid;
      float y[3];
#pragma unroll
      for (int net = 0; net < 3; ++net) {
        const float* q = &S.fpart[(net * MB + s) * NWV];
        float t = S.bias[BIAS_L2 + net];
#pragma unroll
        for (int w = 0; w < NWV; ++w) t += q[w];
        y[net] = elu(t);
      }
      rc[tid * 3] = y[0]; rc[tid * 3 + 1] = y[1]; rc[tid * 3 + 2] = y[2];
    }
  }
  if (wave == 0) {
    float y[3];
    fwd_tail<L>(S, lane, y);
    if (tid < FwdTail<L>::STORING) { got[c * 48 + tid * 3] = y[0]; got[c * 48 + tid * 3 + 1] = y[1]; got[c * 48 + tid * 3 + 2] = y[2]; }
    if (lane < FwdTail<L>::LANES) pre[c * 48 + lane] = fwd_tail_pre<L>(S, lane);
  }
}
extern "C" int sdxpk_forward_tail_check(int layer, const float* fpart, const float* bias, int n, float* ref, float* got, float* pre, hipStream_t st) {
  if (n < 1 || layer < 0 || layer > 2) return -1;
  const void* k = layer == 0 ? reinterpret_cast<const void*>(k_forward_tail_check<0>) : layer == 1 ? reinterpret_cast<const void*>(k_forward_tail_check<1>) : reinterpret_cast<const void*>(k_forward_tail_check<2>);
  if (hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(PLds)) != hipSuccess) return -1;
  if (layer == 0) hipLaunchKernelGGL(k_forward_tail_check<0>, dim3(n), dim3(NTH), sizeof(PLds), st, fpart, bias, ref, got, pre);
  else if (layer == 1) hipLaunchKernelGGL(k_forward_tail_check<1>, dim3(n), dim3(NTH), sizeof(PLds), st, fpart, bias, ref, got, pre);
  else hipLaunchKernelGGL(k_forward_tail_check<2>, dim3(n), dim3(NTH), sizeof(PLds), st, fpart, bias, ref, got, pre);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
// Test entry (tests/test_gpu_persist_head_forward.py): the head forward of phase D, one workgroup of NTH threads per case.  x3 [n][3][MB][U2] goes
// into S.x3, hb [n][ACT + 2] into S.bias[BIAS_HEAD ..], hw [n][ACT + 2][U2] into the registers wh[j][e] = row wave + 8 j, column lane + 64 e (zero
// past the last row, as the kernel's gather leaves them).  out [n][2][MB ACT + 2 MB]: mu [MB][ACT] then val [2][MB] of [0] the form the epoch kernel
// had before head_forward - the value rows' operands read inside their fma chains, the biases behind the wave sums - kept here verbatim as the
// reference, and of [1] head_forward on the same inputs.
__global__ __launch_bounds__(NTH) void k_head_forward_check(const float* x3, const float* hw, const float* hb, float* out) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  PLds& S = *reinterpret_cast<PLds*>(smem_raw);
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const size_t c = blockIdx.x;
  constexpr int A = ACT, NO = MB * ACT + 2 * MB;
  for (int i = tid; i < 3 * MB * U2; i += NTH) (&S.x3[0][0][0])[i] = x3[c * 3 * MB * U2 + i];
  if (tid < A + 2) S.bias[BIAS_HEAD + tid] = hb[c * (A + 2) + tid];
  float wh[HR][4];
#pragma unroll
  for (int j = 0; j < HR; ++j)
#pragma unroll
    for (int e = 0; e < 4; ++e) { const int row = wave + 8 * j; wh[j][e] = row < A + 2 ? hw[(c * (A + 2) + row) * U2 + lane + 64 * e] : 0.0f; }
  auto clear = [&]() {
    if (tid < MB * 32) S.mu[tid / 32][tid % 32] = __builtin_nanf("");
    if (tid < 2 * MB) S.val[tid / MB][tid % MB] = __builtin_nanf("");
    __syncthreads();
  };
  auto copy_out = [&](float* o) {
    __syncthreads();
    if (tid < MB * A) o[tid] = S.mu[tid / A][tid % A];
    else if (tid >= 128 && tid < 128 + 2 * MB) o[MB * A + tid - 128] = S.val[(tid - 128) / MB][(tid - 128) % MB];
    __syncthreads();
  };
  clear();
  {
    // rows wave, wave + 8, wave + 16 (< 23: actor rows, except row 23 = the critic's value on wave 7) and wave + 24 (only wave 0: row 24,
    // the central value): the actor rows of a wave share ONE set of x3 loads
    float q[HR * MB], u[HR], xa[MB][4];   // value MB j + s: lane s < 4 ends with sample s of the wave's rows
#pragma unroll
    for (int s = 0; s < MB; ++s)
#pragma unroll
      for (int e = 0; e < 4; ++e) xa[s][e] = S.x3[0][s][lane + 64 * e];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int s = 0; s < MB; ++s) {
        float t = 0.0f;
#pragma unroll
        for (int e = 0; e < 4; ++e) t += wh[j][e] * xa[s][e];
        q[MB * j + s] = t;
      }
    if (wave == NWV - 1) {          // row 23: critic value (net 1)
#pragma unroll
      for (int s = 0; s < MB; ++s) {
        float t = 0.0f;
#pragma unroll
        for (int e = 0; e < 4; ++e) t += wh[2][e] * S.x3[1][s][lane + 64 * e];
        q[MB * 2 + s] = t;
      }
    } else {
#pragma unroll
      for (int s = 0; s < MB; ++s) {
        float t = 0.0f;
#pragma unroll
        for (int e = 0; e < 4; ++e) t += wh[2][e] * xa[s][e];
        q[MB * 2 + s] = t;
      }
    }
    if (wave == 0) {                // row 24: central value (net 2), the fourth quad of a 16-wide butterfly on this wave only
#pragma unroll
      for (int s = 0; s < MB; ++s) {
        float t = 0.0f;
#pragma unroll
        for (int e = 0; e < 4; ++e) t += wh[3][e] * S.x3[2][s][lane + 64 * e];
        q[MB * 3 + s] = t;
      }
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
        if (row < A + 2) { const float y = u[j] + S.bias[BIAS_HEAD + row]; if (row < A) S.mu[lane][row] = y; else S.val[row - A][lane] = y; }
      }
    }
  }
  copy_out(out + c * 2 * NO);
  clear();
  head_forward(S, wh, wave, lane);
  copy_out(out + c * 2 * NO + NO);
}
extern "C" int sdxpk_head_forward_check(const float* x3, const float* hw, const float* hb, int n, float* out, hipStream_t st) {
  if (n < 1) return -1;
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(k_head_forward_check), hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(PLds)) != hipSuccess) return -1;
  hipLaunchKernelGGL(k_head_forward_check, dim3(n), dim3(NTH), sizeof(PLds), st, x3, hw, hb, out);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
// Test entry (tests/test_gpu_persist_stats_thread.py): the statistics / learning-rate thread of the dY1 shadow, one workgroup of NTH threads per
// case (thread T_STATS does the work, as in the kernel).  in [n][40]: S.stat [MB][8] (columns STAT_ACTOR .. STAT_ENTROPY are read), the six running
// sums (a, c, b, kl, cv, ent), ac_lr, kl_threshold; adaptive [n]: the adaptive_lr flag.  out [n][2][8]: the six sums, last_kl, ac_lr of [0] the
// serial loop the epoch kernel ran before stats_lr_once - every S.stat pair and every running sum read behind the arithmetic in front of it - kept
// here verbatim as the reference, and of [1] stats_lr_once on the same inputs.
__global__ __launch_bounds__(NTH) void k_stats_thread_check(const float* in, const int* adaptive, float* out) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  PLds& S = *reinterpret_cast<PLds*>(smem_raw);
  const int tid = threadIdx.x;
  const size_t c = blockIdx.x;
  const float* ic = in + c * 40;
  const int adaptive_lr = adaptive[c];
  const float kl_threshold = ic[39];
  const float invM = 1.0f / (float)MB;
  auto fill = [&]() {
    if (tid < MB * 8) S.stat[tid / 8][tid % 8] = ic[tid];
    if (tid == 0) {
      PLds::Ctl& C = S.ctl;
      C.sum_a = ic[32]; C.sum_c = ic[33]; C.sum_b = ic[34]; C.sum_kl = ic[35]; C.sum_cv = ic[36]; C.sum_ent = ic[37]; C.ac_lr = ic[38]; C.last_kl = __builtin_nanf("");
    }
    __syncthreads();
  };
  auto copy_out = [&](float* o) {
    __syncthreads();
    if (tid == 0) {
      const PLds::Ctl& C = S.ctl;
      o[0] = C.sum_a; o[1] = C.sum_c; o[2] = C.sum_b; o[3] = C.sum_kl; o[4] = C.sum_cv; o[5] = C.sum_ent; o[6] = C.last_kl; o[7] = C.ac_lr;
    }
    __syncthreads();
  };
  fill();
  if (tid == T_STATS) {
    PLds::Ctl& C = S.ctl;
    float t1 = 0, t2 = 0, t3 = 0, t4 = 0, t5 = 0, t6 = 0;
    for (int s = 0; s < MB; ++s) { t1 += S.stat[s][STAT_ACTOR]; t2 += S.stat[s][STAT_CRITIC]; t3 += S.stat[s][STAT_BOUNDS]; t4 += S.stat[s][STAT_KL]; t5 += S.stat[s][STAT_CV]; t6 += S.stat[s][STAT_ENTROPY]; }
    const float kl = t4 * invM;
    C.sum_a += t1 * invM; C.sum_c += t2 * invM; C.sum_b += t3 * invM; C.sum_kl += kl; C.sum_cv += t5 * invM; C.sum_ent += t6 * invM;
    C.last_kl = kl;
    if (adaptive_lr) {         // legacy schedule: after every minibatch (PS:306-312)
      float klt = kl_threshold;
      SDX_OPAQUE(klt);
      if (kl > 2.0f * klt) C.ac_lr = fmaxf(C.ac_lr / 1.5f, 1e-6f);
      if (kl < 0.5f * klt) C.ac_lr = fminf(C.ac_lr * 1.5f, 1e-2f);
    }
  }
  copy_out(out + c * 16);
  fill();
  if (tid == T_STATS) stats_lr_once(S, invM, adaptive_lr, kl_threshold);
  copy_out(out + c * 16 + 8);
}
extern "C" int sdxpk_stats_thread_check(const float* in, const int* adaptive, int n, float* out, hipStream_t st) {
  if (n < 1) return -1;
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(k_stats_thread_check), hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(PLds)) != hipSuccess) return -1;
  hipLaunchKernelGGL(k_stats_thread_check, dim3(n), dim3(NTH), sizeof(PLds), st, in, adaptive, out);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
// Test entry (tests/test_gpu_persist_head_backward.py): the backward through the heads of phase D, one workgroup of NTH threads per case.  dmu [n][MB][32]
// goes into S.dmu, dv [n][2][MB] into S.dv, x3 [n][3][MB][U2] into S.x3; hw [n][ACT + 2][U2] is the head matrix, of which lane (column c2n, row half c2c)
// holds wc[j] = row min(13 c2c + j, ACT + 1), as the kernel's column view leaves it.  out [n][2][3 MB][NTH]: d2[net][s] per thread of [0] the block the
// epoch kernel had before head_backward - the S.dv values read behind a lane condition, one branch with a read and a drained wait per value, the S.x3
// operands read sample by sample between the chains - kept here verbatim as the reference, and of [1] head_backward on the same inputs.
__global__ __launch_bounds__(NTH) void k_head_backward_check(const float* dmu, const float* dv, const float* x3, const float* hw, float* out) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  PLds& S = *reinterpret_cast<PLds*>(smem_raw);
  const int tid = threadIdx.x;
  const size_t c = blockIdx.x;
  constexpr int A = ACT;
  if (tid < MB * 32) S.dmu[tid / 32][tid % 32] = dmu[c * MB * 32 + tid];
  if (tid < 2 * MB) S.dv[tid / MB][tid % MB] = dv[c * 2 * MB + tid];
  for (int i = tid; i < 3 * MB * U2; i += NTH) (&S.x3[0][0][0])[i] = x3[c * 3 * MB * U2 + i];
  const int c2c = (tid >> 5) & 1, c2n = 32 * (tid >> 6) + (tid & 31);
  float wc[13];
#pragma unroll
  for (int j = 0; j < 13; ++j) wc[j] = hw[(c * (A + 2) + min(13 * c2c + j, A + 1)) * U2 + c2n];
  __syncthreads();
  float* o = out + c * 2 * 3 * MB * NTH;
  {
    float d2[3][MB];
    {
      const int k = c2n, jr = 13 * c2c;
      float a0[MB], a1[MB], a2[MB];
#pragma unroll
      for (int s = 0; s < MB; ++s) a0[s] = 0.0f;
#pragma unroll
      for (int j = 0; j < 13; ++j)
#pragma unroll
        for (int s = 0; s < MB; ++s) a0[s] += S.dmu[s][jr + j] * wc[j];
#pragma unroll
      for (int s = 0; s < MB; ++s) {
        a1[s] = c2c ? S.dv[0][s] * wc[A - 13] : 0.0f; a2[s] = c2c ? S.dv[1][s] * wc[A - 12] : 0.0f;
        d2[0][s] = pair_sum(a0[s]) * elu_g(S.x3[0][s][k]);
        d2[1][s] = pair_sum(a1[s]) * elu_g(S.x3[1][s][k]);
        d2[2][s] = pair_sum(a2[s]) * elu_g(S.x3[2][s][k]);
      }
    }
#pragma unroll
    for (int net = 0; net < 3; ++net)
#pragma unroll
      for (int s = 0; s < MB; ++s) o[(net * MB + s) * NTH + tid] = d2[net][s];
  }
  {
    float d2[3][MB];
    head_backward(S, wc, c2c, c2n, d2);
#pragma unroll
    for (int net = 0; net < 3; ++net)
#pragma unroll
      for (int s = 0; s < MB; ++s) o[(3 * MB + net * MB + s) * NTH + tid] = d2[net][s];
  }
}
extern "C" int sdxpk_head_backward_check(const float* dmu, const float* dv, const float* x3, const float* hw, int n, float* out, hipStream_t st) {
  if (n < 1) return -1;
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(k_head_backward_check), hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(PLds)) != hipSuccess) return -1;
  hipLaunchKernelGGL(k_head_backward_check, dim3(n), dim3(NTH), sizeof(PLds), st, dmu, dv, x3, hw, out);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
// Test entry (tests/test_gpu_persist_loss_phase.py): the loss phase of phase D, one workgroup of NTH threads per case.  in [n][LOSS_IN]: act [MB][32], mu [MB][32],
// ls [32], sgm [32], val [2][MB], then per sample adv, old -log p, return, old value ([4][MB]), then e_clip, critic_coef, bounds_coef, clip_value.
// out [n][2][LOSS_OUT]: gnlp [MB], dv [2][MB], dmu [MB][32], dls [32], stat [MB][3] (actor, critic, central value), z [MB][32] of [0] the block the epoch
// kernel had before loss_request / loss_front / loss_back - lane (s, 31) forms both value-head losses behind the ratio, the dmu thread reads z, sigma, mu and
// gnlp behind the first barrier and divides there - kept here verbatim as the reference, and of [1] the three helpers on the same inputs.
constexpr int LOSS_IN = 2 * MB * 32 + 64 + 2 * MB + 4 * MB + 4, LOSS_OUT = MB + 2 * MB + MB * 32 + 32 + MB * 3 + MB * 32;
__global__ __launch_bounds__(NTH) void k_loss_phase_check(const float* in, float* out) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  PLds& S = *reinterpret_cast<PLds*>(smem_raw);
  const int tid = threadIdx.x;
  const size_t c = blockIdx.x;
  constexpr int A = ACT;
  const float* ic = in + c * LOSS_IN;
  const float* ps = ic + 2 * MB * 32 + 64 + 2 * MB;   // [4][MB]
  const float* cf = ps + 4 * MB;
  struct { float e_clip, critic_coef, bounds_coef; int clip_value; } D = {cf[0], cf[1], cf[2], cf[3] != 0.0f};
  const float invM = 1.0f / (float)MB;
  auto fill = [&]() {
    if (tid < MB * 32) { S.act[tid / 32][tid % 32] = ic[tid]; S.mu[tid / 32][tid % 32] = ic[MB * 32 + tid]; }
    if (tid < 32) { S.ls[tid] = ic[2 * MB * 32 + tid]; S.sgm[tid] = ic[2 * MB * 32 + 32 + tid]; }
    if (tid < 2 * MB) S.val[tid / MB][tid % MB] = ic[2 * MB * 32 + 64 + tid];
    const float nan = __builtin_nanf("");
    if (tid < MB * 32) { S.dmu[tid / 32][tid % 32] = nan; S.z[tid / 32][tid % 32] = nan; }
    if (tid < 32) S.dls[tid] = nan;
    if (tid < MB) { S.gnlp[tid] = nan; S.dv[0][tid] = nan; S.dv[1][tid] = nan; S.stat[tid][STAT_ACTOR] = nan; S.stat[tid][STAT_CRITIC] = nan; S.stat[tid][STAT_CV] = nan; }
    __syncthreads();
  };
  auto copy_out = [&](float* o) {
    __syncthreads();
    if (tid < MB) { o[tid] = S.gnlp[tid]; o[MB + tid] = S.dv[0][tid]; o[2 * MB + tid] = S.dv[1][tid]; }
    if (tid < MB * 32) { o[3 * MB + tid] = S.dmu[tid / 32][tid % 32]; o[3 * MB + MB * 32 + 32 + MB * 3 + tid] = S.z[tid / 32][tid % 32]; }
    if (tid < 32) o[3 * MB + MB * 32 + tid] = S.dls[tid];
    if (tid < MB * 3) o[3 * MB + MB * 32 + 32 + tid] = S.stat[tid / 3][tid % 3 == 0 ? STAT_ACTOR : tid % 3 == 1 ? STAT_CRITIC : STAT_CV];
    __syncthreads();
  };
  fill();
  {
    float pf_adv = 0.0f, pf_nlp = 0.0f, pf_ret = 0.0f, pf_val = 0.0f;
    if (tid < MB * 32 && (tid % 32) == 31) { const int i = tid / 32; pf_adv = ps[i]; pf_nlp = ps[MB + i]; pf_ret = ps[2 * MB + i]; pf_val = ps[3 * MB + i]; }
    SDX_OPAQUE(pf_adv); SDX_OPAQUE(pf_nlp); SDX_OPAQUE(pf_ret); SDX_OPAQUE(pf_val);
    {
      // (only what the gradients need: the KL, bounds and entropy terms of the statistics are formed in the dY1 shadow, on waves 5 and 7)
      float r_nlp = 0.0f;
      if (tid < MB * 32) {
        const int s = tid / 32, a = tid % 32;
        // z of (sample s, action a): formed by the thread that uses it here; S.z is only for the dmu / dlogstd lanes after the barrier below
        const float zz = (a < A) ? (S.act[s][a] - S.mu[s][a]) / S.sgm[a] : 0.0f;
        S.z[s][a] = zz;
        if (a < A) r_nlp = 0.5f * zz * zz + S.ls[a];
      }
      r_nlp = half_sum(r_nlp);
      if (tid < MB * 32 && (tid % 32) == 31) {
        const int s = tid / 32;
        const float nlp = r_nlp + 0.5f * 1.8378770664093453f * (float)A;
        const float adv = pf_adv;
        const float ratio = expf(pf_nlp - nlp);
        const float L1 = -adv * ratio, L2 = -adv * clampf(ratio, 1.0f - D.e_clip, 1.0f + D.e_clip);
        const bool inr = ratio >= 1.0f - D.e_clip && ratio <= 1.0f + D.e_clip;
        S.gnlp[s] = (L1 > L2 || inr) ? adv * ratio : 0.0f;
        const float R = pf_ret, vo = pf_val;
        float closs[2];
        for (int j = 0; j < 2; ++j) {
          const float v = S.val[j][s];
          const float vc = vo + clampf(v - vo, -D.e_clip, D.e_clip);
          const float c1v = (v - R) * (v - R), c2v = (vc - R) * (vc - R);
          float d;
          if (D.clip_value) {
            closs[j] = fmaxf(c1v, c2v);
            const bool inv = fabsf(v - vo) <= D.e_clip;
            d = (c1v > c2v || inv) ? 2.0f * (v - R) : 0.0f;
          } else { closs[j] = c1v; d = 2.0f * (v - R); }
          S.dv[j][s] = (j == 0 ? 0.5f * D.critic_coef : 1.0f) * d * invM;
        }
        S.stat[s][STAT_ACTOR] = fmaxf(L1, L2); S.stat[s][STAT_CRITIC] = closs[0]; S.stat[s][STAT_CV] = closs[1];
      }
    }
    SDX_LDS_BARRIER();   // LDS traffic only: the column view's loads stay in flight (a __syncthreads() would wait for them)
    if (tid < MB * 32) {
      const int s = tid / 32, a = tid % 32;
      float dmu = 0.0f;
      if (a < A) {
        const float sg = S.sgm[a], mu = S.mu[s][a];
        const float hi = fmaxf(mu - 1.1f, 0.0f), lo = fminf(mu + 1.1f, 0.0f);
        dmu = S.gnlp[s] * (-(S.z[s][a] / sg)) * invM + D.bounds_coef * (2.0f * hi + 2.0f * lo) * invM;
      }
      S.dmu[s][a] = dmu;
    }
    if (tid >= T_LS && tid < T_LS + 32) {
      const int a = tid - T_LS;
      float dls = 0.0f;
      if (a < A) for (int s = 0; s < MB; ++s) dls += S.gnlp[s] * (1.0f - S.z[s][a] * S.z[s][a]) * invM;
      S.dls[a] = dls;
    }
    SDX_LDS_BARRIER();   // LDS traffic only: the column view's loads stay in flight (a __syncthreads() would wait for them)
  }
  copy_out(out + c * 2 * LOSS_OUT);
  fill();
  {
    float pf_adv = 0.0f, pf_nlp = 0.0f, pf_ret = 0.0f, pf_val = 0.0f;
    if (tid < MB * 32 && (tid % 32) == 31) { const int i = tid / 32; pf_adv = ps[i]; pf_nlp = ps[MB + i]; }
    if (tid >= T_VLOSS && tid < T_VLOSS + 2 * MB) { const int i = (tid - T_VLOSS) % MB; pf_ret = ps[2 * MB + i]; pf_val = ps[3 * MB + i]; }
    SDX_OPAQUE(pf_adv); SDX_OPAQUE(pf_nlp); SDX_OPAQUE(pf_ret); SDX_OPAQUE(pf_val);
    ZOps zo;
    loss_request(S, tid, zo);
    const LossCfg lc = {D.e_clip, D.critic_coef, D.bounds_coef, (bool)D.clip_value};
    float q, bt;
    loss_front(S, lc, tid, zo, pf_adv, pf_nlp, pf_ret, pf_val, invM, q, bt);
    SDX_LDS_BARRIER();
    loss_back(S, tid, q, bt, invM);
    SDX_LDS_BARRIER();
  }
  copy_out(out + c * 2 * LOSS_OUT + LOSS_OUT);
}
extern "C" int sdxpk_loss_phase_check(const float* in, int n, float* out, hipStream_t st) {
  if (n < 1) return -1;
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(k_loss_phase_check), hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(PLds)) != hipSuccess) return -1;
  hipLaunchKernelGGL(k_loss_phase_check, dim3(n), dim3(NTH), sizeof(PLds), st, in, out);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
// Test entries (tests/test_gpu_persist_head_words.py): the head matrix between the CUs (sdxp_persist_exchange.h: head_owned, head_publish, head_rows_peek /
// head_row24_peek / head_rows_take, head_cols_load), as two launches in stream order - no workgroup waits for another inside a launch.
// sdxpk_head_publish_check: NWG workgroups of one wave; thread t < HPC of workgroup g takes element (hrow, hk) of W [ACT + 2][U2] (bit patterns) as the
// ownership map gives it, writes (hrow, hk) to own [NWG][HPC][2], and the wave publishes with `tag` - workgroup `stale_cu` (if >= 0) with tag - 1.  ll is an
// exchange buffer of sdxpk_head_words_ll_words() 8-byte words.
__global__ __launch_bounds__(64) void k_head_publish_check(const float* W, unsigned tag, int stale_cu, u64* ll, int* own) {
  const int t = threadIdx.x, g = blockIdx.x;
  int he, hrow, hk;
  head_owned(g, t, he, hrow, hk);
  float hw = 0.0f;
  if (t < HPC) { hw = W[hrow * U2 + hk]; own[(g * HPC + t) * 2] = hrow; own[(g * HPC + t) * 2 + 1] = hk; }
  head_publish(lq_rsrc(ll), ll, t, he, hw, g == stale_cu ? tag - 1u : tag);
}
// sdxpk_head_views_check: ONE workgroup of NTH threads takes the row view with the non-polling take and loads the column view, as phase D does:
// wh [NTH][HR][4], wc [NTH][13] (bit patterns), verdict [NWV]: 1 if the wave's take found `tag` on all its words, else 0.
__global__ __launch_bounds__(NTH) void k_head_views_check(u64* ll, unsigned tag, float* wh_out, float* wc_out, int* verdict) {
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const __amdgpu_buffer_rsrc_t q = lq_rsrc(ll);
  u32x4 ph[4];
  u64 p24[4];
  float wh[HR][4];
  head_rows_peek(q, wave, lane, ph);
  head_row24_peek(ll, wave, lane, tag, p24);
  const bool hit = head_rows_take(ph, p24, tag, wh);
  if (lane == 0) verdict[wave] = hit ? 1 : 0;
#pragma unroll
  for (int j = 0; j < HR; ++j)
#pragma unroll
    for (int e = 0; e < 4; ++e) wh_out[(tid * HR + j) * 4 + e] = wh[j][e];
  const int c2c = (tid >> 5) & 1, c2n = 32 * (tid >> 6) + (tid & 31);
  HeadCols hc;
  float wc[13];
  head_cols_load(q, c2c, c2n, hc);
  head_cols_take(hc, c2c, wc);
#pragma unroll
  for (int j = 0; j < 13; ++j) wc_out[tid * 13 + j] = wc[j];
}
extern "C" size_t sdxpk_head_words_ll_words() { return SDXP_LL_WORDS; }
extern "C" int sdxpk_head_publish_check(const float* W, unsigned tag, int stale_cu, unsigned long long* ll, int* own, hipStream_t st) {
  if (stale_cu >= NWG) return -1;
  hipLaunchKernelGGL(k_head_publish_check, dim3(NWG), dim3(64), 0, st, W, tag, stale_cu, ll, own);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
extern "C" int sdxpk_head_views_check(unsigned long long* ll, unsigned tag, float* wh, float* wc, int* verdict, hipStream_t st) {
  hipLaunchKernelGGL(k_head_views_check, dim3(1), dim3(NTH), 0, st, ll, tag, wh, wc, verdict);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
