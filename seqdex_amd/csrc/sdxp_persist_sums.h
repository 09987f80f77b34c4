// sdxp_persist_sums.h - private to the persistent PPO update (included by sdxp_persist.hip and sdxp_persist_checks.hip only): the cross-lane and
// cross-wave sums of k_update_persistent - DPP row sums, the halving butterflies that form N wave sums at once with the bits of N wave_sum
// trees, the workgroup reduction through PLds::red, and the 4x4 Gram accumulators
#pragma once
#include "sdxp_device.h"   // sdx_common.h, dpp_add, wave_sum
#include "sdxp_persist_lds.h"

namespace {
// v + (the value of lane ^ 32), in both lanes: v_permlane32_swap_b32 of v with itself leaves the lower half's values in one result and the
// upper half's in the other
__device__ __forceinline__ float pair_sum(float v) {
  const unsigned u = __builtin_bit_cast(unsigned, v);
  const auto r = __builtin_amdgcn_permlane32_swap(u, u, false, false);
  return __builtin_bit_cast(float, (unsigned)r[0]) + __builtin_bit_cast(float, (unsigned)r[1]);
}
// accumulate the 4x4 Gram (lower triangle, 10 terms) of (a, b, c, d)
__device__ __forceinline__ void gram_acc10(float* p, float a, float b, float c, float d) {
  p[0] += a * a; p[1] += b * a; p[2] += b * b; p[3] += c * a; p[4] += c * b; p[5] += c * c;
  p[6] += d * a; p[7] += d * b; p[8] += d * c; p[9] += d * d;
}
__device__ __forceinline__ int tri16(int i) { const int a = i >> 2, b = i & 3, hi = a > b ? a : b, lo = a > b ? b : a; return hi * (hi + 1) / 2 + lo; }
// sums over each 16-lane DPP row, in every lane of the row: the first four levels of wave_sum (quad_perm, quad_perm, row_half_mirror, row_mirror)
__device__ __forceinline__ float row_sum16(float v) {
  v = dpp_add<0xB1, 0xF>(v); v = dpp_add<0x4E, 0xF>(v); v = dpp_add<0x141, 0xF>(v); v = dpp_add<0x140, 0xF>(v);
  return v;
}
// sums over each 32-lane half of the wave; valid in lanes 16..31 and 48..63
__device__ __forceinline__ float half_sum(float v) { return dpp_add<0x142, 0xA>(row_sum16(v)); }
template <int CTRL, int BANK>
__device__ __forceinline__ float dpp_mov(float old, float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, old), __builtin_bit_cast(int, v), CTRL, 0xF, BANK, false));
}
// v + (the value of the lane CTRL names), every lane of the row a valid source (quad_perm / row_ror): bound_ctrl set, so the move has no `old`
// operand to materialise and folds into ONE v_add_f32_dpp
template <int CTRL>
__device__ __forceinline__ float dpp_pair(float v) {
  asm("" : "+v"(v));   // (the ROUNDED value: a bare product must not be contracted with this add into an fma - the partner adds the rounded one)
  return v + __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xF, 0xF, true));
}
// the two halving levels + the two levels inside the 16-lane DPP row: u2[j] = sum over the row's lanes of value 4 j + (lane & 3).
// A halving level is written as BOTH pair sums - even value + its partner's, odd value + its partner's, one v_add_f32_dpp each, the source a
// plain register - and one select of the sum this lane keeps: 3 instructions per pair.  (Written as two selects - what to keep, what to send -
// in front of one add, the compiler fused the move into the add for fewer than half of the pairs, and the moves that stayed needed a zero `old`
// register each: 129 VALU instructions for N = 30 stand-alone, 101 in this form.)  The lane that keeps a value adds the same two operands as
// before - its own and its partner's - and IEEE addition commutes: the bits are those of the tree lane ^ 1, ^ 2, ^ 4, ^ 8 per value.
template <int N>
__device__ __forceinline__ void row_butterfly(const float (&v)[N], float (&u2)[(N + 3) / 4], int lane) {
  constexpr int N4 = (N + 3) / 4;
  const bool b0 = lane & 1, b1 = lane & 2;
  float u1[2 * N4];
#pragma unroll
  for (int j = 0; j < 2 * N4; ++j) {                         // partner lane ^ 1 (quad_perm [1,0,3,2])
    const float e = 2 * j < N ? dpp_pair<0xB1>(v[2 * j]) : 0.0f, o = 2 * j + 1 < N ? dpp_pair<0xB1>(v[2 * j + 1]) : 0.0f;
    u1[j] = b0 ? o : e;
  }
#pragma unroll
  for (int j = 0; j < N4; ++j) {
    const float e = dpp_pair<0x4E>(u1[2 * j]), o = 2 * (2 * j + 1) < N ? dpp_pair<0x4E>(u1[2 * j + 1]) : 0.0f;
    float t = b1 ? o : e;                                    // partner lane ^ 2 (quad_perm [2,3,0,1]): t = quad sum of value 4 j + (lane & 3)
    float x = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, t), 0x12C, 0xF, 0xF, true));   // lane ^ 4: row_ror:12 (lane + 4) is the partner of banks 0, 2 ...
    x = dpp_mov<0x124, 0xA>(x, t);                           // ... row_ror:4 (lane - 4) into banks 1, 3
    t += x;
    t = dpp_pair<0x128>(t);                                  // lane ^ 8 (row_ror:8): sum over the 16-lane row
    u2[j] = t;
  }
}
// N wave sums at once: the row butterfly, then the rows meet through v_permlane16_swap (partner lane ^ 16: rows 0 + 1, 2 + 3) and
// v_permlane32_swap (lane ^ 32).  Every lane ends with u[j] = the whole wave's sum of value 4 j + (lane & 3).  The pairs of the six levels
// are those of wave_sum's DPP tree (quad_perm, quad_perm, row_half_mirror, row_mirror, row_bcast15, row_bcast31) and IEEE addition
// commutes, so u[j] equals wave_sum(v[4 j + (lane & 3)]) bit for bit - at N, N / 2, N / 4, N / 4, ... adds per level (and a select per pair on the first two) instead of N on all six.
template <int N>
__device__ __forceinline__ void wave_sums(const float (&v)[N], float (&u)[(N + 3) / 4], int lane) {
  // (opaque copies: the sums are those of the ROUNDED values - a value that is a bare product must not be contracted with the butterfly's first
  // add into an fma, through the level's select.  wave_sum of a bare product IS contracted that way, per lane: forward L2, whose values are
  // bare products, has a butterfly of its own - fwd2_sums below.)
  float t[N];
#pragma unroll
  for (int i = 0; i < N; ++i) { t[i] = v[i]; asm("" : "+v"(t[i])); }
  row_butterfly<N>(t, u, lane);
#pragma unroll
  for (int j = 0; j < (N + 3) / 4; ++j) {
    const unsigned x = __builtin_bit_cast(unsigned, u[j]);
    const auto r = __builtin_amdgcn_permlane16_swap(x, x, false, false);
    u[j] = pair_sum(__builtin_bit_cast(float, (unsigned)r[0]) + __builtin_bit_cast(float, (unsigned)r[1]));
  }
}
// Forward L2: the wave sums of the twelve BARE products w[net] x[net][s], with the bits of twelve wave_sum trees.  wave_sum(w x) compiles to
// v_mul (the rounded product) / v_mov_dpp quad_perm:[1,0,3,2] / v_fmac: lane l holds fma(w_l, x_l, rounded product of lane l ^ 1), so the two
// lanes of a pair hold different bits, and of a DPP row only the lanes whose view the rest of the tree carries to lane 63 count - 15, 13, 8,
// 10, 0, 2, 7, 5: row sum = ((v15 + v13) + (v8 + v10)) + ((v0 + v2) + (v7 + v5)), wave sum = (r3 + r2) + (r1 + r0).  Here the first level is
// written out - on every lane, twelve independent fmas, the product through an opaque copy so that it stays rounded - and the other levels run
// as a halving butterfly over exactly those pairs: partner l ^ 2 (the lanes with bit 0 == bit 1 keep samples 0 and 3, the others 1 and 2),
// row_half_mirror (bit 2 == bit 3 keeps the first of the two), row_mirror, then the rows as in wave_sums.  Addition commutes, pairing does
// not.  Lanes 0, 2, 5, 7 (and their mirrors 15, 13, 10, 8) of every row end with u[net] = the wave's sum of sample 0, 1, 2, 3: lanes 1 and 3
// are not on the tree's path, so the storing lanes are not 0..3 (fwd2_sample, fwd2_store).
__device__ __forceinline__ int fwd2_sample(int lane) {
  const bool ka = (((lane >> 1) ^ lane) & 1) == 0, kf = (((lane >> 3) ^ (lane >> 2)) & 1) == 0;
  return kf ? (ka ? 0 : 1) : (ka ? 3 : 2);
}
__device__ __forceinline__ void fwd2_sums(const float (&w)[3], const float (&x)[3][4], float (&u)[3], int lane) {
  const bool ka = (((lane >> 1) ^ lane) & 1) == 0, kf = (((lane >> 3) ^ (lane >> 2)) & 1) == 0;
  float v[3][4];
#pragma unroll
  for (int net = 0; net < 3; ++net)
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      float t = w[net] * x[net][s];
      asm("" : "+v"(t));
      v[net][s] = __builtin_fmaf(w[net], x[net][s], dpp_mov<0xB1, 0xF>(0.0f, t));   // partner lane ^ 1
    }
#pragma unroll
  for (int net = 0; net < 3; ++net) {
    const float k0 = ka ? v[net][0] : v[net][1], s0 = ka ? v[net][1] : v[net][0];
    const float k1 = ka ? v[net][3] : v[net][2], s1 = ka ? v[net][2] : v[net][3];
    const float a = k0 + dpp_mov<0x4E, 0xF>(0.0f, s0), b = k1 + dpp_mov<0x4E, 0xF>(0.0f, s1);   // partner lane ^ 2
    float t = (kf ? a : b) + dpp_mov<0x141, 0xF>(0.0f, kf ? b : a);                              // row_half_mirror: lane ^ 7
    t += dpp_mov<0x140, 0xF>(0.0f, t);                                                           // row_mirror: lane ^ 15
    const unsigned y = __builtin_bit_cast(unsigned, t);
    const auto r = __builtin_amdgcn_permlane16_swap(y, y, false, false);
    u[net] = pair_sum(__builtin_bit_cast(float, (unsigned)r[0]) + __builtin_bit_cast(float, (unsigned)r[1]));
  }
}
// the forward passes' partial dot products, value net MB + s: lane s < MB holds u[net] = this wave's sum of (net, sample s)
static_assert(MB == 4, "lane & 3 of wave_sums is the sample");
__device__ __forceinline__ void fpart_store(PLds& S, const float (&u)[3], int wave, int lane) {
  if (lane < MB) {
#pragma unroll
    for (int net = 0; net < 3; ++net) S.fpart[(net * MB + lane) * NWV + wave] = u[net];
  }
}
// the same slots from fwd2_sums: lanes 0, 2, 5, 7 hold samples 0, 1, 2, 3
__device__ __forceinline__ void fwd2_store(PLds& S, const float (&u)[3], int wave, int lane) {
  if (lane < 8 && ((0xA5 >> lane) & 1)) {
    const int s = fwd2_sample(lane);
#pragma unroll
    for (int net = 0; net < 3; ++net) S.fpart[(net * MB + s) * NWV + wave] = u[net];
  }
}
// 0.0f + col[0] + col[STRIDE] + ... + col[(N - 1) STRIDE], added in ascending order - the bits of the serial loop `t += S.red[w][c]` - with all
// N LDS reads requested in front of the first add.  Written as the plain loop, the compiler (at the kernel's register limit) requested two values,
// waited for them with lgkmcnt(0), added, and only then requested the next two: N / 2 dependent LDS round trips between two barriers of a
// reduction that every wave of the CU waits for.  The compiler barrier keeps the reads in front of the adds; the N values live only here.
template <int N, int STRIDE>
__device__ __forceinline__ float ordered_sum_ahead(const float* col) {
  float r[N];
#pragma unroll
  for (int w = 0; w < N; ++w) r[w] = col[w * STRIDE];
  asm volatile("" ::: "memory");
  float t = 0.0f;
#pragma unroll
  for (int w = 0; w < N; ++w) t += r[w];
  return t;
}
template <int N4>
__device__ __forceinline__ void rows_store(PLds& S, const float (&u2)[N4], int off, int wave, int lane) {
  if ((lane & 15) < 4) {
    float* r = S.red[wave * 4 + (lane >> 4)] + off;
#pragma unroll
    for (int j = 0; j < N4; ++j) r[4 * j + (lane & 3)] = u2[j];
  }
}
// LDS-only barriers (sdx_common.h): __syncthreads() also waits for the wave's outstanding global accesses - in the shadows that is the
// acknowledgement of the exchange words just published and the next minibatch's prefetched rows; nothing here is ordered through HBM
__device__ __forceinline__ void rows_reduce(PLds& S, int n, float* out, int tid) {
  SDX_LDS_BARRIER();
  if (tid < n) out[tid] = ordered_sum_ahead<4 * NWV, 64>(&S.red[0][tid]);
  SDX_LDS_BARRIER();
}
// block-wide sums of N per-thread values (N <= 64); result in out[0..N).  Two "halving" butterfly levels (lane pairs keep the even /
// odd half of the values, so level L costs N / 2^L exchanges instead of N), two more within the 16-lane DPP row, and the 4 rows x 8
// waves meet in LDS: ~3.5 N VALU ops + N/4 LDS writes per wave instead of 7 N + N masked writes for N independent wave sums.
template <int N>
__device__ __forceinline__ void block_sum(PLds& S, const float (&v)[N], float* out, int tid, int wave, int lane) {
  float u2[(N + 3) / 4];
  row_butterfly<N>(v, u2, lane);
  rows_store<(N + 3) / 4>(S, u2, 0, wave, lane);
  rows_reduce(S, N, out, tid);
}
}  // namespace
