// sdxp_persist_exchange.h - private to the persistent PPO update (included by sdxp_persist.hip; sdxp_exbench.hip borrows u64): the inter-CU
// exchange of k_update_persistent - tagged 16-byte words for the chain edges and for rows 0..23 of the head matrix (lq_*: their word-level primitives
// are sdxp_tagged_words.h), tagged 8-byte words for the head matrix's row 24 (ll_*), the layout of SdxpDev::ll, the polling gathers, and the head
// matrix's ownership map, publish and two views (head_*)
#pragma once
#include "sdx_common.h"
#include "sdxp_types.h"
#include "sdxp_persist_lds.h"
#include "sdxp_persist_sums.h"   // dpp_mov
#include "sdxp_tagged_words.h"

namespace {
// ---- (value, tag) exchange words ("LL" protocol): one relaxed 8-byte store at agent scope carries the float and the tag of the
// optimiser step that produced it; a consumer re-reads until the tag it expects shows up.  No fences, no barriers, no reset:
// tags only grow, and the data dependencies of the step (x1 -> x2 -> x3 -> dY1 -> dY0 -> next x1) guarantee that a word is not
// overwritten before every CU has consumed it ("persistent update kernel").
typedef unsigned long long u64;
// The five edges on the step's dependency chain (x1, x2, x3, dY1 and the dY0 norm) travel as 16-BYTE words (v0, v1, v2, tag): the same
// (sample, unit) of the THREE networks in one word (sdxp_tagged_words.h) - the edge's time goes with its word count (DESIGN.md section 4b,
// "the exchange floor").  The head matrix (published a phase ahead, gathered row- and column-wise by different consumers) travels in the same words,
// rows w, w + 8, w + 16 of one column per word (LQ_HW); its 25th row, which one wave reads, keeps 8-byte (value, tag) words (LL_H24).
// Layout of D.ll: 16-byte words LQ_* first, then the 8-byte words of head row 24 at LL_H24 (u64 index).
constexpr unsigned LQ_X1 = 0, LQ_X2 = LQ_X1 + MB * U0, LQ_X3 = LQ_X2 + MB * U1, LQ_DY1 = LQ_X3 + MB * U2, LQ_DY0 = LQ_DY1 + MB * U1,
                   LQ_G0 = LQ_DY0 + MB * U0, LQ_END = LQ_G0 + 16 * NWG;   // LQ_G0: [CU]: the CU's share of layer 0's squared gradient norm, the 3 nets per word (round 6; rounds 4-5: 10 Gram entries per CU)
// LQ_HW: [w < 8][column c < U2]: (W[w][c], W[w + 8][c], W[w + 16][c]) of the (ACT + 2) x U2 head matrix W - rows 0..22 mu, 23 the critic's value, 24 the
// central value's; CU g stores words 8 g .. 8 g + 7, ONE 128-byte line (head_owned).  LL_H24: [c]: W[24][c], stored by CU c.
constexpr unsigned LQ_HW = LQ_END, LQ_HW_END = LQ_HW + 8 * U2;
constexpr size_t LL_H24 = 2 * (size_t)LQ_HW_END, LL_END = LL_H24 + U2;
static_assert(ACT + 2 == 3 * 8 + 1 && NWV == 8 && NWG == U2, "three rows per word and wave, row 24 one column per CU");
static_assert(LQ_HW % 8 == 0, "a CU's eight head words are one 128-byte line");
static_assert(LL_END <= SDXP_LL_WORDS, "exchange buffer too small");
__device__ __forceinline__ __amdgpu_buffer_rsrc_t lq_rsrc(void* ll) { return __builtin_amdgcn_make_buffer_rsrc(ll, 0, SDXP_LL_WORDS * 8, 0x00020000); }
// first look at N packed words, issued some work ahead of where they are needed (lq_peek), and the test whether all of them already
// carried `tag` (lq_take): when a shadow phase outlasts its exchange edge the words are there, and the round trip of the gather
// (about 0.6 us) runs under the shadow's last piece of work instead of after it.  A miss falls back to the polling lq_gather.
template <int N>
__device__ __forceinline__ void lq_peek(__amdgpu_buffer_rsrc_t q, unsigned idx0, unsigned stride, u32x4 (&w)[N]) {
#pragma unroll
  for (int i = 0; i < N; ++i) w[i] = load16(q, idx0 + i * stride);
}
template <int N>
__device__ __forceinline__ bool lq_take(const u32x4 (&w)[N], unsigned tag, float (&o0)[N], float (&o1)[N], float (&o2)[N]) {
  bool ok = true;
#pragma unroll
  for (int i = 0; i < N; ++i) ok = ok && lq_ok(w[i], tag);
#pragma unroll
  for (int i = 0; i < N; ++i) { o0[i] = __uint_as_float(w[i].x); o1[i] = __uint_as_float(w[i].y); o2[i] = __uint_as_float(w[i].z); }
  return __builtin_amdgcn_ballot_w64(!ok) == 0;
}
// gather N packed words idx0 + i * stride carrying `tag` -> the three networks' values; wave-uniform retry as ll_gather
template <int N>
__device__ __forceinline__ bool lq_gather(__amdgpu_buffer_rsrc_t q, unsigned idx0, unsigned stride, unsigned tag, float (&o0)[N], float (&o1)[N], float (&o2)[N],
                                          unsigned* failflag) {
  unsigned spins = 0;
  for (;;) {
    u32x4 w[N];   // (lq_peek and lq_take, spelled out: through either helper, or through load16, both instantiations of the kernel change)
#pragma unroll
    for (int i = 0; i < N; ++i) w[i] = __builtin_amdgcn_raw_buffer_load_b128(q, (idx0 + i * stride) * 16u, 0, 16);
    bool ok = true;
#pragma unroll
    for (int i = 0; i < N; ++i) ok = ok && lq_ok(w[i], tag);
#pragma unroll
    for (int i = 0; i < N; ++i) { o0[i] = __uint_as_float(w[i].x); o1[i] = __uint_as_float(w[i].y); o2[i] = __uint_as_float(w[i].z); }
    if (__builtin_amdgcn_ballot_w64(!ok) == 0) return true;
    SDX_POLL_SLEEP_OR_GIVE_UP(spins, failflag)
  }
}
// take the words of a first look `pw` (if one was `issued`), else gather them; `fail` (PLds::fail) is set in here if they do not arrive
template <int N>
__device__ __forceinline__ void lq_take_or_gather(bool issued, const u32x4 (&pw)[N], __amdgpu_buffer_rsrc_t q, unsigned idx0, unsigned stride, unsigned tag, float (&o0)[N],
                                          float (&o1)[N], float (&o2)[N], unsigned* failflag, int& fail) {
  if (!(issued && lq_take<N>(pw, tag, o0, o1, o2)) && !lq_gather<N>(q, idx0, stride, tag, o0, o1, o2, failflag)) fail = 1;
}
// the gathered words of one edge -> the three networks' LDS images (PLds::x1 / x2 / x3 / dy1): word tid + NTH j of the edge is (sample, unit)
// s U + unit, and an image [MB][U] has the same flat index
template <int N, int U>
__device__ __forceinline__ void image_store(float (&img)[3][MB][U], const float (&v0)[N], const float (&v1)[N], const float (&v2)[N], int tid) {
  static_assert(N * NTH == MB * U, "N words per thread cover the image");
#pragma unroll
  for (int j = 0; j < N; ++j) { (&img[0][0][0])[tid + NTH * j] = v0[j]; (&img[1][0][0])[tid + NTH * j] = v1[j]; (&img[2][0][0])[tid + NTH * j] = v2[j]; }
}
__device__ __forceinline__ void ll_store(u64* p, float v, unsigned tag) {
  __hip_atomic_store(p, ((u64)tag << 32) | (u64)__float_as_uint(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// gather N words p[i * stride] carrying `tag`; false (and *failflag set) if they do not arrive.  The retry loop is wave-uniform
// (all lanes reload until every lane has its words), which keeps the loaded values out of divergent-loop phis.
template <int N>
__device__ __forceinline__ bool ll_gather(const u64* p, size_t stride, unsigned tag, float (&out)[N], unsigned* failflag) {
  unsigned spins = 0;
  for (;;) {
    u64 w[N];
#pragma unroll
    for (int i = 0; i < N; ++i) w[i] = __hip_atomic_load(p + i * stride, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    bool ok = true;
#pragma unroll
    for (int i = 0; i < N; ++i) ok = ok && (unsigned)(w[i] >> 32) == tag;
#pragma unroll
    for (int i = 0; i < N; ++i) out[i] = __uint_as_float((unsigned)w[i]);
    if (__builtin_amdgcn_ballot_w64(!ok) == 0) return true;
    SDX_POLL_SLEEP_OR_GIVE_UP(spins, failflag)
  }
}
// ---- the head matrix between the CUs: who owns an element, how it leaves its owner, and the two views phase D takes of it
// Thread t < HPC of CU g owns element (hrow, hk), and `he` is where it goes: t < 24 is row (g >> 5) + 8 (t >> 3), column 8 (g & 31) + (t & 7), an
// element of word LQ_HW + he, he = 8 g + (t & 7); t = 24 is row 24, column g, word LL_H24 + he, he = g.  (t >= HPC: not used.)
__device__ __forceinline__ void head_owned(int g, int t, int& he, int& hrow, int& hk) {
  const bool r24 = t >= HPC - 1;
  hrow = r24 ? ACT + 1 : (g >> 5) + 8 * (t >> 3);
  hk = r24 ? g : 8 * (g & 31) + (t & 7);
  he = r24 ? g : 8 * g + (t & 7);
}
// publish this CU's elements (`hw` of thread t < HPC, head_owned) with `tag`: ALL lanes of wave 0 call it.  The three rows of a column are lanes l,
// l + 8 (the same DPP row) and l + 16 (the next row: v_permlane16_swap) and meet in lane l < 8, which stores the word; lane 24 stores row 24's.
__device__ __forceinline__ void head_publish(__amdgpu_buffer_rsrc_t q, u64* ll, int t, int he, float hw, unsigned tag) {
  const float v1 = dpp_mov<0x108, 0xF>(0.0f, hw);                                        // row_shl:8: lane l + 8
  const unsigned y = __builtin_bit_cast(unsigned, hw);
  const auto r = __builtin_amdgcn_permlane16_swap(y, y, false, false);                  // r[1]: rows 1, 1, 3, 3 - lane l + 16 for l < 16
  const float v2 = __builtin_bit_cast(float, (unsigned)r[1]);
  if (t < 8) lq_store(q, LQ_HW + (unsigned)he, hw, v1, v2, tag);
  else if (t == HPC - 1) ll_store(ll + LL_H24 + he, hw, tag);
}
// Row view (head forward): wave w holds rows w + 8 j, columns lane + 64 e, as wh[j][e]; rows w, w + 8, w + 16 are the three values of word
// LQ_HW + 256 w + lane + 64 e, row 24 (wave 0, j = 3) four 8-byte words.  head_rows_peek requests them (wave 0: with row 24's), head_rows_take
// tests the tags without polling and hands the values out (false: a word did not carry `tag` - head_rows_gather polls).
__device__ __forceinline__ unsigned head_row_word(int wave, int lane) { return LQ_HW + 256u * (unsigned)wave + (unsigned)lane; }
__device__ __forceinline__ void head_rows_peek(__amdgpu_buffer_rsrc_t q, int wave, int lane, u32x4 (&ph)[4]) { lq_peek<4>(q, head_row_word(wave, lane), 64, ph); }
__device__ __forceinline__ void head_row24_peek(const u64* ll, int wave, int lane, unsigned tag, u64 (&p24)[4]) {
#pragma unroll
  for (int e = 0; e < 4; ++e)   // (waves 1..7 have no fourth row: value 0 with the expected tag)
    p24[e] = wave == 0 ? __hip_atomic_load(ll + LL_H24 + lane + 64 * e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : (u64)tag << 32;
}
__device__ __forceinline__ bool head_rows_take(const u32x4 (&ph)[4], const u64 (&p24)[4], unsigned tag, float (&wh)[HR][4]) {
  bool ok = true;
#pragma unroll
  for (int e = 0; e < 4; ++e) ok = ok && (unsigned)(p24[e] >> 32) == tag;
#pragma unroll
  for (int e = 0; e < 4; ++e) wh[3][e] = __uint_as_float((unsigned)p24[e]);
  const bool ok3 = lq_take<4>(ph, tag, wh[0], wh[1], wh[2]);
  return __builtin_amdgcn_ballot_w64(!ok) == 0 && ok3;
}
__device__ __forceinline__ bool head_rows_gather(__amdgpu_buffer_rsrc_t q, const u64* ll, int wave, int lane, unsigned tag, float (&wh)[HR][4], unsigned* failflag) {
  bool ok = lq_gather<4>(q, head_row_word(wave, lane), 64, tag, wh[0], wh[1], wh[2], failflag);
#pragma unroll
  for (int e = 0; e < 4; ++e) wh[3][e] = 0.0f;
  if (wave == 0) ok = ll_gather<4>(ll + LL_H24 + lane, 64, tag, wh[3], failflag) && ok;   // lane-contiguous words
  return ok;
}
// Column view (heads' backward): lane (column c2n, row half c2c) holds rows min(13 c2c + j, 24) as wc[j], no tags (the caller says why none are needed).
// Word LQ_HW + 256 w + c2n holds rows w, w + 8, w + 16 of the column: the lower half takes its dwords 0, 1 (rows w, w + 8: 0..15, of which it keeps
// 0..12), the upper half its dwords 1, 2 (rows w + 8, w + 16: of which it keeps 13..23) - EIGHT unconditional plain 8-byte loads in which the two halves
// of a wave, lanes l and l ^ 32, read the same four 128-byte lines, and one dword of row 24 (word LL_H24 + c2n).  (As 13 dword loads, one per row, an
// instruction touched eight lines, twice the four of the 8-byte words this layout replaced, and the loss phase under which the loads fly was 0.3 us
// longer on the phase clock.)  head_cols_load only requests - HeadCols: pair[w] = rows w + 8 c2c, w + 8 + 8 c2c, and row 24 -, head_cols_take picks wc[]
// out of the pairs where the heads' backward begins: a select on a loaded value in front of the loss phase would wait for the loads there.
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
struct HeadCols { u32x2 pair[8]; unsigned r24; };
__device__ __forceinline__ void head_cols_load(__amdgpu_buffer_rsrc_t q, int c2c, int c2n, HeadCols& hc) {
  const unsigned v = (LQ_HW + (unsigned)c2n) * 16u + 4u * (unsigned)c2c;
#pragma unroll
  for (int w = 0; w < 8; ++w) hc.pair[w] = __builtin_amdgcn_raw_buffer_load_b64(q, v, 4096 * w, 16);
  hc.r24 = __builtin_amdgcn_raw_buffer_load_b32(q, ((unsigned)LL_H24 + (unsigned)c2n) * 8u, 0, 16);
}
__device__ __forceinline__ void head_cols_take(const HeadCols& hc, int c2c, float (&wc)[13]) {
  static_assert(ACT + 2 == 25, "rows 0..12 and 13..24");
#pragma unroll
  for (int j = 0; j < 13; ++j) {
    const unsigned lo = j < 8 ? hc.pair[j].x : hc.pair[j - 8].y;                                // row j: 0..7, 8..12
    const unsigned hi = j < 3 ? hc.pair[5 + j].x : (j < 11 ? hc.pair[j - 3].y : hc.r24);       // row 13 + j: 13..15, 16..23, 24 (and its repeat)
    wc[j] = __uint_as_float(c2c ? hi : lo);
  }
}
}  // namespace
