// sdxp_persist_exchange.h - private to the persistent PPO update (included by sdxp_persist.hip; sdxp_exbench.hip borrows u64): the inter-CU
// exchange of k_update_persistent - tagged 16-byte words for the chain edges (lq_*: their word-level primitives are sdxp_tagged_words.h), tagged
// 8-byte words for the head matrix (ll_*), the layout of SdxpDev::ll, and the polling gathers
#pragma once
#include "sdx_common.h"
#include "sdxp_types.h"
#include "sdxp_persist_lds.h"
#include "sdxp_tagged_words.h"

namespace {
// ---- (value, tag) exchange words ("LL" protocol): one relaxed 8-byte store at agent scope carries the float and the tag of the
// optimiser step that produced it; a consumer re-reads until the tag it expects shows up.  No fences, no barriers, no reset:
// tags only grow, and the data dependencies of the step (x1 -> x2 -> x3 -> dY1 -> dY0 -> next x1) guarantee that a word is not
// overwritten before every CU has consumed it ("persistent update kernel").
typedef unsigned long long u64;
// The five edges on the step's dependency chain (x1, x2, x3, dY1 and the dY0 norm) travel as 16-BYTE words (v0, v1, v2, tag): the same
// (sample, unit) of the THREE networks in one word (sdxp_tagged_words.h) - the edge's time goes with its word count (DESIGN.md section 4b,
// "the exchange floor").  The head matrix (LL_HW: published a phase ahead, gathered row- and column-wise by different consumers) keeps its 8-byte words.
// Layout of D.ll: 16-byte words LQ_* first, then the 8-byte head words at LL_HW (u64 index).
constexpr unsigned LQ_X1 = 0, LQ_X2 = LQ_X1 + MB * U0, LQ_X3 = LQ_X2 + MB * U1, LQ_DY1 = LQ_X3 + MB * U2, LQ_DY0 = LQ_DY1 + MB * U1,
                   LQ_G0 = LQ_DY0 + MB * U0, LQ_END = LQ_G0 + 16 * NWG;   // LQ_G0: [CU]: the CU's share of layer 0's squared gradient norm, the 3 nets per word (round 6; rounds 4-5: 10 Gram entries per CU)
constexpr size_t LL_HW = 2 * (size_t)LQ_END, LL_END = LL_HW + (ACT + 2) * U2;
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
}  // namespace
