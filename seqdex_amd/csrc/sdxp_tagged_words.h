// sdxp_tagged_words.h - tagged 16-byte exchange words, the part that knows no kernel's shapes: the word type and its one-instruction access, the
// tag spread and payload fold that make a torn word detectable, the store of a tagged word and the give-up rule of a polling gather.
// Included by sdxp_persist_exchange.h (the chain edges of k_update_persistent), sdxp_exbench.hip and sdxp_multirank.hip (the grid-wide
// meeting of k_apply_factors_fused).
#pragma once
#include "sdx_common.h"

namespace {
// A word is (v0, v1, v2, tag'): written and read by one dwordx4 access per lane (device scope, sc1).  A 16-byte access of one lane is not
// architecturally single-copy atomic (no torn word in ~1e10 gathers checked by sdxp_exbench.hip; RCCL's LL128 protocol relies on the same
// hardware behaviour): the last dword carries tag ^ fold(payload) (lq_fold below), so a torn word is rejected and polled again instead of
// being trusted to never occur.
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
// one buffer_load / buffer_store_dwordx4 ... sc1 per lane of 16-byte word q (device scope, as the 8-byte agent-scope atomics lower to): the
// compiler counts these in its s_waitcnt bookkeeping, unlike inline asm
__device__ __forceinline__ u32x4 load16(__amdgpu_buffer_rsrc_t r, unsigned q) { return __builtin_amdgcn_raw_buffer_load_b128(r, q * 16u, 0, 16); }
__device__ __forceinline__ void store16(__amdgpu_buffer_rsrc_t r, unsigned q, u32x4 v) { __builtin_amdgcn_raw_buffer_store_b128(v, r, q * 16u, 0, 16); }
// Tearing is DETECTABLE: the last dword is not the bare tag but tag ^ fold(payload); a consumer accepts a word only when
// last ^ fold(the payload it read) equals the tag it waits for.  A word whose dwords come from two different stores (new tag over a
// stale payload or the reverse) fails the test unless the mixed payload folds to the same value (2^-32, or the stale dwords equal the new
// ones - then nothing is lost) and is simply polled again, like a word that has not arrived.
// (fold = x ^ y ^ z: one v_xor3_b32.  With rotations of y and z in it - to decorrelate equal values of two networks - the checks cost the
// persistent step 0.6 us on its dependent chain, 31.4 instead of 30.8; two networks' values that are equal before AND after a step are unchanged ones)
// Tags advance by 1 per step, so the XOR of two consecutive bare tags is 1, 3, 7, ...: a torn word (new payload over a stale last dword) whose
// payload fold moved by exactly that - one network's value changing by an ulp - would pass.  The tag is therefore spread over all
// 32 bits before it meets the fold (lq_tag: one scalar multiply per gather, off the dependent chain): consecutive tags now differ in ~16
// pseudo-random bit positions, which a slowly varying payload does not reproduce.
__device__ __forceinline__ unsigned lq_fold(unsigned x, unsigned y, unsigned z) { return x ^ y ^ z; }
__device__ __forceinline__ unsigned lq_tag(unsigned tag) { return tag * 0x9E3779B1u; }
__device__ __forceinline__ bool lq_ok(const u32x4& w, unsigned tag) { return (w.w ^ lq_fold(w.x, w.y, w.z)) == lq_tag(tag); }
__device__ __forceinline__ void lq_store(__amdgpu_buffer_rsrc_t q, unsigned idx, float a, float b, float c, unsigned tag) {
  u32x4 w;
  w.x = __float_as_uint(a); w.y = __float_as_uint(b); w.z = __float_as_uint(c); w.w = lq_tag(tag) ^ lq_fold(w.x, w.y, w.z);
  store16(q, idx, w);
}
// The tail of one round of a polling gather that has not found all of its words: sleep, look at the fail flag every 256 spins, and after 2^20
// of them, or when another wave has given up, set the flag and RETURN FALSE from the gather.  (A macro: as a function the kernel's branches
// change.  The loads of a gather are spelled out where they stand for the same reason: through load16, or through a helper that peeks and
// takes, both instantiations of k_update_persistent change.)
#define SDX_POLL_SLEEP_OR_GIVE_UP(spins, failflag)                                                       \
  __builtin_amdgcn_s_sleep(1);                                                                           \
  if ((++spins & 255u) == 0) {                                                                           \
    const unsigned f = __hip_atomic_load(failflag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);          \
    if (spins > (1u << 20) || __builtin_amdgcn_readfirstlane(f) != 0) {                                  \
      __hip_atomic_store(failflag, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);                      \
      return false;                                                                                      \
    }                                                                                                    \
  }
}  // namespace
