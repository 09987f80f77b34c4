// sdx_state.h — sim snapshots (include/seqdex.h sdx_state_*): the segment table that says what an env's state is, and
// the one copy kernel that moves env states env -> snapshot row (save), row -> env (restore) and env -> env (clone).  Included by
// sdx_capi.hip only (it fills the table from sdx_buffers.h); plain C++ loads and stores, so that tests/hipemu compiles it with g++.
#pragma once
#include "sdx_common.h"

#define SDX_ST_MAXSEG 48
#define SDX_ST_MAGIC 0x53445853   // "SXDS": header word 2 of a row that has been saved
#define SDX_ST_THREADS 256
#define SDX_ST_INFLIGHT 4         // 16-byte loads a lane issues before its first store
#define SDX_ST_NGLOB 6
enum { SDX_ST_SAVE = 0, SDX_ST_RESTORE = 1, SDX_ST_CLONE = 2 };

// One per-env buffer: env e owns bytes [e * stride, e * stride + bytes) of base.  In a snapshot row the segment has the slot
// [off, off + round16(bytes) + 16): its bytes start at off + phase, phase = (e * stride) % 16 of the env the row came from.  Strides are
// multiples of 4 only (rb 8 580 B, root 7 384 B), so the phase depends on e % 4 - the same for every env of one class (e & 7) - and a 16-byte
// piece of the slot is 16-byte aligned on the env side too.
struct SdxStateSeg {
  char* base;
  uint32_t stride;
  uint32_t bytes;
  uint32_t off;      // multiple of 16; slots ascend in the table
  uint32_t warm;     // != 0: only the first wcount[e] 4-byte entries are state (a row of the warm-start cache)
};
struct SdxStateTab {
  int32_t nseg, N, var3, nunits;     // var3: the class is additionally env % 3 (InsertSim's base plate); nunits = row_bytes / 16
  uint32_t row_bytes, pad;
  int32_t* wcount;                   // SdxBuf.wcount: travels in the row header
  int32_t* stats;                    // [3] skipped entries: out of range, class mismatch, row never saved
  const uint8_t* unit_seg;           // [nunits] segment of each 16-byte piece of a row (255: the header)
  char* glob[SDX_ST_NGLOB];          // the global part (save_all / restore_all): step_count, stat, cons, dr_grav, dr_frame, dr_draw[N]
  uint32_t glob_bytes[SDX_ST_NGLOB];
  SdxStateSeg seg[SDX_ST_MAXSEG];
};

__device__ __forceinline__ int sdx_state_class(int e, int var3) { return (e & 7) + (var3 ? 8 * (e % 3) : 0); }

typedef uint32_t sdx_u4 __attribute__((vector_size(16)));   // one 128-bit access (a struct of four words is copied through memory)

// every buffer the kernel moves is global memory: saying so gives global_load / global_store instead of flat accesses (g++ has no address spaces)
#ifdef HIPEMU
#define SDX_ST_GLOBAL
#else
#define SDX_ST_GLOBAL __attribute__((address_space(1)))
#endif
typedef const SDX_ST_GLOBAL sdx_u4* sdx_st_ld4;
typedef SDX_ST_GLOBAL sdx_u4* sdx_st_st4;
typedef const SDX_ST_GLOBAL uint32_t* sdx_st_ld1;
typedef SDX_ST_GLOBAL uint32_t* sdx_st_st1;

// One 16-byte piece of a row slot: nb of its bytes are state (16: a whole piece, aligned on both sides; 4..12: the head or tail of a segment)
struct SdxStatePiece { const char* s; char* d; int nb; };
struct SdxStatePieceCtx {
  const SdxStateSeg* seg;
  int nseg, env, count, src, dst;
  const char* src_row;   // the source row, or nullptr when the source is an env
  char* dst_row;
};
__device__ __forceinline__ SdxStatePiece sdx_state_piece(const SdxStatePieceCtx& cx, int u, int si) {
  const bool valid = si < cx.nseg;
  const SdxStateSeg sg = cx.seg[valid ? si : 0];
  const int phase = (int)(((uint32_t)cx.env * sg.stride) & 15u);
  int eff = (int)sg.bytes;
  if (sg.warm && cx.count * 4 < eff) eff = cx.count * 4;
  const int rel = u * 16 - (int)sg.off;       // of this piece inside the slot
  int lo = rel - phase, hi = lo + 16;         // env-side bytes it holds
  lo = lo < 0 ? 0 : lo;
  hi = hi > eff ? eff : hi;
  const size_t in_row = (size_t)sg.off + (size_t)(phase + lo);
  SdxStatePiece p;
  p.nb = valid && hi > lo ? hi - lo : 0;
  p.s = cx.src_row ? cx.src_row + in_row : sg.base + (size_t)cx.src * sg.stride + lo;
  p.d = cx.dst_row ? cx.dst_row + in_row : sg.base + (size_t)cx.dst * sg.stride + lo;
  return p;
}
// heads and tails, up to three 4-byte words: all loads (a lane without the word reads `spare`), then the stores
struct SdxStateWords { uint32_t w0, w1, w2; };
__device__ __forceinline__ SdxStateWords sdx_state_words_load(const SdxStatePiece& p, const char* spare) {
  const bool part = p.nb > 0 && p.nb < 16;
  SdxStateWords r;
  r.w0 = *(sdx_st_ld1)(part ? p.s : spare);
  r.w1 = *(sdx_st_ld1)(part && p.nb > 4 ? p.s + 4 : spare);
  r.w2 = *(sdx_st_ld1)(part && p.nb > 8 ? p.s + 8 : spare);
  return r;
}
__device__ __forceinline__ void sdx_state_words_store(const SdxStatePiece& p, const SdxStateWords& r) {
  if (p.nb > 0 && p.nb < 16) {
    *(sdx_st_st1)p.d = r.w0;
    if (p.nb > 4) *(sdx_st_st1)(p.d + 4) = r.w1;
    if (p.nb > 8) *(sdx_st_st1)(p.d + 8) = r.w2;
  }
}

// grid: (items + with_glob) x parts workgroups; item i moves a[i] -> b[i] (a / b nullptr: i).  save: a env, b row; restore: a row, b env;
// clone: a source env, b destination env.  T is the table of the simulator whose envs are touched; rows / nrows / glob the snapshot's.
__global__ __launch_bounds__(SDX_ST_THREADS) void k_state_copy(const SdxStateTab* __restrict__ T, int mode, char* rows, int nrows, char* glob,
                                                               const int32_t* __restrict__ a_ids, const int32_t* __restrict__ b_ids, int n, int parts) {
  __shared__ SdxStateSeg s_seg[SDX_ST_MAXSEG];
  const int tid = threadIdx.x;
  const int item = blockIdx.x / parts, part = blockIdx.x % parts;
  if (item >= n) {   // the global part
    if (part == 0 && tid < SDX_ST_NGLOB * 4) {
      const int g = tid >> 2, w = tid & 3;
      if ((uint32_t)w * 4 < T->glob_bytes[g]) {
        uint32_t* env_side = (uint32_t*)T->glob[g] + w;
        uint32_t* snap_side = (uint32_t*)(glob + g * 16) + w;
        if (mode == SDX_ST_SAVE) *snap_side = *env_side; else *env_side = *snap_side;
      }
    }
    return;
  }
  const int a = a_ids ? a_ids[item] : item, b = b_ids ? b_ids[item] : item;
  const int N = T->N, var3 = T->var3;
  const size_t row_bytes = T->row_bytes;
  int src, dst, count, bad = -1;   // src / dst: env or row index of either side
  if (mode == SDX_ST_SAVE) {
    src = a; dst = b;
    if (a < 0 || a >= N || b < 0 || b >= nrows) bad = 0;
  } else if (mode == SDX_ST_RESTORE) {
    src = a; dst = b;
    if (a < 0 || a >= nrows || b < 0 || b >= N) bad = 0;
    else {
      const int32_t* hdr = (const int32_t*)(rows + (size_t)a * row_bytes);
      if (hdr[2] != SDX_ST_MAGIC) bad = 2;
      else if (sdx_state_class(hdr[0], var3) != sdx_state_class(b, var3)) bad = 1;
    }
  } else {
    src = a; dst = b;
    if (a < 0 || a >= N || b < 0 || b >= N) bad = 0;
    else if (sdx_state_class(a, var3) != sdx_state_class(b, var3)) bad = 1;
  }
  if (bad >= 0) {   // skipped and counted, never a fault
    if (part == 0 && tid == 0) atomicAdd(&T->stats[bad], 1);
    return;
  }
  const int env = mode == SDX_ST_RESTORE ? dst : src;   // the env whose alignment phases the row has (restore: equal by class)
  count = mode == SDX_ST_RESTORE ? ((const int32_t*)(rows + (size_t)src * row_bytes))[1] : T->wcount[src];
  count = count < 0 ? 0 : (count > SDX_MAXC ? SDX_MAXC : count);
  const int nseg = T->nseg;
  for (int i = tid; i < nseg; i += SDX_ST_THREADS) s_seg[i] = T->seg[i];
  __syncthreads();
  if (part == 0 && tid == 0) {   // the row header / the destination's warm count
    if (mode == SDX_ST_SAVE) {
      int32_t* hdr = (int32_t*)(rows + (size_t)dst * row_bytes);
      hdr[0] = src; hdr[1] = count; hdr[2] = SDX_ST_MAGIC; hdr[3] = 0;
    } else {
      T->wcount[dst] = count;
    }
  }
  const bool src_row = mode == SDX_ST_RESTORE, dst_row = mode == SDX_ST_SAVE;
  const char* src_row_p = rows + (size_t)(src_row ? src : 0) * row_bytes;
  char* dst_row_p = rows + (size_t)(dst_row ? dst : 0) * row_bytes;
  const int nunits = T->nunits;
  const SDX_ST_GLOBAL uint8_t* unit_seg = (const SDX_ST_GLOBAL uint8_t*)T->unit_seg;
  const SdxStatePieceCtx cx = {s_seg, nseg, env, count, src, dst, src_row ? src_row_p : nullptr, dst_row ? dst_row_p : nullptr};
  const char* const spare = (const char*)T;   // 16 readable, aligned bytes: what a lane without a whole piece loads, so that no load is branched around
  for (int u0 = part * (SDX_ST_THREADS * SDX_ST_INFLIGHT) + tid; u0 - tid < nunits; u0 += parts * (SDX_ST_THREADS * SDX_ST_INFLIGHT)) {
    const int u1 = u0 + SDX_ST_THREADS, u2 = u0 + 2 * SDX_ST_THREADS, u3 = u0 + 3 * SDX_ST_THREADS;
    const int i0 = u0 < nunits ? (int)unit_seg[u0] : 255, i1 = u1 < nunits ? (int)unit_seg[u1] : 255;
    const int i2 = u2 < nunits ? (int)unit_seg[u2] : 255, i3 = u3 < nunits ? (int)unit_seg[u3] : 255;
    const SdxStatePiece p0 = sdx_state_piece(cx, u0, i0), p1 = sdx_state_piece(cx, u1, i1), p2 = sdx_state_piece(cx, u2, i2),
                        p3 = sdx_state_piece(cx, u3, i3);
    // four 16-byte loads in flight per lane before the first store
    const sdx_u4 v0 = *(sdx_st_ld4)(p0.nb == 16 ? p0.s : spare), v1 = *(sdx_st_ld4)(p1.nb == 16 ? p1.s : spare);
    const sdx_u4 v2 = *(sdx_st_ld4)(p2.nb == 16 ? p2.s : spare), v3 = *(sdx_st_ld4)(p3.nb == 16 ? p3.s : spare);
    if (p0.nb == 16) *(sdx_st_st4)p0.d = v0;
    if (p1.nb == 16) *(sdx_st_st4)p1.d = v1;
    if (p2.nb == 16) *(sdx_st_st4)p2.d = v2;
    if (p3.nb == 16) *(sdx_st_st4)p3.d = v3;
    if (((p0.nb | p1.nb | p2.nb | p3.nb) & 12) != 0) {   // some piece of this lane is a head or a tail (a few dozen of a row's 4 000)
      const SdxStateWords w0 = sdx_state_words_load(p0, spare), w1 = sdx_state_words_load(p1, spare), w2 = sdx_state_words_load(p2, spare),
                          w3 = sdx_state_words_load(p3, spare);
      sdx_state_words_store(p0, w0); sdx_state_words_store(p1, w1); sdx_state_words_store(p2, w2); sdx_state_words_store(p3, w3);
    }
  }
}

// host: appends a segment to the table (row offsets are assigned in order)
static inline bool sdx_state_add(SdxStateTab* T, void* base, size_t stride, size_t bytes, int warm) {
  if (T->nseg >= SDX_ST_MAXSEG || !base || bytes == 0 || (bytes & 3) || (stride & 3) || ((uintptr_t)base & 15)) return false;
  SdxStateSeg& s = T->seg[T->nseg++];
  s.base = (char*)base;
  s.stride = (uint32_t)stride;
  s.bytes = (uint32_t)bytes;
  s.off = T->row_bytes;
  s.warm = (uint32_t)warm;
  T->row_bytes += (uint32_t)((bytes + 15) & ~(size_t)15) + 16;
  return true;
}

static inline void sdx_state_launch(const SdxStateTab* d_tab, int mode, char* rows, int nrows, char* glob, const int32_t* a_ids,
                                    const int32_t* b_ids, int n, int with_glob, hipStream_t st) {
  // a workgroup moves 256 x 4 pieces of 16 bytes per pass; 4 workgroups per row = one or two passes each for the 65 - 100 KB rows
  const int parts = 4;
  hipLaunchKernelGGL(k_state_copy, dim3((unsigned)(n + (with_glob ? 1 : 0)) * parts), dim3(SDX_ST_THREADS), 0, st, d_tab, mode, rows, nrows, glob,
                     a_ids, b_ids, n, parts);
}
