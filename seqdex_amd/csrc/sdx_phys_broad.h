// sdx_phys_broad.h - private to sdx_physics.hip (included by it only, in its fixed order): block scan, candidate tests and the broadphase mask
#pragma once

__device__ __forceinline__ void tri_index(int idx, int* i, int* j) {   // idx -> (i, j), j <= i, row-major lower triangle
  int r = (int)((SDX_SQRT_FAST(8.0f * (float)idx + 1.0f) - 1.0f) * 0.5f);   // within one of the exact row: two branch-free corrections
  r += (r + 1) * (r + 2) / 2 <= idx;
  r -= r * (r + 1) / 2 > idx;
  *i = r;
  *j = idx - r * (r + 1) / 2;
}

// ---------------------------------------------------------------- block-level exclusive scan of a small count k (NBITS bits), thread order
template <int NT, int NBITS = 4>
__device__ __forceinline__ int block_scan_small(PhysLds& S, int k, int tid, int* total) {
  constexpr int NW = NT / 64;
  const int lane = tid & 63, wave = tid >> 6;
  const uint64_t lt = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
  int pre = 0, wt = 0;
#pragma unroll
  for (int b = 0; b < NBITS; ++b) {
    const uint64_t bal = __ballot((k >> b) & 1);
    pre += __popcll(bal & lt) << b;
    wt += __popcll(bal) << b;
  }
  if (lane == 0) S.wsum[wave] = wt;
  __syncthreads();
  int off = 0, tot = 0;
#pragma unroll
  for (int w = 0; w < NW; ++w) { const int c = S.wsum[w]; if (w < wave) off += c; tot += c; }
  __syncthreads();
  *total = tot;
  return off + pre;
}

// ---------------------------------------------------------------- D: contacts
// candidate test of pair index idx in the fixed enumeration (brick/static, brick/brick i < j, then per robot box: bricks, statics).
// Conservative: a pair can only produce a contact when a sample point of one box lies within `off` of the other box, and the SDF is
// 1-Lipschitz, so |sdf_B(centre of A)| <= radius_A + off (or the same with A and B exchanged) must hold.
__device__ __forceinline__ bool box_near(const PhysLds& S, f3 ca, float ra, f3 cb, f4 qb, f3 hb, float off) {
  return box_sdf_val(qrot(qconj(qb), ca - cb), hb) <= ra + off;
}
// pair index -> (box a | box b << 8); box ids: 0..71 brick, 72..111 robot box, 128.. static body
// (ns, per are compile-time constants at the call sites - the enumeration runs over all SDX_MAX_STATIC slots, unused ones never are
// candidates - so that the divisions below are multiplications: a division by a run-time integer is ~30 instructions, twice per candidate)
__device__ __forceinline__ uint32_t pair_code(int idx, int n1, int n2, int ns, int per) {
  if (idx < n1) return (uint32_t)(idx / ns) | ((uint32_t)(STATIC0 + idx % ns) << 8);
  if (idx < n1 + n2) {
    int i, j;
    tri_index(idx - n1, &i, &j);   // lower triangle without the diagonal: bricks (j, i + 1), j <= i
    return (uint32_t)j | ((uint32_t)(i + 1) << 8);
  }
  const int t = idx - n1 - n2, r = t / per, u = t % per;
  return (uint32_t)(RBOX0 + r) | ((uint32_t)(u < NF ? u : STATIC0 + u - NF) << 8);
}
// (bricks: sphere of radius trad about the centre of mass - it contains the bounding box, whose centre lies a few millimetres off)
__device__ __forceinline__ bool brick_near(const PhysLds& S, f3 ca, float ra, int j, float off) {   // centre / radius against brick j's bounding box
  const f4 qj = ld4(S.bq[j]);
  const int tj = S.btype[j];
  return box_sdf_val(qrot(qconj(qj), ca - ld3(S.bp[j])) - ld3(S.tbc[tj]), ld3(S.tbh[tj])) <= ra + off;
}
__device__ __forceinline__ bool candidate(const PhysLds& S, int idx, int n1, int n2, int ns, int per, int ns_used, float off) {
  if (idx < n1) {
    const int i = idx / ns, st = idx % ns;
    if (st >= ns_used) return false;
    return box_sdf_val(ld3(S.bp[i]) - ld3(S.stc[st]), ld3(S.sth[st])) <= S.trad[S.btype[i]] + off;
  }
  if (idx < n1 + n2) {
    int i, j;
    tri_index(idx - n1, &i, &j);
    i += 1;
    const f3 ci = ld3(S.bp[i]), cj = ld3(S.bp[j]);
    const f3 d = ci - cj;
    const float ri = S.trad[S.btype[i]], rj = S.trad[S.btype[j]];
    const float rr = ri + rj + off;
    if (dot(d, d) > rr * rr) return false;
    return brick_near(S, ci, ri, j, off) || brick_near(S, cj, rj, i, off);
  }
  const int t = idx - n1 - n2, r = t / per, u = t % per;
  if (S.rbl[r] == 0) return false;   // the fixed base never generates contacts
  const f3 rc = ld3(S.rc[r]);
  const float rr0 = S.rrad[r];
  if (u < NF) {
    const f3 cb = ld3(S.bp[u]);
    const f3 d = rc - cb;
    const float rb = S.trad[S.btype[u]];
    const float rr = rr0 + rb + off;
    if (dot(d, d) > rr * rr) return false;
    return brick_near(S, rc, rr0, u, off) || box_near(S, cb, rb, rc, ld4(S.rq[r]), ld3(S.rh[r]), off);
  }
  const int st = u - NF;
  if (st >= ns_used) return false;
  return box_sdf_val(rc - ld3(S.stc[st]), ld3(S.sth[st])) <= rr0 + off;
}

// part 0: candidates [0, n1 + n2) - bricks against static bodies and against each other, which need nothing of this substep's robot
// state; part 1: [n1 + n2, ntot) - the robot boxes, after the forward kinematics.  Lanes 64.. of the block share a part's candidates
// (stride NT - 64) and set bit idx / NT of word idx % NT for a hit (integer atomics on a word that is zero between substeps).
template <int NT>
__device__ __forceinline__ void broad_mask_part(const SdxConst* C, PhysLds& S, int tid, int part) {
  const sdx_scene_desc& sc = C->sc;
  constexpr int ns = SDX_MAX_STATIC, per = NF + SDX_MAX_STATIC;
  constexpr int n1 = NF * ns, n2 = NF * (NF - 1) / 2;
  const int ntot = n1 + n2 + sc.n_rbox * per;
  const int lo = part == 0 ? 0 : n1 + n2, hi = part == 0 ? n1 + n2 : ntot;
#pragma unroll 1
  for (int idx = lo + tid - 64; idx < hi; idx += NT - 64)
    if (candidate(S, idx, n1, n2, ns, per, sc.n_static, sc.contact_offset)) atomicOr(&S_BMASK(S)[idx % NT], 1u << (idx / NT));
}
