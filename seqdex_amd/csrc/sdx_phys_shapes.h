// sdx_phys_shapes.h - private to sdx_physics.hip (included by it only, in its fixed order): signed distance of a box, compound shapes, the contact manifold of a pair of boxes
#pragma once

__device__ __forceinline__ float box_sdf(f3 p, f3 h, f3* g) {
  f3 d = F3(fabsf(p.x) - h.x, fabsf(p.y) - h.y, fabsf(p.z) - h.z);
  f3 s = F3(p.x < 0 ? -1.0f : 1.0f, p.y < 0 ? -1.0f : 1.0f, p.z < 0 ? -1.0f : 1.0f);
  float mx = fmaxf(d.x, fmaxf(d.y, d.z));
  if (mx <= 0) {
    if (d.x >= d.y && d.x >= d.z) *g = F3(s.x, 0, 0);
    else if (d.y >= d.z) *g = F3(0, s.y, 0);
    else *g = F3(0, 0, s.z);
    return mx;
  }
  f3 o = F3(fmaxf(d.x, 0.0f), fmaxf(d.y, 0.0f), fmaxf(d.z, 0.0f));
  float len = sqrtf(dot(o, o));
  *g = F3(s.x * o.x / len, s.y * o.y / len, s.z * o.z / len);
  return len;
}
__device__ __forceinline__ float box_sdf_val(f3 p, f3 h) {
  f3 d = F3(fabsf(p.x) - h.x, fabsf(p.y) - h.y, fabsf(p.z) - h.z);
  float mx = fmaxf(d.x, fmaxf(d.y, d.z));
  if (mx <= 0) return mx;
  f3 o = F3(fmaxf(d.x, 0.0f), fmaxf(d.y, 0.0f), fmaxf(d.z, 0.0f));
  return sqrtf(dot(o, o));
}

// orthonormal tangents of a unit normal without a square root or a branch (Duff et al. 2017); n = (0, 0, +-1) gives t1 = (+-1, 0, 0)... the
// friction pyramid's axes are the world's x and y for a vertical normal.  Recomputed in every solver iteration (12 instructions; the round-2
// construction - cross product with the least-aligned axis, normalised - cost 40).  oracle: tangents()
__device__ __forceinline__ void tangents(f3 n, f3* t1, f3* t2) {
  const float sg = n.z < 0.0f ? -1.0f : 1.0f;
  const float a = -1.0f / (sg + n.z);
  const float b = n.x * n.y * a;
  *t1 = F3(1.0f + sg * n.x * n.x * a, sg * b, -sg * n.x);
  *t2 = F3(b, sg + n.y * n.y * a, -n.y);
}

// ---- shapes.  Box id: 0..71 brick, 72..111 robot box, 128..135 static body; a brick and a static body are COMPOUNDS of boxes (sub index),
// a robot box is one box.  load_bound: the bounding box of a body (broadphase, first separating-axis pass); load_box2: one box of each body of a pair.
#define RBOX0 NF
#define STATIC0 128
static_assert(RBOX0 + SDX_MAX_RBOX <= STATIC0 && STATIC0 + SDX_MAX_STATIC <= 256, "box ids fit 8 bits (7 for the first box of a pair)");
__device__ __forceinline__ bool brick_hollow(const PhysLds& S, int i) { return S.hn > 0 && i == S.seg_brick; }
__device__ __forceinline__ int box_nsub(const PhysLds& S, int id) {
  if (id < NF) return brick_hollow(S, id) ? S.hn : S.tn[S.btype[id]];
  if (id < STATIC0) return 1;
  return S.ssn[id - STATIC0];
}
__device__ __forceinline__ Box load_bound(const PhysLds& S, int id) {
  Box b;
  if (id < NF) {
    const int t = S.btype[id];
    b.q = ld4(S.bq[id]); b.c = ld3(S.bp[id]) + qrot(b.q, ld3(S.tbc[t])); b.h = ld3(S.tbh[t]);
  } else if (id < STATIC0) {
    const int r = id - RBOX0;
    b.c = ld3(S.rc[r]); b.q = ld4(S.rq[r]); b.h = ld3(S.rh[r]);
  } else {
    const int st = id - STATIC0;
    b.c = ld3(S.stc[st]); b.h = ld3(S.sth[st]); b.q.x = 0; b.q.y = 0; b.q.z = 0; b.q.w = 1;
  }
  return b;
}
// Both boxes of a pair with TWO LDS round trips (round 6).  One box at a time (a brick: orientation, position, type -> compound row; a
// robot box: its world rows; a static body: its row, or a row of the HBM table for a compound) compiled to a chain of about ten: type ->
// compound table -> rows, one box after the other, each class of box in its own branch.  Here the rows every class needs are addressed without branches
// (orientation, position, half extents come from the brick / robot-box / static tables by pointer selection; a static body reads the
// identity row S.qid), all of them for both boxes are in flight together, then the bricks' compound rows (which depend on the type) for both.
// A brick's box: centre = position + R x (compound row - centre of mass), half extents = the compound row.  A box of a static COMPOUND
// (the studded base plate, HBM table) is the slow path behind a branch, as before.
__device__ __forceinline__ void load_box2(const SdxConst* C, const PhysLds& S, int ida, int suba, int idb, int subb, Box* A, Box* B) {
  const int id_[2] = {ida, idb}, sub_[2] = {suba, subb};
  f4 q_[2];
  f3 p_[2], h_[2];
  int t_[2], sn_[2], sf_[2];
  const bool hol_any = S.hn > 0;
  const int segb = S.seg_brick;
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int id = id_[k];
    const bool brick = id < NF, rob = !brick && id < STATIC0;
    const int r = rob ? id - RBOX0 : 0, st = (!brick && !rob) ? id - STATIC0 : 0, ib = brick ? id : 0;
    const float* qp = brick ? S.bq[ib] : (rob ? S.rq[r] : S.qid);
    const float* pp = brick ? S.bp[ib] : (rob ? S.rc[r] : S.stc[st]);
    const float* hp = rob ? S.rh[r] : S.sth[st];
    q_[k] = ld4(qp); p_[k] = ld3(pp); h_[k] = ld3(hp);
    t_[k] = S.btype[ib]; sn_[k] = S.ssn[st]; sf_[k] = S.ssf[st];
  }
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    SDX_PIN1(q_[k].x); SDX_PIN1(q_[k].y); SDX_PIN1(q_[k].z); SDX_PIN1(q_[k].w); SDX_PIN3(p_[k]); SDX_PIN3(h_[k]);
    SDX_PIN1(t_[k]); SDX_PIN1(sn_[k]); SDX_PIN1(sf_[k]);
  }
  f3 o_[2], hb_[2];
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const bool hol = hol_any && id_[k] == segb;
    const int sb = id_[k] < NF ? sub_[k] : 0;
    o_[k] = ld3(hol ? S.hsc[sb] : S.tsc[t_[k]][sb]);
    hb_[k] = ld3(hol ? S.hsh[sb] : S.tsh[t_[k]][sb]);
  }
  SDX_PIN3x4(o_[0], hb_[0], o_[1], hb_[1]);
  Box* out_[2] = {A, B};
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int id = id_[k];
    Box b;
    b.q = q_[k];
    if (id < NF) { b.c = p_[k] + qrot(q_[k], o_[k]); b.h = hb_[k]; }
    else { b.c = p_[k]; b.h = h_[k]; }
    if (id >= STATIC0 && sn_[k] > 1) {
      const int r = sf_[k] + sub_[k];
      b.c = ld3(C->sc.static_sub_center[r]); b.h = ld3(C->sc.static_sub_half[r]);
    }
    *out_[k] = b;
  }
}
__device__ __forceinline__ int box_body(const PhysLds& S, int id) {
  if (id < NF) return id;
  if (id < STATIC0) return NF + S.rbl[id - RBOX0];
  return BODY_W;
}
// the second direction of a pair (samples of B against A) exists unless B is the body box of a static (the studs
// of a static compound, boxes 1.., are sampled like a brick's boxes)
__device__ __forceinline__ bool samples_b(int bid, int bsub) { return bid < STATIC0 || bsub > 0; }

// ---- contact manifold of one direction (samples of A against box B); oracle: dir_setup / sample_contact
// Reference face = the face axis of B with the smallest overlap of the two boxes' extents (separating-axis test over B's three face
// normals), on A's side of B's centre.  Samples whose projection falls on that face (within FACE_TOL of its outline) are FACE samples:
// normal = face normal, separation along it; the others use their own signed distance to B.  <= 4 samples per direction: face samples
// in table order first, then the others.  Shallow overlaps only (s_k >= -FACE_DEPTH x contact offset): a deeply interpenetrating pair
// has no meaningful meeting face (kax = -1) and every sample keeps its own signed distance.
#define FACE_TOL 1e-4f
#define FACE_DEPTH 4.0f
#define WARM_SPEED 0.25f   // m/s
#define WARM_DEPTH 1.5f    // contact offsets
struct Dir { f3 t, ex, ey, ez; int kax; float sgn, smax; };   // ex, ey, ez: A's half edges in B's frame: sample = t + sx ex + sy ey + sz ez
__device__ __forceinline__ Dir dir_setup(const Box& A, const Box& B, float off) {
  Dir D;
  const f4 qbi = qconj(B.q);
  D.t = qrot(qbi, A.c - B.c);
  const f4 qrel = qmul(qbi, A.q);
  D.ex = qrot(qrel, F3(A.h.x, 0, 0));
  D.ey = qrot(qrel, F3(0, A.h.y, 0));
  D.ez = qrot(qrel, F3(0, 0, A.h.z));
  const f3 ex = D.ex, ey = D.ey, ez = D.ez;
  const float sx = fabsf(D.t.x) - B.h.x - (fabsf(ex.x) + fabsf(ey.x) + fabsf(ez.x));
  const float sy = fabsf(D.t.y) - B.h.y - (fabsf(ex.y) + fabsf(ey.y) + fabsf(ez.y));
  const float sz = fabsf(D.t.z) - B.h.z - (fabsf(ex.z) + fabsf(ey.z) + fabsf(ez.z));
  if (sx >= sy && sx >= sz) { D.kax = 0; D.sgn = D.t.x < 0 ? -1.0f : 1.0f; }
  else if (sy >= sz) { D.kax = 1; D.sgn = D.t.y < 0 ? -1.0f : 1.0f; }
  else { D.kax = 2; D.sgn = D.t.z < 0 ? -1.0f : 1.0f; }
  D.smax = fmaxf(sx, fmaxf(sy, sz));   // >= off: a face axis of B separates the boxes by the whole contact offset, no sample can be inside it
  if (D.smax < -FACE_DEPTH * off) D.kax = -1;
  return D;
}
__device__ __forceinline__ float sample_contact(const Dir& D, f3 pb, f3 h, f3* g) {
  const f3 d = F3(fabsf(pb.x) - h.x, fabsf(pb.y) - h.y, fabsf(pb.z) - h.z);
  const float lat = D.kax == 0 ? fmaxf(d.y, d.z) : D.kax == 1 ? fmaxf(d.x, d.z) : fmaxf(d.x, d.y);
  if (D.kax >= 0 && lat <= FACE_TOL) {
    const float pk = D.kax == 0 ? pb.x : D.kax == 1 ? pb.y : pb.z, hk = D.kax == 0 ? h.x : D.kax == 1 ? h.y : h.z;
    *g = F3(D.kax == 0 ? D.sgn : 0.0f, D.kax == 1 ? D.sgn : 0.0f, D.kax == 2 ? D.sgn : 0.0f);
    return D.sgn * pk - hk;
  }
  return box_sdf(pb, h, g);
}

constexpr float kSamp[SDX_NSAMP][3] = {   // c_samp as compile-time constants: immediates of the fully unrolled classification loop
    {1, 1, 1}, {1, -1, -1}, {-1, 1, -1}, {-1, -1, 1}, {-1, -1, -1}, {-1, 1, 1}, {1, -1, 1}, {1, 1, -1},
    {0, -1, -1}, {0, 1, -1}, {0, -1, 1}, {0, 1, 1}, {-1, 0, -1}, {1, 0, -1}, {-1, 0, 1}, {1, 0, 1},
    {-1, -1, 0}, {1, -1, 0}, {-1, 1, 0}, {1, 1, 0},
    {-0.5f, -1, -1}, {0.5f, -1, -1}, {-0.5f, 1, -1}, {0.5f, 1, -1}, {-0.5f, -1, 1}, {0.5f, -1, 1}, {-0.5f, 1, 1}, {0.5f, 1, 1}};
__device__ __forceinline__ f3 face_frame(f3 v, int kax) {   // component kax moves to z
  return kax == 0 ? F3(v.y, v.z, v.x) : kax == 1 ? F3(v.x, v.z, v.y) : v;
}
// ---- the <= 4 contacts of a pair of boxes (oracle: collide_pair).  classify_dir: the 28 samples of box A against box
// T in the face frame of that direction -> face samples / other samples inside `incl` as bit masks (incl: the contact offset, or 0 when
// the list is rebuilt after a capacity overflow).  Direction 1 also returns what the selection below needs to place a sample in the
// PAIR's reference frame: the reference axis kref and the face-frame rows (x, y) of the sample basis.
struct FaceBasis { float tx, ty, exx, exy, eyx, eyy, ezx, ezy; };
template <bool DIR2>
__device__ __forceinline__ bool classify_dir(const PhysLds& S, const Box& A, const Box& T, float off, float incl, int* kref, FaceBasis* fb,
                                             uint32_t* mface_out, uint32_t* mother_out) {
  const Dir D = dir_setup(A, T, off);
  if (D.smax >= incl) return false;   // separated: no sample of either direction can be inside the threshold
  const f3 t = face_frame(D.t, D.kax), ex = face_frame(D.ex, D.kax), ey = face_frame(D.ey, D.kax), ez = face_frame(D.ez, D.kax);
  if (!DIR2) {
    *kref = D.kax >= 0 ? D.kax : 2;
    fb->tx = t.x; fb->ty = t.y; fb->exx = ex.x; fb->exy = ex.y; fb->eyx = ey.x; fb->eyy = ey.y; fb->ezx = ez.x; fb->ezy = ez.y;
  }
  const f3 h = face_frame(T.h, D.kax);
  const float ftol = D.kax >= 0 ? FACE_TOL : -1e30f, off2 = incl * incl;
  uint32_t mface = 0, mother = 0;
  // Fully unrolled with the table entries as immediates: 18 instructions per sample (rolled four at a time with the entries from
  // scalar loads: 56, and this loop is VALU-issue bound: 30 k cycles per chunk of 512 box pairs against 11 k).  The loop body must stay
  // this small: with the running extremes of an earlier manifold rule inside it the two unrolled instances cost the WHOLE kernel 220
  // spilled VGPRs, 18 scratch operations inside the solver's iteration loop among them; as it is: 24 spills, none in a loop
  // (python tools/isa_check.py; -DSDX_CLASSIFY_UNROLL=4 is the rolled form)
#ifndef SDX_CLASSIFY_UNROLL
#define SDX_CLASSIFY_UNROLL SDX_NSAMP
#endif
  constexpr int CU = SDX_CLASSIFY_UNROLL;
#pragma unroll CU
  for (int s = 0; s < SDX_NSAMP; ++s) {
    const float k0 = CU == SDX_NSAMP ? kSamp[s][0] : c_samp[s][0], k1 = CU == SDX_NSAMP ? kSamp[s][1] : c_samp[s][1], k2 = CU == SDX_NSAMP ? kSamp[s][2] : c_samp[s][2];
    const f3 pb = ((t + ex * k0) + ey * k1) + ez * k2;
    const float dx = fabsf(pb.x) - h.x, dy = fabsf(pb.y) - h.y, dz = fabsf(pb.z) - h.z;
    const float lat = fmaxf(dx, dy);
    const float sdf = D.sgn * pb.z - h.z;
    const float ox = fmaxf(dx, 0.0f), oy = fmaxf(dy, 0.0f), oz = fmaxf(dz, 0.0f);
    const bool near = fmaxf(lat, dz) <= 0.0f || ox * ox + oy * oy + oz * oz < off2;
    const bool face = lat <= ftol;
    if (face && sdf < incl) mface |= 1u << s;
    if (!face && near) mother |= 1u << s;
  }
  *mface_out = mface;
  *mother_out = mother;
  return true;
}
// The 4 slots of the pair.  Face samples first, chosen to SPAN the patch the boxes meet on: every face sample has lateral coordinates
// (a, b) in B's frame (B's axes without the axis kref of direction 1's reference face; a sample of B: its own table entry x hB);
// p1 = the sample furthest along (1, 0.1), p2 = the one furthest from p1, p3 / p4 = the ones furthest to the left / right of the line
// p1 p2; ties: the first in enumeration order (direction 1 in table order, then direction 2) - a later candidate replaces the incumbent
// only when it beats it by more than MANIFOLD_TIE_L (1 um, p1's score) / MANIFOLD_TIE_A (1e-8 m^2, squared distance and line offset): samples
// of one box edge are all equally far from a line parallel to it, and coincident samples of the two directions score the same, so that
// without the margin rounding decides (seen on the device: one such pair per 8 golden envs chose another sample than the oracle, and
// 16 Jacobi iterations spread that over eight bricks).  Then the remaining face samples in that
// order, then the other samples (edge / corner regions, speculative contacts) the same way.  Returns the number of contacts; sel1 / sel2:
// the chosen samples of the two directions.
#define MANIFOLD_EPS 1e-7f
#define MANIFOLD_TIE_L 1e-6f
#define MANIFOLD_TIE_A 1e-8f
__device__ __forceinline__ int pair_contacts(const PhysLds& S, const Box& A, const Box& B, bool second, float off, float incl, uint32_t* sel1, uint32_t* sel2) {
  uint32_t f1 = 0, o1 = 0, f2 = 0, o2 = 0;
  int kref = 2;
  FaceBasis fb;
  *sel1 = 0; *sel2 = 0;
  if (!classify_dir<false>(S, A, B, off, incl, &kref, &fb, &f1, &o1)) return 0;
  if (second && !classify_dir<true>(S, B, A, off, incl, &kref, &fb, &f2, &o2)) return 0;
  uint32_t s1 = 0, s2 = 0;
  int n = 0;
  const uint64_t fm = (uint64_t)f1 | ((uint64_t)f2 << 32);
  if (fm) {
    const float ha = kref == 0 ? B.h.y : B.h.x, hb = kref == 2 ? B.h.y : B.h.z;
    // (a, b) of candidate id (direction << 5 | sample); the table entries come from the LDS copy of the sample table (per-lane index)
#define SDX_COORDS(id, a, b)                                                                                    \
    {                                                                                                           \
      const float* ks = S.samp[(id) & 31];                                                                      \
      const float kx = ks[0], ky = ks[1], kz = ks[2];                                                           \
      if ((id) < 32) { a = ((fb.tx + fb.exx * kx) + fb.eyx * ky) + fb.ezx * kz; b = ((fb.ty + fb.exy * kx) + fb.eyy * ky) + fb.ezy * kz; } \
      else { a = (kref == 0 ? ky : kx) * ha; b = (kref == 2 ? ky : kz) * hb; }                                  \
    }
    int p1 = -1, p2 = -1, p3 = -1, p4 = -1;
    float a1 = 0.0f, b1 = 0.0f, a2 = 0.0f, b2 = 0.0f, best = -1e30f;
    uint64_t m = fm;
#pragma unroll 1
    while (m) {
      const int id = __ffsll((unsigned long long)m) - 1;
      m &= m - 1;
      float a, b;
      SDX_COORDS(id, a, b)
      const float k = a + 0.1f * b;
      if (k > best + MANIFOLD_TIE_L) { best = k; p1 = id; a1 = a; b1 = b; }
    }
    best = 0.0f;
    m = fm;
#pragma unroll 1
    while (m) {
      const int id = __ffsll((unsigned long long)m) - 1;
      m &= m - 1;
      float a, b;
      SDX_COORDS(id, a, b)
      const float k = (a - a1) * (a - a1) + (b - b1) * (b - b1);
      if (k > best + MANIFOLD_TIE_A) { best = k; p2 = id; a2 = a; b2 = b; }
    }
    if (p2 >= 0) {
      float hi = MANIFOLD_EPS, lo = -MANIFOLD_EPS;
      m = fm;
#pragma unroll 1
      while (m) {
        const int id = __ffsll((unsigned long long)m) - 1;
        m &= m - 1;
        float a, b;
        SDX_COORDS(id, a, b)
        const float k = (a2 - a1) * (b - b1) - (b2 - b1) * (a - a1);
        if (k > hi + MANIFOLD_TIE_A) { hi = k; p3 = id; }
        if (k < lo - MANIFOLD_TIE_A) { lo = k; p4 = id; }
      }
    }
#undef SDX_COORDS
    const int pk[4] = {p1, p2, p3, p4};
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (pk[k] >= 0) { if (pk[k] < 32) s1 |= 1u << pk[k]; else s2 |= 1u << (pk[k] - 32); ++n; }
  }
  uint32_t m;
#define SDX_FILL(mask, sel)                                   \
  m = (mask) & ~(sel);                                        \
  _Pragma("unroll") for (int i = 0; i < 4; ++i)               \
    if (m && n < 4) { (sel) |= m & (0u - m); m &= m - 1; ++n; }
  SDX_FILL(f1, s1) SDX_FILL(f2, s2) SDX_FILL(o1, s1) SDX_FILL(o2, s2)
#undef SDX_FILL
  *sel1 = s1; *sel2 = s2;
  return n;
}

#define LOAD_BOX2(ba, sa, bb, sb) Box A, Bx; load_box2(C, S, ba, sa, bb, sb, &A, &Bx);   // (both boxes of a pair: A, Bx)
__device__ __forceinline__ f3 point_vel(const PhysLds& S, int id, f3 p) {   // id: row of the body table (static world = zeros)
  return ld3(S.bv[id]) + cross(ld3(S.bw[id]), p - ld3(S.bp[id]));
}
