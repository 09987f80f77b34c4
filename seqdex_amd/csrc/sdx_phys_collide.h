// sdx_phys_collide.h - private to sdx_physics.hip (included by it only, in its fixed order): broadphase placement and narrowphase of one substep
#pragma once

template <int NT>
__device__ __forceinline__ void collide(const SdxConst* C, PhysLds& S, int tid, long long* dbg, int abl_bits) {
  const sdx_scene_desc& sc = C->sc;
  const float off = sc.contact_offset;
  constexpr int ns = SDX_MAX_STATIC, per = NF + SDX_MAX_STATIC;
  // ---- broadphase over BODY pairs: lane tid owns candidates tid, tid + NT, ... (ntot <= 16 NT: sdx_create checks); hits as a bit mask; ONE block scan places them (lane-major order)
  constexpr int n1 = NF * ns, n2 = NF * (NF - 1) / 2;
  // (round 6) the candidate tests themselves have run BEFORE this function, on the lanes of waves 1..7 while wave 0 was alone with the
  // forward kinematics, the factorisation and the drive (broad_mask_part; 19 k cycles per substep when they ran here): the hits of lane
  // tid's candidates tid, tid + NT, ... are the bits of S_BMASK[tid] - the same mask, whoever computed it
  const uint32_t mask = ABL(32) ? 0u : S_BMASK(S)[tid];
  SSTAMP(32);
  int np;
  {
    // at most 16 candidates per lane: (72 * 8 + 72 * 71 / 2 + 40 * 80) / 512 < 13 (5 bits of the count, 4 bits of the pair rank)
    int pos = block_scan_small<NT, 5>(S, __popc(mask), tid, &np);
    uint32_t m = mask;
    while (m) {
      const int it = __ffs(m) - 1;
      m &= m - 1;
      // bits 16..28: rank of the candidate in this list's order (lane-major: tid * 16 + trip), the same from solve to solve: the
      // major part of the warm-start key, ascending along the pair list and therefore along the contact list
      if (pos < MAXP) S_PAIRS(S)[pos] = pair_code(tid + it * NT, n1, n2, ns, per) | ((uint32_t)(tid * 16 + it) << 16);
      ++pos;
    }
  }
  int pairs_lost = np > MAXP;   // more candidate pairs than the list holds: the excess (lane-major order) is not tested
  if (np > MAXP) np = MAXP;
  __syncthreads();
  SSTAMP(40);
  SCOUNT(48, np);
  // ---- separating-axis pass over the bounding boxes: a body pair that a face axis of either bounding box separates by the whole contact
  // offset cannot produce a contact (its boxes lie inside the bounding boxes); about half of the sphere-vs-box candidates leave the list
  // here.  Lane tid looks at the consecutive pairs tid * q .. tid * q + q - 1 (order preserved).
  {
    constexpr int QMAX = (MAXP + NT - 1) / NT;
    static_assert(QMAX <= 3, "three survivor slots per lane");
    const int q = (np + NT - 1) / NT;
    uint32_t c0 = 0, c1 = 0, c2 = 0;
    int kept = 0;
#pragma unroll
    for (int k = 0; k < QMAX; ++k) {
      const int pi = tid * q + k;
      if (k < q && pi < np) {
        const uint32_t pr = S_PAIRS(S)[pi];
        const int bb = (pr >> 8) & 0xff;
        const Box A = load_bound(S, pr & 0xff), Bx = load_bound(S, bb);
        bool sep = dir_setup(A, Bx, off).smax >= off;
        if (!sep && bb < STATIC0) sep = dir_setup(Bx, A, off).smax >= off;
        if (!sep) {
          if (kept == 0) c0 = pr; else if (kept == 1) c1 = pr; else c2 = pr;
          ++kept;
        }
      }
    }
    int np2;
    const int pos = block_scan_small<NT, 2>(S, kept, tid, &np2);   // its barrier comes after every lane's reads of the old list
    if (kept > 0) S_PAIRS(S)[pos] = c0;
    if (kept > 1) S_PAIRS(S)[pos + 1] = c1;
    if (kept > 2) S_PAIRS(S)[pos + 2] = c2;
    np = np2;
    __syncthreads();
  }
  SSTAMP(41);
  SCOUNT(49, np);
  // ---- box pairs of the surviving body pairs, FOUR lanes per body pair.  A survivor is either
  //   CONVEX - both sides stand for one convex shape (a brick as the slab compound of its hull, a robot box, a single-box static): it
  //   contributes ONE box pair, the one with the smallest separation bound sigma = the largest face-axis separation of its directions
  //   (oracle: collide_bodies; ties: the first).  Lane `sub` of the quad computes sigma of box pair `sub`, a DPP minimum over the quad finds
  //   the winner, whose index goes to bits 29..30 of the pair word, bit 31 set (no box pair below the contact offset: the pair gets 0
  //   candidates); or
  //   COMPOUND - a hollow brick or the studded base plate on either side: every (box of A) x (box of B) is a candidate.
  // The exclusive prefix sum S_OFF of the candidate counts maps a body pair to its first candidate box pair.
  int nbp;   // candidate box pairs
  {
    static_assert(SDX_MAX_SUB * SDX_MAX_SUB <= 4, "the box pairs of a convex body pair: one per lane of a quad, the winner in two bits");
    const int sub = tid & 3;
#pragma unroll 1
    for (int base = 0; base < np; base += NT / 4) {
      const int pi = base + (tid >> 2);
      const bool on = pi < np;
      const uint32_t pr = on ? S_PAIRS(S)[pi] : 0u;
      const int ba = pr & 0xff, bb = (pr >> 8) & 0xff;
      const int na = on ? box_nsub(S, ba) : 1, nbx = on ? box_nsub(S, bb) : 1;
      int cnt = na * nbx;
      const bool convex = on && !(ba < NF && brick_hollow(S, ba)) && !(bb < NF && brick_hollow(S, bb)) && !(bb >= STATIC0 && nbx > 1);
      float sg = 1e30f;
      if (convex && sub < cnt) {
        const int sa = sub / nbx, sb = sub - sa * nbx;
        LOAD_BOX2(ba, sa, bb, sb)
        sg = dir_setup(A, Bx, off).smax;
        if (samples_b(bb, sb)) sg = fmaxf(sg, dir_setup(Bx, A, off).smax);
      }
      // minimum of (sigma, sub) over the quad (every lane of the wave executes the two DPP steps)
      int wi = sub;
#pragma unroll
      for (int st = 0; st < 2; ++st) {
        const float og = st == 0 ? __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(sg), 0xB1, 0xF, 0xF, true))
                                 : __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(sg), 0x4E, 0xF, 0xF, true));
        const int oi = st == 0 ? __builtin_amdgcn_update_dpp(0, wi, 0xB1, 0xF, 0xF, true) : __builtin_amdgcn_update_dpp(0, wi, 0x4E, 0xF, 0xF, true);
        const bool take = og < sg || (og == sg && oi < wi);
        sg = take ? og : sg;
        wi = take ? oi : wi;
      }
      if (on && sub == 0) {
        if (convex) {
          cnt = sg < off ? 1 : 0;
          S_PAIRS(S)[pi] = pr | ((uint32_t)(wi & 3) << 29) | 0x80000000u;
        }
        S_OFF(S)[pi] = cnt;
      }
    }
    __syncthreads();
    SSTAMP(42);
    // exclusive prefix sum of the counts, three body pairs per lane
    static_assert(MAXP <= 3 * NT, "three body pairs per lane");
    const int i0 = 3 * tid, i1 = 3 * tid + 1, i2 = 3 * tid + 2;
    const int n0 = i0 < np ? S_OFF(S)[i0] : 0, n1 = i1 < np ? S_OFF(S)[i1] : 0, n2 = i2 < np ? S_OFF(S)[i2] : 0;
    const int boff = block_scan_small<NT, 10>(S, n0 + n1 + n2, tid, &nbp);   // <= 3 x (8 boxes of a hollow brick x 33 of a base plate) per lane: 10 bits
    if (i0 < np) S_OFF(S)[i0] = boff;
    if (i1 < np) S_OFF(S)[i1] = boff + n0;
    if (i2 < np) S_OFF(S)[i2] = boff + n0 + n1;
    if (tid == 0) S_OFF(S)[np] = nbp;
    __syncthreads();
  }
  SSTAMP(33);
  SCOUNT(50, nbp);
  // ---- expansion: candidate box pair t = S_OFF[p] + (sub a * nsub(b) + sub b) of body pair p.  Lane tid tests the CONSECUTIVE candidates
  // tid * q2 .. (so the survivors come out in ascending (pair rank, box pair) order: the order of the warm-start keys) with the
  // separating-axis test of the two boxes; survivors as a bit mask, one block scan, then the lane walks its range again and writes
  // (box a | sub a << 7 | box b << 11 | sub b << 19) and (pair rank << 9 | box pair index) per survivor.
  int nsp;
  {
    if (nbp > 32 * NT) { nbp = 32 * NT; pairs_lost = 1; }
    const int q2 = (nbp + NT - 1) / NT;
    const int t0 = tid * q2, t1 = min(t0 + q2, nbp);
    int p = 0;
    if (t0 < t1) {   // the body pair that holds candidate t0: last p with S_OFF[p] <= t0
      int lo = 0, hi = np;
      while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (S_OFF(S)[mid] <= t0) lo = mid; else hi = mid; }
      p = lo;
    }
    uint32_t keep = 0;
    {
      int pp = p, pend = t0 < t1 ? S_OFF(S)[pp + 1] : 0;
      uint32_t pr = t0 < t1 ? S_PAIRS(S)[pp] : 0;
      int nbs = t0 < t1 ? box_nsub(S, (pr >> 8) & 0xff) : 1;
#pragma unroll 1
      for (int t = t0; t < t1; ++t) {
        while (t >= pend) { ++pp; pend = S_OFF(S)[pp + 1]; pr = S_PAIRS(S)[pp]; nbs = box_nsub(S, (pr >> 8) & 0xff); }
        bool sep = false;
        if (!(pr >> 31)) {   // (a convex pair's only candidate has passed its test in the pass above)
          const int sidx = t - S_OFF(S)[pp];
          const int ba = pr & 0xff, bb = (pr >> 8) & 0xff, sa = sidx / nbs, sb = sidx - sa * nbs;
          LOAD_BOX2(ba, sa, bb, sb)
          sep = dir_setup(A, Bx, off).smax >= off;
          if (!sep && samples_b(bb, sb)) sep = dir_setup(Bx, A, off).smax >= off;
        }
        if (!sep) keep |= 1u << (t - t0);
      }
    }
    const int pos0 = block_scan_small<NT, 6>(S, __popc(keep), tid, &nsp);
    {
      int pos = pos0, pp = p, pend = t0 < t1 ? S_OFF(S)[pp + 1] : 0;
      uint32_t pr = t0 < t1 ? S_PAIRS(S)[pp] : 0;
      int nbs = t0 < t1 ? box_nsub(S, (pr >> 8) & 0xff) : 1;
      uint32_t m = keep;
#pragma unroll 1
      while (m) {
        const int t = t0 + __ffs(m) - 1;
        m &= m - 1;
        while (t >= pend) { ++pp; pend = S_OFF(S)[pp + 1]; pr = S_PAIRS(S)[pp]; nbs = box_nsub(S, (pr >> 8) & 0xff); }
        const int sidx = (pr >> 31) ? (int)((pr >> 29) & 3u) : t - S_OFF(S)[pp];
        const int ba = pr & 0xff, bb = (pr >> 8) & 0xff, sa = sidx / nbs, sb = sidx - sa * nbs;
        if (pos < MAXSP) {
          S_SP0(S)[pos] = (uint32_t)ba | ((uint32_t)sa << 7) | ((uint32_t)bb << 11) | ((uint32_t)sb << 19);
          S_SP1(S)[pos] = (((pr >> 16) & 0x1fffu) << 9) | (uint32_t)sidx;
        }
        ++pos;
      }
    }
    if (nsp > MAXSP) { nsp = MAXSP; pairs_lost = 1; }
    __syncthreads();
  }
  SSTAMP(37);
  SCOUNT(51, nsp);
  // ---- narrowphase in two parts.  (1) lane = candidate box pair: the <= 4 samples of the two directions that become contacts
  // (pair_contacts); a block prefix sum of the counts gives every contact its place in pair order, and the lane leaves TWO words per
  // contact there: (boxes, direction, sample) and the contact's identity.  (2) lane = contact (below): geometry of that sample.
  // (Rounds 1-2 emitted from the pair lanes, which kept both boxes alive across the scan and ran up to eight emissions in a row on one lane
  // while its neighbours idled: 36 spilled registers, 120 MB of scratch writes per launch.)
  // Capacity rule (oracle: collide()): a list that would exceed MAXC contacts is rebuilt without its speculative
  // part - only samples that touch or penetrate (inclusion threshold 0 instead of the contact offset); what still does not fit is
  // dropped in enumeration order and counted.  The second pass is the same code in a run-time loop (block-uniform trip count).
  int nc = 0, rebuilt = 0;
  float incl = off;
#pragma unroll 1
  for (int pass = 0; pass < 2; ++pass) {
    nc = 0;
#pragma unroll 1
    for (int base = 0; base < nsp; base += NT) {
      const int pi = base + tid;
      uint32_t s1 = 0, s2 = 0, w0 = 0, w1 = 0;
      int k = 0;
      if (pi < nsp && !ABL(16)) {
        w0 = S_SP0(S)[pi]; w1 = S_SP1(S)[pi];
        const int ba = w0 & 0x7f, sa = (w0 >> 7) & 0xf, bb = (w0 >> 11) & 0xff, sb = (w0 >> 19) & 0x3f;
        LOAD_BOX2(ba, sa, bb, sb)
        k = pair_contacts(S, A, Bx, samples_b(bb, sb), off, incl, &s1, &s2);
      }
      if (pass == 0 && base == 0) SSTAMP(38);
      int tot;
      int c = nc + block_scan_small<NT, 3>(S, k, tid, &tot);
      // (the descriptors go to the impulse rows P[0] / P[1]: the box pair list in cp / cn stays intact for the second pass)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if (s1) {
          const int sm = __ffs(s1) - 1;
          s1 &= s1 - 1;
          if (c < MAXC) { S.P[0][c] = __int_as_float((int)(w0 | ((uint32_t)sm << 26))); S.P[1][c] = __int_as_float((int)((w1 << 6) | (uint32_t)sm)); }
          ++c;
        } else if (s2) {
          const int sm = __ffs(s2) - 1;
          s2 &= s2 - 1;
          if (c < MAXC) { S.P[0][c] = __int_as_float((int)(w0 | (1u << 25) | ((uint32_t)sm << 26))); S.P[1][c] = __int_as_float((int)((w1 << 6) | 0x20u | (uint32_t)sm)); }
          ++c;
        }
      }
      nc += tot;
    }
    if (nc <= MAXC || pass == 1) break;
    incl = 0.0f;      // (the scans' barriers order this pass's LDS writes before the next pass's)
    rebuilt = 1;
  }
  __syncthreads();   // the box pair list in cp / cn is dead from here on
  SSTAMP(39);
  // ---- (2) lane = contact: point, normal, separation of sample s of box A against box B (oracle: emit_mask); the descriptor of contact c
  // sits in P[0][c] / P[1][c], which the same lane overwrites with the results
  {
    const int ncc = nc < MAXC ? nc : MAXC;
#pragma unroll 1
    for (int c = tid; c < ncc; c += NT) {
      const uint32_t d = (uint32_t)__float_as_int(S.P[0][c]), key = (uint32_t)__float_as_int(S.P[1][c]);
      const int dirb = (d >> 25) & 1, sidx = d >> 26;
      const int b0 = d & 0x7f, s0 = (d >> 7) & 0xf, b1 = (d >> 11) & 0xff, sb1 = (d >> 19) & 0x3f;
      const int ba = dirb ? b1 : b0, bb = dirb ? b0 : b1, sa = dirb ? sb1 : s0, sb = dirb ? s0 : sb1;
      LOAD_BOX2(ba, sa, bb, sb)
      const Dir D = dir_setup(A, Bx, off);
      const f3 pb = ((D.t + D.ex * S.samp[sidx][0]) + D.ey * S.samp[sidx][1]) + D.ez * S.samp[sidx][2];   // (the LDS copy: a per-lane index into __constant__ memory is a global load)
      f3 g;
      const float sd = sample_contact(D, pb, Bx.h, &g);
      const f3 n = qrot(Bx.q, g);
      const f3 pw = Bx.c + qrot(Bx.q, pb);
      const f3 p = pw - n * (0.5f * sd);
      S.cp[0][c] = p.x; S.cp[1][c] = p.y; S.cp[2][c] = p.z;
      S.cn[0][c] = n.x; S.cn[1][c] = n.y; S.cn[2][c] = n.z;
      S.P[0][c] = sd;                                       // staged for the owner lane of contact c (solver set-up)
      S.P[1][c] = __int_as_float(box_body(S, ba) | (box_body(S, bb) << 8));
      S_CKEY(S)[c] = key;   // (pair rank << 9 | box pair) << 6 | direction << 5 | sample: 28 bits
    }
  }
  if (tid == 0) {
    S.overflow = nc > MAXC ? nc - MAXC : 0;
    S.nc = nc > MAXC ? MAXC : nc;
    S.np = np;
    S.rebuilt = rebuilt | (pairs_lost << 1);
  }
  __syncthreads();
}
