// sdx_phys_solve.h - private to sdx_physics.hip (included by it only, in its fixed order): the contact solver, solve(), as the list of its stages
#pragma once

// ---------------------------------------------------------------- E: solver
// solve() at the end of this file calls the stages below in order, one phase-clock stamp (SSTAMP, tools/time_physics.py) between two of
// them.  Every stage says what it reads and writes and which aliased row of PhysLds it owns while it runs; the rows' whole life is the
// ownership table in sdx_phys_lds.h.  SSTAMP / SCOUNT / LMAX / ABL expand to uses of `dbg` and `abl_bits`: a stage that uses them takes
// parameters of those names.
constexpr int NB = NF + NL;   // bodies with a CSR list: bricks 0..71, links 72..95
constexpr int LL = 8;         // gather lanes per link (tid = LL * link + sub): the lanes that also run the robot section
constexpr int GU = 4;         // entries per lane and trip of the gather
static_assert((NL * LL) % 64 == 0, "the link lanes (gather and robot section) are whole waves");

// What a lane keeps in registers for the whole solve about its CPT = MAXC / NT contact rows c = tid + q * NT
template <int CPT>
struct SolveRows {
  int ab[CPT];          // body a | body b << 8 (rows of the body table); from loop_registers() on their active-count slots in bits 16..31
  float vtgt[CPT];      // target normal velocity
  float muq[CPT];       // DR: friction of each contact = mean of its two bodies' coefficients (PhysX's default combine mode)
  uint32_t ckey[CPT];   // WARM: identity of the contact (pair, direction, sample)
  float lam[CPT][3];    // accumulated impulses (normal, two tangents); born in row_weights()
  float wA[CPT][3], wB[CPT][3];   // un-split inverse effective masses of both sides; born in row_weights()
};

// ---- set-up, stamps 16 -> 23: contact rows -> lane registers
// Reads the narrowphase's staging rows (separation in P[0], body ids in P[1], keys in S_CKEY = ent); writes R.ab, R.vtgt, R.ckey and, WARM,
// the previous solve's keys (wkey, HBM) into P[2], whose pair list is dead.  The staging rows are free after the barrier of csr_clear().
template <int NT, bool WARM, int CPT>
__device__ __forceinline__ void load_rows(const sdx_scene_desc& sc, PhysLds& S, int tid, int nc, float h, int nold, const uint32_t* wkey, SolveRows<CPT>& R) {
  int (&ab)[CPT] = R.ab;
  float (&vtgt)[CPT] = R.vtgt;
  uint32_t (&ckey)[CPT] = R.ckey;
#pragma unroll
  for (int q = 0; q < CPT; ++q) {
    const int c = tid + q * NT;
    ab[q] = BODY_W | (BODY_W << 8);
    vtgt[q] = 0.0f;
    ckey[q] = 0xffffffffu;
    if (c < nc) {
      const float sep = S.P[0][c];
      ab[q] = __float_as_int(S.P[1][c]);
      vtgt[q] = sep > 0 ? -sep / h : fminf(sc.baumgarte * (-sep) / h, sc.max_depenetration_vel);
      if (WARM) ckey[q] = S_CKEY(S)[c];
    }
  }
  // the previous solve's keys into the free third impulse row (the pair list that lived there is dead)
  if (WARM) for (int i = tid; i < nold; i += NT) S.P[2][i] = __int_as_float((int)wkey[i]);
}

// ---- k_physics<.. | SDX_PHYS_REPORT>, last substep, beside load_rows(): the set-up columns of the contact report (include/seqdex.h
// sdx_contact_report) from the staging rows the lane reads anyway - body pair, identity (S_CKEY, which collide()
// writes whether or not the solver is warm), separation.  Before the barrier of csr_clear(), after which the staging rows are reused.
// Column c is lane c % NT's: every store is coalesced.  The env's rows are addressed from an opaque copy of e (dr_row()): nothing of the
// report lives outside this function.  A row of the body table -> a row of SDX_T_RB: brick i -> SDX_BODY_BRICK0 + i, link k -> k, world -> -1.
__device__ __forceinline__ int report_body_row(int id) { return id < NF ? SDX_BODY_BRICK0 + id : (id != BODY_W ? id - NF : -1); }
template <int NT, int CPT>
__device__ __forceinline__ void report_setup(const sdx_contact_report* table, int e, PhysLds& S, int tid, int nc, const int (&ab)[CPT]) {
  int ee = e;
  SDX_OPAQUE_S(ee);
  const size_t row = (size_t)ee * MAXC;
  int32_t* const body = table->body;   // (the launch's pointers, from their device table: block-uniform loads, here and nowhere earlier)
  uint32_t* const key = table->key;
  float* const separation = table->separation;
#pragma unroll
  for (int q = 0; q < CPT; ++q) {
    const int c = tid + q * NT;
    if (c < nc) {
      if (body) { body[2 * row + c] = report_body_row(ab[q] & 0xff); body[2 * row + MAXC + c] = report_body_row((ab[q] >> 8) & 0xff); }
      if (key) key[row + c] = S_CKEY(S)[c] & 0x0fffffffu;
      if (separation) separation[row + c] = S.P[0][c];
    }
  }
}
// ---- the same, beside solve_exit(): the result columns - point and normal (cp / cn live for the whole solve), the force on side a
// (n lam0 + t1 lam1 + t2 lam2) / h with the basis contact_update() uses, and the count.  Two write sites, so that no register of the
// report is alive across the solver loop.
template <int NT, int CPT>
__device__ __forceinline__ void report_result(const sdx_contact_report* table, int e, const PhysLds& S, int tid, int nc, float h, const float (&lam)[CPT][3]) {
  int ee = e;
  SDX_OPAQUE_S(ee);
  const size_t row = (size_t)ee * 3 * MAXC;
  float* const point = table->point;
  float* const normal = table->normal;
  float* const force = table->force;
  int32_t* const count = table->count;
#pragma unroll
  for (int q = 0; q < CPT; ++q) {
    const int c = tid + q * NT;
    if (c < nc) {
      const f3 p = F3(S.cp[0][c], S.cp[1][c], S.cp[2][c]), n = F3(S.cn[0][c], S.cn[1][c], S.cn[2][c]);
      if (point) { point[row + c] = p.x; point[row + MAXC + c] = p.y; point[row + 2 * MAXC + c] = p.z; }
      if (normal) { normal[row + c] = n.x; normal[row + MAXC + c] = n.y; normal[row + 2 * MAXC + c] = n.z; }
      if (force) {
        f3 t1, t2;
        tangents(n, &t1, &t2);
        const f3 f = (n * lam[q][0] + t1 * lam[q][1] + t2 * lam[q][2]) * (1.0f / h);   // (x 1 / h, as SDX_T_CONTACT is formed)
        force[row + c] = f.x; force[row + MAXC + c] = f.y; force[row + 2 * MAXC + c] = f.z;
      }
    }
  }
  if (tid == 0) count[ee] = nc;
}

// ---- CSR of contact sides per body (bricks AND robot links), ascending contact index inside a body: csr_clear() .. csr_rank()
// stamps 23 -> 24, first part: zero the counts (and, in the last substep, the links' net contact impulses cf)
template <int NT>
__device__ __forceinline__ void csr_clear(PhysLds& S, int tid, bool last_substep) {
  for (int i = tid; i < NB; i += NT) { S.ecount[i] = 0; S.efill[i] = 0; }
  if (last_substep) for (int i = tid; i < NL * 3; i += NT) (&S.cf[0][0])[i] = 0.0f;
  __syncthreads();   // also: every lane has read its (separation, ids, key) out of the staging rows, which the fill list reuses below
}

// ---- stamps 23 -> 24, between csr_clear() and csr_count(): warm-start match
// The old keys ascend in their pair part (bits 6..27: body pair rank, box pair), so the pair's first old contact is a lower bound away; the
// <= 4 contacts of a pair are then compared exactly.  wmatch packs the matched positions (11 bits each, 0x7ff = none); the
// impulses themselves are fetched where the lam registers are born.  The new keys replace the old ones in HBM right away (the
// old ones are in LDS now; the old impulses stay untouched until the end of this solve).
// Reads the old keys in P[2] (theirs until csr_offsets_and_packing() clears S_LANEMAP there) and ckey; writes wkey (HBM).  Yields wmatch, wage.
template <int NT, bool WARM, int CPT>
__device__ __forceinline__ void warm_match(PhysLds& S, int tid, int nc, int nold, const uint32_t (&ckey)[CPT], uint32_t* wkey, uint64_t& wmatch, uint32_t& wage) {
  wmatch = ~0ull;
  wage = 0;   // 8 bits per contact: consecutive solves it has existed (0: new in this solve)
  // lower bound of every slot's pair part among the old keys: a branch-free bisection whose trip count depends on nold only, so the lane's
  // CPT searches advance together - one LDS round trip per halving for all of them (round 6; one search after the other was 10 dependent
  // round trips per slot)
  int wlo[CPT];
#pragma unroll
  for (int q = 0; q < CPT; ++q) wlo[q] = 0;
  if (WARM && nold > 0) {
    int nrem = nold;
    while (nrem > 1) {
      const int half = nrem >> 1;
      uint32_t kv[CPT];
#pragma unroll
      for (int q = 0; q < CPT; ++q) kv[q] = (uint32_t)__float_as_int(S.P[2][wlo[q] + half - 1]);
#pragma unroll
      for (int q = 0; q < CPT; ++q) SDX_PIN1(kv[q]);
#pragma unroll
      for (int q = 0; q < CPT; ++q) wlo[q] = ((kv[q] & 0x0fffffffu) >> 6) < (ckey[q] >> 6) ? wlo[q] + half : wlo[q];
      nrem -= half;
    }
#pragma unroll
    for (int q = 0; q < CPT; ++q) wlo[q] += (((uint32_t)__float_as_int(S.P[2][wlo[q]]) & 0x0fffffffu) >> 6) < (ckey[q] >> 6) ? 1 : 0;
  }
#pragma unroll
  for (int q = 0; q < CPT; ++q) {
    const int c = tid + q * NT;
    if (WARM && c < nc) {
      const uint32_t key = ckey[q];
      uint32_t age = 0;
      if (nold > 0) {
        const int lo = wlo[q];
        int found = 0x7ff;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int i = lo + u;
          const uint32_t ok = i < nold ? (uint32_t)__float_as_int(S.P[2][i]) : 0xffffffffu;
          if ((ok & 0x0fffffffu) == key) { found = i; age = (ok >> 28) + 1u; }
        }
        wmatch = (wmatch & ~(0x7ffull << (11 * q))) | ((uint64_t)found << (11 * q));
      }
      wage |= age << (8 * q);
      wkey[c] = key | ((age < 15u ? age : 15u) << 28);   // bits 28..31: the number of consecutive solves this contact has existed before (saturating at 15: the ramp is over after warm_age <= 16 solves)
    }
  }
}

// ---- stamps 23 -> 24, last part: sides per body (integer atomics on ecount)
template <int NT, int CPT>
__device__ __forceinline__ void csr_count(PhysLds& S, int tid, int nc, const int (&ab)[CPT]) {
#pragma unroll
  for (int q = 0; q < CPT; ++q)
    if (tid + q * NT < nc) {
      const int a = ab[q] & 0xff, b = (ab[q] >> 8) & 0xff;
      if (a != BODY_W) atomicAdd(&S.ecount[a], 1);
      if (b != BODY_W) atomicAdd(&S.ecount[b], 1);
    }
  __syncthreads();
}

// ---- stamps 24 -> 25: offsets (eoff) on wave 0 beside the balanced-gather packing (gtab) on wave 1
// Reads ecount; writes eoff, gtab and zeroes S_LANEMAP, which takes P[2] over from the old warm-start keys (dead since the barrier of
// csr_count()).
template <int NT>
__device__ __forceinline__ void csr_offsets_and_packing(PhysLds& S, int tid) {
  if (tid < 64) {   // exclusive prefix over the 96 bodies on wave 0: two per lane, shuffle scan
    const int i0 = 2 * tid, i1 = 2 * tid + 1;
    const int c0 = i0 < NB ? S.ecount[i0] : 0, c1 = i1 < NB ? S.ecount[i1] : 0;
    int incl = c0 + c1;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int up = __shfl_up(incl, o, 64);
      if (tid >= o) incl += up;
    }
    const int excl = incl - (c0 + c1);
    if (i0 < NB) S.eoff[i0] = excl;
    if (i1 < NB) S.eoff[i1] = excl + c0;
    if (i1 == NB - 1 || i0 == NB - 1) S.eoff[NB] = incl;
  } else if (tid < 128) {
    // ---- balanced brick gather (round 6): wave 1, beside the prefix sum.  The per-pass gather [D] used to give every brick 4 lanes: the
    // brick with the longest list (40 - 60 sides in a settled pile, 19 on average) kept its lanes for 3 - 4 trips while most quads idled -
    // 4 - 5 k of the pass's 9 k cycles.  Now a brick with n sides gets L = 1, 2, 4, 8 or 16 CONSECUTIVE lanes - the power of two at or
    // above ceil(n / K) - each summing a contiguous slice of ceil(n / L) <= K sides; the slices meet in a segmented row scan (DPP).
    // Layout = counting sort by size, largest first: every brick then starts at a multiple of its size and never straddles a 16-lane
    // row.  K is the smallest of 4, 6, 8, 12, ... 96 whose layout fits the brick lanes (all 512 when the hand touches nothing, else
    // those of waves 3..7); lane t holds bricks t and t + 64.
    constexpr int GKT = 10;
    static_assert(NF <= 128, "two bricks per lane of wave 1");
    const int t = tid - 64;
    const bool robot = __ballot(t < NL && S.ecount[NF + (t < NL ? t : 0)] > 0) != 0ull;
    const int nlanes = robot ? NT - NL * 8 : NT, base = robot ? NL * 8 : 0;
    const int n0 = S.ecount[t < NF ? t : 0], n1 = t + 64 < NF ? S.ecount[t + 64 < NF ? t + 64 : 0] : 0;
    const uint64_t lt = t == 0 ? 0ull : (~0ull >> (64 - t));
    int P0 = 0, P1 = 0, start0 = 0, start1 = 0;
#pragma unroll 1
    for (int tk = 0; tk < GKT; ++tk) {
      const int K = (4 + 2 * (tk & 1)) << (tk >> 1), Kmul = (65536 + K - 1) / K;   // ceil(n / K) = ((n + K - 1) * Kmul) >> 16 for n < 2048
      int L0 = ((n0 + K - 1) * Kmul) >> 16, L1 = ((n1 + K - 1) * Kmul) >> 16;
      // size class: 0 (no sides), else the power of two >= min(L, 16)
      P0 = L0 == 0 ? 0 : (L0 > 8 ? 16 : (L0 > 4 ? 8 : (L0 > 2 ? 4 : L0)));
      P1 = L1 == 0 ? 0 : (L1 > 8 ? 16 : (L1 > 4 ? 8 : (L1 > 2 ? 4 : L1)));
      int run = 0;   // lanes of the classes placed so far (wave-uniform)
      start0 = start1 = 0;
#pragma unroll
      for (int c = 16; c >= 1; c >>= 1) {
        const uint64_t b0 = __ballot(P0 == c), b1 = __ballot(P1 == c);
        const int c0 = __popcll(b0);
        if (P0 == c) start0 = run + c * __popcll(b0 & lt);
        if (P1 == c) start1 = run + c * (c0 + __popcll(b1 & lt));
        run += c * (c0 + __popcll(b1));
      }
      if (run <= nlanes) break;   // (K = 96 always fits: at most 16 bricks can have more than 96 sides)
    }
    if (t < NF) S.gtab[t] = (uint32_t)(start0 + base) | ((uint32_t)P0 << 9);
    if (t + 64 < NF) S.gtab[t + 64] = (uint32_t)(start1 + base) | ((uint32_t)P1 << 9);
  }
  S_LANEMAP(S)[tid] = 0;   // (wave 0 and 1 after their work: the row of the old warm-start keys is free since the barrier above)
  __syncthreads();
}

// ---- stamps 25 -> 26: lane map of the chosen packing and the unsorted fill
// Owns S_LANEMAP (P[2]), S_ENT2 (P[0]) and S_EBODY2 (P[1]): a side of body `a` goes to entry eoff[a] + (its order of arrival).
template <int NT, int CPT>
__device__ __forceinline__ void csr_fill(PhysLds& S, int tid, int nc, const int (&ab)[CPT]) {
  if (tid < NF) {   // lane -> (brick, lane of the brick, last lane?) of the chosen packing
    const uint32_t w = S.gtab[tid];
    const int start = w & 511, L = w >> 9;
    for (int j = 0; j < L; ++j) S_LANEMAP(S)[start + j] = (unsigned short)(0x8000 | tid | (j << 7) | ((j == L - 1) << 11));
  }
#pragma unroll
  for (int q = 0; q < CPT; ++q) {
    const int c = tid + q * NT;
    if (c < nc) {
      const int a = ab[q] & 0xff, b = (ab[q] >> 8) & 0xff;
      if (a != BODY_W) { const int i = S.eoff[a] + atomicAdd(&S.efill[a], 1); S_ENT2(S)[i] = (unsigned short)c; S_EBODY2(S)[i] = (unsigned char)a; }
      if (b != BODY_W) { const int i = S.eoff[b] + atomicAdd(&S.efill[b], 1); S_ENT2(S)[i] = (unsigned short)(c | 0x8000); S_EBODY2(S)[i] = (unsigned char)b; }
    }
  }
  __syncthreads();
}

// ---- stamps 26 -> 27, first part: this lane's slice of a brick's list (balanced gather):
// brick | lane of the brick << 7 | last lane << 11 | first entry << 12 | entries << 24; 0 = none.
// Reads S_LANEMAP, gtab, ecount, eoff.  (Read here: link_inertia() rewrites the row that holds the lane map.)
__device__ __forceinline__ uint32_t gather_slice(PhysLds& S, int tid) {
  uint32_t cdesc = 0;
  const uint32_t lm = S_LANEMAP(S)[tid];
  if (lm & 0x8000u) {
    const int b = lm & 0x7f, j = (lm >> 7) & 15;
    const int L = (int)(S.gtab[b] >> 9), n = S.ecount[b];
    const int c = (n + L - 1) / L;                      // entries per lane of this brick
    int cnt = n - j * c;
    cnt = cnt < 0 ? 0 : (cnt > c ? c : cnt);
    cdesc = (lm & 0xfffu) | ((uint32_t)(S.eoff[b] + j * c) << 12) | ((uint32_t)cnt << 24);
  }
  return cdesc;
}

// ---- stamps 26 -> 27: rank pass: entry -> position = number of entries of the same body with a smaller contact index (a contact touches
// a body at most once, so indices are distinct) => every body's list is in ascending contact order, deterministically
// Reads the fill (S_ENT2, S_EBODY2); writes ent, which stops being S_CKEY here.  The fill rows P[0], P[1] are dead after its barrier.
template <int NT>
__device__ __forceinline__ void csr_rank(PhysLds& S, int tid, int abl_bits) {
  const int total = S.eoff[NB];
  for (int i = tid; i < total; i += NT) {
    const int body = S_EBODY2(S)[i];
    const int o = S.eoff[body], n = S.eoff[body + 1] - o;
    const unsigned short v = S_ENT2(S)[i];
    const int key = v & 0x7fff;
    int rank = 0;
    if (ABL(64)) rank = i - o;
    else
#pragma unroll 4
    for (int j = 0; j < n; ++j) rank += (S_ENT2(S)[o + j] & 0x7fff) < key;
    S.ent[o + rank] = v;
  }
  __syncthreads();   // rank pass complete (ent final); the fill list in the P rows is dead from here on
}

// ---- stamps 28 -> 29: link inertia
// Robot: operational-space inverse inertia of every link that carries a contact, Lam_k = J_k Hinv J_k^T (6 x 6, symmetric, about
// the link origin o_k; J_k = the link's geometric Jacobian over the <= 11 dofs of its path), built by the whole block in three stages
// through the (free) impulse rows.  A robot-side row weight is then g^T Lam_k g with g = (d, (p - o_k) x d): no per-contact walk over
// the path, no exchange between the lanes that own a contact and the lanes that own a link.
// Owns W = all three P rows; Lam (W_L) stays there for row_weights().  Yields `touched`: the links that carry contacts in this substep
// (block-uniform).
constexpr int W_T = 0, W_U = NL * 66, W_L = 2 * NL * 66, W_J = 2 * NL * 66 + NL * 21;   // T = J_k [6][11], U = J_k Hinv_sub [6][11], Lam [21], path dofs [11]
static_assert(W_J + NL * 11 <= 3 * MAXC, "the three stages fit the impulse rows");
template <int NT>
__device__ __forceinline__ uint32_t link_inertia(PhysLds& S, int tid, bool has_robot) {
  uint32_t touched = 0;
  float* const W = &S.P[0][0];
  if (has_robot) {
    for (int k = 0; k < NL; ++k) if (S.eoff[NF + k + 1] > S.eoff[NF + k]) touched |= 1u << k;
    // stage 1: lane = (link k, dof j on its path): column of J_k and the dof's slot
    for (int idx = tid; idx < NL * ND; idx += NT) {
      const int k = idx / ND, j = idx % ND;
      const uint32_t ak = S.anc[k];
      if (((touched >> k) & 1u) && ((ak >> j) & 1u)) {
        const int slot = __popc(ak & ((1u << j) - 1u));
        const f3 a = ld3(S.la[j + 1]);
        const f3 lin = cross(a, ld3(S.bp[NF + k]) - ld3(S.bp[NF + j + 1]));
        float* t = W + W_T + k * 66 + slot;
        t[0] = lin.x; t[11] = lin.y; t[22] = lin.z; t[33] = a.x; t[44] = a.y; t[55] = a.z;
        reinterpret_cast<int*>(W + W_J)[k * 11 + slot] = j;
      }
    }
    __syncthreads();
    // stage 2: lane = (link, row r, slot q): U[r][q] = sum_s T[r][s] Hinv[j_s][j_q]
    for (int idx = tid; idx < NL * 66; idx += NT) {
      const int k = idx / 66, rq = idx % 66, r = rq / 11, q = rq % 11;
      const int m = __popc(S.anc[k]);
      if (((touched >> k) & 1u) && q < m) {
        const int* pj = reinterpret_cast<const int*>(W + W_J) + k * 11;
        const float* t = W + W_T + k * 66 + r * 11;
        // (all 11 slots' operands in flight together - slots past the path read slot 0 and are not added; the run-time loop over the m
        // slots was two dependent LDS round trips per slot)
        int pjq = pj[q], pjv[11];
        float tv[11], av[11];
#pragma unroll
        for (int sidx = 0; sidx < 11; ++sidx) { pjv[sidx] = pj[sidx < m ? sidx : 0]; tv[sidx] = t[sidx < m ? sidx : 0]; }
        SDX_PIN1(pjq);
#pragma unroll
        for (int sidx = 0; sidx < 11; ++sidx) SDX_PIN1(pjv[sidx]);
        const float* Aq = S.A[pjq];
#pragma unroll
        for (int sidx = 0; sidx < 11; ++sidx) av[sidx] = Aq[pjv[sidx]];   // Hinv is symmetric: row j_q instead of column j_q
#pragma unroll
        for (int sidx = 0; sidx < 11; ++sidx) { SDX_PIN1(av[sidx]); SDX_PIN1(tv[sidx]); }
        float acc = 0.0f;
#pragma unroll
        for (int sidx = 0; sidx < 11; ++sidx) if (sidx < m) acc += tv[sidx] * av[sidx];
        W[W_U + idx] = acc;
      }
    }
    __syncthreads();
    // stage 3: lane = (link, entry (i, j <= i) of the lower triangle): Lam[i][j] = sum_s U[i][s] T[j][s]
    for (int idx = tid; idx < NL * 21; idx += NT) {
      const int k = idx / 21, e = idx % 21;
      if ((touched >> k) & 1u) {
        int i, j;
        tri_index(e, &i, &j);
        const int m = __popc(S.anc[k]);
        const float* u = W + W_U + k * 66 + i * 11;
        const float* t = W + W_T + k * 66 + j * 11;
        float uv[11], tv[11];
#pragma unroll
        for (int sidx = 0; sidx < 11; ++sidx) { uv[sidx] = u[sidx < m ? sidx : 0]; tv[sidx] = t[sidx < m ? sidx : 0]; }
#pragma unroll
        for (int sidx = 0; sidx < 11; ++sidx) { SDX_PIN1(uv[sidx]); SDX_PIN1(tv[sidx]); }
        float acc = 0.0f;
#pragma unroll
        for (int sidx = 0; sidx < 11; ++sidx) if (sidx < m) acc += uv[sidx] * tv[sidx];
        W[W_L + idx] = acc;
      }
    }
    __syncthreads();
  }
  return touched;
}

// ---- stamps 29 -> 30: row weights and initial impulses
// Writes R.wA, R.wB, R.lam (the per-lane impulse / weight registers are born only here): both brick sides together, robot sides from Lam
// (W_L in the P rows, read-only here), then the warm-start gate on the body table's (v, w) and the cached impulses wlam (HBM): a matched contact
// starts from beta x its cached impulse, ramped over its age (inv_age), unless it is deeper than wdeep or moving.
template <int NT, bool WARM, int CPT>
__device__ __forceinline__ void row_weights(const PhysLds& S, int tid, int nc, bool has_robot, uint64_t wmatch, uint32_t wage, const float* wlam,
                                            float beta, float inv_age, float wdeep, SolveRows<CPT>& R, int abl_bits) {
  const int (&ab)[CPT] = R.ab;
  const float (&vtgt)[CPT] = R.vtgt;
  float (&lam)[CPT][3] = R.lam, (&wA)[CPT][3] = R.wA, (&wB)[CPT][3] = R.wB;
  const float* const W = &S.P[0][0];
#pragma unroll
  for (int q = 0; q < CPT; ++q) {
    const int c = tid + q * NT;
    const bool on = c < nc && !ABL(128);
    const int a = ab[q] & 0xff, b = (ab[q] >> 8) & 0xff;
    f3 p = F3(0, 0, 0), n = F3(0, 0, 1);
    if (on) { p = F3(S.cp[0][c], S.cp[1][c], S.cp[2][c]); n = F3(S.cn[0][c], S.cn[1][c], S.cn[2][c]); }
    f3 t1, t2;
    tangents(n, &t1, &t2);
    const f3 dir[3] = {n, t1, t2};
    {
      // One brick side's weight is bim * (1 + l . (tii * l)) with l = R^T ((p - x) x d) (oracle: brick_w()).  As a function called six times
      // it compiled to ~7 dependent LDS round trips per call (position, orientation, type -> inertia ratios, inverse mass, one after the
      // other: 40 in a row per contact).  Here both sides' rows are loaded together, then the type rows, then the six weights are plain
      // arithmetic.  A side that is not a brick reads brick 0 and is discarded.
      const bool ba = on && a < NF, bb = on && b < NF;
      const int ia = ba ? a : 0, ib = bb ? b : 0;
      f3 xa = ld3(S.bp[ia]), xb = ld3(S.bp[ib]);
      f4 qa = ld4(S.bq[ia]), qb = ld4(S.bq[ib]);
      float ima = S.bim[ia], imb = S.bim[ib];
      int ta = S.btype[ia], tb = S.btype[ib];
      SDX_PIN1(ta); SDX_PIN1(tb);
      f3 iia = ld3(S.tii[ta]), iib = ld3(S.tii[tb]);
      SDX_PIN3x4(xa, xb, iia, iib);
      SDX_PIN1(qa.x); SDX_PIN1(qa.y); SDX_PIN1(qa.z); SDX_PIN1(qa.w); SDX_PIN1(qb.x); SDX_PIN1(qb.y); SDX_PIN1(qb.z); SDX_PIN1(qb.w);
      SDX_PIN1(ima); SDX_PIN1(imb);
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        const f3 la = qrot(qconj(qa), cross(p - xa, dir[r])), lb = qrot(qconj(qb), cross(p - xb, dir[r]));
        const float va = ima * (1.0f + la.x * la.x * iia.x + la.y * la.y * iia.y + la.z * la.z * iia.z);
        const float vb = imb * (1.0f + lb.x * lb.x * iib.x + lb.y * lb.y * iib.y + lb.z * lb.z * iib.z);
        wA[q][r] = ba ? va : 0.0f;
        wB[q][r] = bb ? vb : 0.0f;
        lam[q][r] = 0.0f;
      }
    }
    if (has_robot && on) {
#pragma unroll 1
      for (int side = 0; side < 2; ++side) {
        const int id = side ? b : a;
        if (id >= NF && id != BODY_W) {
          const int k = id - NF;
          const float* L = W + W_L + k * 21;   // lower triangle, row-major: (0,0) (1,0) (1,1) (2,0) ...
          const f3 rr = p - ld3(S.bp[id]);
          float w3[3];
#pragma unroll
          for (int r = 0; r < 3; ++r) {
            const f3 d = dir[r], md = cross(rr, d);
            const float g[6] = {d.x, d.y, d.z, md.x, md.y, md.z};
            float acc = 0.0f;
#pragma unroll
            for (int i = 0; i < 6; ++i) {
              float t = 0.5f * L[i * (i + 1) / 2 + i] * g[i];
#pragma unroll
              for (int j = 0; j < i; ++j) t += L[i * (i + 1) / 2 + j] * g[j];
              acc += g[i] * t;
            }
            w3[r] = 2.0f * acc;
          }
          if (side) { wB[q][0] = w3[0]; wB[q][1] = w3[1]; wB[q][2] = w3[2]; }
          else { wA[q][0] = w3[0]; wA[q][1] = w3[1]; wA[q][2] = w3[2]; }
        }
      }
    }
    // warm start only where the last solve's impulse still means something: the contact is not in deep penetration (that is recovery,
    // not rest) and the two bodies are nearly at rest relative to each other at the contact point (not an impact, not sliding)
    const int wm = (int)((wmatch >> (11 * q)) & 0x7ffull);
    if (WARM && on && wm != 0x7ff && vtgt[q] <= wdeep) {
      const f3 vrel = point_vel(S, a, p) - point_vel(S, b, p);
      // the cached impulse is trusted in proportion to the age of the contact: a contact that has existed for warm_age solves starts
      // from the full fraction, a contact the previous solve saw for the first time (an impact) from nothing
      const float bq = beta * fminf(1.0f, (float)((wage >> (8 * q)) & 0xffu) * inv_age);
      const float l0 = bq * wlam[wm];
      if (l0 > 0.0f && dot(vrel, vrel) <= WARM_SPEED * WARM_SPEED) {
        lam[q][0] = l0; lam[q][1] = bq * wlam[MAXC + wm]; lam[q][2] = bq * wlam[2 * MAXC + wm];
      }
    }
  }
}

// ---- stamps 30 -> 17: pass set-up
// Yields the gather lanes' coordinates (gbeg, gend) and the robot section's path dofs tjp; writes bK, acount, rsync and turns the body
// table to (u, w).  Gather lanes.  Links: LL = 8 per link (only when the hand touches something), lane sub sums entries sub, sub + 8, ...
// of its link's list [gbeg, gend).  Every other lane: the slice of cdesc (balanced gather) - the descriptor itself in gbeg.
template <int NT>
__device__ __forceinline__ void pass_setup(PhysLds& S, int tid, bool has_robot, int nrob, uint32_t cdesc, int& gbeg, int& gend, int& tjp) {
  static_assert(NL * LL + NF * GL <= NT, "one lane per brick for bK behind the link lanes");
  if (has_robot && tid < NL * LL) { gbeg = S.eoff[NF + tid / LL] + tid % LL; gend = S.eoff[NF + tid / LL + 1]; }
  else { gbeg = (int)cdesc; gend = (int)(((cdesc >> 12) & 0xfffu) + (cdesc >> 24)); }
  // world inverse inertia of the substep: lane NL * LL + GL * b computes brick b's bK
  {
    const int gbody = (tid - NL * LL) / GL;
    if (tid >= NL * LL && (tid - NL * LL) % GL == 0 && gbody < NF) {
      const f4 q = ld4(S.bq[gbody]);
      const f3 ex = qrot(q, F3(1, 0, 0)), ey = qrot(q, F3(0, 1, 0)), ez = qrot(q, F3(0, 0, 1));   // columns of R
      const float* ii = S.tii[S.btype[gbody]];
      const float i0 = S.bim[gbody] * ii[0], i1 = S.bim[gbody] * ii[1], i2 = S.bim[gbody] * ii[2];
      S.bK[gbody][0] = i0 * ex.x * ex.x + i1 * ey.x * ey.x + i2 * ez.x * ez.x;
      S.bK[gbody][1] = i0 * ex.y * ex.y + i1 * ey.y * ey.y + i2 * ez.y * ez.y;
      S.bK[gbody][2] = i0 * ex.z * ex.z + i1 * ey.z * ey.z + i2 * ez.z * ez.z;
      S.bK[gbody][3] = i0 * ex.x * ex.y + i1 * ey.x * ey.y + i2 * ez.x * ez.y;
      S.bK[gbody][4] = i0 * ex.x * ex.z + i1 * ey.x * ey.z + i2 * ez.x * ez.z;
      S.bK[gbody][5] = i0 * ex.y * ex.z + i1 * ey.y * ey.z + i2 * ez.y * ez.z;
    }
  }
  // robot section lanes (8 per link): the rs-th and (rs + 8)-th dof on the path base -> link rj (ND = none)
  tjp = ND | (ND << 8);
  {
    const int rj = tid / 8, rs = tid % 8;
    if (rj < NL) {
      int tj0 = ND, tj1 = ND;
      uint32_t m = S.anc[rj];
      for (int t = 0; m; ++t) {
        const int j = __ffs(m) - 1;
        m &= m - 1;
        if (t == rs) tj0 = j;
        if (t == rs + 8) tj1 = j;
      }
      tjp = tj0 | (tj1 << 8);
    }
  }
  // mass splitting: the first iteration splits every body over ALL its contacts, iteration i > 0 over the contacts that were active in
  // iteration i - 1 (counted into the other set while this one is read); slots 0..71 bricks, NF the whole robot, NF + 1 the static world
  for (int i = tid; i < NF + 2; i += NT) {
    S.acount[0][i] = i < NF ? S.ecount[i] : (i == NF ? nrob : 0);
    S.acount[1][i] = 0;
  }
  if (tid == 0) S.rsync = 0;
  __syncthreads();   // every lane has read what it needs of v / w in the body table (warm-start gate of row_weights())
  // body table -> (u, w): u = v - w x x.  Link rows too (their twists are those of the drive phase until the robot section rewrites them)
  for (int i = tid; i < NBODY; i += NT) st3(S.bv[i], ld3(S.bv[i]) - cross(ld3(S.bw[i]), ld3(S.bp[i])));
  __syncthreads();
}

// ---- after stamp 17: what the loop keeps in registers
// The sides' active-count slots into bits 16..31 of R.ab; DR: R.muq from the per-body coefficients bfr / lfr (HBM).
template <bool DR, int CPT>
__device__ __forceinline__ void loop_registers(const sdx_scene_desc& sc, const float* bfr, const float* lfr, SolveRows<CPT>& R, int& gbeg, int& gend, int& tjp) {
  int (&ab)[CPT] = R.ab;
  float (&vtgt)[CPT] = R.vtgt, (&muq)[CPT] = R.muq;
  float (&lam)[CPT][3] = R.lam, (&wA)[CPT][3] = R.wA, (&wB)[CPT][3] = R.wB;
#pragma unroll
  for (int q = 0; q < CPT; ++q) {   // a brick's own slot, NF = the whole robot, NF + 1 = the static world
    const int a = ab[q] & 0xff, b = (ab[q] >> 8) & 0xff;
    const int sa = a < NF ? a : (a != BODY_W ? NF : NF + 1), sb = b < NF ? b : (b != BODY_W ? NF : NF + 1);
    ab[q] = (ab[q] & 0xffff) | (sa << 16) | (sb << 24);
    if (DR) {   // coefficients by body-table row: bricks (bfr), links (lfr), the static world keeps the scene's
      const float fa = a < NF ? bfr[a] : (a != BODY_W ? lfr[a - NF] : sc.friction);
      const float fb = b < NF ? bfr[b] : (b != BODY_W ? lfr[b - NF] : sc.friction);
      muq[q] = 0.5f * (fa + fb);
    }
  }
  // fresh values for the loop: whatever the set-up phases above did to these registers, inside the loop they are plain registers again
#pragma unroll
  for (int q = 0; q < CPT; ++q) {
    SDX_OPAQUE(ab[q]); SDX_OPAQUE(vtgt[q]);
    if (DR) SDX_OPAQUE(muq[q]);
#pragma unroll
    for (int r = 0; r < 3; ++r) { SDX_OPAQUE(lam[q][r]); SDX_OPAQUE(wA[q][r]); SDX_OPAQUE(wB[q][r]); }
  }
  SDX_OPAQUE(gbeg); SDX_OPAQUE(gend); SDX_OPAQUE(tjp);
}

// isa_check: loop stage begin (tools/isa_check.py counts the lines from here to the matching end with the lines of the loop itself)
// ---- [AC] lane = contact: relative velocity from the current body table, active flag -> counted for the NEXT iteration (integer
// atomics), Jacobi update with the counts of the previous iteration; impulse P (on body A) to LDS, zero when inactive
// Reads the body table, cp / cn, acount[cur]; writes R.lam, acount[nxt] and the P rows, from here on the impulses of this pass.
template <int NT, bool WARM, bool DR, int CPT>
__device__ __forceinline__ void contact_update(PhysLds& S, int tid, int nc, int it, float mu, float relax, SolveRows<CPT>& R, long long* dbg, int abl_bits) {
  const int (&ab)[CPT] = R.ab;
  const float (&vtgt)[CPT] = R.vtgt, (&muq)[CPT] = R.muq;
  float (&lam)[CPT][3] = R.lam;
  const float (&wA)[CPT][3] = R.wA, (&wB)[CPT][3] = R.wB;
  const int cur = it & 1, nxt = cur ^ 1;
  LCLOCK(lc_ac0);
#pragma unroll
  for (int q = 0; q < CPT; ++q) {
    int abq = ab[q], ct = tid;
    SDX_OPAQUE(abq); SDX_OPAQUE(ct);
    const int c = ct + q * NT;
    f3 P = F3(0, 0, 0);
    if (c < nc && !ABL(2)) {
      const f3 n = F3(S.cn[0][c], S.cn[1][c], S.cn[2][c]);
      f3 t1, t2;
      tangents(n, &t1, &t2);
      if (WARM && it < 0) {                      // warm start: the whole initial impulse
        if (lam[q][0] > 0.0f) P = n * lam[q][0] + t1 * lam[q][1] + t2 * lam[q][2];
      } else {
        // (bits 16..31 of ab: the two sides' slots in the active-count sets, fixed for the solve - decoding them per iteration cost 28
        // VALU instructions per contact; the counts of the previous iteration are loaded with the geometry, not after the velocity test:
        // one LDS round trip less on the path of every active contact)
        const int a = abq & 0xff, b = (abq >> 8) & 0xff, sa = (abq >> 16) & 0xff, sb = (abq >> 24) & 0xff;
        const f3 p = F3(S.cp[0][c], S.cp[1][c], S.cp[2][c]);
        // (the four body rows in flight together: the plain expression loads side A, waits, then side B into the same registers)
        f3 ua = ld3v(S.bv[a]), wa = ld3v(S.bw[a]), ub = ld3v(S.bv[b]), wb = ld3v(S.bw[b]);
        SDX_PIN3x4(ua, wa, ub, wb);
        const f3 vr = (ua + cross(wa, p)) - (ub + cross(wb, p));
        const float vn = dot(vr, n);
        const float lam0 = lam[q][0], lam1 = lam[q][1], lam2 = lam[q][2];
        if (lam0 > 0.0f || vn < vtgt[q]) {
          if (a != BODY_W) atomicAdd(&S.acount[nxt][sa], 1);
          if (b != BODY_W) atomicAdd(&S.acount[nxt][sb], 1);
          const int ca = S.acount[cur][sa], cb = S.acount[cur][sb];
          const float na = a != BODY_W ? (float)(ca > 1 ? ca : 1) : 0.0f;
          const float nb = b != BODY_W ? (float)(cb > 1 ? cb : 1) : 0.0f;
          const float w0 = na * wA[q][0] + nb * wB[q][0];
          const float w1 = na * wA[q][1] + nb * wB[q][1];
          const float w2 = na * wA[q][2] + nb * wB[q][2];
          const float ln = fmaxf(0.0f, lam0 - relax * (vn - vtgt[q]) * SDX_RCP(w0));
          const float lim = (DR ? muq[q] : mu) * ln;
          float l1 = lam1 - relax * dot(vr, t1) * SDX_RCP(w1);
          l1 = fminf(lim, fmaxf(-lim, l1));
          float l2 = lam2 - relax * dot(vr, t2) * SDX_RCP(w2);
          l2 = fminf(lim, fmaxf(-lim, l2));
          lam[q][0] = ln; lam[q][1] = l1; lam[q][2] = l2;
          P = n * (ln - lam0) + t1 * (l1 - lam1) + t2 * (l2 - lam2);
        }
      }
      S.P[0][c] = P.x; S.P[1][c] = P.y; S.P[2][c] = P.z;
    }
  }
#ifdef SDX_LANE_CLOCK
  { LCLOCK(lc_ac1); LMAX(55, lc_ac1 - lc_ac0); if (tid == NT - 1) LMAX(56, lc_ac1 - lc_ac0); }
#endif
}

// [D], link tail (every lane of link k holds the sums after the reduction; this is its lane d_sub): the wrench (F, M about the link
// origin x) projected on the dofs of the link's path -> Qc for the robot section; last substep: the net impulse on the link so far -> cf
__device__ __forceinline__ void gather_link_tail(PhysLds& S, int k, int d_sub, int tjp, f3 x, const float (&acc)[6], bool last_substep) {
  const int tj0 = tjp & 0xff, tj1 = tjp >> 8;
  const f3 F = F3(acc[0], acc[1], acc[2]), M = F3(acc[3], acc[4], acc[5]);
  // generalised impulse on the d_sub-th (and (d_sub + 8)-th) dof of the path: a_j . (M + (o_k - o_j) x F); la[ND + 1] = 0 for "none"
  S.Qc[k][d_sub] = dot(ld3(S.la[tj0 + 1]), M + cross(x - ld3(S.bp[NF + tj0 + 1]), F));
  if (d_sub < 4) S.Qc[k][d_sub + 8] = dot(ld3(S.la[tj1 + 1]), M + cross(x - ld3(S.bp[NF + tj1 + 1]), F));
  if (last_substep && d_sub == 0) { S.cf[k][0] += acc[0]; S.cf[k][1] += acc[1]; S.cf[k][2] += acc[2]; }   // net impulse on the link so far
}

// [D], brick tail (the brick's LAST lane after the scan): w += Iw^-1 M, u += F / m - dw x x, from the operands gather() requested before the scan
__device__ __forceinline__ void gather_brick_tail(PhysLds& S, int d_body, f3 x, const float (&acc)[6], float (&K_)[6], float imb_, f3 u_, f3 w_) {
  SDX_PIN4(K_); SDX_PIN1(K_[4]); SDX_PIN1(K_[5]); SDX_PIN1(imb_); SDX_PIN3(u_); SDX_PIN3(w_);
  const float* K = K_;
  const f3 dw = F3(K[0] * acc[3] + K[3] * acc[4] + K[4] * acc[5], K[3] * acc[3] + K[1] * acc[4] + K[5] * acc[5],
                   K[4] * acc[3] + K[5] * acc[4] + K[2] * acc[5]);
  st3(S.bv[d_body], (u_ + F3(acc[0], acc[1], acc[2]) * imb_) - cross(dw, x));
  st3(S.bw[d_body], w_ + dw);
}

// ---- [D] gather (LL lanes per link, a slice per brick lane): F = sum(+-P), M = sum(+-(p - x) x P) about the body's reference point x; each
// lane sums its slice in ascending contact order, the partial sums are combined in a fixed order (deterministic); inactive contacts carry
// P = 0.  Bricks: gather_brick_tail().  Links: gather_link_tail(), right away (8 lanes, <= 2 dofs each) -> Qc for the robot section.
// Reads ent, the P rows, cp, bp; writes the brick rows of the body table, Qc, cf and zeroes acount[cur] for the pass after the next.
template <int NT>
__device__ __forceinline__ void gather(PhysLds& S, int tid, int it, bool has_robot, bool last_substep, int gbeg, int gend, int tjp, long long* dbg, int abl_bits) {
  const int cur = it & 1;
  LCLOCK(lc_d0);
  int td = tid;
  SDX_OPAQUE(td);   // lane coordinates re-derived per iteration instead of living in registers across the loop
  const bool d_link = has_robot && td < NL * LL;   // waves 0..2 of an env whose hand touches something: link lanes; every other lane is a brick lane
  const uint32_t cd = (uint32_t)gbeg;              // (brick lanes: the slice descriptor)
  const int d_body = d_link ? NF + td / LL : (int)(cd & 0x7fu), d_sub = d_link ? td % LL : 0;
  const int gstride = d_link ? LL : 1;
  const int ibeg = d_link ? gbeg : (int)((cd >> 12) & 0xfffu);
  float acc[6] = {0, 0, 0, 0, 0, 0};
  const f3 x = ld3(S.bp[d_body]);
  // four entries per trip (the index loads, then the payloads, in flight together); not unrolled further: the decoded
  // addresses of a longer window would be kept in registers across the whole iteration loop
  // two entries at a time: index loads pinned in front of the 12 payload loads, those in front of the arithmetic (four dependent LDS
  // round trips per trip of four entries instead of eight; all GU = 4 entries of a trip at once spill inside the loop)
#pragma unroll 1
  for (int i = ibeg; i < (ABL(1) ? ibeg : gend); i += GU * gstride) {
#pragma unroll
    for (int h2 = 0; h2 < GU; h2 += 2) {
      const int i0 = i + h2 * gstride, i1 = i0 + gstride;
      int e0 = S.ent[i0 < gend ? i0 : i], e1 = S.ent[i1 < gend ? i1 : i];
      SDX_PIN1(e0); SDX_PIN1(e1);
      const int c0 = e0 & 0x7fff, c1 = e1 & 0x7fff;
      f3 P0 = F3(S.P[0][c0], S.P[1][c0], S.P[2][c0]), C0 = F3(S.cp[0][c0], S.cp[1][c0], S.cp[2][c0]);
      f3 P1 = F3(S.P[0][c1], S.P[1][c1], S.P[2][c1]), C1 = F3(S.cp[0][c1], S.cp[1][c1], S.cp[2][c1]);
      SDX_PIN3x4(P0, C0, P1, C1);
      {
        const float sg = i0 < gend ? ((e0 & 0x8000) ? -1.0f : 1.0f) : 0.0f;
        const f3 P = P0 * sg;
        const f3 M = cross(C0 - x, P);
        acc[0] += P.x; acc[1] += P.y; acc[2] += P.z; acc[3] += M.x; acc[4] += M.y; acc[5] += M.z;
      }
      {
        const float sg = i1 < gend ? ((e1 & 0x8000) ? -1.0f : 1.0f) : 0.0f;
        const f3 P = P1 * sg;
        const f3 M = cross(C1 - x, P);
        acc[0] += P.x; acc[1] += P.y; acc[2] += P.z; acc[3] += M.x; acc[4] += M.y; acc[5] += M.z;
      }
    }
  }
#ifdef SDX_LANE_CLOCK
  { LCLOCK(lc_d1); LMAX(57, lc_d1 - lc_d0); LMAX(58, (gend - ibeg + gstride - 1) / gstride); }
#endif
  // the brick update's operands (inverse inertia, inverse mass, u, w: 13 numbers) are requested BEFORE the lane reductions and pinned
  // after them: their LDS round trip runs under the DPP adds instead of after them (every lane loads: the branch comes later)
  const int tb = d_link ? 0 : d_body;
  float K_[6], imb_ = S.bim[tb];
#pragma unroll
  for (int r = 0; r < 6; ++r) K_[r] = S.bK[tb][r];
  f3 u_ = ld3(S.bv[tb]), w_ = ld3(S.bw[tb]);
  if (d_link) {
#pragma unroll
    for (int r = 0; r < 6; ++r) {
      acc[r] = sum4(acc[r]);
      acc[r] += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(acc[r]), 0x141, 0xF, 0xF, true));
    }
  } else {
    // the slices of a brick sit on consecutive lanes of one 16-lane row: inclusive segmented scan (row_shr 1, 2, 4, 8; lane `so` of the
    // brick adds the value `sh` lanes back while that lane still belongs to the brick), after which the brick's LAST lane holds the
    // sums - slices in ascending contact order, combined in the scan's fixed tree (deterministic)
    const int so = (int)((cd >> 7) & 15u);
#define SDX_SEG_STEP(sh)                                                                                                    \
    {                                                                                                                       \
      const bool take = so >= (sh);                                                                                         \
      _Pragma("unroll") for (int r = 0; r < 6; ++r) {                                                                       \
        const float t = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(acc[r]), 0x110 + (sh), 0xF, 0xF, true)); \
        acc[r] += take ? t : 0.0f;                                                                                          \
      }                                                                                                                     \
    }
    SDX_SEG_STEP(1) SDX_SEG_STEP(2) SDX_SEG_STEP(4) SDX_SEG_STEP(8)
#undef SDX_SEG_STEP
  }
  if (!d_link) {
    if ((cd >> 11) & 1u) {
      gather_brick_tail(S, d_body, x, acc, K_, imb_, u_, w_);
      S.acount[cur][d_body] = 0;   // read by [AC] before the pass's first barrier; it is the set [AC] of the next iteration counts into
    }
  } else {
    gather_link_tail(S, d_body - NF, d_sub, tjp, x, acc, last_substep);
  }
  if (td == NL * LL) { S.acount[cur][NF] = 0; }
#ifdef SDX_LANE_CLOCK
  { LCLOCK(lc_d2); LMAX(59, lc_d2 - lc_d0); }
#endif
}

// ---- robot section, ONE stage on 8 lanes per link = waves 0..2, which are also the link gather's: they meet at their OWN barrier (an LDS
// counter) while waves 3..7 are still gathering the bricks - the section touches nothing those read or write (Qc, qd / qdb, the link
// rows of the body table) - and the pass closes with the one workgroup barrier of solve()'s loop (round 6; a workgroup barrier in front of
// this section made every pass of an env whose hand touches bricks brick gather + robot section long instead of the longer of the two).
// Every group sums the generalised impulses of all 23 dofs from the Qc rows of the touched links below each dof (3 dofs per lane),
// shares them inside the group lane to lane (ds_bpermute: no LDS space - the impulse rows are still being read by the brick
// gather), then qd += Hinv dQ for the (<= 2) path dofs of this lane and the link's twist.
// `arrivals`: what the waves' own barrier has counted once all of them are here = waves x (passes so far, this one included).  Reads Hinv,
// Qc and the copy qpar of the joint velocities (0: qd, 1: qdb); writes the other copy and the link rows of the body table.
template <int NT>
__device__ __forceinline__ void robot_section(PhysLds& S, int tid, int arrivals, int qpar, uint32_t touched, int tjp, long long* dbg) {
  int tr = tid;
  SDX_OPAQUE(tr);
  if (tr < NL * 8) {
    // (requested before the waves meet: row `lane` of Hinv as six 16-byte loads and the joint velocity it belongs to)
    const int li = tr & 63, ri = li < ND ? li : 0;
    const float* qsrc = qpar ? S.qdb : S.qd;
    float* qdst = qpar ? S.qd : S.qdb;
    f4v arow[HP / 4];
#pragma unroll
    for (int k4 = 0; k4 < HP / 4; ++k4) arow[k4] = *reinterpret_cast<const f4v*>(&S.A[ri][4 * k4]);
    const float qi = qsrc[li < ND ? li : ND];   // (qd[ND] = 0)
    WAVES_BARRIER(&S.rsync, arrivals, NL * 8);
    SSTAMP(21);
    const int rj = tr / 8, rs = tr % 8;
    float qa[3];
#pragma unroll
    for (int u = 0; u < 3; ++u) {
      const int j = rs + 8 * u;
      float acc = 0.0f;
      if (j < ND) {
        // the position of dof j in the path of a link below it = the number of dofs above j: the same for every such link
        const int slot = __popc(S.anc[j + 1] & ((1u << j) - 1u));
        uint32_t m = S.desc[j] & touched;
#pragma unroll
        for (int t = 0; t < 6; ++t) {          // (independent loads: in flight together)
          const int k = m ? __ffs(m) - 1 : 0;
          acc += m ? S.Qc[k][slot] : 0.0f;
          m &= m - 1;
        }
        while (m) {
          const int k = __ffs(m) - 1;
          m &= m - 1;
          acc += S.Qc[k][slot];
        }
      }
      qa[u] = acc;
    }
    // qd += Hinv dQ, ONCE per wave: lane i < 23 multiplies row i of Hinv with Q, whose entry j every 8-lane group holds in lane j % 8
    // (v_readlane from the wave's first group: no LDS).  Round 5 had every lane multiply the rows of its (<= 2) path dofs: 46 + 23 LDS
    // loads per lane in three dependent batches; now 6 + 2.
    float dq = 0.0f;
#pragma unroll
    for (int j = 0; j < ND; ++j) {
      const f4v a4 = arow[j >> 2];
      const float aij = (j & 3) == 0 ? a4.x : ((j & 3) == 1 ? a4.y : ((j & 3) == 2 ? a4.z : a4.w));
      dq += aij * SDX_READLANE(qa[j >> 3], j & 7);
    }
    const float qn = li < ND ? qi + dq : 0.0f;
    if (tr < ND) qdst[tr] = qn;               // the other copy: groups still read the source copy of this pass
    const int tj0 = tjp & 0xff, tj1 = tjp >> 8;
    const float q0 = __shfl(qn, tj0, 64), q1 = __shfl(qn, tj1, 64);   // (tj = ND, "no dof": lane ND of the wave holds 0)
    const f3 pk = ld3(S.bp[NF + rj]);
    const f3 a0 = ld3(S.la[tj0 + 1]) * q0, a1 = ld3(S.la[tj1 + 1]) * q1;
    f3 w = a0 + a1;
    f3 v = cross(a0, pk - ld3(S.bp[NF + tj0 + 1])) + cross(a1, pk - ld3(S.bp[NF + tj1 + 1]));
    w.x = sum8(w.x); w.y = sum8(w.y); w.z = sum8(w.z);
    v.x = sum8(v.x); v.y = sum8(v.y); v.z = sum8(v.z);
    if (rs == 0 && rj > 0) { st3(S.bw[NF + rj], w); st3(S.bv[NF + rj], v - cross(w, pk)); }
  }
}
// isa_check: loop stage end

// ---- exit: the joint velocities into qd, the bricks' rows of the body table back to (v, w); WARM: the impulse cache (wlam, wcount: HBM)
template <int NT, bool WARM, int CPT>
__device__ __forceinline__ void solve_exit(PhysLds& S, int tid, int nc, int qpar, const float (&lam)[CPT][3], int32_t* wcount, float* wlam) {
  if (qpar && tid < ND) S.qd[tid] = S.qdb[tid];   // (lane tid is also the one that integrates dof tid)
  // body table back to (v, w) for the bricks (the link twists are rebuilt from qd by the next FK pass)
  for (int i = tid; i < NF; i += NT) st3(S.bv[i], ld3(S.bv[i]) + cross(ld3(S.bw[i]), ld3(S.bp[i])));
  // ---- the cache for the next solve (keys were written during the set-up)
  if (WARM) {
#pragma unroll
    for (int q = 0; q < CPT; ++q) {
      const int c = tid + q * NT;
      if (c < nc) { wlam[c] = lam[q][0]; wlam[MAXC + c] = lam[q][1]; wlam[2 * MAXC + c] = lam[q][2]; }
    }
    if (tid == 0) *wcount = nc;
    // no agent-scope fence: the next reader is this workgroup's next substep, many workgroup barriers later on the same CU (the
    // vector L1 is shared by the waves of a workgroup), or the next launch
  }
}

// Warm start (oracle: solve()): wcount / wkey / wlam are THIS env's impulse cache in HBM.  A contact that existed
// in the previous solve (same pair, direction and sample) starts from sc.warm_start x the impulses it ended with; iteration -1 of the
// loop below spreads those impulses over the bodies with the gather machinery of a normal iteration.  WARM is a template parameter:
// the default (cold) solver carries none of this code (it cost 2.6 % of the kernel as a run-time switch).
// REPORT (k_physics<.. | SDX_PHYS_REPORT>): the last substep also writes this env's columns of the contact report whose pointers stand in
// the device table rp (report_setup(), report_result()); like WARM a template parameter, so that the kernels without the flag carry none of it.
template <int NT, bool WARM, bool DR = false, bool REPORT = false>
__device__ __forceinline__ void solve(const SdxConst* C, PhysLds& S, int tid, float h, bool last_substep, long long* dbg,
                                      int32_t* wcount, uint32_t* wkey, float* wlam, int abl_bits, const float* bfr = nullptr, const float* lfr = nullptr,
                                      const sdx_contact_report* rp = nullptr, int e = 0) {
  constexpr int CPT = MAXC / NT;   // contact rows owned by one lane
  static_assert(CPT * NT == MAXC, "NT must divide SDX_MAXC");
  static_assert(CPT * 11 <= 64 && MAXC < 0x7ff, "11-bit cache positions of a lane's contacts in one 64-bit word");
  const sdx_scene_desc& sc = C->sc;
  const int nc = S.nc;
  const float mu = sc.friction, relax = sc.jacobi_relax;
  SSTAMP(16);
  SolveRows<CPT> R;
  // the warm-start gate's constants (block-uniform; computed here, at the top: born inside row_weights() they cost the randomization
  // variant 14 more VGPR spills)
  const float beta = sc.warm_start;
  const float inv_age = sc.warm_age > 0.0f ? 1.0f / sc.warm_age : 1e30f;
  // depth gate expressed on the velocity target the lane keeps anyway: sep < -WARM_DEPTH * offset <=> vtgt > baumgarte * depth / h
  const float wdeep = sc.baumgarte * (WARM_DEPTH * sc.contact_offset) / h;
  int nold = WARM ? *wcount : 0;   // block-uniform
  if (nold > MAXC) nold = MAXC;
  load_rows<NT, WARM>(sc, S, tid, nc, h, nold, wkey, R);
  if (REPORT) { if (last_substep) report_setup<NT>(rp, e, S, tid, nc, R.ab); }
  SSTAMP(23);
  csr_clear<NT>(S, tid, last_substep);
  uint64_t wmatch;
  uint32_t wage;
  warm_match<NT, WARM>(S, tid, nc, nold, R.ckey, wkey, wmatch, wage);
  csr_count<NT>(S, tid, nc, R.ab);
  SSTAMP(24);
  csr_offsets_and_packing<NT>(S, tid);
  SSTAMP(25);
  csr_fill<NT>(S, tid, nc, R.ab);
  SSTAMP(26);
  const int rbeg = S.eoff[NF], nrob = S.eoff[NB] - rbeg;   // the robot's sides: entries [rbeg, rbeg + nrob), grouped by link
  const bool has_robot = nrob > 0;                          // block-uniform
  const uint32_t cdesc = gather_slice(S, tid);
  if (tid == 0) S.nrob = nrob;
  SCOUNT(52, nc); SCOUNT(53, S.eoff[NB]); SCOUNT(54, nrob);
  csr_rank<NT>(S, tid, abl_bits);
  SSTAMP(27);   // (27 closes the rank pass, 28 opens the link inertia: tools/time_physics.py reads both)
  SSTAMP(28);
  const uint32_t touched = link_inertia<NT>(S, tid, has_robot);
  SSTAMP(29);
  row_weights<NT, WARM>(S, tid, nc, has_robot, wmatch, wage, wlam, beta, inv_age, wdeep, R, abl_bits);
  SSTAMP(30);
  int gbeg, gend, tjp;
  pass_setup<NT>(S, tid, has_robot, nrob, cdesc, gbeg, gend, tjp);
  SSTAMP(17);
  loop_registers<DR>(sc, bfr, lfr, R, gbeg, gend, tjp);
  int qpar = 0;   // robot section: joint velocities are read from S.qd (0) / S.qdb (1) and written to the other
  const int it0 = (WARM && nold > 0) ? -1 : 0;
  for (int it = it0; it < (ABL(4) ? 1 : sc.solver_iters); ++it) {   // it = -1: only the gather of the warm-start impulses
#ifdef SDX_PHASE_CLOCK
    if (it == 1) dbg = nullptr;
#endif
    SSTAMP(18);
    contact_update<NT, WARM, DR>(S, tid, nc, it, mu, relax, R, dbg, abl_bits);
    __syncthreads();
    SSTAMP(20);
    gather<NT>(S, tid, it, has_robot, last_substep, gbeg, gend, tjp, dbg, abl_bits);
    if (has_robot && !ABL(8)) {   // (waves 0..2, beside the brick gather of waves 3..7)
      robot_section<NT>(S, tid, (NL * LL / 64) * (it - it0 + 1), qpar, touched, tjp, dbg);
      qpar ^= 1;
    }
    __syncthreads();
    SSTAMP(22);
  }
  solve_exit<NT, WARM>(S, tid, nc, qpar, R.lam, wcount, wlam);
  if (REPORT) { if (last_substep) report_result<NT>(rp, e, S, tid, nc, h, R.lam); }
}
