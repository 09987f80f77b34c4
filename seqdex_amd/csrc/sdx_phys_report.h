// sdx_phys_report.h - private to sdx_physics.hip (included by it only, after sdx_phys_osc.h): k_contact_wrenches, the per-body contact
// wrenches and the sensor / filter force matrix from a contact report (include/seqdex.h sdx_contact_wrenches).  The
// report itself is written by k_physics<.. | SDX_PHYS_REPORT> (report_setup(), report_result() in sdx_phys_solve.h).
#pragma once

// The pointers of an armed report, by value into their device table (SdxBuf.cscratch) in front of the physics launch that reads them there.
static_assert(sizeof(sdx_contact_report) <= 16 * sizeof(float), "the table fits the cscratch row of sdx_buffers.h");
__global__ __launch_bounds__(64) void k_report_table(sdx_contact_report R, sdx_contact_report* __restrict__ table) {
  if (threadIdx.x == 0 && blockIdx.x == 0) *table = R;
}

#define CW_NT 512   // threads per env: one workgroup per env, a lane per contact column in the staging trips

// Only a robot link or a free brick can be a side of a contact: their rows of SDX_T_RB map to the slots 0 .. CW_NSLOT - 1 (links, then
// bricks).  The static world is CW_WORLD; any other number - which only a report that the kernel did not write can hold - is CW_NONE and
// belongs to no list.
constexpr int CW_NSLOT = NL + NF, CW_WORLD = 0xff, CW_NONE = 0xfe, CW_GL = 4;   // CW_GL: gather lanes per slot
static_assert(CW_NSLOT * CW_GL <= CW_NT && (CW_NSLOT * CW_GL) % 64 == 0, "the gather lanes are whole waves of the block");
static_assert(2 * MAXC <= 0x8000, "an entry is a contact index and a side bit in 16 bits");
__device__ __forceinline__ int cw_slot(int row) {
  if (row >= 0 && row < NL) return row;
  if (row >= SDX_BODY_BRICK0 && row < SDX_BODY_BRICK0 + NF) return NL + row - SDX_BODY_BRICK0;
  return row == -1 ? CW_WORLD : CW_NONE;
}

// Layout: a CSR of contact sides per slot, like the solver's (csr_count() .. csr_rank()): counts by integer atomics, offsets by a wave
// scan, an unsorted fill, then the rank pass that puts every list in ascending contact order - the sums below then run in that order
// whatever the atomics did.  Forces and points are staged in LDS by coalesced loads, so the gathers never touch HBM.  53 KiB of LDS.
struct CwLds {
  float f[3][MAXC], p[3][MAXC];            // force on side a, point
  unsigned char sa[MAXC], sb[MAXC];        // slots of the two sides
  unsigned short fill[2 * MAXC], ent[2 * MAXC];   // contact | side b << 15: in order of arrival / ascending (contact, side) inside a slot
  int count[CW_NSLOT], cfill[CW_NSLOT], off[CW_NSLOT + 1];
  float net[CW_NSLOT][6];
  unsigned char sslot[32], fslot[32];      // the pairs' sensor and filter slots
};

__global__ __launch_bounds__(CW_NT) void k_contact_wrenches(const float* __restrict__ rb, sdx_contact_report R, float* __restrict__ net,
                                                            sdx_contact_pairs prs, float* __restrict__ pair) {
  __shared__ CwLds S;
  const int e = blockIdx.x, tid = threadIdx.x;
  int nc = R.count[e];
  nc = nc < 0 ? 0 : (nc > MAXC ? MAXC : nc);   // block-uniform; no column at or beyond it is read
  for (int i = tid; i < CW_NSLOT; i += CW_NT) { S.count[i] = 0; S.cfill[i] = 0; }
  if (tid < 32) {
    S.sslot[tid] = (unsigned char)(tid < prs.n_sensor ? cw_slot(prs.sensor_body[tid]) : CW_NONE);
    S.fslot[tid] = (unsigned char)(tid < prs.n_filter ? cw_slot(prs.filter_body[tid]) : CW_NONE);
  }
  __syncthreads();
  // ---- stage the columns, count the sides per slot
  const size_t col = (size_t)e * MAXC;
  for (int c = tid; c < nc; c += CW_NT) {
    const int a = cw_slot(R.body[2 * col + c]), b = cw_slot(R.body[2 * col + MAXC + c]);
    S.sa[c] = (unsigned char)a; S.sb[c] = (unsigned char)b;
#pragma unroll
    for (int k = 0; k < 3; ++k) { S.f[k][c] = R.force[3 * col + k * MAXC + c]; S.p[k][c] = R.point[3 * col + k * MAXC + c]; }
    if (a < CW_NSLOT) atomicAdd(&S.count[a], 1);
    if (b < CW_NSLOT) atomicAdd(&S.count[b], 1);
  }
  __syncthreads();
  if (tid < 64) {   // exclusive prefix over the slots on wave 0: two per lane, shuffle scan
    const int i0 = 2 * tid, i1 = 2 * tid + 1;
    const int c0 = i0 < CW_NSLOT ? S.count[i0] : 0, c1 = i1 < CW_NSLOT ? S.count[i1] : 0;
    int incl = c0 + c1;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int up = __shfl_up(incl, o, 64);
      if (tid >= o) incl += up;
    }
    const int excl = incl - (c0 + c1);
    if (i0 < CW_NSLOT) S.off[i0] = excl;
    if (i1 < CW_NSLOT) S.off[i1] = excl + c0;
    if (i1 == CW_NSLOT - 1 || i0 == CW_NSLOT - 1) S.off[CW_NSLOT] = incl;
  }
  __syncthreads();
  // ---- unsorted fill: a side of slot s goes to entry off[s] + (its order of arrival); the counts bound every index by 2 nc
  for (int c = tid; c < nc; c += CW_NT) {
    const int a = S.sa[c], b = S.sb[c];
    if (a < CW_NSLOT) S.fill[S.off[a] + atomicAdd(&S.cfill[a], 1)] = (unsigned short)c;
    if (b < CW_NSLOT) S.fill[S.off[b] + atomicAdd(&S.cfill[b], 1)] = (unsigned short)(c | 0x8000);
  }
  __syncthreads();
  // ---- rank pass: position = entries of the same slot with a smaller (contact, side) - distinct inside a slot, so every list comes out
  // in ascending contact order, deterministically
  const int total = S.off[CW_NSLOT];
  for (int i = tid; i < total; i += CW_NT) {
    const unsigned short v = S.fill[i];
    const int c = v & 0x7fff, s = (v & 0x8000) ? S.sb[c] : S.sa[c];
    const int o = S.off[s], n = S.off[s + 1] - o, key = 2 * c + (v >> 15);
    int rank = 0;
#pragma unroll 4
    for (int j = 0; j < n; ++j) { const int w = S.fill[o + j]; rank += 2 * (w & 0x7fff) + (w >> 15) < key; }
    S.ent[o + rank] = v;
  }
  __syncthreads();
  // ---- net wrench per slot: lane j of the slot's CW_GL sums entries j, j + CW_GL, ... in ascending order, the lanes meet in sum4()'s fixed tree
  if (net && tid < CW_NSLOT * CW_GL) {
    const int s = tid / CW_GL, j = tid % CW_GL;
    const int row = s < NL ? s : SDX_BODY_BRICK0 + s - NL;
    const f3 x = ld3(rb + ((size_t)e * SDX_BODIES + row) * 13);
    float acc[6] = {0, 0, 0, 0, 0, 0};
    const int end = S.off[s + 1];
    for (int i = S.off[s] + j; i < end; i += CW_GL) {
      const int v = S.ent[i], c = v & 0x7fff;
      const float sg = (v & 0x8000) ? -1.0f : 1.0f;
      const f3 F = F3(S.f[0][c], S.f[1][c], S.f[2][c]) * sg;
      const f3 M = cross(F3(S.p[0][c], S.p[1][c], S.p[2][c]) - x, F);
      acc[0] += F.x; acc[1] += F.y; acc[2] += F.z; acc[3] += M.x; acc[4] += M.y; acc[5] += M.z;
    }
#pragma unroll
    for (int r = 0; r < 6; ++r) acc[r] = sum4(acc[r]);
    if (j == 0) {
#pragma unroll
      for (int r = 0; r < 6; ++r) S.net[s][r] = acc[r];
    }
  }
  __syncthreads();
  if (net)   // all SDX_BODIES rows, coalesced; a body that can carry no contact is +0
    for (int i = tid; i < SDX_BODIES * 6; i += CW_NT) {
      const int s = cw_slot(i / 6);
      net[(size_t)e * SDX_BODIES * 6 + i] = s < CW_NSLOT ? S.net[s][i % 6] : 0.0f;
    }
  // ---- force on sensor s from filter f: one lane per pair walks the sensor's list in ascending order (the lanes of one sensor read the
  // same entries: LDS broadcasts)
  if (pair) {
    const int ns = prs.n_sensor, nf = prs.n_filter;
    for (int q = tid; q < ns * nf; q += CW_NT) {
      const int ss = S.sslot[q / nf], ff = S.fslot[q % nf];
      f3 acc = F3(0, 0, 0);
      if (ss < CW_NSLOT && ff != CW_NONE) {
        const int end = S.off[ss + 1];
        for (int i = S.off[ss]; i < end; ++i) {
          const int v = S.ent[i], c = v & 0x7fff;
          const bool sideb = (v & 0x8000) != 0;
          if ((sideb ? S.sa[c] : S.sb[c]) == ff) {
            const f3 F = F3(S.f[0][c], S.f[1][c], S.f[2][c]);
            acc = sideb ? acc - F : acc + F;
          }
        }
      }
      float* o = pair + ((size_t)e * ns * nf + q) * 3;
      o[0] = acc.x; o[1] = acc.y; o[2] = acc.z;
    }
  }
}
