// sdx_phys_dynamics.h - private to sdx_physics.hip (included by it only, after the headers of the step): k_dof_dynamics, the joint-space
// dynamics of the robot at the CURRENT SDX_T_DOF / SDX_T_TARGETS (include/seqdex.h sdx_dof_dynamics)
#pragma once

#define DYN_NT 256   // threads per env: wave 0 does the forward kinematics, all four waves share the 276 entries of the triangle

// The rows of PhysLds that fk_wave0, crba_entry and bias_torque touch, under their names (sdx_phys_robot.h takes the layout as a template
// parameter).  11 KiB against the 80 KiB of PhysLds: the LDS (160 KiB) would allow 14 workgroups per CU; the registers (98 / 122 VGPRs: 4 waves
// per SIMD) allow 4, against the 2 of k_kinematics.
struct DynLds {
  float q[ND], qd[ND + 1], tgt[ND];
  float lq[NL][4], la[NL + 1][3], lc[NL][3], lI[NL][6], lmass[NL], lmf[NL];
  float lal[NL + 1][3], lao[NL][3], lF[NL][3], lN[NL][3];
  alignas(16) float A[ND][HP];   // M, both triangles
  uint32_t anc[NL], desc[ND];
  int par[NL + 1];
  float bp[NBODY][3];            // (the body table's layout: link k is row NF + k, the brick rows are unused)
  alignas(16) float bv[NBODY][4];
  alignas(16) float bw[NBODY][4];
  float rc[SDX_MAX_RBOX][3], rq[SDX_MAX_RBOX][4];   // fk_wave0 places the robot's collision boxes; nobody reads them here
  int rbl[SDX_MAX_RBOX];
};
static_assert(sizeof(DynLds) <= 12 * 1024, "k_dof_dynamics: the registers, not the LDS, bound the workgroups per CU");

// entry (i, j), i >= j, of the joint-space inertia M(q): the sum of mass_matrix (sdx_phys_robot.h), restated here because any change to the
// step's own loop, a call to a shared function included, changes the register allocation of k_physics<512>
__device__ __forceinline__ float crba_entry(DynLds& S, int i, int j) {
  float s = 0.0f;
  if ((S.anc[i + 1] >> j) & 1u) {
    const f3 ai = ld3(S.la[i + 1]), aj = ld3(S.la[j + 1]);
    const f3 pi = ld3(S.bp[NF + i + 1]), pj = ld3(S.bp[NF + j + 1]);
    {   // links below dof i = bits of desc[i] (all of them > i); four links' operands in flight at a time, same terms, ascending k
      const uint32_t below = S.desc[i];
      constexpr int FB = 4;
#pragma unroll 1
      for (int k0 = i + 1; k0 < NL; k0 += FB) {
        f3 ck_[FB];
        float I_[FB][6], mk_[FB];
#pragma unroll
        for (int u = 0; u < FB; ++u) {
          const int k = k0 + u < NL ? k0 + u : NL - 1;
          ck_[u] = ld3(S.lc[k]); mk_[u] = S.lmass[k];
#pragma unroll
          for (int r = 0; r < 6; ++r) I_[u][r] = S.lI[k][r];
        }
#pragma unroll
        for (int u = 0; u < FB; ++u) { SDX_PIN3(ck_[u]); SDX_PIN1(mk_[u]); SDX_PIN4(I_[u]); SDX_PIN1(I_[u][4]); SDX_PIN1(I_[u][5]); }
#pragma unroll
        for (int u = 0; u < FB; ++u) {
          const f3 li = cross(ai, ck_[u] - pi), lj = cross(aj, ck_[u] - pj);
          const float* I = I_[u];
          const f3 Ia = F3(I[0] * aj.x + I[3] * aj.y + I[4] * aj.z, I[3] * aj.x + I[1] * aj.y + I[5] * aj.z,
                           I[4] * aj.x + I[5] * aj.y + I[2] * aj.z);
          const float term = mk_[u] * dot(li, lj) + dot(ai, Ia);
          if (k0 + u < NL && ((below >> (k0 + u)) & 1u)) s += term;
        }
      }
    }
  }
  return s;
}
// velocity-product bias torque of dof tl: the tc loop of k_physics' drive block, restated for the same reason
__device__ __forceinline__ float bias_torque(DynLds& S, int tl) {
  float tc = 0.0f;
  const f3 aj = ld3(S.la[tl + 1]), oj = ld3(S.bp[NF + tl + 1]);
  {   // links below dof tl = bits of desc[tl]; four links' operands in flight at a time, the same terms added in the same (ascending) order
    const uint32_t below = S.desc[tl];
    constexpr int FB = 4;
#pragma unroll
    for (int k0 = 1; k0 < NL; k0 += FB) {
      f3 lc_[FB], lF_[FB], lN_[FB];
#pragma unroll
      for (int u = 0; u < FB; ++u) if (k0 + u < NL) { lc_[u] = ld3(S.lc[k0 + u]); lF_[u] = ld3(S.lF[k0 + u]); lN_[u] = ld3(S.lN[k0 + u]); }
#pragma unroll
      for (int u = 0; u < FB; ++u) if (k0 + u < NL) { SDX_PIN3(lc_[u]); SDX_PIN3(lF_[u]); SDX_PIN3(lN_[u]); }
#pragma unroll
      for (int u = 0; u < FB; ++u) if (k0 + u < NL) {
        const float term = dot(aj, cross(lc_[u] - oj, lF_[u]) + lN_[u]);
        if ((below >> (k0 + u)) & 1u) tc += term;
      }
    }
  }
  return tc;
}

// One env per workgroup.  mass [N, ND, ND] = M(q) + armature (no implicit drive terms), bias [N, ND] = C(q, qd) qd, drive [N, ND] = the
// clamped PD torque of the first substep of the next launch; a nullptr output costs no stores and, where separable, no arithmetic (the
// link inertias serve the mass matrix only, the velocity-product wrenches the bias only).  The terms and their order are the step's:
// fk_wave0, crba_entry, bias_torque and the `t` of k_physics.
template <bool DR>
__global__ __launch_bounds__(DYN_NT) void k_dof_dynamics(const SdxConst* __restrict__ C, SdxBuf B, float* __restrict__ mass, float* __restrict__ bias,
                                                         float* __restrict__ drive) {
  __shared__ DynLds S;
  const sdx_scene_desc& sc = C->sc;
  const int e = blockIdx.x, tid = threadIdx.x;
  if (tid < ND) {
    S.q[tid] = B.dof[((size_t)e * ND + tid) * 2];
    S.qd[tid] = B.dof[((size_t)e * ND + tid) * 2 + 1];
    S.tgt[tid] = B.targets[(size_t)e * ND + tid];
    uint32_t d = 0;
    for (int k = 1; k < NL; ++k) d |= ((C->anc[k] >> tid) & 1u) << k;
    S.desc[tid] = d;
  }
  if (tid < NL) {   // (as load_constants does: this env's link mass factors are row 0 of SDX_T_DR_LINK)
    const float f = DR ? B.dr_link[(size_t)e * 2 * NL + tid] : 1.0f;
    S.anc[tid] = C->anc[tid];
    S.lmass[tid] = DR ? sc.link_mass[tid] * f : sc.link_mass[tid];
    S.lmf[tid] = f;
  }
  if (tid < SDX_MAX_RBOX) S.rbl[tid] = tid < sc.n_rbox ? sc.rbox_link[tid] : 0;
  if (tid <= NL) S.par[tid] = tid < NL ? (tid == 0 ? 0 : sc.parent[tid]) : NL;
  if (tid == 0) {
    S.qd[ND] = 0.0f; st3(S.la[NL], F3(0, 0, 0)); st3(S.lal[NL], F3(0, 0, 0));
    st3(S.bp[BODY_W], F3(0, 0, 0)); st3(S.bv[BODY_W], F3(0, 0, 0)); st3(S.bw[BODY_W], F3(0, 0, 0));
  }
  __syncthreads();
  if (tid < 64 && (mass || bias)) fk_wave0(C, S, tid, mass != nullptr, bias != nullptr, nullptr, DR);   // (the drive needs no kinematics)
  __syncthreads();
  if (mass) {
    for (int idx = tid; idx < ND * (ND + 1) / 2; idx += DYN_NT) {
      int i, j;
      tri_index(idx, &i, &j);
      float s = crba_entry(S, i, j);
      if (i == j) s += sc.armature[i];
      S.A[i][j] = s;
      S.A[j][i] = s;
    }
  }
  // the last wave has one entry of the triangle per lane, the first two: it takes the 23 bias sums and drive torques
  const int dj = tid - (DYN_NT - 64);
  if (dj >= 0 && dj < ND) {
    if (bias) bias[(size_t)e * ND + dj] = bias_torque(S, dj);
    if (drive) {
      const float h = sc.dt / (float)sc.substeps;
      const float* drow = DR ? B.dr_dof + (size_t)e * 4 * ND : nullptr;   // this env's [kp; kd; lower; upper]
      const float t = DR ? drow[dj] * (S.tgt[dj] - S.q[dj]) - (drow[ND + dj] + h * drow[dj]) * S.qd[dj]
                         : sc.kp[dj] * (S.tgt[dj] - S.q[dj]) - (sc.kd[dj] + h * sc.kp[dj]) * S.qd[dj];
      drive[(size_t)e * ND + dj] = fminf(sc.effort[dj], fmaxf(-sc.effort[dj], t));
    }
  }
  if (mass) {
    __syncthreads();
    float* M = mass + (size_t)e * ND * ND;   // full rows, consecutive lanes consecutive words
    for (int i = tid; i < ND * ND; i += DYN_NT) M[i] = S.A[i / ND][i % ND];
  }
}
