// sdx_phys_robot.h - private to sdx_physics.hip (included by it only, in its fixed order): forward kinematics, link twists, mass matrix (uses the broadphase mask of sdx_phys_broad.h)
#pragma once

// ---------------------------------------------------------------- A: FK, on wave 0 only (lane = link; levels by wave-synchronous hand-off)
// world inertia times vector: R I R^T x with I = (xx yy zz xy xz yz) in the link frame
__device__ __forceinline__ f3 inertia_mul(f4 q, const float* I, f3 x) {
  const f3 l = qrot(qconj(q), x);
  return qrot(q, F3(I[0] * l.x + I[3] * l.y + I[4] * l.z, I[3] * l.x + I[1] * l.y + I[5] * l.z, I[4] * l.x + I[5] * l.y + I[2] * l.z));
}
// link twists from qd, on wave 0: w_k = sum_j a_j qd_j, v_k = sum_j (a_j qd_j) x (p_k - p_j) over the dofs j on the path (<= 11 of them:
// 7 arm joints + 4 of one finger).  Fixed trip count, no branches: an exhausted path reads dof ND, whose velocity slot is zero
template <class LDS>
__device__ __forceinline__ void twists_wave0(LDS& S, int tid) {
  if (tid > 0 && tid < NL) {
    f3 w = F3(0, 0, 0), v = F3(0, 0, 0);
    const f3 pk = ld3(S.bp[NF + tid]);
    uint32_t m = S.anc[tid];
    // Operands of FOUR path terms at a time are loaded before their arithmetic (SDX_PIN*): the plain loop below compiles to two dependent
    // LDS round trips per term - 22 in a row on the one wave everybody else is waiting for (round 6, ISA reading).  Same terms, same order.
    constexpr int FB = 4;
#pragma unroll
    for (int t0 = 0; t0 < 11; t0 += FB) {
      f3 la_[FB], pj_[FB];
      float qd_[FB];
#pragma unroll
      for (int u = 0; u < FB; ++u) if (t0 + u < 11) {
        const int j = m ? __ffs(m) - 1 : ND;
        m &= m - 1;
        la_[u] = ld3(S.la[j + 1]); qd_[u] = S.qd[j]; pj_[u] = ld3(S.bp[NF + j + 1]);
      }
#pragma unroll
      for (int u = 0; u < FB; ++u) if (t0 + u < 11) { SDX_PIN3(la_[u]); SDX_PIN3(pj_[u]); SDX_PIN1(qd_[u]); }
#pragma unroll
      for (int u = 0; u < FB; ++u) if (t0 + u < 11) {
        const f3 aj = la_[u] * qd_[u];
        w = w + aj;
        v = v + cross(aj, pk - pj_[u]);
      }
    }
    st3(S.bw[NF + tid], w);
    st3(S.bv[NF + tid], v);
  }
}

// called by every lane of wave 0 (tid < 64).  Only the link POSES form a serial chain over the tree depth (one quaternion product and
// one rotation per level); everything else is one lane per link in parallel: joint axes / centres of mass, then the twists and the
// velocity-product terms as sums over the (<= 11) dofs of each link's path - the same terms in the same order as the recursions
// w_k = w_p + a_k qd_k, al_k = al_p + w_p x (a_k qd_k), ao_k = ao_p + al_p x r + w_p x (w_p x r) (recursive Newton-Euler at zero joint
// acceleration, fixed base, no gravity on the robot).  with_bias: the velocity-product wrenches the drive needs; with_inertia: the world
// inertia tensors the mass matrix needs.
// lmf: scale link masses and inertias by S.lmf (domain randomization; false = the scene's masses and inertias)
// LDS: PhysLds, or the rows of it that k_dof_dynamics keeps (sdx_phys_dynamics.h DynLds)
template <class LDS>
__device__ __forceinline__ void fk_wave0(const SdxConst* C, LDS& S, int tid, bool with_inertia, bool with_bias, long long* dbg = nullptr,
                                         bool lmf = false) {
  const sdx_scene_desc& sc = C->sc;
  const bool link = tid > 0 && tid < NL;
  // this lane's link constants, fetched once (all loads in flight together)
  int par = 0, dep = -1;
  f4 ql = {0, 0, 0, 1};
  f3 jp = F3(0, 0, 0), axl = F3(0, 0, 1), com = F3(0, 0, 0);
  float mass = 0.0f, I6[6] = {0, 0, 0, 0, 0, 0};
  if (link) {
    par = sc.parent[tid]; dep = C->depth[tid];
    const f4 jq = ld4(sc.joint_quat[tid]);
    const f3 ax = ld3(sc.joint_axis[tid]);
    jp = ld3(sc.joint_pos[tid]); com = ld3(sc.link_com[tid]);
    mass = sc.link_mass[tid];
#pragma unroll
    for (int i = 0; i < 6; ++i) I6[i] = sc.link_inertia[tid][i];
    float sn, cs;
    sincosf(0.5f * S.q[tid - 1], &sn, &cs);
    f4 qa; qa.x = ax.x * sn; qa.y = ax.y * sn; qa.z = ax.z * sn; qa.w = cs;
    ql = qmul(jq, qa);            // rotation parent frame -> link frame
    axl = qrot(jq, ax);           // joint axis in the parent frame
  }
  if (tid == 0) {
    st4(S.lq[0], ld4(sc.base_quat));
    st3(S.bp[NF + 0], ld3(sc.base_pos));
    st3(S.la[0], F3(0, 0, 1));
    st3(S.bv[NF + 0], F3(0, 0, 0));
    st3(S.bw[NF + 0], F3(0, 0, 0));
    st3(S.lal[0], F3(0, 0, 0)); st3(S.lao[0], F3(0, 0, 0)); st3(S.lF[0], F3(0, 0, 0)); st3(S.lN[0], F3(0, 0, 0));
    st3(S.lc[0], ld3(sc.base_pos) + qrot(ld4(sc.base_quat), ld3(sc.link_com[0])));
    com = ld3(sc.link_com[0]);
#pragma unroll
    for (int i = 0; i < 6; ++i) I6[i] = sc.link_inertia[0][i];
  }
  WAVE_SYNC();
  SSTAMP(7);
  // ---- the serial part: poses, level by level
  const int max_depth = C->max_depth;
  for (int d = 1; d <= max_depth; ++d) {
    if (link && dep == d) {
      f4 qp = ld4(S.lq[par]);
      f3 pp = ld3(S.bp[NF + par]);
      SDX_PIN1(qp.x); SDX_PIN1(qp.y); SDX_PIN1(qp.z); SDX_PIN1(qp.w); SDX_PIN3(pp);   // (the parent's two rows in one LDS round trip per level)
      st4(S.lq[tid], qnormalize(qmul(qp, ql)));
      st3(S.bp[NF + tid], pp + qrot(qp, jp));
    }
    WAVE_SYNC();
  }
  SSTAMP(8);
  // ---- one lane per link: world joint axis, centre of mass
  f4 qk = {0, 0, 0, 1};
  f3 dk = F3(0, 0, 0);
  if (link) {
    qk = ld4(S.lq[tid]);
    st3(S.la[tid], qrot(ld4(S.lq[par]), axl));
    dk = qrot(qk, com);
    st3(S.lc[tid], ld3(S.bp[NF + tid]) + dk);
  }
  WAVE_SYNC();
  SSTAMP(9);
  twists_wave0(S, tid);            // w_k, v_k from the dofs on the path
  SSTAMP(10);
  if (with_bias) {
    WAVE_SYNC();
    // al_k = sum over the links m on the path of w_par(m) x (a_m qd_m)
    f3 alk = F3(0, 0, 0);
    if (link) {
      uint32_t m = S.anc[tid];
      constexpr int FB = 4;
#pragma unroll
      for (int t0 = 0; t0 < 11; t0 += FB) {
        int pm_[FB];
        f3 la_[FB], wp_[FB];
        float qd_[FB];
#pragma unroll
        for (int u = 0; u < FB; ++u) if (t0 + u < 11) {
          const int j = m ? __ffs(m) - 1 : ND;
          m &= m - 1;
          pm_[u] = S.par[j + 1]; la_[u] = ld3(S.la[j + 1]); qd_[u] = S.qd[j];
        }
#pragma unroll
        for (int u = 0; u < FB; ++u) if (t0 + u < 11) SDX_PIN1(pm_[u]);
#pragma unroll
        for (int u = 0; u < FB; ++u) if (t0 + u < 11) wp_[u] = ld3(S.bw[NF + pm_[u]]);
#pragma unroll
        for (int u = 0; u < FB; ++u) if (t0 + u < 11) { SDX_PIN3(wp_[u]); SDX_PIN3(la_[u]); SDX_PIN1(qd_[u]); }
#pragma unroll
        for (int u = 0; u < FB; ++u) if (t0 + u < 11) alk = alk + cross(wp_[u], la_[u] * qd_[u]);
      }
      st3(S.lal[tid], alk);
    }
    WAVE_SYNC();
    SSTAMP(11);
    // ao_k = sum over the links m on the path of al_par(m) x r_m + w_par(m) x (w_par(m) x r_m), r_m = p_m - p_par(m)
    if (link) {
      f3 aok = F3(0, 0, 0);
      uint32_t m = S.anc[tid];
      constexpr int FB = 4;
#pragma unroll
      for (int t0 = 0; t0 < 11; t0 += FB) {
        int pm_[FB];
        f3 pj_[FB], pp_[FB], wp_[FB], al_[FB];
#pragma unroll
        for (int u = 0; u < FB; ++u) if (t0 + u < 11) {
          const int j = m ? __ffs(m) - 1 : ND;
          m &= m - 1;
          pm_[u] = S.par[j + 1]; pj_[u] = ld3(S.bp[NF + j + 1]);
        }
#pragma unroll
        for (int u = 0; u < FB; ++u) if (t0 + u < 11) SDX_PIN1(pm_[u]);
#pragma unroll
        for (int u = 0; u < FB; ++u) if (t0 + u < 11) { pp_[u] = ld3(S.bp[NF + pm_[u]]); wp_[u] = ld3(S.bw[NF + pm_[u]]); al_[u] = ld3(S.lal[pm_[u]]); }
#pragma unroll
        for (int u = 0; u < FB; ++u) if (t0 + u < 11) { SDX_PIN3(pj_[u]); SDX_PIN3(pp_[u]); SDX_PIN3(wp_[u]); SDX_PIN3(al_[u]); }
#pragma unroll
        for (int u = 0; u < FB; ++u) if (t0 + u < 11) {
          const f3 r = pj_[u] - pp_[u], wp = wp_[u];
          aok = aok + cross(al_[u], r) + cross(wp, cross(wp, r));
        }
      }
      st3(S.lao[tid], aok);
      const f3 wk = ld3(S.bw[NF + tid]);
      const f3 acom = aok + cross(alk, dk) + cross(wk, cross(wk, dk));
      if (lmf) {   // the link's mass and inertia x its factor, applied where they are stored (loaded early, they cost the variant scratch)
        const float f = S.lmf[tid];
        st3(S.lF[tid], acom * (mass * f));
        st3(S.lN[tid], (inertia_mul(qk, I6, alk) + cross(wk, inertia_mul(qk, I6, wk))) * f);
      } else {
        st3(S.lF[tid], acom * mass);
        st3(S.lN[tid], inertia_mul(qk, I6, alk) + cross(wk, inertia_mul(qk, I6, wk)));
      }
    }
  }
  SSTAMP(12);
  if (tid < sc.n_rbox) {
    const int k = S.rbl[tid];
    const f4 q = ld4(S.lq[k]);
    st3(S.rc[tid], ld3(S.bp[NF + k]) + qrot(q, ld3(sc.rbox_center[tid])));
    st4(S.rq[tid], qmul(q, ld4(sc.rbox_quat[tid])));
  }
  if (with_inertia && tid < NL) {   // world inertia R I R^T of each link (xx yy zz xy xz yz)
    const f4 q = ld4(S.lq[tid]);
    const f3 ex = qrot(q, F3(1, 0, 0)), ey = qrot(q, F3(0, 1, 0)), ez = qrot(q, F3(0, 0, 1));  // columns of R
    const f3 c0 = ex * I6[0] + ey * I6[3] + ez * I6[4];
    const f3 c1 = ex * I6[3] + ey * I6[1] + ez * I6[5];
    const f3 c2 = ex * I6[4] + ey * I6[5] + ez * I6[2];
    S.lI[tid][0] = c0.x * ex.x + c1.x * ey.x + c2.x * ez.x;
    S.lI[tid][1] = c0.y * ex.y + c1.y * ey.y + c2.y * ez.y;
    S.lI[tid][2] = c0.z * ex.z + c1.z * ey.z + c2.z * ez.z;
    S.lI[tid][3] = c0.x * ex.y + c1.x * ey.y + c2.x * ez.y;
    S.lI[tid][4] = c0.x * ex.z + c1.x * ey.z + c2.x * ez.z;
    S.lI[tid][5] = c0.y * ex.z + c1.y * ey.z + c2.y * ez.z;
    if (lmf) {
      const float f = S.lmf[tid];
#pragma unroll
      for (int i = 0; i < 6; ++i) S.lI[tid][i] *= f;
    }
  }
  WAVE_SYNC();
}

// ---------------------------------------------------------------- B: H = M + implicit PD terms, Hinv (once per step)
// off: bit i = the PD drive of dof i is off for this launch (sdx_apply_dof_forces): its implicit terms stay out of H.  Constant 0 outside the
// SDX_PHYS_FORCE instantiations of k_physics
template <int NT, bool DR = false>
__device__ __forceinline__ void mass_matrix(const SdxConst* C, PhysLds& S, int tid, float h, long long* dbg, const float* drow = nullptr, uint32_t off = 0u) {
  const sdx_scene_desc& sc = C->sc;
  for (int idx = tid; idx < ND * (ND + 1) / 2; idx += NT) {
    int i, j;
    tri_index(idx, &i, &j);
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
    if (off != 0u && i == j && ((off >> i) & 1u)) s += sc.armature[i];   // (the diagonal line of a dof whose drive is off)
    else if (DR) { if (i == j) s += sc.armature[i] + h * drow[ND + i] + h * h * drow[i]; }   // drow: this env's [kp; kd; lower; upper]
    else if (i == j) s += sc.armature[i] + h * sc.kd[i] + h * h * sc.kp[i];
    S.A[i][j] = s;
    S.A[j][i] = s;
  }
  __syncthreads();
  SSTAMP(34);
  if (tid < 64) {
    // Cholesky on wave 0 with the matrix in registers: lane i holds row i of H; right-looking - column j is scaled, then every lane
    // subtracts l_ij l_kj from its entries k > j, with l_kj read from lane k (v_readlane: wave-uniform, no LDS, no hand-off).  The
    // upper triangle carries don't-care values; lanes >= ND carry zeros.  (The left-looking LDS version took 35 k of the 58 k cycles of
    // this phase: 23 dependent columns with a wave-synchronous hand-off each.)
    float a[ND];
#pragma unroll
    for (int k = 0; k < ND; ++k) a[k] = tid < ND ? S.A[tid][k] : 0.0f;
#pragma unroll
    for (int j = 0; j < ND; ++j) {
      const float d = sqrtf(SDX_READLANE(a[j], j));
      const float lij = tid == j ? d : a[j] / d;
      a[j] = lij;
#pragma unroll
      for (int k = j + 1; k < ND; ++k) a[k] -= lij * SDX_READLANE(lij, k);
    }
    SSTAMP(35);
    // T = L^-1, lane = column c: t[i] = ([i == c] - sum_{k < i} L[i][k] t[k]) / L[i][i], t[k] = 0 above the diagonal.  L[i][k] is the same
    // for every lane: row i of L goes through LDS (lane i writes its row into the free second impulse row, every lane reads it back as
    // 16-byte broadcast loads that do not depend on the recurrence and run ahead of it).  Round 5 fetched each L[i][k] with a v_readlane
    // in front of its fma: 253 readlane -> fma pairs in one dependent chain, 9 k cycles; the sums and their order are the same.
    const int c = tid;
    float* Lrow = &S.P[1][0];   // [ND][HP]
    if (tid < ND) {
#pragma unroll
      for (int k = 0; k < ND; ++k) Lrow[tid * HP + k] = a[k];
    }
    WAVE_SYNC();
    float t[ND];
#pragma unroll
    for (int i = 0; i < ND; ++i) {
      float li[HP];
#pragma unroll
      for (int k4 = 0; k4 <= i / 4; ++k4) {
        const f4v x = *reinterpret_cast<const f4v*>(Lrow + i * HP + 4 * k4);
        li[4 * k4] = x.x; li[4 * k4 + 1] = x.y; li[4 * k4 + 2] = x.z; li[4 * k4 + 3] = x.w;
      }
      float sacc = (i == c) ? 1.0f : 0.0f;
#pragma unroll
      for (int k = 0; k < i; ++k) sacc -= li[k] * t[k];
      t[i] = i >= c ? sacc / li[i] : 0.0f;
    }
    if (tid < ND) {
#pragma unroll
      for (int i = 0; i < ND; ++i) S_T(S)[i][c] = t[i];
    }
  } else {
    broad_mask_part<NT>(C, S, tid, 1);   // the robot boxes' candidates (their poses are this substep's: FK is done) beside the factorisation
  }
  __syncthreads();
  SSTAMP(36);
  // Hinv = T^T T
  for (int idx = tid; idx < ND * (ND + 1) / 2; idx += NT) {
    int i, j;
    tri_index(idx, &i, &j);
    float s = 0.0f;
    for (int k = i; k < ND; ++k) s += S_T(S)[k][i] * S_T(S)[k][j];
    S.A[i][j] = s;
    S.A[j][i] = s;
  }
  __syncthreads();
}
