// sdx_phys_osc.h - private to sdx_physics.hip (included by it only, after sdx_phys_dynamics.h): k_osc_torques, the operational-space
// (end-effector impedance) torques of the arm at the CURRENT SDX_T_DOF (include/seqdex.h sdx_osc_torques)
#pragma once

#define OSC_NA 7   // arm dofs: the columns of SDX_T_JAC_EEF
#define OSC_WAVES 3   // waves per SIMD asked of the register allocator: 129 VGPRs without scratch; at 4 (128 VGPRs) one to three of them spill

// The serial part runs in double: it is a few hundred dependent operations on one wave whatever the type, and in float32 the two
// factorisations lose up to 4 x what a float32 LAPACK evaluation of the same law loses at a near-singular arm; in
// double the row is the float32 rounding of the law applied to the kernel's own float32 M7, J and bias.
typedef double osc_t;

// in-place Cholesky of the lower triangle of an SPD matrix, L L^T = A, with 1 / L_jj on the diagonal (one division per column).  N is a
// compile-time constant and every loop unrolls, so that every index is static and the triangle lives in registers (a runtime index into a
// private array would put it in scratch).  Wave-uniform.
template <int N>
__device__ __forceinline__ void osc_cholesky(osc_t (&A)[N][N]) {
#pragma unroll
  for (int j = 0; j < N; ++j) {
    osc_t d = A[j][j];
#pragma unroll
    for (int k = 0; k < j; ++k) d -= A[j][k] * A[j][k];
    const osc_t rd = 1.0 / sqrt(d);
    A[j][j] = rd;
#pragma unroll
    for (int i = j + 1; i < N; ++i) {
      osc_t s = A[i][j];
#pragma unroll
      for (int k = 0; k < j; ++k) s -= A[i][k] * A[j][k];
      A[i][j] = s * rd;
    }
  }
}
template <int N>
__device__ __forceinline__ void osc_forward(const osc_t (&L)[N][N], osc_t (&y)[N]) {   // y <- L^-1 y
#pragma unroll
  for (int i = 0; i < N; ++i) {
    osc_t s = y[i];
#pragma unroll
    for (int k = 0; k < i; ++k) s -= L[i][k] * y[k];
    y[i] = s * L[i][i];
  }
}
template <int N>
__device__ __forceinline__ void osc_backward(const osc_t (&L)[N][N], osc_t (&y)[N]) {   // y <- L^-T y
#pragma unroll
  for (int i = N - 1; i >= 0; --i) {
    osc_t s = y[i];
#pragma unroll
    for (int k = i + 1; k < N; ++k) s -= L[k][i] * y[k];
    y[i] = s * L[i][i];
  }
}

// what the lanes of wave 0 hand to each other in the serial part
struct OscTail {
  osc_t Y[OSC_NA][OSC_NA];   // rows 0..5: Y^T = (L^-1 J^T)^T, row 6: L^-1 u_null
  osc_t A[6][6], F[6], g[6], un[OSC_NA];
};

// One env per workgroup, k_dof_dynamics' sibling: the same loads, fk_wave0, then
//   wave 1  the 28 entries of the arm triangle of M(q) + armature (crba_entry: the hand's links at their current pose are in the sums)
//   wave 2  the 7 velocity-product bias sums (bias_torque), only when compensate_bias
//   wave 3  the 42 entries of the hand base's Jacobian, the terms of write_kinematics' SDX_T_JAC_EEF row
// and after one barrier wave 0 alone: the two factorisations with every lane the same numbers (as control_ik_solve in sdx_task.hip), the
// right-hand sides and the products between them one per lane through OscTail.  The law of DESIGN.md section 23 as it is evaluated:
//   M7 = L L^T;  Y = L^-1 J^T (row r of Y^T = L^-1 J[r]), so J M7^-1 J^T = Y^T Y and J M7^-1 x = Y^T (L^-1 x): forward solves only
//   A = Y^T Y + damping^2 I = L6 L6^T;  F = kp dpose - kd J qd;  w = A^-1 F;  u_null = M7 (kp_null (q_null - q) - kd_null qd)
//   u = J^T (w - A^-1 Y^T L^-1 u_null) + u_null (+ bias)
// torques [N, ND]: u clamped to +-effort on the arm, +0.0f on the hand; wrench [N, 6] (or nullptr) = w.
template <bool DR>
__global__ __launch_bounds__(DYN_NT, OSC_WAVES) void k_osc_torques(const SdxConst* __restrict__ C, SdxBuf B, sdx_osc_attr at, const float* __restrict__ dpose,
                                                        float* __restrict__ torques, float* __restrict__ wrench) {
  __shared__ DynLds S;
  __shared__ float SJ[6][OSC_NA], Sb[OSC_NA];
  __shared__ OscTail T;
  const sdx_scene_desc& sc = C->sc;
  const int e = blockIdx.x, tid = threadIdx.x;
  const bool comp = at.compensate_bias != 0;
  if (tid < ND) {
    S.q[tid] = B.dof[((size_t)e * ND + tid) * 2];
    S.qd[tid] = B.dof[((size_t)e * ND + tid) * 2 + 1];
    uint32_t d = 0;
    for (int k = 1; k < NL; ++k) d |= ((C->anc[k] >> tid) & 1u) << k;
    S.desc[tid] = d;
  }
  if (tid < NL) {   // (as k_dof_dynamics does: this env's link mass factors are row 0 of SDX_T_DR_LINK)
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
  if (tid < 64) fk_wave0(C, S, tid, true, comp, nullptr, DR);
  __syncthreads();
  const int lane = tid & 63, wave = tid >> 6;
  if (wave == 1 && lane < OSC_NA * (OSC_NA + 1) / 2) {
    int i, j;
    tri_index(lane, &i, &j);
    float s = crba_entry(S, i, j);
    if (i == j) s += sc.armature[i];
    S.A[i][j] = s;
  }
  if (wave == 2 && lane < OSC_NA) Sb[lane] = comp ? bias_torque(S, lane) : 0.0f;
  if (wave == 3 && lane < 6 * OSC_NA) {
    const int r = lane / OSC_NA, j = lane % OSC_NA, ee = sc.hand_base_body;
    const f3 a = ld3(S.la[j + 1]);
    const f3 lin = cross(a, ld3(S.bp[NF + ee]) - ld3(S.bp[NF + j + 1]));
    SJ[r][j] = r == 0 ? lin.x : r == 1 ? lin.y : r == 2 ? lin.z : r == 3 ? a.x : r == 4 ? a.y : a.z;
  }
  __syncthreads();
  if (wave != 0) return;

  // ---- wave 0 alone.  Uniform: M7, u_null and the 7 x 7 factor (every lane the same registers)
  osc_t M[OSC_NA][OSC_NA];   // the lower triangle, then its Cholesky factor
  {
    osc_t x[OSC_NA];
#pragma unroll
    for (int k = 0; k < OSC_NA; ++k) x[k] = (osc_t)at.kp_null[k] * ((osc_t)at.q_null[k] - (osc_t)S.q[k]) - (osc_t)at.kd_null[k] * (osc_t)S.qd[k];
#pragma unroll
    for (int i = 0; i < OSC_NA; ++i)
#pragma unroll
      for (int j = 0; j <= i; ++j) M[i][j] = (osc_t)S.A[i][j];
#pragma unroll
    for (int i = 0; i < OSC_NA; ++i) {
      osc_t s = 0.0;
#pragma unroll
      for (int k = 0; k < OSC_NA; ++k) s += (k <= i ? M[i][k] : M[k][i]) * x[k];
      T.un[i] = s;   // (every lane stores the same number)
    }
  }
  osc_cholesky<OSC_NA>(M);
  WAVE_SYNC();
  // ---- one right-hand side per lane: lanes 0..5 the rows of J (row r of Y^T = L^-1 J[r]) and F, lane 6 u_null
  {
    const int r = tid < OSC_NA ? tid : OSC_NA - 1, jr = r < 6 ? r : 5;
    osc_t y[OSC_NA], v = 0.0;
#pragma unroll
    for (int k = 0; k < OSC_NA; ++k) {
      const osc_t j = (osc_t)SJ[jr][k];
      v += j * (osc_t)S.qd[k];
      y[k] = r < 6 ? j : T.un[k];
    }
    float kp = 0.0f, kd = 0.0f;   // (a select chain: the attributes are kernel arguments, a lane index into them would be a copy in scratch)
#pragma unroll
    for (int c = 0; c < 6; ++c) if (jr == c) { kp = at.kp[c]; kd = at.kd[c]; }
    osc_forward<OSC_NA>(M, y);
    if (tid < OSC_NA) {
#pragma unroll
      for (int k = 0; k < OSC_NA; ++k) T.Y[r][k] = y[k];
    }
    if (tid < 6) T.F[r] = (osc_t)kp * (osc_t)dpose[(size_t)e * 6 + r] - (osc_t)kd * v;
  }
  WAVE_SYNC();
  // ---- one product per lane: lanes 0..20 the triangle of A = Y^T Y + damping^2 I, lanes 21..26 g = Y^T (L^-1 u_null)
  {
    int r, c;
    tri_index(tid < 21 ? tid : 0, &r, &c);
    if (tid >= 21) { r = tid < 27 ? tid - 21 : 5; c = 6; }
    osc_t s = tid < 21 && r == c ? (osc_t)at.damping * (osc_t)at.damping : 0.0;
#pragma unroll
    for (int k = 0; k < OSC_NA; ++k) s += T.Y[r][k] * T.Y[c][k];
    if (tid < 21) T.A[r][c] = s;
    else if (tid < 27) T.g[r] = s;
  }
  WAVE_SYNC();
  // ---- uniform again: the 6 x 6 factor and the two solves
  osc_t A[6][6], F[6], g[6];
#pragma unroll
  for (int r = 0; r < 6; ++r) {
#pragma unroll
    for (int c = 0; c <= r; ++c) A[r][c] = T.A[r][c];
    F[r] = T.F[r]; g[r] = T.g[r];
  }
  osc_cholesky<6>(A);
  osc_forward<6>(A, F); osc_backward<6>(A, F);   // F is now the wrench w
  osc_forward<6>(A, g); osc_backward<6>(A, g);
  // ---- one output per lane
  const int j = tid < OSC_NA ? tid : 0;
  osc_t s = 0.0;
  float wout = 0.0f;
#pragma unroll
  for (int r = 0; r < 6; ++r) {
    s += (osc_t)SJ[r][j] * (F[r] - g[r]);
    if (tid == r) wout = (float)F[r];
  }
  s += T.un[j];
  if (comp) s += (osc_t)Sb[j];
  if (tid < ND) {
    const float lim = sc.effort[tid], out = (float)s;
    // (+ 0.0f: a sum of zeros of either sign leaves as +0.0f; the hand's columns are +0.0f, so that their PD drives see no torque)
    torques[(size_t)e * ND + tid] = tid < OSC_NA ? fminf(lim, fmaxf(-lim, out)) + 0.0f : 0.0f;
  }
  if (wrench && tid < 6) wrench[(size_t)e * 6 + tid] = wout;
}
