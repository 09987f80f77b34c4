// sdx_phys_ik.h - private to sdx_physics.hip (included by it only, after sdx_phys_osc.h): k_solve_ik, the pose solver - the 23 joint angles
// that put the hand base at a pose and the four fingertips at points (include/seqdex.h sdx_solve_ik)
#pragma once

#define IK_NT 64      // one wave per env: the whole iteration is one dependent chain (7 joint levels, a 6 x 6 factor, a step), nothing to share out
#define IK_NA 7       // arm dofs: links 1 .. 7 in a serial chain, link 7 the hand base (sdx_solve_ik checks the scene for this shape)
#define IK_NFD 4      // dofs of a finger: links 8 + 4 f .. 11 + 4 f in a serial chain below the hand base

// one joint of fk_wave0 (sdx_phys_robot.h), the same operations in the same order: the pose of link k and its axis in the world from the
// pose (qp, pp) of its parent and its angle.  k may differ from lane to lane (the fingers): the scene's rows are read from memory
__device__ __forceinline__ void ik_joint(const sdx_scene_desc& sc, int k, float ang, f4 qp, f3 pp, f4* qk, f3* pk, f3* ak) {
  const f4 jq = ld4(sc.joint_quat[k]);
  const f3 ax = ld3(sc.joint_axis[k]);
  float sn, cs;
  sincosf(0.5f * ang, &sn, &cs);
  f4 qa; qa.x = ax.x * sn; qa.y = ax.y * sn; qa.z = ax.z * sn; qa.w = cs;
  *qk = qnormalize(qmul(qp, qmul(jq, qa)));
  *pk = pp + qrot(qp, ld3(sc.joint_pos[k]));
  *ak = qrot(qp, qrot(jq, ax));
}
// dq <- dq / max(1, max_j |dq_j| / max_step);  q <- clamp(q + dq, lower, upper)
template <int N>
__device__ __forceinline__ void ik_step(float (&q)[N], const osc_t (&dq)[N], const float (&lo)[N], const float (&up)[N], float max_step) {
  osc_t m = 0.0;
#pragma unroll
  for (int j = 0; j < N; ++j) m = fmax(m, fabs(dq[j]));
  const osc_t scale = 1.0 / fmax(1.0, m / (osc_t)max_step);
#pragma unroll
  for (int j = 0; j < N; ++j) q[j] = fminf(up[j], fmaxf(lo[j], (float)((osc_t)q[j] + dq[j] * scale)));
}

// One env per workgroup of one wave.  The law of DESIGN.md section 25 as it is evaluated:
//   stage 1 (bit 0), every lane the same numbers in registers (as the factorisations of k_osc_torques): up to max_iters times
//     the 7 joint levels of the arm;  e = [target - p7 ; s 2 xyz(target (x) conj(q7))];  stop when both parts meet their tolerance;
//     J = the terms of SDX_T_JAC_EEF;  A = J J^T + damping_arm^2 I = L L^T;  dq = J^T A^-1 e;  ik_step
//   stage 2 (bits 1..4), lane f = finger f below the arm of stage 1 (lanes 4.. repeat the four and store nothing): the same loop on the
//     finger's 4 levels, the point c = p_tip + R_tip tip_offset[f], a 3 x 4 Jacobian of c, a 3 x 3 system with damping_finger
// Positions, axes and Jacobian entries are float32 and fk_wave0's: the pose that sdx_refresh_kinematics shows at q_out is the pose the loop
// stopped at.  A, its factor, the two solves and the step are double (osc_t): they are a hundred dependent operations per iteration on one
// wave whatever the type, and in double the step is the float32 rounding of the law applied to the kernel's own J and e.
// Nothing is indexed at run time but memory: every register array is unrolled with static indices (no scratch).  q0 and q_out may be the
// same buffer: every lane has read its part before the barrier, and writes after it.
__global__ __launch_bounds__(IK_NT) void k_solve_ik(const SdxConst* __restrict__ C, SdxBuf B, sdx_ik_attr at, const float* q0, const float* __restrict__ base_pos,
                                                    const float* __restrict__ base_quat, const float* __restrict__ tip_pos, float* q_out,
                                                    float* __restrict__ err_out, int32_t* __restrict__ info_out) {
  const sdx_scene_desc& sc = C->sc;
  const int e = blockIdx.x, tid = threadIdx.x;
  const float* drow = B.dr_on ? B.dr_dof + (size_t)e * 4 * ND : nullptr;   // this env's [kp; kd; lower; upper]: the limits the physics enforces
  const bool arm_on = (at.task_mask & 1u) != 0;
  const bool arm_stops = at.pos_tol > 0.0f && at.rot_tol > 0.0f, fin_stops = at.pos_tol > 0.0f;   // a tolerance of 0 is never met, not even by an error of 0
  // ---- stage 1: the arm, wave-uniform
  float q[IK_NA], lo[IK_NA], up[IK_NA];
#pragma unroll
  for (int j = 0; j < IK_NA; ++j) {
    q[j] = q0 ? q0[(size_t)e * ND + j] : B.dof[((size_t)e * ND + j) * 2];
    lo[j] = drow ? drow[2 * ND + j] : sc.lower[j];
    up[j] = drow ? drow[3 * ND + j] : sc.upper[j];
  }
  f3 tp = F3(0, 0, 0);
  f4 tq = {0, 0, 0, 1};
  if (arm_on) { tp = ld3(base_pos + (size_t)e * 3); tq = ld4(base_quat + (size_t)e * 4); }
  f4 q7;
  f3 p7;
  float arm_pos = 0.0f, arm_rot = 0.0f;
  int arm_it = 0;
  bool arm_conv = false;
  for (;;) {
    f3 p[IK_NA + 1], a[IK_NA + 1];
    f4 qk = ld4(sc.base_quat);
    p[0] = ld3(sc.base_pos);
#pragma unroll
    for (int k = 1; k <= IK_NA; ++k) ik_joint(sc, k, q[k - 1], qk, p[k - 1], &qk, &p[k], &a[k]);
    q7 = qk; p7 = p[IK_NA];
    if (!arm_on) break;   // (the fingers need the hand base's pose at q0)
    const f3 ep = tp - p7;
    const f4 r = qmul(tq, qconj(q7));
    const float sg = r.w < 0.0f ? -2.0f : 2.0f;
    const f3 er = F3(sg * r.x, sg * r.y, sg * r.z);
    arm_pos = sqrtf(dot(ep, ep)); arm_rot = sqrtf(dot(er, er));
    if (arm_stops && arm_pos <= at.pos_tol && arm_rot <= at.rot_tol) { arm_conv = true; break; }
    if (arm_it >= at.max_iters) break;
    f3 jl[IK_NA];   // the linear rows of J, column by column; the angular rows are the axes a[1 .. 7]
#pragma unroll
    for (int j = 0; j < IK_NA; ++j) jl[j] = cross(a[j + 1], p7 - p[j + 1]);
    osc_t A[6][6], y[6] = {ep.x, ep.y, ep.z, er.x, er.y, er.z};
#pragma unroll
    for (int r_ = 0; r_ < 6; ++r_)
#pragma unroll
      for (int c = 0; c <= r_; ++c) {
        osc_t s = r_ == c ? (osc_t)at.damping_arm * (osc_t)at.damping_arm : 0.0;
#pragma unroll
        for (int j = 0; j < IK_NA; ++j) {
          const float jr = r_ == 0 ? jl[j].x : r_ == 1 ? jl[j].y : r_ == 2 ? jl[j].z : r_ == 3 ? a[j + 1].x : r_ == 4 ? a[j + 1].y : a[j + 1].z;
          const float jc = c == 0 ? jl[j].x : c == 1 ? jl[j].y : c == 2 ? jl[j].z : c == 3 ? a[j + 1].x : c == 4 ? a[j + 1].y : a[j + 1].z;
          s += (osc_t)jr * (osc_t)jc;
        }
        A[r_][c] = s;
      }
    osc_cholesky<6>(A);
    osc_forward<6>(A, y); osc_backward<6>(A, y);
    osc_t dq[IK_NA];
#pragma unroll
    for (int j = 0; j < IK_NA; ++j)
      dq[j] = (osc_t)jl[j].x * y[0] + (osc_t)jl[j].y * y[1] + (osc_t)jl[j].z * y[2] + (osc_t)a[j + 1].x * y[3] + (osc_t)a[j + 1].y * y[4] + (osc_t)a[j + 1].z * y[5];
    ik_step<IK_NA>(q, dq, lo, up, at.max_step);
    ++arm_it;
  }
  // ---- stage 2: the fingers, one per lane
  const int f = tid & 3, d0 = IK_NA + IK_NFD * f;   // the finger's first dof; its links are d0 + 1 .. d0 + 4
  const bool fin_on = ((at.task_mask >> (1 + f)) & 1u) != 0;
  float fq[IK_NFD], flo[IK_NFD], fup[IK_NFD];
#pragma unroll
  for (int i = 0; i < IK_NFD; ++i) {
    fq[i] = q0 ? q0[(size_t)e * ND + d0 + i] : B.dof[((size_t)e * ND + d0 + i) * 2];
    flo[i] = drow ? drow[2 * ND + d0 + i] : sc.lower[d0 + i];
    fup[i] = drow ? drow[3 * ND + d0 + i] : sc.upper[d0 + i];
  }
  float fin_err = 0.0f;
  int fin_it = 0;
  bool fin_conv = false;
  if (fin_on) {
    f3 off = F3(0, 0, 0);   // (a select chain: the attributes are kernel arguments, a lane index into them would be a copy in scratch)
#pragma unroll
    for (int g = 0; g < 4; ++g) if (f == g) off = F3(at.tip_offset[g][0], at.tip_offset[g][1], at.tip_offset[g][2]);
    const f3 tc = ld3(tip_pos + ((size_t)e * 4 + f) * 3);
    for (;;) {
      f3 p[IK_NFD], a[IK_NFD], pk = p7;
      f4 qk = q7;
#pragma unroll
      for (int i = 0; i < IK_NFD; ++i) { ik_joint(sc, d0 + 1 + i, fq[i], qk, pk, &qk, &p[i], &a[i]); pk = p[i]; }
      const f3 c = pk + qrot(qk, off);
      const f3 ec = tc - c;
      fin_err = sqrtf(dot(ec, ec));
      if (fin_stops && fin_err <= at.pos_tol) { fin_conv = true; break; }
      if (fin_it >= at.max_iters) break;
      f3 jl[IK_NFD];
#pragma unroll
      for (int i = 0; i < IK_NFD; ++i) jl[i] = cross(a[i], c - p[i]);
      osc_t A[3][3], y[3] = {ec.x, ec.y, ec.z};
#pragma unroll
      for (int r_ = 0; r_ < 3; ++r_)
#pragma unroll
        for (int c_ = 0; c_ <= r_; ++c_) {
          osc_t s = r_ == c_ ? (osc_t)at.damping_finger * (osc_t)at.damping_finger : 0.0;
#pragma unroll
          for (int i = 0; i < IK_NFD; ++i) {
            const float jr = r_ == 0 ? jl[i].x : r_ == 1 ? jl[i].y : jl[i].z, jc = c_ == 0 ? jl[i].x : c_ == 1 ? jl[i].y : jl[i].z;
            s += (osc_t)jr * (osc_t)jc;
          }
          A[r_][c_] = s;
        }
      osc_cholesky<3>(A);
      osc_forward<3>(A, y); osc_backward<3>(A, y);
      osc_t dq[IK_NFD];
#pragma unroll
      for (int i = 0; i < IK_NFD; ++i) dq[i] = (osc_t)jl[i].x * y[0] + (osc_t)jl[i].y * y[1] + (osc_t)jl[i].z * y[2];
      ik_step<IK_NFD>(fq, dq, flo, fup, at.max_step);
      ++fin_it;
    }
  }
  const uint32_t fin_bits = (uint32_t)(__ballot(fin_conv) & 0xFull);   // lanes 0 .. 3: fingers ff, mf, rf, th
  __syncthreads();   // q_out may be q0: every lane has read
  if (tid < IK_NA) {
    float v = q[0];
#pragma unroll
    for (int j = 1; j < IK_NA; ++j) if (tid == j) v = q[j];
    q_out[(size_t)e * ND + tid] = v;
  }
  if (tid < 4) {
#pragma unroll
    for (int i = 0; i < IK_NFD; ++i) q_out[(size_t)e * ND + d0 + i] = fq[i];
    if (err_out) err_out[(size_t)e * 6 + 2 + f] = fin_err;
    if (info_out) info_out[(size_t)e * 6 + 2 + f] = fin_it;
  }
  if (tid == 0) {
    if (err_out) { err_out[(size_t)e * 6] = arm_pos; err_out[(size_t)e * 6 + 1] = arm_rot; }
    if (info_out) { info_out[(size_t)e * 6] = (int32_t)((arm_conv ? 1u : 0u) | (fin_bits << 1)); info_out[(size_t)e * 6 + 1] = arm_it; }
  }
}
