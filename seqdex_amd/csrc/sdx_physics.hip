// sdx_physics.hip — the per-env physics step: one workgroup per env, TWO workgroups resident per CU.
//
// Replaces gym.simulate()/fetch_results() (BT:138-144) and the refresh_* calls (GS:1091-1095) of the reference, whose arithmetic
// lives in the closed Isaac Gym / PhysX binary.  The step is OUR definition ("SDX-1"), restated independently in
// plain C in oracle/physics_oracle.c:
//   A FK  B joint-space inertia + implicit-PD matrix, Cholesky inverse  C implicit PD drive, velocity-product terms, gravity
//   D sampled-SDF box/box contacts (<= 4 per pair of boxes; every shape a compound of boxes)  E active-set mass-split Jacobi on accumulated impulses
//   F semi-implicit Euler;  then outputs: rigid-body states, end-effector Jacobian, net arm contact forces.
//
// Shape of the kernel (rewritten in round 2, restructured in round 3):
//   * 512 threads (8 waves, <= 128 VGPRs) per env, two workgroups per CU (LDS <= 80 KiB each), so one env's barrier / latency phases overlap
//     the other env's arithmetic; launch order = envs by the cost of their previous step, longest first (k_order);
//   * contact geometry (point, normal) stays in LDS; each lane keeps only what changes or divides per iteration for its 3 contacts in
//     registers (accumulated impulses, un-split inverse masses of both sides, target velocity, body ids);
//   * per solver iteration: [AC] relative velocity, active flag -> counted for the NEXT iteration (integer LDS atomics), Jacobi update with
//     the counts of the previous one, impulse to LDS | barrier | [D] CSR gather per body (8 lanes per link, 1..16 per brick by the length
//     of its list); links project their wrench on the dofs of their path | the link lanes' own barrier | robot only: every 8-lane group
//     sums the generalised impulses, applies Hinv and rebuilds its link's twist | barrier.  The solver is the list of its stages, one
//     function per phase-clock interval of tools/time_physics.py (sdx_phys_solve.h);
//   * everything serial (FK levels, Cholesky in registers, drive, twists) runs on wave 0 with wave-synchronous hand-offs instead of
//     workgroup barriers; the other waves meet it at the next barrier;
//   * broadphase: every lane tests its strided candidate BODY pairs (bounding boxes) into a bit mask, ONE block scan places all hits; the
//     surviving body pairs are expanded into the box pairs of the two compounds (consecutive candidates per lane, separating-axis test);
//     narrowphase: lane = box pair picks the samples, lane = contact computes their geometry.
//
// One translation unit in eleven files.  The device code of the phases lives in headers that only this file includes, in this order (each
// may use what the ones before it define; none forward-declares a function of another):
//   sdx_phys_lds.h      constants, wave hand-offs (WAVE_SYNC, WAVES_BARRIER, WAVE_SIGNAL / WAVES_WAIT), PhysLds and the table of its overlays,
//                       Box, the clock / ablation macros
//   sdx_phys_shapes.h   signed distance of a box, compound shapes, dir_setup ... pair_contacts, point_vel
//   sdx_phys_broad.h    tri_index, block_scan_small, the candidate tests, broad_mask_part
//   sdx_phys_robot.h    A / B: inertia_mul, twists_wave0, fk_wave0, mass_matrix
//   sdx_phys_collide.h  D: collide
//   sdx_phys_solve.h    E: solve and its stages: load_rows, warm_match, csr_clear .. csr_rank, link_inertia, row_weights, pass_setup,
//                       loop_registers; per pass contact_update [AC], gather [D], robot_section; solve_exit; the contact report's two
//                       write sites report_setup, report_result
//   sdx_phys_dynamics.h k_dof_dynamics: mass matrix, bias and drive torques outside any step (sdx_dof_dynamics)
//   sdx_phys_osc.h      k_osc_torques: operational-space torques of the arm outside any step (sdx_osc_torques)
//   sdx_phys_ik.h       k_solve_ik: arm and fingertip inverse kinematics outside any step (sdx_solve_ik)
//   sdx_phys_report.h   k_contact_wrenches: per-body wrenches and sensor / filter forces from a contact report (sdx_contact_wrenches)
//   this file           write_kinematics, load_constants, k_physics (C the drive and F the integration are in its body), k_order,
//                       k_kinematics, the launchers
#include <stdlib.h>

#include "sdx_kernels.h"   // (includes sdx_common.h)

#include "sdx_phys_lds.h"
#include "sdx_phys_shapes.h"
#include "sdx_phys_broad.h"
#include "sdx_phys_robot.h"
#include "sdx_phys_collide.h"
#include "sdx_phys_solve.h"
#include "sdx_phys_dynamics.h"
#include "sdx_phys_osc.h"
#include "sdx_phys_ik.h"
#include "sdx_phys_report.h"

// ---------------------------------------------------------------- outputs shared by step and refresh
template <int NT>
__device__ __forceinline__ void write_kinematics(const SdxConst* C, PhysLds& S, const SdxBuf& B, int e, int tid) {
  const sdx_scene_desc& sc = C->sc;
  float* rb_e = B.rb + (size_t)e * SDX_BODIES * 13;
  for (int i = tid; i < NL * 13; i += NT) {
    const int k = i / 13, c = i % 13;
    float v;
    if (c < 3) v = S.bp[NF + k][c];
    else if (c < 7) v = S.lq[k][c - 3];
    else if (c < 10) v = S.bv[NF + k][c - 7];
    else v = S.bw[NF + k][c - 10];
    rb_e[i] = v;
  }
  if (tid < 42) {  // geometric Jacobian of the hand-base body origin wrt the 7 arm dofs (GS:1601)
    const int r = tid / 7, j = tid % 7, ee = sc.hand_base_body;
    const f3 a = ld3(S.la[j + 1]);
    const f3 lin = cross(a, ld3(S.bp[NF + ee]) - ld3(S.bp[NF + j + 1]));
    const float v = r == 0 ? lin.x : r == 1 ? lin.y : r == 2 ? lin.z : r == 3 ? a.x : r == 4 ? a.y : a.z;
    B.jac[(size_t)e * 42 + tid] = v;
  }
}

// per-env constants into LDS (bricks, robot boxes, statics, ancestor masks)
template <int NT, bool DR = false>
__device__ __forceinline__ void load_constants(const SdxConst* C, PhysLds& S, int e, int tid, const SdxBuf* Bp = nullptr) {
  const sdx_scene_desc& sc = C->sc;
  const int segb = seg_actor(e) - SDX_ACTOR_BRICK0;
  if (tid == 0) {
    S.seg_brick = segb;
    st3(S.bp[BODY_W], F3(0, 0, 0)); st3(S.bv[BODY_W], F3(0, 0, 0)); st3(S.bw[BODY_W], F3(0, 0, 0));   // the static world
  }
  if (DR) {   // this env's link mass factors (SDX_T_DR_LINK row 0)
    if (tid < NL) {
      const float f = Bp->dr_link[(size_t)e * 2 * NL + tid];
      S.anc[tid] = C->anc[tid]; S.lmass[tid] = sc.link_mass[tid] * f; S.lmf[tid] = f;
    }
  } else if (tid < NL) { S.anc[tid] = C->anc[tid]; S.lmass[tid] = sc.link_mass[tid]; }
  if (tid < ND) {
    uint32_t d = 0;
    for (int k = 1; k < NL; ++k) d |= ((C->anc[k] >> tid) & 1u) << k;
    S.desc[tid] = d;
  }
  if (tid <= NL) S.par[tid] = tid < NL ? (tid == 0 ? 0 : sc.parent[tid]) : NL;
  if (tid == 0) { S.qd[ND] = 0.0f; st3(S.la[NL], F3(0, 0, 0)); st3(S.lal[NL], F3(0, 0, 0)); }
  const int segt = sc.brick_type[segb];
  for (int i = tid; i < NF; i += NT) {
    const int t = sc.brick_type[i];
    S.btype[i] = (unsigned char)t;
    S.bim[i] = (i == segb ? 1.0f / sc.seg_mass_scale : 1.0f) / sc.brick_mass[t];
    if (DR) S.bim[i] /= Bp->dr_brick[(size_t)e * 2 * NF + i];
  }
  // collision compounds of the 8 brick types (centre-of-mass frame) and the hollow compound of this env's target brick
  if (tid < SDX_NBRICK_TYPES) {
    const int t = tid;
    const f3 com = ld3(sc.brick_com[t]), bc = ld3(sc.brick_center[t]) - com, bh = ld3(sc.brick_half[t]);
    S.tn[t] = sc.brick_nsub[t];
    st3(S.tbc[t], bc); st3(S.tbh[t], bh);
    S.trad[t] = sqrtf(dot(bc, bc)) + C->brick_radius[t];
    S.tii[t][0] = sc.brick_mass[t] / sc.brick_inertia[t][0]; S.tii[t][1] = sc.brick_mass[t] / sc.brick_inertia[t][1];
    S.tii[t][2] = sc.brick_mass[t] / sc.brick_inertia[t][2];
    for (int k = 0; k < SDX_MAX_SUB; ++k) { st3(S.tsc[t][k], ld3(sc.brick_sub_center[t][k]) - com); st3(S.tsh[t][k], ld3(sc.brick_sub_half[t][k])); }
  }
  if (tid >= 128 && tid < 128 + SDX_NSAMP * 3) (&S.samp[0][0])[tid - 128] = (&c_samp[0][0])[tid - 128];
  if (tid >= 256 && tid < 260) S.qid[tid - 256] = tid == 259 ? 1.0f : 0.0f;
  if (tid >= 64 && tid < 64 + SDX_MAX_SUB_HOLLOW) {
    const int k = tid - 64;
    st3(S.hsc[k], ld3(sc.hollow_sub_center[segt][k]) - ld3(sc.brick_com[segt])); st3(S.hsh[k], ld3(sc.hollow_sub_half[segt][k]));
    if (k == 0) S.hn = sc.seg_hollow ? sc.hollow_nsub[segt] : 0;
  }
  if (tid < SDX_MAX_RBOX) {
    const bool on = tid < sc.n_rbox;
    S.rbl[tid] = on ? sc.rbox_link[tid] : 0;
    st3(S.rh[tid], on ? ld3(sc.rbox_half[tid]) : F3(0, 0, 0));
    S.rrad[tid] = on ? C->rbox_radius[tid] : 0.0f;
  }
  if (tid < SDX_MAX_STATIC) {   // InsertSim's base plate is one of three by env % 3: a row of the static-body table each (sdx_scene_desc.static_var_*)
    const int row = tid == sc.static_var_slot ? sc.static_var_row[e % 3] : tid;
    st3(S.stc[tid], ld3(sc.static_center[row])); st3(S.sth[tid], ld3(sc.static_half[row]));
    S.ssf[tid] = sc.static_sub_first[row]; S.ssn[tid] = tid < sc.n_static ? sc.static_sub_n[row] : 1;
  }
}

// ---------------------------------------------------------------- the step kernel
// NTD = threads | SDX_PHYS_DR | SDX_PHYS_FORCE.  k_physics<512 | SDX_PHYS_DR> is the domain-randomization variant: drive gains, joint limits, link / brick
// masses, friction and gravity come from this env's rows of SDX_T_DR_* instead of the scene constants.  (The flag rides in the low bit of
// the thread count so that k_physics<512> keeps its symbol and its code: a second template parameter renames the symbol, a __global__
// wrapper around a shared body changes the default kernel's register allocation.)
#define SDX_PHYS_DR 1
// k_physics<.. | SDX_PHYS_FORCE>: the external wrench of include/seqdex.h sdx_apply_rigid_body_forces acts on the
// free bricks beside gravity and on the robot links beside their velocity-product wrenches.  A second flag bit, for the same reason.
#define SDX_PHYS_FORCE 2
// k_physics<.. | SDX_PHYS_REPORT>: the last substep's solve also writes the contact report of include/seqdex.h sdx_set_contact_report (DESIGN.md
// section 24) into the caller's buffers.  Their seven pointers are read from B.cscratch, a device copy of the struct that k_report_table
// (sdx_phys_report.h) writes in front of every such launch: SdxBuf does not grow, so no kernel that takes arguments behind the buffer
// table sees them move, and the pointers are loaded where they are used instead of living in the argument registers.  A third flag
// bit, for the same reason as the other two: k_physics<512 .. 515> keep symbol and code.
#define SDX_PHYS_REPORT 4
#define SDX_PHYS_FLAGS (SDX_PHYS_DR | SDX_PHYS_FORCE | SDX_PHYS_REPORT)
// k_physics<.. | SDX_PHYS_DR>: row e of one of the SDX_T_DR_* tensors, addressed from an opaque copy of e at the point of use (nothing is
// hoisted to the kernel's entry and kept alive over the substeps)
__device__ __forceinline__ const float* dr_row(const float* base, int e, int width, int off) {
  int ee = e;
  SDX_OPAQUE_S(ee);
  return base + (size_t)ee * width + off;
}
// k_physics<.. | SDX_PHYS_FORCE>: the world wrench (F, T) on one body in this substep; false: its rows are all zero and the body is stepped
// as without the feature (x + 0 would turn a -0 into +0).  body: its row of the caller's tensors [N, SDX_BODIES, 3]; slot: its row of
// B.ext_world (bricks 0.., links NF..); q: its orientation at the start of the step, used by the first substep of a SDX_SPACE_LOCAL
// wrench, which leaves the rotated rows in B.ext_world for the later ones (the same lane reads what it wrote).  Addressed like DR_ROW:
// nothing is kept over the substeps.
__device__ __forceinline__ bool ext_wrench(const SdxBuf& B, int e, int body, int slot, f4 q, bool first, f3& F, f3& T) {
  int ee = e;
  SDX_OPAQUE_S(ee);
  F = F3(0, 0, 0);
  T = F3(0, 0, 0);
  const bool local = B.ext_space == SDX_SPACE_LOCAL;
  float* w = B.ext_world + ((size_t)ee * (NF + NL) + slot) * 6;
  if (local && !first) {
    F = ld3(w);
    T = ld3(w + 3);
  } else {
    const size_t at = ((size_t)ee * SDX_BODIES + body) * 3;
    if (B.ext_force) F = ld3(B.ext_force + at);
    if (B.ext_torque) T = ld3(B.ext_torque + at);
    if (local) {
      F = qrot(q, F);
      T = qrot(q, T);
      st3(w, F);
      st3(w + 3, T);
    }
  }
  return F.x != 0.0f || F.y != 0.0f || F.z != 0.0f || T.x != 0.0f || T.y != 0.0f || T.z != 0.0f;
}
// k_physics<.. | SDX_PHYS_FORCE>: the actuation torque of dof j in this substep (include/seqdex.h sdx_apply_dof_forces; 0: none pending, or
// a zero row - the dof is stepped as without the call).  Addressed like DR_ROW: nothing is kept over the substeps.
__device__ __forceinline__ float dof_force(const SdxBuf& B, int e, int j) {
  int ee = e;
  SDX_OPAQUE_S(ee);
  return B.dof_force ? B.dof_force[(size_t)ee * ND + j] : 0.0f;
}
template <int NTD>
__global__ __launch_bounds__(NTD & ~SDX_PHYS_FLAGS, 2 * (NTD & ~SDX_PHYS_FLAGS) / 256) void k_physics(const SdxConst* __restrict__ C, SdxBuf B) {
  constexpr int NT = NTD & ~SDX_PHYS_FLAGS;
  constexpr bool DR = (NTD & SDX_PHYS_DR) != 0;
  constexpr bool FORCE = (NTD & SDX_PHYS_FORCE) != 0;
  constexpr bool REPORT = (NTD & SDX_PHYS_REPORT) != 0;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  PhysLds& S = *reinterpret_cast<PhysLds*>(smem);
  // launch order: B.order lists the envs by the cost of their previous step, longest first (k_order below)
  // (the loaded index is wave-uniform, but only readfirstlane tells the compiler: every address derived from it stays in scalar registers)
  const int e = B.order ? SDX_UNIFORM(B.order[blockIdx.x]) : (int)blockIdx.x, tid = threadIdx.x;
  const sdx_scene_desc& sc = C->sc;
  float* root_e = B.root + (size_t)e * SDX_ACTORS * 13;
  const float h = sc.dt / (float)sc.substeps;
#ifdef SDX_PHASE_CLOCK
  const int abl_bits = (int)B.dbg[63];
#else
  constexpr int abl_bits = 0;
#endif

  // this env's cycle count decides its place in the NEXT launch's order (k_order below): the clock is read by thread 0 at entry and exit
  const long long t_in = (long long)__builtin_readcyclecounter();
#ifdef SDX_PHASE_CLOCK
  if (threadIdx.x == 0) {
    B.dbg[64 + 2 * e] = t_in;                 // (entry, exit) of every env
    if (e == B.dbg_env) B.dbg[13] = t_in;     // kernel entry of the debug env
  }
#endif
  // ---- load per-env state (coalesced rows) into LDS.  The state rows are requested first and stored last: their HBM / L2 round trips run
  // beside the (dependent) loads of the scene constants instead of after them
  static_assert(NF <= NT, "one brick per lane");
  float r_q = 0.0f, r_qd = 0.0f, r_tg = 0.0f;
  if (tid < ND) {
    r_q = B.dof[((size_t)e * ND + tid) * 2];
    r_qd = B.dof[((size_t)e * ND + tid) * 2 + 1];
    r_tg = B.targets[(size_t)e * ND + tid];
  }
  const float* srow = root_e + (SDX_ACTOR_BRICK0 + (tid < NF ? tid : 0)) * 13;
  const f3 r_p = ld3(srow), r_v = ld3(srow + 7), r_w = ld3(srow + 10);
  const f4 r_o = ld4(srow + 3);
  const f3 r_com = ld3(sc.brick_com[sc.brick_type[tid < NF ? tid : 0]]);
  load_constants<NT, DR>(C, S, e, tid, &B);
  if (DR && blockIdx.x == 0 && tid == 0) B.dr_frame[0] += 1;   // gym.get_frame_count: one per launch (read by the next launch's sampling)
  // this env's rows of SDX_T_DR_* (include/seqdex.h): [kp; kd; lower; upper], [link mass factor; link friction], [brick mass factor; friction].
  // Addressed where they are used (DR_ROW): pointers and gravity held over the whole kernel pushed the variant into scratch
#define DR_ROW(field, width, off) (DR ? dr_row(B.field, e, (width), (off)) : nullptr)
  if (tid < ND) { S.q[tid] = r_q; S.qd[tid] = r_qd; S.tgt[tid] = r_tg; }
  if (tid < NF) {
    const f4 q = qnormalize(r_o);
    st4(S.bq[tid], q);
    st3(S.bp[tid], r_p + qrot(q, r_com));
    st3(S.bv[tid], r_v);
    st3(S.bw[tid], r_w);
  }
  for (int i = tid; i < NT; i += NT) S_BMASK(S)[i] = 0u;
  if (tid == 0) S.fkflag = 0;
  __syncthreads();

  const int nsub = sc.substeps;
  for (int sub = 0; sub < nsub; ++sub) {
    // per-substep opaque copies of the constants pointer and the thread index: without them every loop-invariant load and address
    // of the substep body (scene constants, per-lane offsets) is hoisted in front of the loop and parked in scratch - 48 spills per
    // lane, 100 MB of scratch writes per launch at N = 1024 (profiles/r2_kphysics_pmc_write.csv before this change)
    const SdxConst* Cs = C;
    SDX_OPAQUE_S(Cs);
    int tl = threadIdx.x;
    SDX_OPAQUE(tl);
    const sdx_scene_desc& scl = Cs->sc;
    PSTAMP(0);
    if (sub == 0) {   // M(q) is evaluated once per step (frozen over the substeps)
      // wave 0: forward kinematics + inertias; waves 1..7 meanwhile: the broadphase tests of the brick / brick and brick / static
      // candidates (part 0), which depend on nothing the robot does in this substep
      if (tl < 64) fk_wave0(Cs, S, tl, true, true, e == B.dbg_env ? B.dbg : nullptr, DR);
      else if (!ABL(32)) broad_mask_part<NT>(Cs, S, tl, 0);
      __syncthreads();
      PSTAMP(1);
      if (!ABL(512)) mass_matrix<NT, DR>(Cs, S, tl, h, e == B.dbg_env ? B.dbg : nullptr, DR_ROW(dr_dof, 4 * ND, 0), FORCE ? B.dof_off : 0u);   // (part 1 of the mask beside its wave-0 section)
      else { if (tl >= 64) broad_mask_part<NT>(Cs, S, tl, 1); __syncthreads(); }
      PSTAMP(2);
    }
    // A + C on wave 0 (FK, implicit PD drive (P1), velocity-product bias torques, twists); the other waves: gravity on the free bricks
    if (ABL(256) && sub != 0) {
      if (tl >= 64) { broad_mask_part<NT>(Cs, S, tl, 0); broad_mask_part<NT>(Cs, S, tl, 1); }
    } else if (tl < 64) {
      if (sub != 0) { fk_wave0(Cs, S, tl, false, true, nullptr, DR); WAVE_SIGNAL(&S.fkflag, sub); }   // (the robot boxes are placed: part 1 of the mask may start)
      if (FORCE) {   // the external wrench of link tl enters where its inertial wrench does: (lF, lN) -= (F, T); nothing but the drive below reads them
        if (tl > 0 && tl < NL) {
          f3 F, T;
          if (ext_wrench(B, e, tl, NF + tl, ld4(S.lq[tl]), sub == 0, F, T)) { st3(S.lF[tl], ld3(S.lF[tl]) - F); st3(S.lN[tl], ld3(S.lN[tl]) - T); }
        }
        WAVE_SYNC();
      }
      if (tl < ND) {
        const float* drow = DR_ROW(dr_dof, 4 * ND, 0);
        const float t = DR ? drow[tl] * (S.tgt[tl] - S.q[tl]) - (drow[ND + tl] + h * drow[tl]) * S.qd[tl]   // (drow: kp, kd rows)
                           : scl.kp[tl] * (S.tgt[tl] - S.q[tl]) - (scl.kd[tl] + h * scl.kp[tl]) * S.qd[tl];
        // velocity-product bias torque of dof tl: inertial wrenches of the links below it, projected on its axis
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
        if (FORCE) {   // sdx_apply_dof_forces: a drive that is off gives nothing; the actuation torque has the effort limit of its own
          int jl = tl;
          SDX_OPAQUE_AFTER(jl, tc);   // (nothing of this block is hoisted in front of the bias sum, whose operands fill the registers)
          float drive = (B.dof_off >> jl) & 1u ? 0.0f : fminf(scl.effort[tl], fmaxf(-scl.effort[tl], t));
          const float u = dof_force(B, e, jl);
          if (u != 0.0f) drive += fminf(scl.effort[tl], fmaxf(-scl.effort[tl], u));
          S.tau[tl] = drive - tc;
        } else
        S.tau[tl] = fminf(scl.effort[tl], fmaxf(-scl.effort[tl], t)) - tc;   // the effort limit applies to the drive only
      }
      WAVE_SYNC();
      if (tl < ND) {
        float s = 0.0f;
        for (int j = 0; j < ND; ++j) s += S.A[tl][j] * S.tau[j];
        S.qd[tl] += h * s;
      }
      WAVE_SYNC();
      twists_wave0(S, tl);
    } else {
      for (int i = tl - 64; i < NF; i += NT - 64) {
        if (DR) {   // (opaque per brick: a product hoisted out of the loop is not fused with the add - the default kernel's v_fma here)
          float g0 = B.dr_grav[0], g1 = B.dr_grav[1], g2 = B.dr_grav[2];
          SDX_OPAQUE(g0); SDX_OPAQUE(g1); SDX_OPAQUE(g2);
          S.bv[i][0] += g0 * h; S.bv[i][1] += g1 * h; S.bv[i][2] += g2 * h;
        }
        else { S.bv[i][0] += scl.gravity[0] * h; S.bv[i][1] += scl.gravity[1] * h; S.bv[i][2] += scl.gravity[2] * h; }
        if (FORCE) {   // v += F h / m, w += R diag(1 / I) R^T T h: the solver's inverse mass, and its inverse inertia bim x tii at this substep's orientation
          const f4 q = ld4(S.bq[i]);
          f3 F, T;
          if (ext_wrench(B, e, SDX_BODY_BRICK0 + i, i, q, sub == 0, F, T)) {
            const float s = S.bim[i] * h;
            const f3 ii = ld3(S.tii[S.btype[i]]), l = qrot(qconj(q), T);
            st3(S.bv[i], ld3(S.bv[i]) + F * s);
            st3(S.bw[i], ld3(S.bw[i]) + qrot(q, F3(l.x * ii.x, l.y * ii.y, l.z * ii.z) * s));
          }
        }
      }
      // later substeps: both parts of the broadphase mask beside wave 0's FK + drive (the first substep had them beside FK and the factorisation)
      if (sub != 0 && !ABL(32)) {
        broad_mask_part<NT>(Cs, S, tl, 0);
        WAVES_WAIT(&S.fkflag, sub);
        broad_mask_part<NT>(Cs, S, tl, 1);
      }
    }
    __syncthreads();
    PSTAMP(3);
    collide<NT>(Cs, S, tl, (sub == 0 && e == B.dbg_env) ? B.dbg : nullptr, abl_bits);
    if (tl == 0 && B.cstats) {   // capacity statistics of this substep (integer atomics: order-independent)
      atomicMax(&B.cstats[0], S.nc + S.overflow);
      if (S.overflow) atomicAdd(&B.cstats[1], 1);
      if (S.rebuilt & 1) atomicAdd(&B.cstats[2], 1);
      if (S.rebuilt & 2) atomicAdd(&B.cstats[3], 1);
    }
    PSTAMP(4);
    if (scl.warm_start > 0.0f)
      solve<NT, true, DR, REPORT>(Cs, S, tl, h, sub == nsub - 1, (sub == 0 && e == B.dbg_env) ? B.dbg : nullptr, B.wcount + e, B.wkey + (size_t)e * MAXC, B.wlam + (size_t)e * 3 * MAXC, abl_bits, DR_ROW(dr_brick, 2 * NF, NF), DR_ROW(dr_link, 2 * NL, NL), REPORT ? reinterpret_cast<const sdx_contact_report*>(B.cscratch) : nullptr, e);
    else
      solve<NT, false, DR, REPORT>(Cs, S, tl, h, sub == nsub - 1, (sub == 0 && e == B.dbg_env) ? B.dbg : nullptr, nullptr, nullptr, nullptr, abl_bits, DR_ROW(dr_brick, 2 * NF, NF), DR_ROW(dr_link, 2 * NL, NL), REPORT ? reinterpret_cast<const sdx_contact_report*>(B.cscratch) : nullptr, e);
    PSTAMP(5);
    // F: integrate
    if (tl < ND) {
      float v = S.qd[tl] * (1.0f - h * scl.robot_angular_damping);   // GS:546
      v = fminf(scl.vel_limit[tl], fmaxf(-scl.vel_limit[tl], v));
      float qn = S.q[tl] + h * v;
      const float* drow = DR_ROW(dr_dof, 4 * ND, 0);
      const float lo = DR ? drow[2 * ND + tl] : scl.lower[tl], up = DR ? drow[3 * ND + tl] : scl.upper[tl];
      if (qn < lo) { qn = lo; v = fmaxf(v, 0.0f); }
      if (qn > up) { qn = up; v = fminf(v, 0.0f); }
      S.q[tl] = qn;
      S.qd[tl] = v;
    }
    for (int i = tl; i < NF; i += NT) {
      const f3 v = ld3(S.bv[i]), w = ld3(S.bw[i]);
      st3(S.bp[i], ld3(S.bp[i]) + v * h);
      const f4 q = ld4(S.bq[i]);
      f4 wq; wq.x = w.x; wq.y = w.y; wq.z = w.z; wq.w = 0.0f;
      const f4 dq = qmul(wq, q);
      f4 nq; nq.x = q.x + 0.5f * h * dq.x; nq.y = q.y + 0.5f * h * dq.y; nq.z = q.z + 0.5f * h * dq.z;
      nq.w = q.w + 0.5f * h * dq.w;
      st4(S.bq[i], qnormalize(nq));
    }
    for (int i = tl; i < NT; i += NT) S_BMASK(S)[i] = 0u;   // (the contact rows are dead between the solve and the next substep's collide)
    __syncthreads();
    PSTAMP(6);
  }

#undef DR_ROW
#ifdef SDX_PHASE_CLOCK
  if (threadIdx.x == 0 && e == B.dbg_env) B.dbg[15] = (long long)__builtin_readcyclecounter();   // end of the last substep
#endif
  // ---- outputs (refresh_* of GS:1091-1095): wave 0 refreshes the kinematics at the integrated joint positions; the brick rows, the contact
  // forces and the step's statistics depend on none of that and are written by waves 1..7 meanwhile
  float* rb_e = B.rb + (size_t)e * SDX_BODIES * 13;
  if (tid < 64) {
    fk_wave0(C, S, tid, false, false);
  } else {
    for (int i = tid - 64; i < NF * 13; i += NT - 64) {
      const int k = i / 13, c = i % 13;
      float v;
      if (c < 3) {
        const f3 o = ld3(S.bp[k]) - qrot(ld4(S.bq[k]), ld3(sc.brick_com[sc.brick_type[k]]));
        v = c == 0 ? o.x : c == 1 ? o.y : o.z;
      } else if (c < 7) v = S.bq[k][c - 3];
      else if (c < 10) v = S.bv[k][c - 7];
      else v = S.bw[k][c - 10];
      root_e[SDX_ACTOR_BRICK0 * 13 + i] = v;
      rb_e[SDX_BODY_BRICK0 * 13 + i] = v;
    }
    for (int i = tid - 64; i < NL * 3; i += NT - 64) B.contact[(size_t)e * SDX_BODIES * 3 + i] = (&S.cf[0][0])[i] * (1.0f / h);   // net impulse of the last substep / h
  }
  __syncthreads();
  if (tid < ND) {
    B.dof[((size_t)e * ND + tid) * 2] = S.q[tid];
    B.dof[((size_t)e * ND + tid) * 2 + 1] = S.qd[tid];
  }
  write_kinematics<NT>(C, S, B, e, tid);
  if (tid == 0) {
    B.ncontacts[e] = S.nc + S.overflow;
    // what this step cost: the next launch's order.  Round 6: the measured cycles of the env (units of 4096) instead of (hand touches
    // something, contact count), whose correlation with the cycles was 0.5 - a fifth of the launch was slots waiting for the slowest pair
    if (B.cost) B.cost[e] = (int)(((long long)__builtin_readcyclecounter() - t_in) >> 12);
  }
#ifdef SDX_PHASE_CLOCK
  __syncthreads();
  if (threadIdx.x == 0) {
    const long long t_out = (long long)__builtin_readcyclecounter();
    B.dbg[64 + 2 * e + 1] = t_out;
    if (e == B.dbg_env) B.dbg[14] = t_out;    // all outputs issued
  }
#endif
}

// ---- launch order of the next step: the envs by the cycles their last step took (k_physics measures them), longest first, in 256 buckets of
// 4096 cycles.  With 2 workgroups per CU and N = 1024 every CU slot runs two envs back to back; in env order two slow ones can meet on one
// slot (makespan 2 x slow), longest-first pairs the slowest with the fastest.  (Rounds 3-5 sorted by "hand touches something" and the contact
// count; round 6 measured a correlation of 0.5 between that key and the cycles: env 589 k cycles on average, 505 k / 656 k at the 10th / 90th
// percentile, 854 k the slowest - and the launch took 1.42 M cycles where the slots' average load was 1.18 M.)
// The order inside a bucket is whatever the atomics give, and the buckets depend on clocks: neither can change any result (envs are independent).
__global__ __launch_bounds__(1024) void k_order(SdxBuf B) {
  __shared__ int hist[256], base[256];
  const int tid = threadIdx.x;
  if (tid < 256) hist[tid] = 0;
  __syncthreads();
  for (int e = tid; e < B.N; e += 1024) {
    const int c = B.cost[e];
    atomicAdd(&hist[c < 0 ? 0 : (c > 255 ? 255 : c)], 1);
  }
  __syncthreads();
  if (tid == 0) {
    int run = 0;
    for (int k = 255; k >= 0; --k) { base[k] = run; run += hist[k]; }
  }
  __syncthreads();
  for (int e = tid; e < B.N; e += 1024) {
    const int c = B.cost[e];
    B.order[atomicAdd(&base[c < 0 ? 0 : (c > 255 ? 255 : c)], 1)] = e;
  }
}

// kinematics only: rigid-body states of the 24 links + end-effector Jacobian from SDX_T_DOF (one wave per env)
__global__ __launch_bounds__(64) void k_kinematics(const SdxConst* __restrict__ C, SdxBuf B) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  PhysLds& S = *reinterpret_cast<PhysLds*>(smem);
  const int e = blockIdx.x, tid = threadIdx.x;
  if (tid < ND) {
    S.q[tid] = B.dof[((size_t)e * ND + tid) * 2];
    S.qd[tid] = B.dof[((size_t)e * ND + tid) * 2 + 1];
  }
  if (tid < NL) S.anc[tid] = C->anc[tid];
  if (tid < SDX_MAX_RBOX) S.rbl[tid] = tid < C->sc.n_rbox ? C->sc.rbox_link[tid] : 0;
  if (tid <= NL) S.par[tid] = tid < NL ? (tid == 0 ? 0 : C->sc.parent[tid]) : NL;
  if (tid == 0) {
    S.qd[ND] = 0.0f; st3(S.la[NL], F3(0, 0, 0)); st3(S.lal[NL], F3(0, 0, 0));
    st3(S.bp[BODY_W], F3(0, 0, 0)); st3(S.bv[BODY_W], F3(0, 0, 0)); st3(S.bw[BODY_W], F3(0, 0, 0));
  }
  WAVE_SYNC();
  fk_wave0(C, S, tid, false, false);
  write_kinematics<64>(C, S, B, e, tid);
  if (B.jac_full) {   // acquire_jacobian_tensor(sim, "hand") (GS:241): [23 links (fixed base excluded), 6, 23 dofs]
    float* J = B.jac_full + (size_t)e * (NL - 1) * 6 * ND;
    for (int i = tid; i < (NL - 1) * 6 * ND; i += 64) {
      const int k = i / (6 * ND) + 1, r = (i / ND) % 6, j = i % ND;
      float v = 0.0f;
      if ((S.anc[k] >> j) & 1u) {
        const f3 a = ld3(S.la[j + 1]);
        const f3 lin = cross(a, ld3(S.bp[NF + k]) - ld3(S.bp[NF + j + 1]));
        v = r == 0 ? lin.x : r == 1 ? lin.y : r == 2 ? lin.z : r == 3 ? a.x : r == 4 ? a.y : a.z;
      }
      J[i] = v;
    }
  }
}

extern "C" size_t sdxk_physics_lds_bytes() { return sizeof(PhysLds); }
// threads per env: 512 (8 waves, <= 128 VGPRs), two envs per CU
static void physics_init() {
  static bool done = false;
  if (!done) {
    done = true;
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k_physics<512>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(PhysLds));
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k_physics<512 | SDX_PHYS_DR>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(PhysLds));
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k_physics<512 | SDX_PHYS_FORCE>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(PhysLds));
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k_physics<512 | SDX_PHYS_DR | SDX_PHYS_FORCE>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(PhysLds));
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k_physics<512 | SDX_PHYS_REPORT>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(PhysLds));
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k_physics<512 | SDX_PHYS_REPORT | SDX_PHYS_DR>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(PhysLds));
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k_physics<512 | SDX_PHYS_REPORT | SDX_PHYS_FORCE>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(PhysLds));
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k_physics<512 | SDX_PHYS_REPORT | SDX_PHYS_DR | SDX_PHYS_FORCE>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(PhysLds));
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k_kinematics), hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(PhysLds));
  }
}
extern "C" int sdxk_physics_threads() { return 512; }
// report: the armed contact report of this launch (sdx_set_contact_report), or nullptr / count == nullptr: none - the kernels without the flag run
extern "C" void sdxk_physics_report(const SdxConst* C, const SdxBuf* B, const sdx_contact_report* report, hipStream_t st) {
  physics_init();
  // an external wrench (sdx_apply_rigid_body_forces), actuation torques or drives that are off (sdx_apply_dof_forces) ride with this launch
  const bool force = B->ext_force || B->ext_torque || B->dof_force || B->dof_off;
  if (report && report->count && B->cscratch) {   // the same four, with the report's stores in the last substep
    // the pointers of THIS launch, by value into the device table the kernel reads them from (stream-ordered: a later call that arms other
    // buffers or disarms does not reach a launch that is already enqueued)
    hipLaunchKernelGGL(k_report_table, dim3(1), dim3(64), 0, st, *report, reinterpret_cast<sdx_contact_report*>(B->cscratch));
    if (force && B->dr_on) hipLaunchKernelGGL(k_physics<512 | SDX_PHYS_REPORT | SDX_PHYS_DR | SDX_PHYS_FORCE>, dim3(B->N), dim3(512), sizeof(PhysLds), st, C, *B);
    else if (force) hipLaunchKernelGGL(k_physics<512 | SDX_PHYS_REPORT | SDX_PHYS_FORCE>, dim3(B->N), dim3(512), sizeof(PhysLds), st, C, *B);
    else if (B->dr_on) hipLaunchKernelGGL(k_physics<512 | SDX_PHYS_REPORT | SDX_PHYS_DR>, dim3(B->N), dim3(512), sizeof(PhysLds), st, C, *B);
    else hipLaunchKernelGGL(k_physics<512 | SDX_PHYS_REPORT>, dim3(B->N), dim3(512), sizeof(PhysLds), st, C, *B);
  }
  else if (force && B->dr_on) hipLaunchKernelGGL(k_physics<512 | SDX_PHYS_DR | SDX_PHYS_FORCE>, dim3(B->N), dim3(512), sizeof(PhysLds), st, C, *B);
  else if (force) hipLaunchKernelGGL(k_physics<512 | SDX_PHYS_FORCE>, dim3(B->N), dim3(512), sizeof(PhysLds), st, C, *B);
  else if (B->dr_on) hipLaunchKernelGGL(k_physics<512 | SDX_PHYS_DR>, dim3(B->N), dim3(512), sizeof(PhysLds), st, C, *B);   // domain randomization on
  else hipLaunchKernelGGL(k_physics<512>, dim3(B->N), dim3(512), sizeof(PhysLds), st, C, *B);
  if (B->order && B->cost) hipLaunchKernelGGL(k_order, dim3(1), dim3(1024), 0, st, *B);
}
extern "C" void sdxk_physics(const SdxConst* C, const SdxBuf* B, hipStream_t st) { sdxk_physics_report(C, B, nullptr, st); }
extern "C" void sdxk_kinematics(const SdxConst* C, const SdxBuf* B, hipStream_t st) {
  physics_init();
  hipLaunchKernelGGL(k_kinematics, dim3(B->N), dim3(64), sizeof(PhysLds), st, C, *B);
}
extern "C" void sdxk_dof_dynamics(const SdxConst* C, const SdxBuf* B, float* mass, float* bias, float* drive, hipStream_t st) {
  if (B->dr_on) hipLaunchKernelGGL(k_dof_dynamics<true>, dim3(B->N), dim3(DYN_NT), 0, st, C, *B, mass, bias, drive);
  else hipLaunchKernelGGL(k_dof_dynamics<false>, dim3(B->N), dim3(DYN_NT), 0, st, C, *B, mass, bias, drive);
}
extern "C" void sdxk_osc_torques(const SdxConst* C, const SdxBuf* B, const sdx_osc_attr* attr, const float* dpose, float* torques, float* wrench,
                                 hipStream_t st) {
  if (B->dr_on) hipLaunchKernelGGL(k_osc_torques<true>, dim3(B->N), dim3(DYN_NT), 0, st, C, *B, *attr, dpose, torques, wrench);
  else hipLaunchKernelGGL(k_osc_torques<false>, dim3(B->N), dim3(DYN_NT), 0, st, C, *B, *attr, dpose, torques, wrench);
}
extern "C" void sdxk_solve_ik(const SdxConst* C, const SdxBuf* B, const sdx_ik_attr* attr, const float* q0, const float* base_pos, const float* base_quat,
                              const float* tip_pos, float* q_out, float* err_out, int32_t* info_out, hipStream_t st) {
  hipLaunchKernelGGL(k_solve_ik, dim3(B->N), dim3(IK_NT), 0, st, C, *B, *attr, q0, base_pos, base_quat, tip_pos, q_out, err_out, info_out);
}
extern "C" void sdxk_contact_wrenches(const SdxBuf* B, const sdx_contact_report* report, float* net, const sdx_contact_pairs* pairs, float* pair,
                                      hipStream_t st) {
  sdx_contact_pairs none = {};
  hipLaunchKernelGGL(k_contact_wrenches, dim3(B->N), dim3(CW_NT), 0, st, B->rb, *report, net, pair ? *pairs : none, pair);
}
