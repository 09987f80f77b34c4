// sdx_kernels.h — the one declaration of every host launcher that crosses a file boundary of libseqdex_hip.so.  Included by
// sdx_capi.hip (the caller) and by every file that defines one of them, so that a definition whose parameters differ from the
// declaration fails to compile instead of linking silently.  SdxBuf goes to a launcher by pointer and to its kernels by value.
#pragma once
#include "sdx_common.h"

extern "C" {
// sdx_task.hip
void sdxk_pre_physics(const SdxConst* C, const SdxBuf* B, const float* actions, const uint8_t* mask, const int32_t* choice, int flags, hipStream_t st);
void sdxk_post_physics(const SdxConst* C, const SdxBuf* B, int flags, hipStream_t st);
void sdxk_orient_pregrasp(const SdxConst* C, const SdxBuf* B, const uint8_t* mask, int mode, int iter, hipStream_t st);
void sdxk_orient_post_reset(const SdxConst* C, const SdxBuf* B, const uint8_t* mask, hipStream_t st);
void sdxk_search_set_hand(const SdxConst* C, const SdxBuf* B, const uint8_t* mask, int mode, hipStream_t st);
void sdxk_scripted_grasp(const SdxConst* C, const SdxBuf* B, float* state, float* act, hipStream_t st);
void sdxk_set_indexed(const SdxBuf* B, int id, const float* src, const int32_t* ids, int n, hipStream_t st);
// sdx_physics.hip
void sdxk_physics(const SdxConst* C, const SdxBuf* B, hipStream_t st);
// the same launch with an armed contact report (sdx_set_contact_report): its last substep also writes the caller's buffers
void sdxk_physics_report(const SdxConst* C, const SdxBuf* B, const sdx_contact_report* report, hipStream_t st);
void sdxk_kinematics(const SdxConst* C, const SdxBuf* B, hipStream_t st);
// sdx_camera.hip
void sdxk_seg_camera(const SdxConst* C, const SdxBuf* B, hipStream_t st);
void sdxk_render_view(const SdxConst* C, const SdxBuf* B, const sdx_view_desc* v, const int32_t* env_ids, int n, float* depth, int16_t* label, uint8_t* rgb, hipStream_t st);
// sdx_randomize.hip
void sdxk_dr_defaults(const SdxConst* C, const SdxBuf* B, hipStream_t st);
void sdxk_dr_sample(const SdxConst* C, const SdxBuf* B, const sdx_dr_desc* desc, int first, const uint8_t* mask, hipStream_t st);
void sdxk_noise(const SdxConst* C, const SdxBuf* B, const sdx_noise_attr* attr, const float* src, float* dst, int W, int act, hipStream_t st);
// sdx_physics.hip k_dof_dynamics: mass [N,23,23], bias [N,23], drive [N,23] (device, any of them nullptr) from the current dof / targets
void sdxk_dof_dynamics(const SdxConst* C, const SdxBuf* B, float* mass, float* bias, float* drive, hipStream_t st);
// sdx_physics.hip k_osc_torques: torques [N,23] and wrench [N,6] (device, wrench may be nullptr) from the current dof and dpose [N,6]
void sdxk_osc_torques(const SdxConst* C, const SdxBuf* B, const sdx_osc_attr* attr, const float* dpose, float* torques, float* wrench, hipStream_t st);
// sdx_physics.hip k_solve_ik: q_out [N,23], err_out [N,6] and info_out [N,6] (device, the last two may be nullptr) from q0 [N,23] (nullptr: the
// current dof positions) and the targets base_pos [N,3], base_quat [N,4], tip_pos [N,4,3] (nullptr where attr->task_mask does not select them)
void sdxk_solve_ik(const SdxConst* C, const SdxBuf* B, const sdx_ik_attr* attr, const float* q0, const float* base_pos, const float* base_quat,
                   const float* tip_pos, float* q_out, float* err_out, int32_t* info_out, hipStream_t st);
// sdx_physics.hip k_contact_wrenches: net [N,165,6] and pair [N,n_sensor,n_filter,3] (device, either may be nullptr; pairs is read only
// with pair) from the caller's contact report and the current body positions
void sdxk_contact_wrenches(const SdxBuf* B, const sdx_contact_report* report, float* net, const sdx_contact_pairs* pairs, float* pair, hipStream_t st);
// mode SDX_FP_STEP: the whole rule for one step (resets from reset_buf); SDX_FP_RESET: rows <- 0 and a new probability for the envs of mask
// (nullptr: every env); SDX_FP_DRAW: a new probability for every env, rows untouched.  factor: decay^(dt / decay_interval)
enum { SDX_FP_STEP = 0, SDX_FP_RESET = 1, SDX_FP_DRAW = 2 };
void sdxk_force_perturb(const SdxConst* C, const SdxBuf* B, const sdx_force_perturb_attr* attr, float factor, float* rb_forces, float* prob,
                        const uint8_t* mask, int mode, hipStream_t st);
// sdxp_rollout.hip (the PPO library's MFMA linear layer, which Search's RetriGraspTValue in sdx_task.hip borrows)
void sdxpk_linear(const float* X, const float* W, const float* b, float* Y, int M, int N, int K, int elu_flag, const double* nmean, const double* nvar, hipStream_t st);
}
