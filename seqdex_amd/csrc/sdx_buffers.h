// sdx_buffers.h — the one table of the device buffers of SdxBuf (sdx_common.h): a flat X-macro list, one row per buffer, that
// sdx_capi.hip walks to allocate (sdx_create), to fill the tensor registry (sdx_tensor) and to build the snapshot segment table
// (sdx_state.h).  A row is X(field, elements allocated, snapshot class, state elements per env, tensor); its expressions are evaluated
// where the table is walked, with N envs (int64_t), W = obs_w, P = pile_slots, search / warm = the scene is BlockAssemblySearch / asks
// for the solver's warm start in scope.  A buffer of 0 elements is not allocated: its pointer stays nullptr, which the kernels test.
//
// The snapshot class says what a sim snapshot does with the buffer; there is no default, a new row has to decide:
//   ENV       env state: every buffer a later call reads before it writes.  n = the elements per env that are state, also the buffer's
//             row stride (obs / obs_c are ALLOCATED at SDX_NUM_OBS per env but indexed, exposed and snapshotted at obs_w); n == 0: no
//             segment (seg_image / tvt_buf belong to Search; wcount travels in the row header instead)
//   ENV_WARM  env state of the warm-start cache: n / SDX_MAXC rows of SDX_MAXC entries per env, of each row only the first wcount[e]
//   GLOBAL    global state, whole: what save_all / restore_all move besides the env rows (at most 16 bytes each)
//   LOG       logs and diagnostics (the harvest / pile / T-value rings with their counts and keys, cstats, dbg);  SCRATCH  scratch and
//             scheduling hints;  CONFIG  configuration.  Not in the table: the randomization descriptor, dr_on, act_pre, orient_mask.
// The ENV rows stand in ROW-LAYOUT order, the ENV_WARM rows last: their order is the order of the segments in a snapshot row, which
// decides the alignment phases k_state_copy sees.  The GLOBAL rows stand in the order of the snapshot's global slots; the last slot is
// the one tail element dr_draw[N] (gravity's draw count) of the per-env buffer dr_draw.
// TENSOR(id, dtype, shape...) exposes the buffer as SDX_T_<id>; the placeholder tensors of a simulator without the camera or the warm
// start (SEG_IMAGE {1,1,1}, TVALUE_OBS -> seg_pix {1,1}, WARM_KEYS / WARM_LAMBDA {1}; marked on their rows) replace the row's in tensors_register.
#pragma once
#include "sdx_common.h"

#define SDX_BUFFERS(X)                                                                                                                   \
  X(root, N * SDX_ACTORS * 13, ENV, SDX_ACTORS * 13, TENSOR(ROOT, F32, N * SDX_ACTORS, 13))                                             \
  X(dof, N * SDX_NDOF * 2, ENV, SDX_NDOF * 2, TENSOR(DOF, F32, N * SDX_NDOF, 2))                                                        \
  X(rb, N * SDX_BODIES * 13, ENV, SDX_BODIES * 13, TENSOR(RB, F32, N, SDX_BODIES, 13))                                                  \
  X(contact, N * SDX_BODIES * 3, ENV, SDX_BODIES * 3, TENSOR(CONTACT, F32, N, SDX_BODIES * 3))                                          \
  X(jac, N * 42, ENV, 42, TENSOR(JAC_EEF, F32, N, 6, 7))                                                                                \
  X(jac_full, N * (SDX_NLINK - 1) * 6 * SDX_NDOF, ENV, (SDX_NLINK - 1) * 6 * SDX_NDOF, TENSOR(JACOBIAN, F32, N, SDX_NLINK - 1, 6, SDX_NDOF)) \
  X(targets, N * SDX_NDOF, ENV, SDX_NDOF, TENSOR(TARGETS, F32, N, SDX_NDOF))                                                            \
  X(prev_targets, N * SDX_NDOF, ENV, SDX_NDOF, TENSOR(PREV_TARGETS, F32, N, SDX_NDOF))                                                  \
  X(obs, N * SDX_NUM_OBS, ENV, W, TENSOR(OBS, F32, N, W))                                                                               \
  X(states, N * SDX_NUM_STATES, ENV, SDX_NUM_STATES, TENSOR(STATES, F32, N, SDX_NUM_STATES))                                            \
  X(obs_c, N * SDX_NUM_OBS, ENV, W, TENSOR(OBS_CLAMPED, F32, N, W))                                                                     \
  X(states_c, N * SDX_NUM_STATES, ENV, SDX_NUM_STATES, TENSOR(STATES_CLAMPED, F32, N, SDX_NUM_STATES))                                  \
  X(rew, N, ENV, 1, TENSOR(REW, F32, N))                                                                                                \
  X(reset, N, ENV, 1, TENSOR(RESET, I64, N))                                                                                            \
  X(progress, N, ENV, 1, TENSOR(PROGRESS, I64, N))                                                                                      \
  X(randomize, N, ENV, 1, TENSOR(RANDOMIZE, I64, N))                                                                                    \
  X(actions, N * SDX_NDOF, ENV, SDX_NDOF, TENSOR(ACTIONS, F32, N, SDX_NDOF))                                                            \
  X(init_pos, N * 3, ENV, 3, TENSOR(INIT_POS, F32, N, 3))                                                                               \
  X(init_rot, N * 4, ENV, 4, TENSOR(INIT_ROT, F32, N, 4))                                                                               \
  X(successes, N, ENV, 1, TENSOR(SUCCESSES, F32, N))                                                                                    \
  X(meta_rew, N, ENV, 1, TENSOR(META_REW, F32, N))                                                                                      \
  X(finger_dist, N, ENV, 1, TENSOR(FINGER_DIST, F32, N))                                                                                \
  X(tvalue, N, ENV, 1, TENSOR(TVALUE, F32, N))                                                                                          \
  X(arm_contacts, N * 6, ENV, 6, TENSOR(ARM_CONTACTS, F32, N, 6))                                                                       \
  X(student_obs, N * 30, ENV, 30, TENSOR(STUDENT_OBS, F32, N, 30))                                                                      \
  X(success_buf, N, ENV, 1, TENSOR(SUCCESS_BUF, I64, N))                                                                                \
  X(pile_choice, N, ENV, 1, TENSOR(PILE_CHOICE, I32, N))                                                                                \
  X(ncontacts, N, ENV, 1, TENSOR(NCONTACTS, I32, N))                                                                                    \
  X(cam_rot, N * 4, ENV, 4, TENSOR(CAM_ROT, F32, N, 4))                                                                                 \
  X(insert_aux, N * 8, ENV, 8, TENSOR(INSERT_AUX, F32, N, 8))                                                                           \
  X(seg_stats, N * 4, ENV, 4, NO_TENSOR)                                                                                                \
  X(seg_pix, N * 4, ENV, 4, TENSOR(SEG_PIXELS, F32, N, 4))                                                                              \
  X(emergence, N, ENV, 1, TENSOR(EMERGENCE, F32, N))                                                                                    \
  X(seg_image, search ? N * 128 * 128 : 1, ENV, search ? 128 * 128 : 0, TENSOR(SEG_IMAGE, I16, N, 128, 128)) /* not Search: placeholder {1,1,1} */ \
  X(tvt_buf, search ? N * 652 : 0, ENV, search ? 652 : 0, TENSOR(TVALUE_OBS, F32, N, 652)) /* not Search: placeholder seg_pix {1,1} */  \
  X(dr_dof, N * 4 * SDX_NDOF, ENV, 4 * SDX_NDOF, TENSOR(DR_DOF, F32, N, 4, SDX_NDOF))                                                   \
  X(dr_link, N * 2 * SDX_NLINK, ENV, 2 * SDX_NLINK, TENSOR(DR_LINK, F32, N, 2, SDX_NLINK))                                              \
  X(dr_brick, N * 2 * SDX_NFREE, ENV, 2 * SDX_NFREE, TENSOR(DR_BRICK, F32, N, 2, SDX_NFREE))                                            \
  X(dr_draw, N + 1, ENV, 1, NO_TENSOR)                                                                                                  \
  X(wcount, N, ENV, 0, TENSOR(WARM_COUNT, I32, N))                                                                                      \
  X(wkey, warm ? N * SDX_MAXC : 1, ENV_WARM, warm ? SDX_MAXC : 0, TENSOR(WARM_KEYS, I32, N, SDX_MAXC)) /* not warm: placeholder {1} */  \
  X(wlam, warm ? N * 3 * SDX_MAXC : 1, ENV_WARM, warm ? 3 * SDX_MAXC : 0, TENSOR(WARM_LAMBDA, F32, N, 3, SDX_MAXC)) /* not warm: placeholder {1} */ \
  X(step_count, 1, GLOBAL, 0, NO_TENSOR)                                                                                                   \
  X(stat, 4, GLOBAL, 0, NO_TENSOR)                                                                                                         \
  X(cons, 1, GLOBAL, 0, TENSOR(CONS_SUCCESSES, F32, 1))                                                                                    \
  X(dr_grav, 3, GLOBAL, 0, TENSOR(DR_GRAVITY, F32, 3))                                                                                     \
  X(dr_frame, 2, GLOBAL, 0, TENSOR(DR_FRAME, I64, 2))                                                                                      \
  X(dbg, 64 + 2 * N, LOG, 0, TENSOR(DEBUG, I64, 64 + 2 * N))                                                                               \
  X(cstats, 4, LOG, 0, TENSOR(CONTACT_STATS, I32, 4))                                                                                      \
  X(harvest_hand, 8 * SDX_HARVEST_SLOTS * SDX_NDOF * 2, LOG, 0, TENSOR(HARVEST_HAND, F32, 8, SDX_HARVEST_SLOTS, SDX_NDOF, 2))              \
  X(harvest_obj, 8 * SDX_HARVEST_SLOTS * 13, LOG, 0, TENSOR(HARVEST_OBJ, F32, 8, SDX_HARVEST_SLOTS, 13))                                   \
  X(harvest_count, 8, LOG, 0, TENSOR(HARVEST_COUNT, I32, 8))                                                                               \
  X(harvest_key, 8 * SDX_HARVEST_SLOTS, LOG, 0, TENSOR(HARVEST_KEYS, I64, 8, SDX_HARVEST_SLOTS))                                           \
  X(pile_harvest, 8 * P * SDX_NBRICK * 13, LOG, 0, TENSOR(PILE_HARVEST, F32, 8, P, SDX_NBRICK, 13))                                        \
  X(pile_harvest_count, 8, LOG, 0, TENSOR(PILE_HARVEST_COUNT, I32, 8))                                                                     \
  X(pile_key, 8 * P, LOG, 0, TENSOR(PILE_HARVEST_KEYS, I64, 8, P))                                                                         \
  X(tv_succ, SDX_TV_LOG_SLOTS * 4, LOG, 0, TENSOR(TV_SUCCESS, F32, SDX_TV_LOG_SLOTS, 4))                                                   \
  X(tv_fail, SDX_TV_LOG_SLOTS * 4, LOG, 0, TENSOR(TV_FAILURE, F32, SDX_TV_LOG_SLOTS, 4))                                                   \
  X(tv_count, 2, LOG, 0, TENSOR(TV_COUNT, I32, 2))                                                                                         \
  X(tv_key, 2 * SDX_TV_LOG_SLOTS, LOG, 0, TENSOR(TV_KEYS, I64, 2, SDX_TV_LOG_SLOTS))                                                       \
  X(cscratch, 16, SCRATCH, 0, NO_TENSOR) /* the pointer table of an armed contact report (a sdx_contact_report: 56 bytes) */               \
  X(order, N, SCRATCH, 0, NO_TENSOR)                                                                                                       \
  X(cost, N, SCRATCH, 0, NO_TENSOR)                                                                                                        \
  X(tvt_h, search ? N * (1024 + 512 + 128 + 4) : 0, SCRATCH, 0, NO_TENSOR)                                                                 \
  X(ext_world, N * (SDX_NFREE + SDX_NLINK) * 6, SCRATCH, 0, NO_TENSOR)                                                                     \
  X(piles, 8 * SDX_NBRICK * 13, CONFIG, 0, NO_TENSOR)                                                                                      \
  X(tv_w, SDX_TV_PARAMS, CONFIG, 0, NO_TENSOR)                                                                                             \
  X(tvt_w, search ? 1024 * 652 + 1024 + 512 * 1024 + 512 + 128 * 512 + 128 + 2 * 128 + 2 : 0, CONFIG, 0, NO_TENSOR)

// Compile-time check: a row whose class is none of these does not compile, and every pointer of SdxBuf but dr_on (an alias of dr_draw) and
// ext_force / ext_torque / dof_force (the caller's buffers of one launch) has a row.
enum SdxSnap { SDX_SNAP_ENV = 1, SDX_SNAP_ENV_WARM, SDX_SNAP_GLOBAL, SDX_SNAP_LOG, SDX_SNAP_SCRATCH, SDX_SNAP_CONFIG };
#define SDX_BUF_ROW_CLASS(field, count, snap, n, tensor) SDX_SNAP_##snap,
static constexpr SdxSnap sdx_buf_snap[] = {SDX_BUFFERS(SDX_BUF_ROW_CLASS)};
static_assert(sizeof(SdxBuf) == 48 /* its scalars and padding */ + sizeof(void*) * (sizeof(sdx_buf_snap) / sizeof(sdx_buf_snap[0]) + 4), "sdx_buffers.h: a pointer of SdxBuf has no row in SDX_BUFFERS, or a row no pointer (or SdxBuf's scalars changed: then adjust the 48)");
