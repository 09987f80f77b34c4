/* seqdex.h — C ABI of libseqdex_hip.so: the MI355X-native replacement for the two
 * third-party engines on the BlockAssemblyGraspSim hot path of sequential-dexterity/SeqDex.
 *
 *   SIM  (sdx_*) : what the task calls on Isaac Gym's tensor API          (SURVEY.md §8(b) seam 2)
 *   TASK (sdx_*) : the reference-owned per-step tensor code, fused on GPU  (§8(a) rows T1-T9)
 *   PPO  (sdxp_*): what rl_games' A2CAgent does per epoch                 (§8(a) rows R1-R9)
 *
 * Citations are file:line under /root/reference/dexteroushandenvs/:
 *   GS = tasks/block_assembly/allegro_hand_block_assembly_grasp_sim.py
 *   BT = tasks/hand_base/base_task.py     VR = tasks/hand_base/vec_task_rlgames.py
 *   PS = policy_sequencing/policy_seq_runner.py   RC = utils/rl_games_custom.py
 *   YG = cfg/lego/ppo_continuous_grasp.yaml
 *
 * Conventions: every function returns 0 on success or a negative sdx_status; no exceptions cross the
 * boundary; handles are opaque; every buffer returned by *_tensor() is device memory owned by the
 * library, stable until *_destroy(); all device work is enqueued on the caller's hipStream_t (passed as
 * void* so that this header needs no HIP include) and is stream-ordered with no hidden synchronisation
 * unless the function's comment says "blocking".  One host thread per handle.  Quaternions are xyzw.
 */
#ifndef SEQDEX_H
#define SEQDEX_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SDX_ABI_VERSION 8

/* ---- fixed scene dimensions of BlockAssemblyGraspSim (GS:523-1058) ---- */
#define SDX_NLINK 24        /* robot bodies after collapse_fixed_joints (GS:543); body 0 is the fixed base  */
#define SDX_NDOF 23         /* 7 arm + 16 hand revolute DOF (GS:561, 580-590)                               */
#define SDX_MAX_RBOX 40     /* robot collision boxes (URDF boxes, slab compounds of the fingertip / palm hulls, bounding boxes of the arm) */
#define SDX_NBRICK 132      /* 72 free (GS:717-746) + 60 fixed floor bricks (GS:748-808)                     */
#define SDX_NFREE 72
#define SDX_NBRICK_TYPES 8  /* GS:706                                                                        */
#define SDX_MAX_STATIC 8    /* static bodies one env sees: table, 5 bin walls, merged brick floor, base plate                        */
#define SDX_MAX_STATIC_TAB 10 /* rows of the static-body table: the 8 above + the two other base-plate variants of InsertSim          */
#define SDX_MAX_STATIC_SUB 112 /* boxes of all static bodies: 7 single boxes + up to 3 base plates of 1 + 16 x 2 boxes (body, studs)  */
#define SDX_MAX_SUB 2       /* boxes of a free brick's collision compound: slabs of its convex hull (GS:717-731: one hull per brick) */
#define SDX_MAX_SUB_HOLLOW 8 /* boxes of the hollow compound (4 walls + the slabs above the cavity) of the brick being inserted    */
#define SDX_ACTORS 142      /* hand, object, goal, table, 5 bin boxes, 132 bricks, base plate                */
#define SDX_BODIES 165      /* 24 hand links + one body per other actor                                      */
#define SDX_ACTOR_BRICK0 9  /* first brick actor inside an env                                               */
#define SDX_BODY_BRICK0 32  /* first brick rigid body inside an env                                          */
#define SDX_ACTOR_PLATE (SDX_ACTORS - 1) /* the base plate, the last actor of an env                            */
#define SDX_NUM_OBS 396     /* 132 x 3 stacked frames (GS:207-209)                                           */
#define SDX_NUM_STATES 564  /* 188 x 3 (GS:204-210)                                                          */
#define SDX_NUM_ACTIONS 23  /* GS:211                                                                        */
#define SDX_OBS_FRAME 132
#define SDX_STATE_FRAME 188
#define SDX_PILE_HARVEST_SLOTS 512 /* Orient's ring of pile states per brick-type group; SDX_PILE_SLOTS=10000 in the environment of
                                       sdx_create gives the reference's length (OR:1485: 10 000 = 549 MB)                          */
#define SDX_TV_LOG_SLOTS 1048576 /* rows of each T-value dataset ring (success / failure): large enough that the runs of the chain
                                  * never wrap it (a wrapped ring's surviving rows depend on the order the slots were claimed in)      */
#define SDX_HARVEST_SLOTS 5001 /* ring of grasp terminal states per brick-type group (GS:1440: index wraps after 5000) */
#define SDX_TV_PARAMS 42562 /* GraspInsertTValue 4-256-128-64-2 weights+biases (terminal_value_function.py:30-46) */
#define SDX_RETRI_TV_PARAMS 1257346 /* RetriGraspTValue 650-1024-512-128-2 weights+biases (terminal_value_function.py:12-28) */
#define SDX_RETRI_TV_IN 650    /* 65 x 10 (SE:397) */

typedef enum {
  SDX_OK = 0,
  SDX_ERR_INVALID = -1,     /* bad argument / null pointer / bad id                     */
  SDX_ERR_HIP = -2,         /* a HIP runtime call failed; see sdx_last_error()          */
  SDX_ERR_NO_DEVICE = -3,   /* no gfx950 device visible: the product path has NO CPU fallback */
  SDX_ERR_STATE = -4,       /* call order violated (e.g. step before initial states)    */
  SDX_ERR_NOMEM = -5
} sdx_status;

typedef enum { SDX_F32 = 0, SDX_I64 = 1, SDX_I32 = 2, SDX_U8 = 3, SDX_F64 = 4, SDX_I16 = 5 } sdx_dtype;

/* values of sdx_scene_desc.task_kind (documented at the field) */
typedef enum { SDX_TASK_GRASP = 0, SDX_TASK_ORIENT = 1, SDX_TASK_INSERT = 2, SDX_TASK_SEARCH = 3 } sdx_task_kind;

/* Tensor ids for sdx_tensor().  Shapes use N = num_envs. */
typedef enum {
  SDX_T_ROOT = 0,        /* f32 [N*142,13]  acquire_actor_root_state_tensor      GS:237,321              */
  SDX_T_DOF = 1,         /* f32 [N*23,2]    acquire_dof_state_tensor             GS:238,313-316          */
  SDX_T_RB = 2,          /* f32 [N,165,13]  acquire_rigid_body_state_tensor      GS:239,318              */
  SDX_T_CONTACT = 3,     /* f32 [N,165*3]   acquire_net_contact_force_tensor     GS:240,322              */
  SDX_T_JAC_EEF = 4,     /* f32 [N,6,7]     jacobian_tensor[:, 7-1, :, :7]       GS:241,1601             */
  SDX_T_TARGETS = 5,     /* f32 [N,23]      cur_targets == PD targets            GS:329,1638             */
  SDX_T_PREV_TARGETS = 6,/* f32 [N,23]      prev_targets                         GS:328,1636             */
  SDX_T_OBS = 7,         /* f32 [N,396]     task.obs_buf (unclamped)             BT:57, GS:1299-1332     */
  SDX_T_STATES = 8,      /* f32 [N,564]     task.states_buf (unclamped)          BT:59, GS:1220-1280     */
  SDX_T_OBS_CLAMPED = 9, /* f32 [N,396]     clamp(obs_buf,+-5) as VR:171 returns                         */
  SDX_T_STATES_CLAMPED = 10, /* f32 [N,564] clamp(states_buf,+-5) as VR:172 returns                      */
  SDX_T_REW = 11,        /* f32 [N]         task.rew_buf                         BT:61, GS:1061          */
  SDX_T_RESET = 12,      /* i64 [N]         task.reset_buf (initialised to 1)    BT:63                   */
  SDX_T_PROGRESS = 13,   /* i64 [N]         task.progress_buf                    BT:65                   */
  SDX_T_RANDOMIZE = 14,  /* i64 [N]         task.randomize_buf                   BT:67, GS:1642          */
  SDX_T_ACTIONS = 15,    /* f32 [N,23]      task.actions (clamped copy)          GS:1570, VR:166         */
  SDX_T_INIT_POS = 16,   /* f32 [N,3]       segmentation_target_init_pos         GS:453,1547             */
  SDX_T_INIT_ROT = 17,   /* f32 [N,4]       segmentation_target_init_rot         GS:454,1548             */
  SDX_T_SUCCESSES = 18,  /* f32 [N]         successes                            GS:337,1552             */
  SDX_T_META_REW = 19,   /* f32 [N]         meta_rew_buf                         GS:367,1069,1553        */
  SDX_T_CONS_SUCCESSES = 20, /* f32 [1]     consecutive_successes                GS:338,1771-1774        */
  SDX_T_FINGER_DIST = 21,/* f32 [N]         arm_hand_finger_dist                 GS:1164-1165            */
  SDX_T_TVALUE = 22,     /* f32 [N]         tvalue                               GS:1200-1201            */
  SDX_T_ARM_CONTACTS = 23,/* f32 [N,6]      contacts (bodies 1..6 >= 0.1 N)      GS:1159-1162            */
  SDX_T_STUDENT_OBS = 24,/* f32 [N,30]      extras["student_obs_buf"]            GS:458                  */
  SDX_T_SUCCESS_BUF = 25,/* i64 [N]         extras["success_buf"]                GS:459                  */
  SDX_T_PILE_CHOICE = 26,/* i32 [N]         saved-pile index drawn at the last reset of each env  GS:1510 */
  SDX_T_NCONTACTS = 27,  /* i32 [N]         contact points generated in the last substep (diagnostic)    */
  SDX_T_DEBUG = 28,      /* i64 [64 + 2N]   profiling build only: [0, 64) phase time stamps (s_memtime) of env SDX_DEBUG_ENV in the last k_physics, then (entry, exit) stamps of every env */
  SDX_T_HARVEST_HAND = 29, /* f32 [8,5001,23,2] saved_grasp_hand_ternimal_states per brick-type group   GS:391-417 */
  SDX_T_HARVEST_OBJ = 30,  /* f32 [8,5001,13]   saved_grasp_object_ternimal_states                       GS:391-417 */
  SDX_T_HARVEST_COUNT = 31,/* i32 [8]           terminal states harvested so far (ring index = count % 5001) GS:1417,1440 */
  SDX_T_INSERT_AUX = 32,   /* f32 [N,8]         InsertSim: [0:3] rot_err (IS:1539), [3] |brick - site|, [4] rot_dist (IS:1656-1660) */
  SDX_T_TV_SUCCESS = 33,   /* f32 [SDX_TV_LOG_SLOTS,4] camera-frame target quaternions of successful episode ends (ring)   GS:1404-1412, IS:1392-1400 */
  SDX_T_TV_FAILURE = 34,   /* f32 [SDX_TV_LOG_SLOTS,4] ... of failed ones                                                  GS:1420-1438, IS:1401-1410 */
  SDX_T_TV_COUNT = 35,     /* i32 [2]           rows logged so far: [success, failure] (ring index = count % SDX_TV_LOG_SLOTS)                      */
  SDX_T_PILE_HARVEST = 36, /* f32 [8,S,132,13]  Orient: brick states of finished episodes that left the target brick reachable (ring per
                            *                    brick-type group; S = 512 for task_kind 1 (Orient) and 3 (Search, SE:1398-1420), else 1) = the saved piles the next task starts from    OR:1463-1488, GS:412-413 */
  SDX_T_PILE_HARVEST_COUNT = 37, /* i32 [8]     pile states harvested so far (ring index = count % S)                                    */
  SDX_T_SEG_IMAGE = 38,    /* i16 [N,128,128]   Search: segmentation image of the last render (0 = background / robot / bin, i+1 = brick i)  SE:877 */
  SDX_T_SEG_PIXELS = 39,   /* f32 [N,4]         Search: target pixel count, centroid row, centroid column, count of the render before   SE:1232-1241 */
  SDX_T_EMERGENCE = 40,    /* f32 [N]           Search: extras["emergence_reward"] = 5 x change of the pixel count                    SE:1640-1646 */
  SDX_T_JACOBIAN = 41,     /* f32 [N,23,6,23]   acquire_jacobian_tensor(sim, "hand") of a fixed-base articulation: link k+1 is row k, rows 0..2 linear,
                            *                    3..5 angular; the task reads [:, 7-1, :, :7] (GS:241,1601).  Refreshed by sdx_refresh_kinematics()
                            *                    (= gym.refresh_jacobian_tensors, GS:1095), NOT by sdx_step/sdx_simulate, which keep SDX_T_JAC_EEF current */
  SDX_T_TVALUE_OBS = 42,   /* f32 [N,652]       Search: t_value_obs_buf, ten 65-number frames (SE:375,1155-1166), newest last; columns 650, 651 are row
                            *                    padding (zeros).  Frame = obs_buf[:, 0:62] with [26:30] = camera-frame target quaternion, then the target's
                            *                    pixel centroid / 128 and pixel count / 100 */
  SDX_T_CONTACT_STATS = 43, /* i32 [4]           since create, in env-SUBSTEPS: [0] the largest number of contact points one env generated in one substep;
                            *                    [1] substeps in which an env still exceeded the per-env capacity (1536) after the rebuild of [2] and lost
                            *                    the excess in enumeration order - must stay 0 for results to mean anything, bench.py and the full-size
                            *                    tests check it; [2] substeps whose contact list was rebuilt without its speculative contacts (samples
                            *                    that neither touch nor penetrate) because it would not fit; [3] substeps in which a pair list overflowed
                            *                    (body pairs > 1535, candidate box pairs > 16384, surviving box pairs > 3072: the excess was not tested, its contacts are MISSING) - like [1] it
                            *                    must stay 0, the full-size tests assert it and bench.py flags it */
  SDX_T_WARM_COUNT = 44,   /* i32 [N]           contacts in each env's warm-start cache (scene.warm_start); the engine clears an
                            *                    env's entry when it resets the env; sdx_state_save / restore / clone (below) carry the cache with the state */
  SDX_T_CAM_ROT = 45,      /* f32 [N,4]         camera_view_segmentation_target_rot: the target brick's quaternion in the camera frame, the input of
                            *                    GraspInsertTValue (GS:1196-1201, OR:1201); written by sdx_compute_observations / sdx_post_physics */
  SDX_T_TV_KEYS = 46,      /* i64 [2,SDX_TV_LOG_SLOTS]  (step << 24 | env) of the append that filled each slot of the success / failure ring.  Ring
                            *                    slots are claimed with atomics, i.e. in hardware order; sorting a ring's rows by these keys gives the
                            *                    order a serial loop over steps and envs produces (what seqdex_amd.sim.ring_rows does) */
  SDX_T_HARVEST_KEYS = 47, /* i64 [8,SDX_HARVEST_SLOTS] the same for the grasp terminal-state rings */
  SDX_T_PILE_HARVEST_KEYS = 48, /* i64 [8,slots] the same for the pile rings of Orient / Search */
  SDX_T_WARM_KEYS = 49,    /* i32 [N,1536]     diagnostic view of the warm-start cache: identity of each cached contact of the last solve (body-pair rank
                            *                    13 bits | box pair 9 | direction 1 | sample 5, age in the 4 bits above), ascending; rows are valid up to
                            *                    SDX_T_WARM_COUNT; [1] when scene.warm_start == 0 (the cold solver keeps no cache) */
  SDX_T_WARM_LAMBDA = 50,  /* f32 [N,3,1536]   the accumulated impulses (normal, two tangents) of those contacts */
  /* domain randomization (sdx_set_randomization below): the per-env physics parameters k_physics reads while randomization is on.  They
   * always exist and hold the scene's values (factors 1) until a randomization writes them; the caller may also write them directly */
  SDX_T_DR_DOF = 51,       /* f32 [N,4,23]      kp, kd, lower, upper of every DOF - the limits the PHYSICS enforces (the task's action scaling keeps the
                            *                    scene's, as the reference reads them from the asset before randomizing, GS:561-590)              */
  SDX_T_DR_LINK = 52,      /* f32 [N,2,24]      hand link mass factor (inertia scales with it), hand link friction coefficient                     */
  SDX_T_DR_BRICK = 53,     /* f32 [N,2,72]      free brick mass factor (inertia scales with it; composes with seg_mass_scale), brick friction      */
  SDX_T_DR_GRAVITY = 54,   /* f32 [3]           gravity of every env                                                                             */
  SDX_T_DR_FRAME = 55,     /* i64 [2]           [0] frame = physics launches made while randomization was on (gym.get_frame_count), [1] the frame
                            *                    of the last gravity ("non-env") randomization (BT:237,248)                                      */
  SDX_T_COUNT = 56
} sdx_tensor_id;

/* Compact scene constants (row A0/A1 of SURVEY.md §8(a)); produced by tools/compile_scene.py from the
 * reference's URDF/STL/OBJ assets and shipped as seqdex_amd/scene_data/grasp_sim_scene.json. */
typedef struct {
  int32_t abi_version;                 /* = SDX_ABI_VERSION */
  /* robot kinematic tree */
  float base_pos[3];                   /* GS:624-626 */
  float base_quat[4];
  int32_t parent[SDX_NLINK];           /* -1 for body 0 */
  float joint_pos[SDX_NLINK][3];       /* joint frame origin in the parent body frame */
  float joint_quat[SDX_NLINK][4];      /* joint frame rotation in the parent body frame */
  float joint_axis[SDX_NLINK][3];      /* revolute axis in the child frame */
  float lower[SDX_NDOF], upper[SDX_NDOF];
  float kp[SDX_NDOF], kd[SDX_NDOF], effort[SDX_NDOF], vel_limit[SDX_NDOF], armature[SDX_NDOF]; /* GS:580-590 */
  float link_mass[SDX_NLINK];
  float link_com[SDX_NLINK][3];        /* body frame */
  float link_inertia[SDX_NLINK][6];    /* about COM, body frame: xx yy zz xy xz yz */
  int32_t n_rbox;
  int32_t rbox_link[SDX_MAX_RBOX];
  float rbox_center[SDX_MAX_RBOX][3];
  float rbox_quat[SDX_MAX_RBOX][4];
  float rbox_half[SDX_MAX_RBOX][3];
  /* bricks.  Collision shape of a brick = a COMPOUND of axis-aligned boxes in the brick's frame: the slabs of
   * the mesh's convex hull for a free brick (the reference loads every brick as ONE convex hull, GS:717-731), or - for each env's target
   * brick when seg_hollow != 0 - the hollow compound of the mesh itself (walls, roof, upper part: what V-HACD resolves, IS:698-709),
   * whose underside takes the studs of a base plate.  brick_half / brick_center = the bounding box of either compound (broadphase,
   * segmentation camera); the body's reference point is its centre of mass brick_com. */
  float brick_half[SDX_NBRICK_TYPES][3];
  float brick_center[SDX_NBRICK_TYPES][3];   /* centre of the bounding box in the brick's mesh frame */
  float brick_com[SDX_NBRICK_TYPES][3];      /* centre of mass (centroid of the convex hull) in the mesh frame */
  float brick_mass[SDX_NBRICK_TYPES];        /* 567 x hull volume */
  float brick_inertia[SDX_NBRICK_TYPES][3];  /* diagonal of the hull's inertia tensor about the centre of mass, mesh axes (the xz products
                                              * of the four wedge-shaped types, <= 0.37 Ixx, are dropped) */
  int32_t brick_nsub[SDX_NBRICK_TYPES];
  float brick_sub_center[SDX_NBRICK_TYPES][SDX_MAX_SUB][3];   /* mesh frame */
  float brick_sub_half[SDX_NBRICK_TYPES][SDX_MAX_SUB][3];
  int32_t seg_hollow;                        /* != 0: the target brick of every env collides as its hollow compound */
  int32_t hollow_nsub[SDX_NBRICK_TYPES];
  float hollow_sub_center[SDX_NBRICK_TYPES][SDX_MAX_SUB_HOLLOW][3];
  float hollow_sub_half[SDX_NBRICK_TYPES][SDX_MAX_SUB_HOLLOW][3];
  int32_t brick_type[SDX_NBRICK];
  /* static bodies (world frame, axis aligned).  Rows 0..n_static-1 of the table are what an env sees; a body is a compound of the
   * boxes static_sub_*[first .. first + n) and static_center / static_half is its bounding box (a single-box body: the box itself).
   * The studs of a compound (boxes 1.. of a body) are SAMPLED like a brick's boxes (both directions of a pair), a body box only
   * receives the other shape's samples. */
  int32_t n_static;
  float static_center[SDX_MAX_STATIC_TAB][3];
  float static_half[SDX_MAX_STATIC_TAB][3];
  int32_t static_sub_first[SDX_MAX_STATIC_TAB];
  int32_t static_sub_n[SDX_MAX_STATIC_TAB];
  int32_t n_static_sub;
  float static_sub_center[SDX_MAX_STATIC_SUB][3];
  float static_sub_half[SDX_MAX_STATIC_SUB][3];
  /* default actor states for everything that is not a brick (written into ROOT at create) */
  float object_init_state[13];         /* GS:687-689,927-929 */
  float goal_reset_pos[3];             /* goal_init_state + goal_displacement, GS:694-700,1348 */
  float static_actor_pos[6][3];        /* table + 5 bin walls, actor slots 3..8 */
  float base_plate_pos[3];             /* GS:838 */
  float fixed_brick_pos[SDX_NBRICK - SDX_NFREE][3];
  float free_spawn_pos[SDX_NFREE][3];  /* GS:737-742 */
  float free_spawn_quat[4];
  /* task constants */
  int32_t hand_base_body;              /* 7, GS:355 */
  int32_t fingertip_body[4];           /* link_3.0, link_7.0, link_11.0, link_15.0: ff, mf, rf, th  GS:183-186 */
  float camera_offset_quat[4];         /* GS:887-888 */
  float camera_offset_pos[3];          /* GS:889 */
  float arm_prepare_pose[7];           /* GS:267 */
  float finger_reset_unscaled[16];     /* GS:1531 */
  float insert_pose_a[7], insert_pose_b[7]; /* GS:278,281 */
  float max_episode_length;            /* 150, EG:6 */
  float act_moving_average;            /* 1.0, EG:16 */
  float av_factor;                     /* 0.1, GS:151 */
  float clip_obs, clip_actions;        /* 5, 1: VR:18 */
  /* simulation parameters (CF:188, EG:155-167) and our solver constants */
  float dt;
  int32_t substeps;
  int32_t solver_iters;
  float contact_offset;
  float gravity[3];
  float friction;
  float baumgarte;                     /* position-error feedback factor  */
  float max_depenetration_vel;
  float jacobi_relax;                  /* relaxation on the mass-split Jacobi update */
  float warm_start;                    /* every solve starts from this fraction of the impulses the same contacts
                                        * (pair, direction, sample) ended the previous solve with; 0 = start from zero */
  float warm_age;                      /* the fraction ramps up linearly with the number of consecutive solves a contact has existed and
                                        * reaches warm_start after warm_age of them (0: no ramp; at most 16: the age is a 4-bit saturating counter, sdx_create
                                        * rejects larger values); DESIGN.md section 3.E */
  float robot_angular_damping;         /* asset_options.angular_damping of the arm-hand asset (GS:546: 0.01 1/s): every substep scales the joint
                                        * velocities by (1 - h x damping) - for a chain of revolute joints the joint-space image of PhysX's
                                        * per-link angular damping */
  float grasp_tvalue_gate;             /* BlockAssemblyGraspSim harvests a terminal state only when its transition value exceeds this: 0.8 (GS:1406) */
  float orient_tvalue_gate;            /* BlockAssemblyOrient binarises its transition value at this threshold before anything reads it: 0.99
                                        * (OR:1203); a chain run with an early, not yet confident T-value may lower it (say so when you do) */
  /* which task's per-step tensor code the pre/post-physics kernels run (sdx_task_kind): SDX_TASK_GRASP = 0 = BlockAssemblyGraspSim (GS),
   * SDX_TASK_ORIENT = 1 = BlockAssemblyOrient (OR = tasks/block_assembly/allegro_hand_block_assembly_orient.py; targets/IK OR:1720-1778),
   * SDX_TASK_INSERT = 2 = BlockAssemblyInsertSim (IS; position action + fixed wrist orientation IS:1526-1572, 75-number observation IS:1280-1298,
   *     insertion reward IS:1640-1695, reset from harvested grasp states IS:1416-1494),
   * SDX_TASK_SEARCH = 3 = BlockAssemblySearch (SE; tracking IK 0.24 above the target SE:1565-1575, 62-number observation SE:1220-1230, its own asymmetric
   *     state SE:1168-1218, reward SE:1660-1711, reset with 60 settling steps and a segmentation render SE:1274-1538) */
  int32_t task_kind;
  float target_euler[3];               /* Orient: fixed wrist orientation of the tracking IK, OR:477 */
  float seg_mass_scale;                /* mass (and inertia) factor of each env's target brick: 1 (GS:980-981), 50 in Orient (OR:977) */
  /* task_kind 2 = BlockAssemblyInsertSim (IS = tasks/block_assembly/allegro_hand_block_assembly_insert_sim.py): the base plate is
   * one of 4x4x{1,2,4} chosen by env % 3 (IS:971-977): env e sees row static_var_row[e % 3] of the static-body table in slot
   * `static_var_slot`; -1 = every env sees rows 0..n_static-1 as they are. */
  int32_t static_var_slot;
  int32_t static_var_row[3];
  /* task_kind 3 = BlockAssemblySearch (SE = tasks/block_assembly/allegro_hand_block_assembly_search.py): the fixed segmentation camera
   * (128 x 128; set_camera_location SE:875; Isaac Gym's default horizontal field of view 90 degrees) */
  float seg_cam_pos[3];
  float seg_cam_target[3];
  float seg_cam_hfov_deg;
  float search_default_arm[7];         /* arm_hand_default_dof_pos[:7]: hand parked out of the camera's view, SE:203 */
  float search_finger_pose[16];        /* finger joints (radians) of the default AND the prepare pose, SE:205-206,220-222 */
} sdx_scene_desc;

/* ---- domain randomization (BaseTask.apply_randomizations, BT:229-420; called by every BlockAssembly task at create and in each
 * reset_idx, GS:106-107,515-516,1395-1396).  The definition restates Isaac Gym's gymutil sampling rules:
 *   schedule factor s: linear = min(frame, schedule_steps) / schedule_steps, constant = (frame < schedule_steps ? 0 : 1), none = 1
 *   range transform:   additive: both ends x s; scaling: end x s + (1 - s).  gaussian range = [mu, sigma]: mu as an end, sigma x s
 *   distribution:      gaussian mu + sigma z (z from Box-Muller), uniform lo + (hi - lo) u, loguniform exp(log lo + (log hi - log lo) u)
 *   buckets:           num_buckets > 0 snaps the sample down to the grid lo + (hi - lo) k / num_buckets, k in [0, num_buckets), with
 *                      [lo, hi] = the UNtransformed range (gaussian: mu -+ 2 sqrt(sigma)); below the grid: k = 0
 *   operation:         value = default + sample (additive) or default x sample (scaling); default = the sdx_scene_desc value
 *   s == 0:            the attribute is not sampled, value = default (deviation: gymutil snaps the identity sample to a bucket)
 * When: sdx_set_randomization samples every env and gravity at the current frame.  Afterwards, at the start of sdx_step /
 * sdx_pre_physics (before any reset physics, Orient's and Search's settling launches included), an env with reset_buf != 0 and
 * randomize_buf >= frequency is re-sampled and its randomize_buf set to 0; gravity is re-sampled when some env resets and
 * frame - last_rand_frame >= frequency.  sdx_reset_idx applies the same rule with its env mask in place of reset_buf, before it
 * resets the envs.  All on the device, no host synchronisation.
 * Randomness: u = hash(seed, env x 287 + slot, draw) (the counter RNG of DESIGN.md section 6; draw = how many times this env was sampled):
 * a sample depends on seed, env, slot and draw only, not on N or launch order. */
typedef enum { SDX_DR_NONE = 0, SDX_DR_GAUSSIAN = 1, SDX_DR_UNIFORM = 2, SDX_DR_LOGUNIFORM = 3 } sdx_dr_distribution;
typedef enum { SDX_DR_ADDITIVE = 1, SDX_DR_SCALING = 2 } sdx_dr_operation;
typedef enum { SDX_DR_SCHED_NONE = 0, SDX_DR_SCHED_LINEAR = 1, SDX_DR_SCHED_CONSTANT = 2 } sdx_dr_schedule;
typedef struct {
  int32_t distribution;      /* sdx_dr_distribution; SDX_DR_NONE = this quantity is not randomized (keeps its current row value) */
  int32_t operation;         /* sdx_dr_operation */
  int32_t schedule;          /* sdx_dr_schedule */
  int32_t schedule_steps;
  int32_t num_buckets;       /* 0 = continuous */
  float range[2];            /* [lo, hi] or [mu, sigma] */
} sdx_dr_attr;
typedef struct {
  int32_t frequency;         /* randomization_params.frequency (BT:231: default 1) */
  sdx_dr_attr gravity;       /* sim_params.gravity: one sample per component                                  */
  sdx_dr_attr dof_stiffness, dof_damping, dof_lower, dof_upper;   /* actor_params.hand.dof_properties, per env and DOF */
  sdx_dr_attr link_mass;     /* actor_params.hand.rigid_body_properties.mass, per env and link                */
  sdx_dr_attr link_friction; /* actor_params.hand.rigid_shape_properties.friction, per env and link           */
  sdx_dr_attr brick_mass;    /* actor_params.lego.rigid_body_properties.mass: every free brick                 */
  sdx_dr_attr brick_friction;/* actor_params.lego.rigid_shape_properties.friction: every free brick            */
} sdx_dr_desc;

/* One of randomization_params.observations / .actions (BaseTask.apply_randomizations BT:259-329, applied by BaseTask.step BT:131-132,
 * 149-150): noise on the policy's observation or on the executed action (sdx_set_noise below).
 *   distribution SDX_DR_GAUSSIAN (range = [mu, sigma]) or SDX_DR_UNIFORM (range = [lo, hi]); SDX_DR_NONE = this side is off
 *   range            the white part, drawn anew every step;  range_correlated  the correlated part, one draw per (env, column) that
 *                    stays until the next non-env randomization ([0, 0] = none) */
typedef struct {
  int32_t distribution;      /* sdx_dr_distribution without SDX_DR_LOGUNIFORM */
  int32_t operation;         /* sdx_dr_operation */
  int32_t schedule;          /* sdx_dr_schedule */
  int32_t schedule_steps;
  float range[2];            /* [mu, sigma] or [lo, hi] of the white part */
  float range_correlated[2]; /* [mu, sigma] or [lo, hi] of the correlated part */
} sdx_noise_attr;

typedef struct sdx_sim* sdx_handle;

/* Scene build: replaces create_sim/add_ground/load_asset/create_env/create_actor/prepare_sim
 * (GS:505-1058, BT:83-84).  Blocking.  Fails with SDX_ERR_NO_DEVICE when no GPU is present. */
int sdx_create(const sdx_scene_desc* scene, int32_t num_envs, int32_t device, uint64_t seed, sdx_handle* out);
int sdx_destroy(sdx_handle h);

/* acquire_*_tensor + gymtorch.wrap_tensor (GS:237-241,313-322) and the BaseTask buffers (BT:57-68). */
int sdx_tensor(sdx_handle h, int32_t id, void** dev_ptr, int64_t shape[4], int32_t* ndim, int32_t* dtype);

/* Saved pile states: replaces pickle.load(".../saved_searching_ternimal_states_good_mo_tvalue.pkl")
 * (GS:412-413): host float32 [8, K, 132, 13].  Blocking copy to HBM. */
int sdx_load_initial_states(sdx_handle h, const float* piles_host, int32_t K);

/* GraspInsertTValue parameters (GS:417-419): host float32[SDX_TV_PARAMS] packed as
 * W1[256,4] b1[256] W2[128,256] b2[128] W3[64,128] b3[64] W4[2,64] b4[2].  Blocking. */
int sdx_set_tvalue_weights(sdx_handle h, const float* params_host, int32_t n);

/* BlockAssemblySearch only (task_kind 3): RetriGraspTValue(650, 2) parameters (SE:395-410): host float32[SDX_RETRI_TV_PARAMS] packed as
 * W1[1024,650] b1[1024] W2[512,1024] b2[512] W3[128,512] b3[128] W4[2,128] b4[2] (torch layout W[out][in]).  Every step the task
 * evaluates it on SDX_T_TVALUE_OBS as it stood BEFORE this step's frame is appended and stores sigmoid(out)[:, 1] in SDX_T_TVALUE
 * (SE:1133-1134); like the reference's, the value reaches compute_hand_reward but does not enter the reward (SE:1687).  Blocking. */
int sdx_set_retri_tvalue_weights(sdx_handle h, const float* params_host, int32_t n);

/* BaseTask.step(actions) (BT:130-150) fused: pre_physics_step (GS:1555-1638, device-side masked reset
 * instead of reset_buf.nonzero()) -> simulate x controlFreqInv (BT:138-140) -> post_physics_step
 * (GS:1640-1658).  actions: device f32 [N,23], clamped to +-clip_actions inside (VR:166). */
int sdx_step(sdx_handle h, const float* actions_dev, void* stream);

/* The three stages of sdx_step as separate entry points (used by the parity tests and by callers that keep
 * reference-style task code on top of the simulator). */
int sdx_pre_physics(sdx_handle h, const float* actions_dev, void* stream);   /* GS:1555-1638 */
int sdx_simulate(sdx_handle h, void* stream);                                /* BT:140 + refresh_* GS:1091-1095 */
int sdx_post_physics(sdx_handle h, void* stream);                            /* GS:1640-1645 */

/* compute_observations() only (GS:1090-1218): obs/states frames + stacking, no progress++/reward. */
int sdx_compute_observations(sdx_handle h, void* stream);

/* reset_idx(env_ids) (GS:1361-1553) for envs with env_mask_dev[i] != 0 (device u8 [N]).
 * pile_choice_dev: device i32 [N] saved-pile index per env, or NULL to draw it from the counter RNG
 * (the reference uses python random.sample, GS:1510). */
int sdx_reset_idx(sdx_handle h, const uint8_t* env_mask_dev, const int32_t* pile_choice_dev, void* stream);

/* refresh_rigid_body_state / jacobian after the caller overwrote DOF/ROOT through the tensor views
 * (set_dof_state_tensor_indexed / set_actor_root_state_tensor_indexed, GS:1514,1543): recomputes FK,
 * link velocities and the end-effector Jacobian from SDX_T_DOF. */
/* Search: render the segmentation camera of every env from the current ROOT / RB states -> SDX_T_SEG_IMAGE, SDX_T_SEG_PIXELS,
 * SDX_T_EMERGENCE (gym.render_all_camera_sensors + the pixel statistics of SE:1232-1241,1640-1646).  task_kind 3 only. */
int sdx_render_segmentation(sdx_handle h, void* stream);
int sdx_refresh_kinematics(sdx_handle h, void* stream);

/* set_actor_root_state_tensor_indexed / set_dof_state_tensor_indexed / set_dof_position_target_tensor_indexed
 * (GS:1355,1514,1539,1543; gymtorch.unwrap_tensor(...) + int32 sim-domain actor indices): applies the rows of `src_dev` that belong to
 * the listed actors.  id selects the state: SDX_T_ROOT (src f32 [N*142,13]: rows of the listed actors -> SDX_T_ROOT and the actor's
 * body row of SDX_T_RB; the robot's fixed base ignores it), SDX_T_DOF (src f32 [N*23,2]) or SDX_T_TARGETS (src f32 [N,23]): the
 * listed actors must be hand actors (slot 0 of an env, index env*142) and all 23 rows of that env are taken; SDX_T_DOF also refreshes
 * the link states and Jacobians of every env (sdx_refresh_kinematics).  src_dev may be the library's own tensor (the caller edited
 * it in place, as the reference does with root_state_tensor / dof_state) or a tensor of the caller's (as the reference's cur_targets).
 * actor_ids_dev: device i32 [n]; actor index = env * SDX_ACTORS + slot.  Out-of-range ids are ignored. */
int sdx_set_indexed(sdx_handle h, int32_t id, const float* src_dev, const int32_t* actor_ids_dev, int32_t n, void* stream);

/* Domain randomization on (desc != NULL) or off (NULL).  On: k_physics reads the per-env rows SDX_T_DR_* instead of the scene constants
 * (contact friction = the mean of the two bodies' coefficients, PhysX's default combine mode; static bodies keep sdx_scene_desc.friction)
 * and the first randomization is enqueued on `stream`.  A desc whose attributes are all SDX_DR_NONE turns the per-env path on without
 * sampling (the rows keep what they hold: a caller-supplied sampler writes them).  Off: the rows are reset to the scene's values and the
 * physics returns to the scene constants.  Stream-ordered; frequency >= 1, enums, finite ranges, lo <= hi (uniform, loguniform: lo > 0),
 * sigma >= 0 (gaussian) are checked (SDX_ERR_INVALID). */
int sdx_set_randomization(sdx_handle h, const sdx_dr_desc* desc, void* stream);

/* Observation and action noise (randomization_params.observations / .actions).  NULL or distribution SDX_DR_NONE
 * turns a side off; with both off nothing is launched.  Needs randomization to be on (a desc whose attributes are all SDX_DR_NONE is
 * enough), because the noise is a pure function of that path's counters: SDX_ERR_STATE otherwise.  sdx_set_randomization(NULL) turns the
 * noise off too.  Stream-ordered (the next sdx_step / sdx_pre_physics / sdx_post_physics uses the new blocks).  Checked
 * (SDX_ERR_INVALID with a message): distribution gaussian or uniform, known operation and schedule, schedule_steps > 0 with a
 * schedule, finite numbers, sigma >= 0 (gaussian) and lo <= hi (uniform) in range and range_correlated.
 *   schedule  s = the factor of sdx_set_randomization, evaluated at SDX_T_DR_FRAME[1] (the frame of the last non-env randomization: the
 *             reference freezes the scaled numbers when it rebuilds its lambda at that event, BT:260-329).  Gaussian additive: all
 *             four numbers x s; gaussian scaling: sigma x s, mu x s + (1 - s); uniform additive: all four ends x s; uniform scaling:
 *             end x s + (1 - s) - for both parts.  (A scaling block at s = 0 therefore multiplies by 2: both parts become 1.)
 *   operand   per (env, column): corr + white.  white = mu + sigma z or lo + (hi - lo) u, drawn anew at every step.  corr = mu_c +
 *             sigma_c z or, for the uniform distribution too, lo_c + (hi_c - lo_c) z with z standard normal (BT:326); it changes when
 *             SDX_T_DR_FRAME[1] does: some env resets and frame - last_rand_frame >= frequency, whether or not gravity is randomized.
 *   random    column pair p = column / 2 shares one hash(seed ^ tag, env x 256 + p, counter): u0, u1 = its two 24-bit uniforms,
 *             z = sqrt(-2 log u0) x (cos, sin)(2 pi u1) and u = (u0, u1) for the (even, odd) column.  counter = gravity's draw count
 *             (corr) or the step counter (white; actions see the steps completed before this one, observations those including it);
 *             tags 0x0B5C / 0x0B57 (observations corr / white), 0xAC7C / 0xAC77 (actions).  Nothing depends on N or launch order, no
 *             state is kept: sdx_state_save_all / restore_all reproduce the noise.
 *   observations  SDX_T_OBS_CLAMPED = clamp(op(SDX_T_OBS, operand), +-clip_obs) over every column of the row, written by sdx_step and
 *             sdx_post_physics after the task's kernel (not by sdx_compute_observations: BT:149 sits in step).  SDX_T_OBS stays the clean
 *             row (so the frames GraspSim stacks carry no earlier noise, GS:1330-1332), SDX_T_STATES* and SDX_T_TVALUE_OBS get none.
 *   actions   a' = op(clamp(a, +-clip_actions), operand), not clamped again (VR:166, then BT:131); SDX_T_ACTIONS, the targets and the
 *             action columns of the observation see a'.  The caller's buffer is not written.  Uses the blocks and counters in force
 *             before this step's re-sampling; the observations use those after it.
 *   zero      an additive block whose four scaled numbers are all zero (frame 0 of a linear schedule) leaves its tensor bit for bit
 *             what it is without noise.
 * op(x, o) = x + o (additive) or x o (scaling). */
int sdx_set_noise(sdx_handle h, const sdx_noise_attr* observations, const sdx_noise_attr* actions, void* stream);

/* External forces and torques on rigid bodies (gym.apply_rigid_body_force_tensors).  forces_dev / torques_dev:
 * caller-owned device f32 [N, SDX_BODIES, 3], indexed like SDX_T_RB; either may be NULL (no forces / no torques).  The wrench applies to
 * the NEXT physics launch only - the one of sdx_simulate, or of sdx_step after its pre-physics kernel (not the settling launches of an
 * Orient / Search reset event) - and is then forgotten.  A second call before that launch REPLACES the pending wrench, both pointers
 * NULL clears it.  Nothing is enqueued here: the pointers travel by value with that launch, which reads the buffers on ITS stream, so
 * they must stay alive and unchanged until it has run (`stream` is unused).  space is not SDX_SPACE_ENV / SDX_SPACE_LOCAL: SDX_ERR_INVALID.
 *   point     the force acts at the body's centre of mass, the torque about it.
 *   frames    SDX_SPACE_ENV: the env's world axes.  SDX_SPACE_LOCAL: the body's axes, rotated to world ONCE per step with the
 *             orientation the body has at the start of the step; the world wrench is held constant over the substeps.
 *   bodies    free bricks (rows SDX_BODY_BRICK0 .. + SDX_NFREE - 1): every substep v += F h / m, w += R diag(1 / I) R^T T h with the mass
 *             and inertia the solver uses (seg_mass_scale on the target brick, the SDX_T_DR_BRICK factor while randomization is on), no
 *             gyroscopic term.  Robot links 1 .. SDX_NLINK - 1: tau_j += sum over the links k below dof j of a_j . ((c_k - o_j) x F_k + T_k),
 *             beside the velocity-product wrenches; the effort limit keeps applying to the drive only.  Rows of bodies that cannot move
 *             are ignored: link 0, the fixed bricks, the statics, the object and goal actors.
 *   contacts  SDX_T_CONTACT stays the sum of the contact impulses.
 *   zero      a body whose force and torque rows are all zero is stepped bit for bit as without the call, negative zeros included. */
typedef enum { SDX_SPACE_ENV = 0, SDX_SPACE_LOCAL = 1 } sdx_force_space;
int sdx_apply_rigid_body_forces(sdx_handle h, const float* forces_dev, const float* torques_dev, int32_t space, void* stream);

/* Joint torques (gym.set_dof_actuation_force_tensor with DOF_MODE_EFFORT per DOF).  dof_forces_dev: caller-owned
 * device f32 [N, SDX_NDOF] or NULL; drive_off_mask bit j: the PD drive of DOF j is off (a bit >= SDX_NDOF: SDX_ERR_INVALID).  The rules of
 * sdx_apply_rigid_body_forces: nothing is enqueued (`stream` is unused), pointer and mask travel by value with the NEXT physics launch -
 * sdx_simulate, or sdx_step's own, not the settling launches - and are then forgotten; a second call before it REPLACES them, NULL with
 * mask 0 clears them; the buffer must stay alive and unchanged until that launch has run.  A pending slot of its own: neither
 * sdx_apply_rigid_body_forces nor the sampler of sdx_set_force_perturbation touches it.  Not part of a snapshot.
 *   torque    every substep tau_j = (bit j ? 0 : clamp(PD_j, +-effort_j)) + clamp(u_j, +-effort_j) - tc_j, u held constant over the substeps.
 *   off       a DOF whose drive is off also drops the implicit terms h kd + h^2 kp from the diagonal of H (the env's SDX_T_DR_DOF gains
 *             while randomization is on); its armature, joint limits and velocity limit keep applying.
 *   zero      a DOF whose u_j is zero (of either sign) and whose bit is clear is stepped bit for bit as without the call. */
int sdx_apply_dof_forces(sdx_handle h, const float* dof_forces_dev, uint32_t drive_off_mask, void* stream);
/* Joint-space dynamics of the robot (acquire_mass_matrix_tensor, the DOF force tensor) from the CURRENT SDX_T_DOF and
 * SDX_T_TARGETS: one launch on `stream`, part of no step.  Caller-owned device buffers, any of them NULL (all three: SDX_ERR_INVALID):
 *   mass_dev  f32 [N, SDX_NDOF, SDX_NDOF]  M(q) + armature, symmetric bit for bit, without the implicit PD terms of the step's H
 *   bias_dev  f32 [N, SDX_NDOF]            C(q, qd) qd (no gravity acts on the robot): the step's tc
 *   drive_dev f32 [N, SDX_NDOF]            the clamped PD torque that the first substep of the next launch would apply (h = dt / substeps;
 *                                          the drive-off mask is not applied)
 * While randomization is on, the gains are the env's SDX_T_DR_DOF rows and masses and inertias carry the SDX_T_DR_LINK factors, as in the step. */
int sdx_dof_dynamics(sdx_handle h, float* mass_dev, float* bias_dev, float* drive_dev, void* stream);

/* Operational-space (end-effector impedance) torques of the arm: from the CURRENT SDX_T_DOF to a torque row for
 * sdx_apply_dof_forces in one launch on `stream`, part of no step; it reads SDX_T_DOF (and SDX_T_DR_LINK while randomization is on) and
 * writes the caller's buffers only.  With the 7 arm DOFs and the hand base link (the link of SDX_T_JAC_EEF), per env:
 *   M7 = sdx_dof_dynamics' mass[0:7, 0:7] (the hand's links at their current pose in it), b = its bias[0:7]
 *   J  = [6, 7], what sdx_refresh_kinematics would put in SDX_T_JAC_EEF at this q (computed here: no refresh needed), v = J qd[0:7]
 *   A  = J M7^-1 J^T + damping^2 I;  F = kp . dpose - kd . v;  w = A^-1 F  (both solves Cholesky)
 *   u_null = M7 (kp_null . (q_null - q) - kd_null . qd)
 *   u  = J^T w + u_null - J^T A^-1 J M7^-1 u_null + (compensate_bias ? b : 0)
 *   dpose_dev   f32 [N, 6]         the pose error control_ik takes: position difference, then the rotation vector
 *   torques_dev f32 [N, SDX_NDOF]  u clamped to +-effort on DOFs 0..6, +0.0f on the 16 hand DOFs: with drive_off_mask 0x7f the hand keeps
 *                                  its PD drives
 *   wrench_dev  f32 [N, 6] or NULL w
 * SDX_ERR_INVALID with a message: attr, dpose_dev or torques_dev NULL; a gain, q_null or damping that is not finite; a negative gain or
 * damping. */
typedef struct {
  float kp[6], kd[6];                       /* task-space stiffness and damping: rows 0..2 linear, 3..5 angular */
  float kp_null[7], kd_null[7], q_null[7];  /* the posture spring-damper acting in the null space of J */
  float damping;                            /* the damped-least-squares term of A (control_ik uses 0.05) */
  int32_t compensate_bias;                  /* non-zero: add the velocity-product bias */
} sdx_osc_attr;
int sdx_osc_torques(sdx_handle h, const sdx_osc_attr* attr, const float* dpose_dev, float* torques_dev, float* wrench_dev, void* stream);

/* Pose solver: the 23 joint angles that put the hand base at a pose and the four fingertips at points, by damped
 * least squares iterated inside ONE launch on `stream`, part of no step.  It reads SDX_T_DOF positions only when q0_dev is NULL, and rows
 * 2 and 3 of SDX_T_DR_DOF while randomization is on: the limits it honours are the ones the physics enforces (the scene's lower / upper
 * otherwise).  It writes the caller's buffers only; q0_dev and q_out_dev may be the same buffer.  Caller-owned device buffers:
 *   q0_dev        f32 [N, SDX_NDOF] or NULL   start configuration (NULL: the positions of SDX_T_DOF)
 *   base_pos_dev  f32 [N, 3]                  hand-base target position, env frame          (may be NULL when bit 0 is clear)
 *   base_quat_dev f32 [N, 4] xyzw             hand-base target orientation, as an SDX_T_RB row holds it (may be NULL when bit 0 is clear)
 *   tip_pos_dev   f32 [N, 4, 3]               fingertip targets ff, mf, rf, th, env frame   (may be NULL when bits 1..4 are clear)
 *   q_out_dev     f32 [N, SDX_NDOF]           the solution
 *   err_out_dev   f32 [N, 6] or NULL          error norms at q_out from a final forward kinematics: |position error| and |rotation error|
 *                                             of the base, |position error| of the four tips; +0.0f for a task that is not selected
 *   info_out_dev  i32 [N, 6] or NULL          column 0: bit t set = task t met its tolerance (the bits of task_mask); column 1: iterations
 *                                             of the arm; columns 2..5: iterations of each finger
 * The law, per env.  Forward kinematics and link axes are those of sdx_refresh_kinematics: q_out written to SDX_T_DOF and refreshed shows
 * the solved pose in SDX_T_RB.  With p_k, R_k the frame of link k and a_k the world axis of its joint:
 *   stage 1 (bit 0), on DOFs 0..6, from q <- q0, up to max_iters times:
 *     e  = [target_pos - p7 ; r],  r = s 2 xyz(target_quat (x) conj(quat7)), s = -1 if that product's w < 0, else +1
 *          (the pose error of control_ik and of torque_control.pose_error)
 *     stop, converged, if |e_pos| <= pos_tol and |r| <= rot_tol (a tolerance of 0 is never met, not even by an error of 0)
 *     J  = [6, 7], column j = [a_{j+1} x (p7 - p_{j+1}) ; a_{j+1}]: the terms of SDX_T_JAC_EEF
 *     dq = J^T (J J^T + damping_arm^2 I)^-1 e   (Cholesky);   dq <- dq / max(1, max_j |dq_j| / max_step)
 *     q[0:7] <- clamp(q[0:7] + dq, lower, upper)
 *   stage 2 (bits 1..4), for each selected finger f on its DOFs 7 + 4 f .. 10 + 4 f (links 8 + 4 f .. 11 + 4 f), with the arm at the result
 *   of stage 1 (at q0 when bit 0 is clear): the same loop with the point c = p_tip + R_tip tip_offset[f] of link fingertip_body[f],
 *     e = target - c,  J = [3, 4], column i = a_i x (c - p_i),  a 3 x 3 system with damping_finger,  stop when |e| <= pos_tol.
 * The iteration count of a task is the number of steps it took.  DOFs of tasks that are not selected leave as the bits of q0; a task that
 * meets its tolerance at q0 takes 0 iterations and leaves its DOFs bit-equal.  For finite targets and q0 inside the limits every output is
 * finite and inside the limits.  There is no null-space posture term, no collision check, and arm and fingers are not solved together.
 * SDX_ERR_INVALID with a message: attr or q_out_dev NULL; a NULL target that a selected task needs; task_mask 0 or with a bit above 4;
 * max_iters outside 1..256; a number of attr that is not finite or is negative; max_step <= 0; a scene whose robot is not a 7-link arm
 * chain carrying four 4-link finger chains that end in fingertip_body. */
typedef struct {
  uint32_t task_mask;        /* bit 0: hand-base pose (solves DOFs 0..6); bits 1..4: fingertip ff, mf, rf, th (solves that finger's 4 DOFs) */
  int32_t  max_iters;        /* 1..256 */
  float    damping_arm;      /* DLS term of the 6x6 arm system   (control_ik uses 0.05) */
  float    damping_finger;   /* DLS term of the 3x3 finger systems (lever arms are centimetres: 0.01) */
  float    max_step;         /* rad: a step is scaled down so that its largest |dq_j| is at most this; > 0 */
  float    pos_tol, rot_tol; /* m, and the length of the rotation part of the pose error; 0 = never stop early */
  float    tip_offset[4][3]; /* the controlled point of each fingertip, in the frame of sdx_scene_desc.fingertip_body[f] */
} sdx_ik_attr;
int sdx_solve_ik(sdx_handle h, const sdx_ik_attr* attr, const float* q0_dev,
                 const float* base_pos_dev, const float* base_quat_dev, const float* tip_pos_dev,
                 float* q_out_dev, float* err_out_dev, int32_t* info_out_dev, void* stream);

/* Random pushes on the target brick (the reference's forceScale / forceProbRange / forceDecay / forceDecayInterval, morb.py:1495-1516;
 * DESIGN.md section 21).  rb_forces_dev f32 [N, SDX_BODIES, 3] and prob_dev f32 [N] are CALLER-OWNED device buffers (the task's rb_forces
 * and random_force_prob): they are read and written by the launches of the calls that follow, must stay alive while the sampler is on,
 * and are NOT part of a sim snapshot (copy them beside sdx_state_save_all / restore_all to repeat a run's pushes).  attr NULL or
 * force_scale <= 0 turns the sampler off.  Independent of sdx_set_randomization.  Checked (SDX_ERR_INVALID with a message): finite
 * numbers, 0 < prob_lo <= prob_hi <= 1, decay in (0, 1], decay_interval > 0, non-NULL buffers.  On the call itself every env draws
 * its probability (enqueued on `stream`); rb_forces_dev is left as it is.
 * While on, sdx_step and sdx_pre_physics launch k_force_perturb once, in this order:
 *   1 reset  envs that reset in this call (reset_buf, as the randomization sampler reads it): their rows <- 0,
 *            prob[e] <- exp((log lo - log hi) u + log hi);  sdx_reset_idx does this step for the envs of its mask
 *   2 decay  rb_forces *= decay^(dt / decay_interval) over the whole tensor (the factor is rounded once from double)
 *   3 push   where u' < prob[e]: the row of the env's target brick <- z m force_scale, z three standard normals, m the brick's mass as the
 *            physics sees it (brick_mass x seg_mass_scale, x the SDX_T_DR_BRICK factor while randomization is on)
 * and (rb_forces_dev, NULL, SDX_SPACE_ENV) becomes the pending wrench of that step's physics launch, REPLACING the caller's own pending
 * wrench: extra forces are added into rb_forces_dev (they then decay like the pushes).
 * Random numbers are stateless: hash(seed ^ 0xF0CE, env x 256 + slot, step counter); slot 0: u' (first 24-bit uniform), slot 1: z_x, z_y
 * (cos, sin of one Box-Muller pair, in double, rounded once), slot 2: z_z (cos), slot 3: u. */
typedef struct { float force_scale, prob_lo, prob_hi, decay, decay_interval; } sdx_force_perturb_attr;
int sdx_set_force_perturbation(sdx_handle h, const sdx_force_perturb_attr* attr, float* rb_forces_dev, float* prob_dev, void* stream);

/* Contact report (gym.get_env_rigid_contacts, per contact and on the device): the contact list of a step's LAST
 * solve - the last substep's, the list whose impulses SDX_T_CONTACT and the warm-start cache describe - written by the physics launch
 * itself into CALLER-OWNED device buffers.  Per env e the first count[e] columns of every row are written, in the solver's list order;
 * columns beyond count[e] are left as they are.  count[e] = min(SDX_T_NCONTACTS[e], SDX_MAX_CONTACTS), and with the warm start on it is
 * SDX_T_WARM_COUNT[e] and key is SDX_T_WARM_KEYS & 0x0fffffff column by column; key is written whether or not the solver is warm.
 *   sides     a contact has a side a and a side b (the narrowphase samples a box of side a against a box of side b).  normal points out of
 *             side b towards side a: the normal impulse pushes side a along +normal.  force acts on side a, side b receives -force.
 *   force     (normal lam0 + t1 lam1 + t2 lam2) / h with the accumulated impulses the last solve ended with, h = dt / substeps, and the
 *             solver's own tangent basis: an impulse of ONE substep over its length, like SDX_T_CONTACT.
 * sdx_set_contact_report arms the report: while armed it is written by EVERY physics launch of sdx_simulate / sdx_step, on that launch's
 * stream (not by the settling launches of an Orient / Search reset event); the buffers must stay alive until the report is disarmed
 * (report == NULL) and the last such launch has run.  Any pointer but count may be NULL (that column is not written); a non-NULL report
 * with count == NULL: SDX_ERR_INVALID with a message.  Nothing is enqueued by the call itself (`stream` is unused); the struct is copied.
 * Armed or not, every other result of a step is bit for bit the same.  Not part of a snapshot. */
#define SDX_MAX_CONTACTS 1536   /* contacts per env a solve can take: the capacity of the report's rows */
typedef struct {
  int32_t*  count;       /* i32 [N]                        required */
  int32_t*  body;        /* i32 [N, 2, SDX_MAX_CONTACTS]   side a, side b: row of SDX_T_RB (link k -> k, free brick i -> SDX_BODY_BRICK0 + i), static world -> -1 */
  uint32_t* key;         /* u32 [N, SDX_MAX_CONTACTS]      identity = bits 0..27 of the SDX_T_WARM_KEYS entry, age nibble zero */
  float*    point;       /* f32 [N, 3, SDX_MAX_CONTACTS]   env frame */
  float*    normal;      /* f32 [N, 3, SDX_MAX_CONTACTS]   unit; the direction in which the normal impulse pushes side a */
  float*    force;       /* f32 [N, 3, SDX_MAX_CONTACTS]   on side a (side b receives the negative), env axes: impulse of the last substep / h */
  float*    separation;  /* f32 [N, SDX_MAX_CONTACTS]      the narrowphase's separation (negative: penetration) */
} sdx_contact_report;
int sdx_set_contact_report(sdx_handle h, const sdx_contact_report* report, void* stream);

/* Per-body contact wrenches and sensor / filter force matrices from a report (acquire_net_contact_force_tensor for all SDX_BODIES rows
 * plus the torque a force sensor would feel; IsaacLab's ContactSensor.force_matrix_w): one launch on `stream`, part of no step.  It reads
 * the report's count / body / point / force (count[e] clamped to [0, SDX_MAX_CONTACTS]; columns beyond it are never touched and may hold
 * anything) and the positions of the CURRENT SDX_T_RB.
 *   net_dev   f32 [N, SDX_BODIES, 6] or NULL: per body row the sum of the contact forces on it (side a +force, side b -force), then the
 *             sum of (point - x) x force about the position x of its SDX_T_RB row.  Rows of bodies without contacts are +0.
 *   pair_dev  f32 [N, n_sensor, n_filter, 3] or NULL: the force on sensor body s from filter body f: +force where (a, b) = (s, f),
 *             -force where (a, b) = (f, s).  A filter row that no contact side can have matches nothing.
 * Deterministic: every sum runs over ascending contact index with a fixed combination tree, without float atomics; two calls on the same
 * report agree bit for bit.  SDX_ERR_INVALID with a message: report NULL or its count / body / point / force NULL; both outputs NULL;
 * pair_dev without pairs; n_sensor / n_filter outside 0..32; a sensor row outside [0, SDX_BODIES). */
typedef struct {
  int32_t n_sensor, n_filter;      /* 0..32 each */
  int32_t sensor_body[32];         /* rows of SDX_T_RB */
  int32_t filter_body[32];         /* rows of SDX_T_RB, or -1 = the static world */
} sdx_contact_pairs;
int sdx_contact_wrenches(sdx_handle h, const sdx_contact_report* report, float* net_dev, const sdx_contact_pairs* pairs, float* pair_dev,
                         void* stream);

/* View camera: depth, label and colour images of the listed envs from the current SDX_T_ROOT / SDX_T_RB, for
 * looking at the engine; no task's step launches it.  k_seg_camera's pinhole model: f = normalize(target - pos), r = normalize(f x up),
 * u = r x f, ray through pixel centre (row, col) d = f + r px + u py, row 0 on top; since d . f = 1 the depth of a hit is its distance
 * along the optical axis (metres, +inf where nothing is hit).  What is drawn: SDX_VIEW_BOUNDS = the boxes of the segmentation camera
 * (132 brick bounding boxes, the static bounding boxes, the robot boxes); SDX_VIEW_COLLISION = what k_physics collides (slab compounds,
 * the hollow target brick when seg_hollow, fixed bricks as bounding boxes, every static slot's boxes with slot static_var_slot showing
 * row static_var_row[env % 3], the robot boxes).  A box that strictly contains the ray origin is skipped.  Labels (i16): brick index + 1,
 * robot link l -> -1 - l, static slot s -> -100 - s, background 0.  rgb: class colour x (0.35 + 0.65 |n . d| / |d|), n the entering face.
 * env_ids_dev: device i32 [n], any subset / order / repeats (ids outside [0, N) leave their image untouched).  Outputs are caller-owned
 * device buffers [n, height, width] (rgb: [n, height, width, 3]); any may be NULL.  Stream-ordered, no host synchronisation, no state. */
typedef enum { SDX_VIEW_BOUNDS = 0, SDX_VIEW_COLLISION = 1 } sdx_view_geometry;
typedef struct {
  float pos[3], target[3], up[3];  /* env frame, or the frame of rigid body attach_body when attach_body >= 0 */
  int32_t attach_body;             /* -1, or a row of SDX_T_RB in [0, SDX_NLINK): the camera rides on that link */
  float hfov_deg;                  /* horizontal field of view; square pixels: vertical half extent = tan(hfov/2) * height / width */
  int32_t width, height;           /* 1..2048 each; need not be multiples of anything */
  int32_t geometry;                /* sdx_view_geometry */
} sdx_view_desc;
int sdx_render_view(sdx_handle h, const sdx_view_desc* view, const int32_t* env_ids_dev, int32_t n,
                    float* depth_out_dev, int16_t* label_out_dev, uint8_t* rgb_out_dev, void* stream);

/* ---- Sim snapshots: save, restore and clone the complete state of envs on the device, so that a run continues
 * from a restored or cloned state bit for bit (set_*_state_tensor_indexed / mj_copyData, for every buffer at once).
 * A snapshot is `rows` rows of device memory; an ENV ROW holds every per-env buffer that a later call reads before it writes: the
 * actor / DOF / body / contact / Jacobian states, targets, the stacked observation and state frames with their clamped copies, reward,
 * reset / progress / randomize counters, actions, the init pose, success and T-value bookkeeping, the camera rows (Search: the
 * segmentation image and the ten-frame T-value buffer too), the randomization rows SDX_T_DR_DOF / LINK / BRICK with the env's draw counter,
 * and the warm-start cache (the count, and the first `count` keys and impulses; a count outside [0, 1536] is clamped).  The GLOBAL part,
 * which only save_all / restore_all move: the step counter (it keys every reset draw and the ring keys), the double-buffered reset
 * statistics and SDX_T_CONS_SUCCESSES, SDX_T_DR_GRAVITY, SDX_T_DR_FRAME and gravity's draw counter.
 * NOT part of any snapshot: the logs (the harvest, pile and T-value rings with their counts and keys, SDX_T_CONTACT_STATS, SDX_T_DEBUG),
 * the launch-order hints of k_physics, and configuration (loaded piles, T-value weights, the randomization descriptor and whether it is
 * on), a pending external wrench, pending joint actuation (sdx_apply_dof_forces) and the caller-owned buffers of sdx_set_force_perturbation (the task's rb_forces and
 * random_force_prob: copy them beside the snapshot), and the contact report (sdx_set_contact_report: whether it is armed, and the caller's
 * buffers; the next physics launch rewrites them).  A restore_all rewinds the step counter: ring rows appended afterwards can REPEAT the keys of rows appended before the restore.
 * Env classes: a row may only be put into an env of the class it came from - env & 7 (the target brick), and additionally env % 3 for
 * InsertSim (the base plate and the insertion site); the RNG keys stay with the destination env.  Each row records its source env.
 * restore and clone never fault on a bad entry: they skip it and count it in sdx_state_stats - [0] env id or row index out of range
 * (save counts these too), [1] class mismatch, [2] restore of a row that was never saved.
 * Across handles: a snapshot remembers its layout (task kind, warm start on / off, observation width, varying base plate, bytes per row)
 * and may be saved from / restored into any simulator with the same layout; another layout is SDX_ERR_INVALID.  restore_all also needs the
 * same number of envs, and gives SDX_ERR_STATE when the snapshot's last save was not save_all.
 * create, destroy and stats block; the others are stream-ordered with no host synchronisation, allocation or blocking copy (they may be
 * captured); n == 0 is SDX_OK without a launch.  Id arrays are device i32 [n]. */
typedef struct sdx_state* sdx_state_handle;
int sdx_state_create(sdx_handle h, int32_t rows, sdx_state_handle* out);   /* blocking; rows >= 1 */
int sdx_state_destroy(sdx_state_handle s);                                 /* blocking */
/* env env_ids_dev[i] -> row rows_dev[i]; rows_dev NULL = row i.  Rows must be unique. */
int sdx_state_save(sdx_handle h, sdx_state_handle s, const int32_t* env_ids_dev, const int32_t* rows_dev, int32_t n, void* stream);
/* row rows_dev[i] -> env env_ids_dev[i]; rows_dev NULL = row i.  A row may be repeated (fan-out), envs must be unique. */
int sdx_state_restore(sdx_handle h, sdx_state_handle s, const int32_t* rows_dev, const int32_t* env_ids_dev, int32_t n, void* stream);
/* every env (row e = env e; needs rows >= N) plus the global part */
int sdx_state_save_all(sdx_handle h, sdx_state_handle s, void* stream);
int sdx_state_restore_all(sdx_handle h, sdx_state_handle s, void* stream);
/* env src[i] -> env dst[i] inside one simulator.  A source may be repeated (fan-out); destination envs must be unique and none of them
 * may also be a source. */
int sdx_state_clone(sdx_handle h, const int32_t* src_env_ids_dev, const int32_t* dst_env_ids_dev, int32_t n, void* stream);
int sdx_state_stats(sdx_handle h, int32_t out[3]);                         /* blocking; counters since sdx_create */

int sdx_num_envs(sdx_handle h);
const char* sdx_last_error(sdx_handle h);   /* never NULL; h may be NULL for create-time errors */

/* ======================================================================================= PPO */

typedef struct {
  int32_t num_actors;        /* N envs (TR:81-85 injects num_actors)                     */
  int32_t horizon;           /* 8    YG:49 */
  int32_t minibatch;         /* 4    YG:50 (must divide horizon*num_actors)              */
  int32_t mini_epochs;       /* 5    YG:51 */
  int32_t cv_minibatch;      /* 4    YG:75 */
  int32_t cv_mini_epochs;    /* 5    YG:76 */
  int32_t obs_dim;           /* 396 */
  int32_t state_dim;         /* 564 */
  int32_t act_dim;           /* 23  */
  int32_t units[3];          /* 1024, 512, 256   YG:23 */
  float gamma, tau;          /* 0.99, 0.95  YG:35-36 */
  float lr, cv_lr;           /* 3e-4 YG:38, 1e-3 YG:77 */
  float e_clip;              /* 0.1  YG:46 */
  float grad_norm;           /* 1.0  YG:42 */
  float critic_coef;         /* 1    YG:52 */
  float entropy_coef;        /* 0    YG:43 */
  float bounds_loss_coef;    /* 1e-3 YG:63 */
  float kl_threshold;        /* 0.02 YG:54 */
  int32_t clip_value;        /* 1    YG:47 */
  int32_t truncate_grads;    /* 1    YG:44 */
  int32_t normalize_advantage; /* 1  YG:34 */
  int32_t cv_normalize_input;  /* 1  YG:82 */
  int32_t adaptive_lr;       /* 1: lr_schedule adaptive, schedule_type legacy (YG:53, PS:306-312) */
  int32_t world_size;        /* data-parallel ranks; gradients are averaged by the CALLER (RCCL) between
                                sdxp_backward_* and sdxp_apply_* when world_size > 1 */
  int32_t obs_cols;          /* columns of the caller's observation rows if fewer than obs_dim (0 = obs_dim): the network input is
                                zero-padded to obs_dim, which must be a multiple of 4 (BlockAssemblyOrient: 186 -> 188) */
  int32_t mixed_precision;   /* rl_games' `mixed_precision` (App. C; False in YG): 1 = the trunk GEMMs of the large-minibatch update path
                                (minibatch_size > 8) run on bf16 MFMA with fp32 accumulation; weights, Adam state, activations in HBM, losses,
                                heads and the rollout stay fp32 (BASELINE.json configs[4]: "bf16 policy").  Ignored by the rank-MB paths */
} sdxp_config;

typedef enum {
  SDXP_T_AC_PARAMS = 0,      /* f32 [P_ac]   actor MLP | mu | logstd | critic MLP | value  (flat)   */
  SDXP_T_AC_GRADS = 1,       /* f32 [P_ac]   flat gradient: the buffer RCCL all-reduces             */
  SDXP_T_CV_PARAMS = 2,      /* f32 [P_cv]   central value MLP (flat)                               */
  SDXP_T_CV_GRADS = 3,       /* f32 [P_cv]                                                          */
  /* experience buffer, stored env-major [N,H,...] == swap_and_flatten01 order (PS:338-339) */
  SDXP_T_MB_OBS = 4,         /* f32 [N,H,obs]     experience_buffer 'obses'   PS:346                */
  SDXP_T_MB_STATES = 5,      /* f32 [N,H,state]   'states'                    PS:352                */
  SDXP_T_MB_ACTIONS = 6,     /* f32 [N,H,act]                                                       */
  SDXP_T_MB_MUS = 7,         /* f32 [N,H,act]     overwritten by update_mu_sigma (RC:1358)          */
  SDXP_T_MB_SIGMAS = 8,      /* f32 [N,H,act]                                                       */
  SDXP_T_MB_NEGLOGP = 9,     /* f32 [N,H]                                                           */
  SDXP_T_MB_VALUES = 10,     /* f32 [N,H]                                                           */
  SDXP_T_MB_REWARDS = 11,    /* f32 [N,H]                                                           */
  SDXP_T_MB_DONES = 12,      /* f32 [N,H]         dones stored BEFORE the step, PS:347              */
  SDXP_T_RETURNS = 13,       /* f32 [N*H]   env-major after swap_and_flatten01, PS:338-339          */
  SDXP_T_ADVANTAGES = 14,    /* f32 [N*H]   normalised, RC:1645-1651                                */
  SDXP_T_CV_RMS_MEAN = 15,   /* f64 [state] running mean of the central-value input normalisation   */
  SDXP_T_CV_RMS_VAR = 16,    /* f64 [state]                                                         */
  SDXP_T_STATS = 17,         /* raw control block (struct SdxpCtrl, csrc/sdxp_types.h) as f32 words  */
  SDXP_T_LAST_VALUES = 18,   /* f32 [N]                                                             */
  SDXP_T_AC_ADAM_M = 19, SDXP_T_AC_ADAM_V = 20, SDXP_T_CV_ADAM_M = 21, SDXP_T_CV_ADAM_V = 22,
  SDXP_T_DEBUG = 23,         /* i64 [64]    phase time stamps of the last HEAD / CTRL kernels (profiling aid)      */
  SDXP_T_ALL_GRADS = 24,     /* f32 [..]    one buffer over AC_GRADS | pad | CV_GRADS | pad | KL word | pad (multiples of 64): a
                              * multi-rank caller all-reduces THIS once per optimiser step and calls sdxp_apply(which, -INFINITY) */
  SDXP_T_FACTORS = 25,       /* f32 [F]     this rank's rank-MB factors of the current minibatch (sdxp_backward_factors)       */
  SDXP_T_FACTORS_ALL = 26,   /* f32 [world,F] all ranks' factors: the caller all-gathers SDXP_T_FACTORS into it              */
  SDXP_T_COUNT = 27
} sdxp_tensor_id;

typedef struct sdxp_agent* sdxp_handle;

/* A2CAgent.__init__ + network build (R1,R2): torch-default Linear init (kaiming_uniform a=sqrt5) drawn from a
 * counter RNG under `seed`, biases zero, logstd zero (YG:8-29, App. C).  Blocking.
 * Shapes accepted (SDX_ERR_INVALID with a message otherwise): obs_dim and state_dim multiples of 4 in [4, 1024] (the rollout's first
 * trunk layer normalises through 1 024-entry tables, its dataset copy moves a row as at most 256 16-byte pieces), units[0], units[1]
 * multiples of 4, units[2] == 256, act_dim <= 32, batch_size % minibatch == 0, equal minibatch / mini_epochs for both optimisers. */
int sdxp_create(const sdxp_config* cfg, int32_t device, uint64_t seed, sdxp_handle* out);
int sdxp_destroy(sdxp_handle h);
int sdxp_tensor(sdxp_handle h, int32_t id, void** dev_ptr, int64_t shape[4], int32_t* ndim, int32_t* dtype);
int64_t sdxp_param_count(sdxp_handle h, int32_t which /*0 actor-critic, 1 central value*/);

/* get_action_values (RC:1697-1723): actor forward, a = mu + sigma*eps (eps from the counter RNG, or from
 * eps_dev f32 [N,act] when non-NULL), neglogp (RC:2114-2126), central value on states; stores row t of the
 * experience buffer (PS:345-352): obs, states, actions, mus, sigmas, neglogp, values, dones_dev (the task's i64
 * reset_buf as returned by the PREVIOUS env step, PS:347; NULL = 0).
 * actions_out_dev f32 [N,act] receives the sampled (unclamped) actions. */
int sdxp_act(sdxp_handle h, int32_t t, const float* obs_dev, const float* states_dev, const int64_t* dones_dev,
             const float* eps_dev, float* actions_out_dev, void* stream);
/* post_step (PS:355-373): rewards row t (reward_shaper scale 1, YG:32-33) + episode statistics
 * (current_rewards/current_lengths, game_rewards/game_lengths) from the i64 dones returned by THIS env step. */
int sdxp_store_rewards(sdxp_handle h, int32_t t, const float* rew_dev, const int64_t* dones_after_dev, void* stream);
/* play_steps tail (PS:329-339) + prepare_dataset (RC:1639-1651): last_values = V(states), GAE (R5), returns,
 * flatten env-major, advantage normalisation with unbiased std (R6); updates the CV running mean/std. */
int sdxp_finish_rollout(sdxp_handle h, const float* last_states_dev, const int64_t* last_dones_dev, void* stream);
/* The three stages of sdxp_finish_rollout one by one, for callers that keep rl_games-style driver code (PS:329-343):
 * get_values (RC:1725-1745; the central value of `states`, f32 [N] out), discount_values (PS:331-336; raw advantages ->
 * SDXP_T_ADVANTAGES, returns -> SDXP_T_RETURNS, both env-major), prepare_dataset (RC:1645-1651; advantage normalisation in place). */
int sdxp_get_values(sdxp_handle h, const float* states_dev, float* values_out_dev, void* stream);
int sdxp_discount_values(sdxp_handle h, const float* last_values_dev, const int64_t* last_dones_dev, void* stream);
int sdxp_prepare_dataset(sdxp_handle h, void* stream);
/* train_central_value + the actor-critic minibatch loop of train_epoch (PS:294-326, RC:1339-1365): all
 * mini-epochs, contiguous unshuffled minibatches, loss R7, grad-norm clip, Adam, legacy adaptive LR after
 * every minibatch (R8).  Single-rank fast path: everything stays on the device. */
int sdxp_update(sdxp_handle h, void* stream);
/* Which implementation sdxp_update runs on this handle: 1 = persistent kernel (one launch per epoch, weights and Adam moments
 * resident in the VGPR files of 256 CUs; needs the shipped shapes, minibatch_size 4 and a 256-CU device), 0 = hipGraph of the
 * multi-kernel optimiser step (any minibatch_size in {2,4,8}; forced with SDXP_UPDATE_IMPL=graph), 2 = GEMM-shaped step for
 * minibatch_size > 8 (cfg/lego/ppo_continuous_insert.yaml: 4096): fp32-MFMA forward / data-gradient / weight-gradient GEMMs,
 * explicit flat gradients, clip_grad_norm_ + Adam (sdxp_bigmb.hip). */
int sdxp_update_impl(sdxp_handle h);
/* Waits for the update launched on `stream`.  SDX_OK, or SDX_ERR_STATE when the persistent kernel timed out (its 256 workgroups were
 * not co-resident): nothing was applied, the inputs it had touched are restored and the handle has switched to the hipGraph
 * path - call sdxp_update again to repeat the epoch.  Optional after the hipGraph path (always SDX_OK there). */
int sdxp_update_status(sdxp_handle h, void* stream);
/* Multi-rank path, one minibatch at a time so that the caller can all-reduce SDXP_T_*_GRADS in between:
 * which = 0 actor-critic, 1 central value; mb = minibatch index within the epoch. */
int sdxp_backward(sdxp_handle h, int32_t which, int32_t mb, void* stream);
/* Factor-exchange form of the multi-rank step (preferred: 194 KB all-gather instead of a 13.4 MB all-reduce per step):
 * sdxp_backward_factors(mb) -> all_gather(SDXP_T_FACTORS_ALL, SDXP_T_FACTORS) -> sdxp_grads_from_factors -> sdxp_apply(0, -INFINITY),
 * sdxp_apply(1).  The *_GRADS buffers then hold the same rank SUM an all-reduce would have produced. */
int sdxp_backward_factors(sdxp_handle h, int32_t mb, void* stream);
int sdxp_grads_from_factors(sdxp_handle h, void* stream);
/* = sdxp_grads_from_factors + sdxp_apply(0, -INFINITY) + sdxp_apply(1), fused into three launches */
int sdxp_apply_factors(sdxp_handle h, void* stream);
/* kl: the rank-averaged KL for the LR schedule; NaN = take SdxpCtrl.last_kl that the caller all-reduced (SUM) in place through
 * SDXP_T_STATS; -INFINITY = take the KL word of SDXP_T_ALL_GRADS that the caller all-reduced (SUM) with the gradients. */
int sdxp_apply(sdxp_handle h, int32_t which, float kl_allreduced_or_nan, void* stream);
/* Optimiser state kept in the device control block, for checkpoints (rl_games restores the same items: the Adam step counters of
 * optimizer.state_dict(), running_mean_std.count of the central value, last_lr; A2CBase.set_full_state_weights).  Both calls block.
 * sdxp_set_state also re-derives the bias-correction powers 0.9^t / 0.999^t. */
typedef struct {
  double rms_count;          /* RunningMeanStd.count of the central-value input normalisation (1.0 after create) */
  int32_t ac_t, cv_t;        /* Adam step counters of the actor-critic / central-value optimisers                 */
  float ac_lr, cv_lr;        /* current learning rates (ac_lr moves with the adaptive schedule, PS:306-312)       */
} sdxp_opt_state;
int sdxp_get_state(sdxp_handle h, sdxp_opt_state* out, void* stream);
int sdxp_set_state(sdxp_handle h, const sdxp_opt_state* in, void* stream);
const char* sdxp_last_error(sdxp_handle h);

/* ------------------------------------------------------------------------------------------------------------------------------
 * Transition-value trainer (policy_sequencing/transition_value_trainer.py:127-248 = TT): fits GraspInsertTValue
 * (terminal_value_function.py:30-46; parameter packing as sdx_set_tvalue_weights) to success / failure camera-frame quaternions.
 * The datasets are device arrays [n, 4] - e.g. the SDX_T_TV_SUCCESS / SDX_T_TV_FAILURE rings the task kernels fill at episode ends
 * (the reference writes them to HDF5 groups data/success_dataset, data/failure_dataset: GS:470-480,1404-1432, IS:1392-1410). */
typedef struct sdxtv_trainer* sdxtv_handle;
typedef enum {
  SDXTV_T_PARAMS = 0,    /* f32 [42562]  W1 b1 W2 b2 W3 b3 W4 b4, torch layout W[out][in]                      TT:181      */
  SDXTV_T_GRADS = 1,     /* f32 [42562]  gradient of the last sdxtv_step                                                    */
  SDXTV_T_ADAM_M = 2,    /* f32 [42562]                                                                         TT:187      */
  SDXTV_T_ADAM_V = 3,    /* f32 [42562]                                                                                     */
  SDXTV_T_BATCH = 4,     /* f32 [B, 4]   t_value_obs_buf: rows [0, B/2) success, [B/2, B) failure                TT:207,213-222 */
  SDXTV_T_LOSS = 5,      /* f32 [1]      BCEWithLogitsLoss of the last step                                     TT:228      */
  SDXTV_T_OUTPUT = 6,    /* f32 [B, 2]   predict_success_confident of the last step                             TT:225      */
  SDXTV_T_COUNT = 7
} sdxtv_tensor_id;
int sdxtv_create(int32_t batch /* 1024, TT:190 */, int32_t device, uint64_t seed, sdxtv_handle* out);
int sdxtv_destroy(sdxtv_handle h);
int sdxtv_tensor(sdxtv_handle h, int32_t id, void** dev_ptr, int64_t shape[4], int32_t* ndim, int32_t* dtype);
/* draw a batch (TT:211-222): B/2 random success rows and B/2 random failure rows, + U(-1,1) * 0.05, renormalised -> SDXTV_T_BATCH */
int sdxtv_sample(sdxtv_handle h, const float* succ_dev, int32_t n_succ, const float* fail_dev, int32_t n_fail, void* stream);
/* forward, BCEWithLogitsLoss against the one-hot [failure, success] labels, backward, Adam step (TT:225-231) on SDXTV_T_BATCH */
int sdxtv_step(sdxtv_handle h, float lr /* 1e-3 */, void* stream);
/* iters x (sdxtv_sample, sdxtv_step): train_rollout (TT:209-231) */
int sdxtv_train(sdxtv_handle h, const float* succ_dev, int32_t n_succ, const float* fail_dev, int32_t n_fail, int32_t iters, float lr,
                void* stream);
/* net(x) for n <= batch rows -> out_dev [n, 2] (validation pass TT:235-246) */
int sdxtv_predict(sdxtv_handle h, const float* x_dev, int32_t n, float* out_dev, void* stream);
const char* sdxtv_last_error(sdxtv_handle h);

#ifdef __cplusplus
}
#endif
#endif /* SEQDEX_H */
