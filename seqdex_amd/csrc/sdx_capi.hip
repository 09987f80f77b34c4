// sdx_capi.hip — host side of the sdx_* C ABI declared in include/seqdex.h (simulator + task seam): argument checks, the buffers
// (sdx_buffers.h) and the order of the launches.  It defines no __global__ or __device__ function of its own: the kernels live in
// sdx_task / sdx_physics / sdx_camera / sdx_randomize.hip behind the launchers of sdx_kernels.h, the snapshot copy kernel in sdx_state.h.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "sdx_buffers.h"
#include "sdx_const_build.h"
#include "sdx_kernels.h"
#include "sdx_state.h"

struct sdx_sim {
  int device = 0;
  SdxConst* d_const = nullptr;
  SdxConst h_const;
  SdxBuf buf;
  uint8_t* orient_mask = nullptr;   // device copy of the reset flags of an Orient reset event
  std::vector<void*> allocs;
  struct TensorInfo { void* ptr; int64_t shape[4]; int ndim; int dtype; } tinfo[SDX_T_COUNT];
  sdx_dr_desc dr{};           // the randomization in force (meaningful while buf.dr_on != nullptr)
  sdx_noise_attr noise_obs{}, noise_act{};   // sdx_set_noise: distribution SDX_DR_NONE = off (always off while randomization is off)
  // sdx_apply_rigid_body_forces: the wrench of the next physics launch (the caller's buffers; both nullptr: none pending)
  const float *ext_force = nullptr, *ext_torque = nullptr;
  int32_t ext_space = SDX_SPACE_ENV;
  // sdx_apply_dof_forces: the actuation torques and the drives that are off in the next physics launch (a slot of its own: neither
  // sdx_apply_rigid_body_forces nor the force-perturbation sampler touches it)
  const float* dof_force = nullptr;
  uint32_t dof_off = 0;
  // sdx_set_force_perturbation: on while fp_forces != nullptr; fp_factor = decay^(dt / decay_interval)
  sdx_force_perturb_attr fp{};
  float fp_factor = 1.0f;
  float *fp_forces = nullptr, *fp_prob = nullptr;
  sdx_contact_report report{};   // sdx_set_contact_report: armed while report.count != nullptr (the caller's buffers)
  float* act_pre = nullptr;   // [N,23] the clamped and noised actions of this step (scratch of k_noise -> k_pre_physics)
  SdxStateTab st_tab{};       // what an env's state is (sdx_state.h); d_st_tab: its device copy
  SdxStateTab* d_st_tab = nullptr;
  std::string err;
};

static thread_local std::string g_create_err = "";

// what the task kind decides about the buffers: the row width of obs / obs_c, and the length of the pile ring per brick-type group
static int task_obs_width(int task_kind) {
  switch (task_kind) {
    case SDX_TASK_ORIENT: case SDX_TASK_SEARCH: return 186;   // 62 x 3, only the first 62 are ever written (OR:191-207)
    case SDX_TASK_INSERT: return 75;                          // one frame (IS:172)
    default: return SDX_NUM_OBS;
  }
}
static int task_pile_slots(int task_kind) {   // Orient and Search harvest piles
  if (task_kind != SDX_TASK_ORIENT && task_kind != SDX_TASK_SEARCH) return 1;
  // SDX_PILE_SLOTS=10000: the reference's ring length (OR:1485; 549 MB of the 288 GB); default SDX_PILE_HARVEST_SLOTS
  const char* ps = getenv("SDX_PILE_SLOTS");
  const long v = ps ? atol(ps) : 0;
  return v >= 16 && v <= 10000 ? (int)v : SDX_PILE_HARVEST_SLOTS;
}

#define HIPCHK(h, call)                                                                              \
  do {                                                                                               \
    hipError_t _e = (call);                                                                          \
    if (_e != hipSuccess) {                                                                          \
      char _b[512];                                                                                  \
      snprintf(_b, sizeof(_b), "%s failed: %s (%s:%d)", #call, hipGetErrorString(_e), __FILE__, __LINE__); \
      if (h) (h)->err = _b; else g_create_err = _b;                                                  \
      return SDX_ERR_HIP;                                                                            \
    }                                                                                                \
  } while (0)

template <typename T>
static int dalloc(sdx_sim* h, T** p, size_t count) {
  void* q = nullptr;
  hipError_t e = hipMalloc(&q, count * sizeof(T));
  if (e != hipSuccess) { h->err = std::string("hipMalloc failed: ") + hipGetErrorString(e); return SDX_ERR_NOMEM; }
  e = hipMemset(q, 0, count * sizeof(T));
  if (e != hipSuccess) { h->err = std::string("hipMemset failed: ") + hipGetErrorString(e); return SDX_ERR_HIP; }
  h->allocs.push_back(q);
  *p = (T*)q;
  return SDX_OK;
}

static void set_tensor(sdx_sim* h, int id, void* p, int dtype, std::initializer_list<int64_t> shape) {
  auto& t = h->tinfo[id];
  t.ptr = p;
  t.dtype = dtype;
  t.ndim = (int)shape.size();
  int i = 0;
  for (auto s : shape) t.shape[i++] = s;
  for (; i < 4; ++i) t.shape[i] = 1;
}

// the actions k_pre_physics takes.  With action noise on: h->act_pre, already clamped and noised (flag 8), computed here - before this
// step's re-sampling, from the blocks and counters in force until now.  The caller's buffer is only read.
static const float* noise_actions(sdx_sim* h, const float* actions_dev, int* flags, hipStream_t st) {
  if (h->noise_act.distribution == SDX_DR_NONE) return actions_dev;
  sdxk_noise(h->d_const, &h->buf, &h->noise_act, actions_dev, h->act_pre, SDX_NDOF, 1, st);
  *flags |= 8;
  return h->act_pre;
}
// post_physics_step, then the observation noise of BaseTask.step (BT:149-150) on the policy's row
static void post_physics_step(sdx_sim* h, hipStream_t st) {
  sdxk_post_physics(h->d_const, &h->buf, 1, st);
  if (h->noise_obs.distribution != SDX_DR_NONE) sdxk_noise(h->d_const, &h->buf, &h->noise_obs, h->buf.obs, h->buf.obs_c, h->buf.obs_w, 0, st);
}

// the physics launch a pending external wrench and pending joint actuation apply to (sdx_simulate; sdx_step's own, not the settling launches of a reset event): the
// caller's pointers travel by value in that launch's copy of the buffer table, and the wrench is forgotten.  An armed contact report
// (sdx_set_contact_report) travels by value too, as an argument of its own, with every such launch until it is disarmed.
static void physics_step(sdx_sim* h, hipStream_t st) {
  if (!h->ext_force && !h->ext_torque && !h->dof_force && !h->dof_off) { sdxk_physics_report(h->d_const, &h->buf, &h->report, st); return; }
  SdxBuf b = h->buf;
  b.ext_force = h->ext_force; b.ext_torque = h->ext_torque; b.ext_space = h->ext_space;
  b.dof_force = h->dof_force; b.dof_off = h->dof_off;
  h->ext_force = h->ext_torque = h->dof_force = nullptr;
  h->dof_off = 0;
  sdxk_physics_report(h->d_const, &b, &h->report, st);
}
// the random pushes of this step (sdx_set_force_perturbation), before the step's resets clear the flags: the task's rb_forces become the
// pending wrench, replacing the caller's own
static void force_perturb_step(sdx_sim* h, hipStream_t st) {
  if (!h->fp_forces) return;
  sdxk_force_perturb(h->d_const, &h->buf, &h->fp, h->fp_factor, h->fp_forces, h->fp_prob, nullptr, SDX_FP_STEP, st);
  h->ext_force = h->fp_forces; h->ext_torque = nullptr; h->ext_space = SDX_SPACE_ENV;
}

// ---------------------------------------------------------------- the buffer table (sdx_buffers.h), walked three times with these names
#define BUF_TABLE_NAMES(h)                                                                                      \
  SdxBuf& B = (h)->buf;                                                                                         \
  const int64_t N = B.N, W = B.obs_w, P = B.pile_slots;                                                         \
  const bool search = (h)->h_const.sc.task_kind == SDX_TASK_SEARCH, warm = (h)->h_const.sc.warm_start > 0.0f;   \
  (void)N; (void)W; (void)P; (void)search; (void)warm

static int buffers_alloc(sdx_sim* h) {
  BUF_TABLE_NAMES(h);
  int rc = dalloc(h, &h->act_pre, (size_t)N * SDX_NDOF);
#define X(field, count, snap, n, tensor) if (rc == SDX_OK && (count) > 0) rc = dalloc(h, &B.field, (size_t)(count));
  SDX_BUFFERS(X)
#undef X
  return rc;
}

static void tensors_register(sdx_sim* h) {
  BUF_TABLE_NAMES(h);
#define TENSOR(id, dtype, ...) set_tensor(h, SDX_T_##id, p_, SDX_##dtype, {__VA_ARGS__});
#define NO_TENSOR
#define X(field, count, snap, n, tensor) { void* const p_ = B.field; (void)p_; tensor }
  SDX_BUFFERS(X)
#undef X
#undef NO_TENSOR
#undef TENSOR
  if (!search) {   // placeholders: the camera and the temporal buffer belong to Search
    set_tensor(h, SDX_T_SEG_IMAGE, B.seg_image, SDX_I16, {1, 1, 1});
    set_tensor(h, SDX_T_TVALUE_OBS, B.seg_pix, SDX_F32, {1, 1});
  }
  if (!warm) {     // placeholders: the impulse cache only exists with the warm start (k_physics<.., false> never reads it)
    set_tensor(h, SDX_T_WARM_KEYS, B.wkey, SDX_I32, {1});
    set_tensor(h, SDX_T_WARM_LAMBDA, B.wlam, SDX_F32, {1});
  }
}

// sim snapshots (include/seqdex.h sdx_state_*): the segment table = the ENV / ENV_WARM rows in table order, the
// global part = the GLOBAL rows and the one tail element dr_draw[N]
static int state_table_build(sdx_sim* h) {
  BUF_TABLE_NAMES(h);
  SdxStateTab& S = h->st_tab;
  const sdx_scene_desc& sc = h->h_const.sc;
  S.N = B.N;
  S.var3 = (sc.static_var_slot >= 0 || sc.task_kind == SDX_TASK_INSERT) ? 1 : 0;   // the base plate / the insertion site depend on env % 3
  S.row_bytes = 16;   // the row header: source env, warm count, SDX_ST_MAGIC, 0
  S.wcount = B.wcount;
  bool ok = true;
  int ng = 0;
  auto row = [&](SdxSnap snap, char* p, size_t sz, size_t count, size_t n) {   // sz: bytes per element
    if (snap == SDX_SNAP_ENV && n > 0) ok = ok && sdx_state_add(&S, p, n * sz, n * sz, 0);
    if (snap == SDX_SNAP_ENV_WARM) for (size_t r = 0; r < n / SDX_MAXC; ++r) ok = ok && sdx_state_add(&S, p + r * SDX_MAXC * sz, n * sz, SDX_MAXC * sz, 1);
    if (snap == SDX_SNAP_GLOBAL) { if (ng < SDX_ST_NGLOB) { S.glob[ng] = p; S.glob_bytes[ng] = (uint32_t)(count * sz); } ++ng; }
  };
#define X(field, count, snap, n, tensor) row(SDX_SNAP_##snap, (char*)B.field, sizeof(*B.field), (size_t)(count), (size_t)(n));
  SDX_BUFFERS(X)
#undef X
  row(SDX_SNAP_GLOBAL, (char*)(B.dr_draw + N), sizeof(*B.dr_draw), 1, 0);
  if (!ok || ng != SDX_ST_NGLOB) { h->err = "sdx_create: state segment table (a buffer is missing, misaligned or not a multiple of 4 bytes per env)"; return SDX_ERR_INVALID; }
  S.nunits = (int32_t)(S.row_bytes / 16);
  std::vector<uint8_t> us((size_t)S.nunits, 255);
  for (int i = 0; i < S.nseg; ++i) {
    const uint32_t slot = ((S.seg[i].bytes + 15) & ~15u) + 16;
    for (uint32_t u = S.seg[i].off / 16; u < (S.seg[i].off + slot) / 16; ++u) us[u] = (uint8_t)i;
  }
  uint8_t* d_us = nullptr;
  int rc;
  if ((rc = dalloc(h, &d_us, us.size())) != SDX_OK) return rc;
  if ((rc = dalloc(h, &S.stats, 4)) != SDX_OK) return rc;
  if ((rc = dalloc(h, &h->d_st_tab, 1)) != SDX_OK) return rc;
  S.unit_seg = d_us;
  HIPCHK(h, hipMemcpy(d_us, us.data(), us.size(), hipMemcpyHostToDevice));
  HIPCHK(h, hipMemcpy(h->d_st_tab, &S, sizeof(S), hipMemcpyHostToDevice));
  return SDX_OK;
}

struct sdx_state {
  int device = 0;
  int32_t sig[5] = {0, 0, 0, 0, 0};   // layout signature: task kind, warm start on, obs_w, var3, row bytes
  int32_t rows = 0;
  int32_t full_n = -1;                // N of the simulator whose save_all was the last save, -1: the last save was not a save_all
  char* d_rows = nullptr;
  char* d_glob = nullptr;             // [SDX_ST_NGLOB x 16 bytes]
};
static void state_sig(const sdx_sim* h, int32_t sig[5]) {
  sig[0] = h->h_const.sc.task_kind; sig[1] = h->h_const.sc.warm_start > 0.0f; sig[2] = h->buf.obs_w; sig[3] = h->st_tab.var3;
  sig[4] = (int32_t)h->st_tab.row_bytes;
}
static bool state_sig_ok(sdx_sim* h, const sdx_state* s, const char* what) {
  int32_t sig[5];
  state_sig(h, sig);
  if (memcmp(sig, s->sig, sizeof(sig)) == 0) return true;
  char b[320];
  snprintf(b, sizeof(b), "%s: the snapshot's layout (task kind %d, warm start %d, obs_w %d, varying base plate %d, %d bytes per row) is not this "
           "simulator's (%d, %d, %d, %d, %d)", what, s->sig[0], s->sig[1], s->sig[2], s->sig[3], s->sig[4], sig[0], sig[1], sig[2], sig[3], sig[4]);
  h->err = b;
  return false;
}
static int check_launch(sdx_handle h, const char* what);

extern "C" int sdx_state_create(sdx_handle h, int32_t rows, sdx_state_handle* out) {
  if (!h) return SDX_ERR_INVALID;
  if (!out || rows < 1) { h->err = "sdx_state_create: rows >= 1 and a non-NULL out"; return SDX_ERR_INVALID; }
  HIPCHK(h, hipSetDevice(h->device));
  sdx_state* s = new sdx_state();
  s->device = h->device;
  s->rows = rows;
  state_sig(h, s->sig);
  const size_t bytes = (size_t)rows * h->st_tab.row_bytes;
  hipError_t e = hipMalloc((void**)&s->d_rows, bytes);
  if (e == hipSuccess) e = hipMalloc((void**)&s->d_glob, SDX_ST_NGLOB * 16);
  if (e != hipSuccess) {
    if (s->d_rows) (void)hipFree(s->d_rows);
    delete s;
    h->err = std::string("sdx_state_create: hipMalloc failed: ") + hipGetErrorString(e);
    return SDX_ERR_NOMEM;
  }
  e = hipMemset(s->d_rows, 0, bytes);   // no row has been saved: header word 2 != SDX_ST_MAGIC
  if (e == hipSuccess) e = hipMemset(s->d_glob, 0, SDX_ST_NGLOB * 16);
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e != hipSuccess) {
    (void)hipFree(s->d_rows); (void)hipFree(s->d_glob);
    delete s;
    h->err = std::string("sdx_state_create: hipMemset failed: ") + hipGetErrorString(e);
    return SDX_ERR_HIP;
  }
  *out = s;
  return SDX_OK;
}
extern "C" int sdx_state_destroy(sdx_state_handle s) {
  if (!s) return SDX_ERR_INVALID;
  (void)hipSetDevice(s->device);
  (void)hipDeviceSynchronize();
  (void)hipFree(s->d_rows);
  (void)hipFree(s->d_glob);
  delete s;
  return SDX_OK;
}
extern "C" int sdx_state_save(sdx_handle h, sdx_state_handle s, const int32_t* env_ids_dev, const int32_t* rows_dev, int32_t n, void* stream) {
  if (!h) return SDX_ERR_INVALID;
  if (!s || n < 0 || (n > 0 && !env_ids_dev)) { h->err = "sdx_state_save: snapshot / env_ids NULL or n < 0"; return SDX_ERR_INVALID; }
  if (!state_sig_ok(h, s, "sdx_state_save")) return SDX_ERR_INVALID;
  if (n == 0) return SDX_OK;
  s->full_n = -1;
  sdx_state_launch(h->d_st_tab, SDX_ST_SAVE, s->d_rows, s->rows, s->d_glob, env_ids_dev, rows_dev, n, 0, (hipStream_t)stream);
  return check_launch(h, "sdx_state_save");
}
extern "C" int sdx_state_restore(sdx_handle h, sdx_state_handle s, const int32_t* rows_dev, const int32_t* env_ids_dev, int32_t n, void* stream) {
  if (!h) return SDX_ERR_INVALID;
  if (!s || n < 0 || (n > 0 && !env_ids_dev)) { h->err = "sdx_state_restore: snapshot / env_ids NULL or n < 0"; return SDX_ERR_INVALID; }
  if (!state_sig_ok(h, s, "sdx_state_restore")) return SDX_ERR_INVALID;
  if (n == 0) return SDX_OK;
  sdx_state_launch(h->d_st_tab, SDX_ST_RESTORE, s->d_rows, s->rows, s->d_glob, rows_dev, env_ids_dev, n, 0, (hipStream_t)stream);
  return check_launch(h, "sdx_state_restore");
}
extern "C" int sdx_state_save_all(sdx_handle h, sdx_state_handle s, void* stream) {
  if (!h) return SDX_ERR_INVALID;
  if (!s) { h->err = "sdx_state_save_all: snapshot NULL"; return SDX_ERR_INVALID; }
  if (!state_sig_ok(h, s, "sdx_state_save_all")) return SDX_ERR_INVALID;
  if (s->rows < h->buf.N) { h->err = "sdx_state_save_all: the snapshot has fewer rows than the simulator has envs"; return SDX_ERR_INVALID; }
  s->full_n = h->buf.N;
  sdx_state_launch(h->d_st_tab, SDX_ST_SAVE, s->d_rows, s->rows, s->d_glob, nullptr, nullptr, h->buf.N, 1, (hipStream_t)stream);
  return check_launch(h, "sdx_state_save_all");
}
extern "C" int sdx_state_restore_all(sdx_handle h, sdx_state_handle s, void* stream) {
  if (!h) return SDX_ERR_INVALID;
  if (!s) { h->err = "sdx_state_restore_all: snapshot NULL"; return SDX_ERR_INVALID; }
  if (!state_sig_ok(h, s, "sdx_state_restore_all")) return SDX_ERR_INVALID;
  if (s->full_n < 0) { h->err = "sdx_state_restore_all: the snapshot's last save was not sdx_state_save_all (it holds no global state)"; return SDX_ERR_STATE; }
  if (s->full_n != h->buf.N) { h->err = "sdx_state_restore_all: the snapshot was taken from a simulator with another number of envs"; return SDX_ERR_INVALID; }
  sdx_state_launch(h->d_st_tab, SDX_ST_RESTORE, s->d_rows, s->rows, s->d_glob, nullptr, nullptr, h->buf.N, 1, (hipStream_t)stream);
  return check_launch(h, "sdx_state_restore_all");
}
extern "C" int sdx_state_clone(sdx_handle h, const int32_t* src_env_ids_dev, const int32_t* dst_env_ids_dev, int32_t n, void* stream) {
  if (!h) return SDX_ERR_INVALID;
  if (n < 0 || (n > 0 && (!src_env_ids_dev || !dst_env_ids_dev))) { h->err = "sdx_state_clone: env ids NULL or n < 0"; return SDX_ERR_INVALID; }
  if (n == 0) return SDX_OK;
  sdx_state_launch(h->d_st_tab, SDX_ST_CLONE, nullptr, 0, nullptr, src_env_ids_dev, dst_env_ids_dev, n, 0, (hipStream_t)stream);
  return check_launch(h, "sdx_state_clone");
}
extern "C" int sdx_state_stats(sdx_handle h, int32_t out[3]) {
  if (!h) return SDX_ERR_INVALID;
  if (!out) { h->err = "sdx_state_stats: out NULL"; return SDX_ERR_INVALID; }
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipDeviceSynchronize());
  HIPCHK(h, hipMemcpy(out, h->st_tab.stats, 3 * sizeof(int32_t), hipMemcpyDeviceToHost));
  return SDX_OK;
}

// the shape tables k_physics indexes without further checks, and the warm start's ramp: the error text, or nullptr
static const char* scene_check(const sdx_scene_desc* scene) {
  const int ns = scene->n_static, nr = scene->n_rbox;
  bool ok = ns >= 0 && ns <= SDX_MAX_STATIC && nr >= 0 && nr <= SDX_MAX_RBOX && scene->n_static_sub >= 0 && scene->n_static_sub <= SDX_MAX_STATIC_SUB;
  // candidate body pairs of the broadphase: <= 16 per lane of the 512-thread workgroup (the pair rank's 13 bits)
  ok = ok && SDX_NFREE * SDX_MAX_STATIC + SDX_NFREE * (SDX_NFREE - 1) / 2 + nr * (SDX_NFREE + SDX_MAX_STATIC) <= 16 * 512;   // (the enumeration runs over all static slots)
  for (int t = 0; ok && t < SDX_NBRICK_TYPES; ++t)
    ok = scene->brick_nsub[t] >= 1 && scene->brick_nsub[t] <= SDX_MAX_SUB && scene->hollow_nsub[t] >= 0 && scene->hollow_nsub[t] <= SDX_MAX_SUB_HOLLOW &&
         (!scene->seg_hollow || scene->hollow_nsub[t] >= 1);
  for (int r = 0; ok && r < SDX_MAX_STATIC_TAB; ++r) {
    const bool used = r < ns || (scene->static_var_slot >= 0 && (r == scene->static_var_row[0] || r == scene->static_var_row[1] || r == scene->static_var_row[2]));
    if (used) ok = scene->static_sub_n[r] >= 1 && scene->static_sub_n[r] <= 63 && scene->static_sub_first[r] >= 0 &&
                   scene->static_sub_first[r] + scene->static_sub_n[r] <= scene->n_static_sub;
  }
  if (scene->static_var_slot >= ns) ok = false;
  for (int k = 0; ok && scene->static_var_slot >= 0 && k < 3; ++k) ok = scene->static_var_row[k] >= 0 && scene->static_var_row[k] < SDX_MAX_STATIC_TAB;
  if (!ok) return "sdx_create: scene shape tables out of range (n_static, n_rbox, brick / static compounds)";
  // the warm start's contact age is a 4-bit saturating counter in the cache key (k_physics solve()): a ramp longer than 16 solves would never end
  if (!(scene->warm_age >= 0.0f && scene->warm_age <= 16.0f)) return "sdx_create: warm_age must lie in [0, 16] (the contact age saturates at 16 solves)";
  return nullptr;
}

// initial actor states (what create_actor's start poses give, GS:897-1000), the default saved piles, the launch order and the reset flags
static int initial_state_upload(sdx_sim* h, const sdx_scene_desc* scene) {
  SdxBuf& B = h->buf;
  const int N = B.N;
  std::vector<float> root((size_t)N * SDX_ACTORS * 13, 0.0f), rbv((size_t)N * SDX_BODIES * 13, 0.0f);
  std::vector<float> pile0((size_t)SDX_NBRICK * 13, 0.0f);
  for (int i = 0; i < SDX_NBRICK; ++i) {
    float* s = &pile0[(size_t)i * 13];
    if (i < SDX_NFREE) {
      memcpy(s, scene->free_spawn_pos[i], 12);
      memcpy(s + 3, scene->free_spawn_quat, 16);
    } else {
      memcpy(s, scene->fixed_brick_pos[i - SDX_NFREE], 12);
      s[6] = 1.0f;
    }
  }
  for (int e = 0; e < N; ++e) {
    float* r = &root[(size_t)e * SDX_ACTORS * 13];
    for (int a = 0; a < SDX_ACTORS; ++a) r[a * 13 + 6] = 1.0f;
    memcpy(r, scene->base_pos, 12);
    memcpy(r + 3, scene->base_quat, 16);
    memcpy(r + 13, scene->object_init_state, 13 * 4);
    memcpy(r + 26, scene->goal_reset_pos, 12);
    for (int s = 0; s < 6; ++s) memcpy(r + (3 + s) * 13, scene->static_actor_pos[s], 12);
    memcpy(r + SDX_ACTOR_BRICK0 * 13, pile0.data(), pile0.size() * 4);
    memcpy(r + SDX_ACTOR_PLATE * 13, scene->base_plate_pos, 12);
    float* b = &rbv[(size_t)e * SDX_BODIES * 13];
    for (int a = 1; a < SDX_ACTORS; ++a) memcpy(b + (SDX_NLINK + a - 1) * 13, r + a * 13, 13 * 4);
  }
  HIPCHK(h, hipMemcpy(B.root, root.data(), root.size() * 4, hipMemcpyHostToDevice));
  HIPCHK(h, hipMemcpy(B.rb, rbv.data(), rbv.size() * 4, hipMemcpyHostToDevice));
  std::vector<float> p8;   // default saved piles: K=1, the spawn lattice for every type group (replaced by sdx_load_initial_states)
  for (int t = 0; t < 8; ++t) p8.insert(p8.end(), pile0.begin(), pile0.end());
  HIPCHK(h, hipMemcpy(B.piles, p8.data(), p8.size() * 4, hipMemcpyHostToDevice));
  std::vector<int32_t> iota((size_t)N);   // k_physics launch order: env order until the first step has costs
  for (int i = 0; i < N; ++i) iota[i] = i;
  HIPCHK(h, hipMemcpy(B.order, iota.data(), (size_t)N * sizeof(int32_t), hipMemcpyHostToDevice));
  std::vector<int64_t> ones(N, 1);  // reset_buf = ONES: every env resets on the first step (BT:63)
  HIPCHK(h, hipMemcpy(B.reset, ones.data(), (size_t)N * 8, hipMemcpyHostToDevice));
  return SDX_OK;
}

// everything of sdx_create that can fail with a live handle: the caller destroys it
static int create_on_device(sdx_sim* h, const sdx_scene_desc* scene, int32_t num_envs, uint64_t seed) {
  HIPCHK(h, hipSetDevice(h->device));
  sdx_build_const(scene, &h->h_const);
  int rc;
  if ((rc = dalloc(h, &h->d_const, 1)) != SDX_OK) return rc;
  HIPCHK(h, hipMemcpy(h->d_const, &h->h_const, sizeof(h->h_const), hipMemcpyHostToDevice));
  SdxBuf& B = h->buf;
  memset(&B, 0, sizeof(B));   // dr_on = nullptr: randomization is off
  B.N = num_envs;
  B.task_kind = scene->task_kind;
  B.orient_gate = scene->orient_tvalue_gate;
  B.obs_w = task_obs_width(scene->task_kind);
  B.pile_slots = task_pile_slots(scene->task_kind);
  B.K = 1;
  B.seed = seed;
  { const char* de = getenv("SDX_DEBUG_ENV"); B.dbg_env = de ? atoi(de) : 0; }
  if ((rc = buffers_alloc(h)) != SDX_OK) return rc;
  tensors_register(h);
  if ((rc = initial_state_upload(h, scene)) != SDX_OK) return rc;
  if ((rc = state_table_build(h)) != SDX_OK) return rc;
  sdxk_dr_defaults(h->d_const, &B, 0);      // the randomization rows hold the scene's values
  sdxk_kinematics(h->d_const, &B, 0);       // first refresh (GS:243-246)
  HIPCHK(h, hipDeviceSynchronize());
  return SDX_OK;
}

extern "C" int sdx_create(const sdx_scene_desc* scene, int32_t num_envs, int32_t device, uint64_t seed, sdx_handle* out) {
  if (!scene || !out || num_envs <= 0) { g_create_err = "sdx_create: bad argument"; return SDX_ERR_INVALID; }
  if (scene->abi_version != SDX_ABI_VERSION) { g_create_err = "sdx_create: scene.abi_version mismatch"; return SDX_ERR_INVALID; }
  if (const char* why = scene_check(scene)) { g_create_err = why; return SDX_ERR_INVALID; }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { g_create_err = "sdx_create: no HIP device visible; libseqdex_hip has no CPU fallback"; return SDX_ERR_NO_DEVICE; }
  if (device < 0 || device >= ndev) { g_create_err = "sdx_create: bad device index"; return SDX_ERR_INVALID; }
  sdx_sim* h = new sdx_sim();
  h->device = device;
  const int rc = create_on_device(h, scene, num_envs, seed);
  if (rc != SDX_OK) { g_create_err = h->err; sdx_destroy(h); return rc; }
  *out = h;
  return SDX_OK;
}

extern "C" int sdx_destroy(sdx_handle h) {
  if (!h) return SDX_ERR_INVALID;
  (void)hipSetDevice(h->device);
  (void)hipDeviceSynchronize();
  for (void* p : h->allocs) (void)hipFree(p);
  delete h;
  return SDX_OK;
}

extern "C" int sdx_tensor(sdx_handle h, int32_t id, void** dev_ptr, int64_t shape[4], int32_t* ndim, int32_t* dtype) {
  if (!h) return SDX_ERR_INVALID;
  if (id < 0 || id >= SDX_T_COUNT || !dev_ptr || !shape || !ndim || !dtype) { h->err = "sdx_tensor: bad argument"; return SDX_ERR_INVALID; }
  const auto& t = h->tinfo[id];
  *dev_ptr = t.ptr;
  for (int i = 0; i < 4; ++i) shape[i] = t.shape[i];
  *ndim = t.ndim;
  *dtype = t.dtype;
  return SDX_OK;
}

extern "C" int sdx_load_initial_states(sdx_handle h, const float* piles_host, int32_t K) {
  if (!h) return SDX_ERR_INVALID;
  if (!piles_host || K <= 0) { h->err = "sdx_load_initial_states: bad argument"; return SDX_ERR_INVALID; }
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipDeviceSynchronize());
  float* p = nullptr;
  const size_t count = (size_t)8 * K * SDX_NBRICK * 13;
  int rc = dalloc(h, &p, count);
  if (rc != SDX_OK) return rc;
  HIPCHK(h, hipMemcpy(p, piles_host, count * 4, hipMemcpyHostToDevice));
  h->buf.piles = p;  // the previous table stays allocated until destroy (cheap, avoids a free under a live stream)
  h->buf.K = K;
  return SDX_OK;
}

extern "C" int sdx_set_tvalue_weights(sdx_handle h, const float* w, int32_t n) {
  if (!h) return SDX_ERR_INVALID;
  if (!w || n != SDX_TV_PARAMS) { h->err = "sdx_set_tvalue_weights: expected SDX_TV_PARAMS floats"; return SDX_ERR_INVALID; }
  // host layout (torch): W[out][in] then b; device layout: W^T[in][out] then b
  std::vector<float> t(SDX_TV_PARAMS);
  const int dims[5] = {4, 256, 128, 64, 2};
  size_t o = 0;
  for (int l = 0; l < 4; ++l) {
    const int in = dims[l], out = dims[l + 1];
    for (int i = 0; i < in; ++i)
      for (int j = 0; j < out; ++j) t[o + (size_t)i * out + j] = w[o + (size_t)j * in + i];
    o += (size_t)in * out;
    for (int j = 0; j < out; ++j) t[o + j] = w[o + j];
    o += out;
  }
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipMemcpy(h->buf.tv_w, t.data(), t.size() * 4, hipMemcpyHostToDevice));
  return SDX_OK;
}

extern "C" int sdx_set_retri_tvalue_weights(sdx_handle h, const float* w, int32_t n) {
  if (!h) return SDX_ERR_INVALID;
  if (h->h_const.sc.task_kind != SDX_TASK_SEARCH) { h->err = "sdx_set_retri_tvalue_weights: RetriGraspTValue belongs to BlockAssemblySearch (task_kind 3)"; return SDX_ERR_STATE; }
  if (!w || n != SDX_RETRI_TV_PARAMS) { h->err = "sdx_set_retri_tvalue_weights: expected SDX_RETRI_TV_PARAMS floats"; return SDX_ERR_INVALID; }
  // device layout = host layout with the rows of W1 padded from 650 to 652 columns (16-byte rows for the float4 loads of the GEMM)
  std::vector<float> t((size_t)1024 * 652 + (n - (size_t)1024 * 650), 0.0f);
  for (int r = 0; r < 1024; ++r) memcpy(&t[(size_t)r * 652], w + (size_t)r * 650, 650 * sizeof(float));
  memcpy(&t[(size_t)1024 * 652], w + (size_t)1024 * 650, (n - (size_t)1024 * 650) * sizeof(float));
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipDeviceSynchronize());
  HIPCHK(h, hipMemcpy(h->buf.tvt_w, t.data(), t.size() * 4, hipMemcpyHostToDevice));
  return SDX_OK;
}

static int check_launch(sdx_handle h, const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) { h->err = std::string(what) + ": " + hipGetErrorString(e); return SDX_ERR_HIP; }
  return SDX_OK;
}

static bool dr_attr_ok(const sdx_dr_attr& a) {
  if (a.distribution == SDX_DR_NONE) return true;
  if (a.distribution < SDX_DR_NONE || a.distribution > SDX_DR_LOGUNIFORM) return false;
  if (a.operation != SDX_DR_ADDITIVE && a.operation != SDX_DR_SCALING) return false;
  if (a.schedule < SDX_DR_SCHED_NONE || a.schedule > SDX_DR_SCHED_CONSTANT || (a.schedule != SDX_DR_SCHED_NONE && a.schedule_steps <= 0)) return false;
  if (a.num_buckets < 0 || !std::isfinite(a.range[0]) || !std::isfinite(a.range[1])) return false;
  if (a.distribution == SDX_DR_LOGUNIFORM && !(a.range[0] > 0.0f && a.range[1] > 0.0f)) return false;
  if (a.distribution == SDX_DR_GAUSSIAN && a.range[1] < 0.0f) return false;   // sigma (its square root makes the bucket grid)
  if (a.distribution != SDX_DR_GAUSSIAN && a.range[0] > a.range[1]) return false;
  return true;
}
extern "C" int sdx_set_randomization(sdx_handle h, const sdx_dr_desc* desc, void* stream) {
  if (!h) return SDX_ERR_INVALID;
  hipStream_t st = (hipStream_t)stream;
  if (!desc) {
    h->buf.dr_on = nullptr;
    h->noise_obs = sdx_noise_attr{};   // the noise lives on this path's counters: off with it
    h->noise_act = sdx_noise_attr{};
    sdxk_dr_defaults(h->d_const, &h->buf, st);
    return check_launch(h, "sdx_set_randomization");
  }
  const sdx_dr_attr* at[9] = {&desc->gravity, &desc->dof_stiffness, &desc->dof_damping, &desc->dof_lower, &desc->dof_upper,
                              &desc->link_mass, &desc->link_friction, &desc->brick_mass, &desc->brick_friction};
  bool ok = desc->frequency >= 1;
  for (int i = 0; i < 9; ++i) ok = ok && dr_attr_ok(*at[i]);
  if (!ok) { h->err = "sdx_set_randomization: bad desc (frequency >= 1, known distribution / operation / schedule, schedule_steps > 0, finite ranges)"; return SDX_ERR_INVALID; }
  h->dr = *desc;
  h->buf.dr_on = h->buf.dr_draw;
  sdxk_dr_sample(h->d_const, &h->buf, &h->dr, 1, nullptr, st);
  return check_launch(h, "sdx_set_randomization");
}

// what sdx_set_noise checks of one block; *why names the first thing that is wrong
static bool noise_attr_ok(const sdx_noise_attr& a, const char** why) {
  if (a.distribution == SDX_DR_NONE) return true;
  *why = "distribution must be SDX_DR_NONE, SDX_DR_GAUSSIAN or SDX_DR_UNIFORM";
  if (a.distribution != SDX_DR_GAUSSIAN && a.distribution != SDX_DR_UNIFORM) return false;
  *why = "operation must be SDX_DR_ADDITIVE or SDX_DR_SCALING";
  if (a.operation != SDX_DR_ADDITIVE && a.operation != SDX_DR_SCALING) return false;
  *why = "unknown schedule, or a schedule without schedule_steps > 0";
  if (a.schedule < SDX_DR_SCHED_NONE || a.schedule > SDX_DR_SCHED_CONSTANT || (a.schedule != SDX_DR_SCHED_NONE && a.schedule_steps <= 0)) return false;
  *why = "range and range_correlated must be finite";
  if (!std::isfinite(a.range[0]) || !std::isfinite(a.range[1]) || !std::isfinite(a.range_correlated[0]) || !std::isfinite(a.range_correlated[1])) return false;
  *why = "a gaussian's sigma must be >= 0 (range[1], range_correlated[1])";
  if (a.distribution == SDX_DR_GAUSSIAN && (a.range[1] < 0.0f || a.range_correlated[1] < 0.0f)) return false;
  *why = "uniform needs lo <= hi (range, range_correlated)";
  if (a.distribution == SDX_DR_UNIFORM && (a.range[0] > a.range[1] || a.range_correlated[0] > a.range_correlated[1])) return false;
  return true;
}
extern "C" int sdx_set_noise(sdx_handle h, const sdx_noise_attr* observations, const sdx_noise_attr* actions, void* stream) {
  if (!h) return SDX_ERR_INVALID;
  (void)stream;   // the blocks travel with the launches of the calls that follow: nothing to enqueue here
  const sdx_noise_attr off{};
  const sdx_noise_attr &o = observations ? *observations : off, &a = actions ? *actions : off;
  const char* why = "";
  if (!noise_attr_ok(o, &why)) { h->err = std::string("sdx_set_noise: observations: ") + why; return SDX_ERR_INVALID; }
  if (!noise_attr_ok(a, &why)) { h->err = std::string("sdx_set_noise: actions: ") + why; return SDX_ERR_INVALID; }
  if (!h->buf.dr_on) {
    h->err = "sdx_set_noise: randomization is off (call sdx_set_randomization first, an all-SDX_DR_NONE desc is enough): the noise follows its frame and refresh counters";
    return SDX_ERR_STATE;
  }
  h->noise_obs = o;
  h->noise_act = a;
  return SDX_OK;
}

extern "C" int sdx_apply_rigid_body_forces(sdx_handle h, const float* forces_dev, const float* torques_dev, int32_t space, void* stream) {
  if (!h) return SDX_ERR_INVALID;
  (void)stream;   // nothing to enqueue: the pointers travel with the next physics launch
  if (space != SDX_SPACE_ENV && space != SDX_SPACE_LOCAL) { h->err = "sdx_apply_rigid_body_forces: space must be SDX_SPACE_ENV or SDX_SPACE_LOCAL"; return SDX_ERR_INVALID; }
  h->ext_force = forces_dev;
  h->ext_torque = torques_dev;
  h->ext_space = space;
  return SDX_OK;
}
extern "C" int sdx_apply_dof_forces(sdx_handle h, const float* dof_forces_dev, uint32_t drive_off_mask, void* stream) {
  if (!h) return SDX_ERR_INVALID;
  (void)stream;   // nothing to enqueue: pointer and mask travel with the next physics launch
  if (drive_off_mask >> SDX_NDOF) { h->err = "sdx_apply_dof_forces: drive_off_mask has a bit beyond DOF 22"; return SDX_ERR_INVALID; }
  h->dof_force = dof_forces_dev;
  h->dof_off = drive_off_mask;
  return SDX_OK;
}
extern "C" int sdx_dof_dynamics(sdx_handle h, float* mass_dev, float* bias_dev, float* drive_dev, void* stream) {
  if (!h) return SDX_ERR_INVALID;
  if (!mass_dev && !bias_dev && !drive_dev) { h->err = "sdx_dof_dynamics: mass_dev, bias_dev and drive_dev are all NULL"; return SDX_ERR_INVALID; }
  sdxk_dof_dynamics(h->d_const, &h->buf, mass_dev, bias_dev, drive_dev, (hipStream_t)stream);
  return check_launch(h, "sdx_dof_dynamics");
}
extern "C" int sdx_osc_torques(sdx_handle h, const sdx_osc_attr* attr, const float* dpose_dev, float* torques_dev, float* wrench_dev, void* stream) {
  if (!h) return SDX_ERR_INVALID;
  const char* why = nullptr;
  if (!attr) why = "sdx_osc_torques: attr is NULL";
  else if (!dpose_dev) why = "sdx_osc_torques: dpose_dev is NULL";
  else if (!torques_dev) why = "sdx_osc_torques: torques_dev is NULL";
  else {
    const auto gain = [](float v) { return std::isfinite(v) && v >= 0.0f; };
    bool gains = true, posture = true;
    for (int r = 0; r < 6; ++r) gains = gains && gain(attr->kp[r]) && gain(attr->kd[r]);
    for (int j = 0; j < 7; ++j) {
      gains = gains && gain(attr->kp_null[j]) && gain(attr->kd_null[j]);
      posture = posture && std::isfinite(attr->q_null[j]);
    }
    if (!gains) why = "sdx_osc_torques: kp, kd, kp_null and kd_null must be finite and not negative";
    else if (!posture) why = "sdx_osc_torques: q_null must be finite";
    else if (!gain(attr->damping)) why = "sdx_osc_torques: damping must be finite and not negative";
  }
  if (why) { h->err = why; return SDX_ERR_INVALID; }
  sdxk_osc_torques(h->d_const, &h->buf, attr, dpose_dev, torques_dev, wrench_dev, (hipStream_t)stream);
  return check_launch(h, "sdx_osc_torques");
}
extern "C" int sdx_solve_ik(sdx_handle h, const sdx_ik_attr* attr, const float* q0_dev, const float* base_pos_dev, const float* base_quat_dev,
                            const float* tip_pos_dev, float* q_out_dev, float* err_out_dev, int32_t* info_out_dev, void* stream) {
  if (!h) return SDX_ERR_INVALID;
  const char* why = nullptr;
  if (!attr) why = "sdx_solve_ik: attr is NULL";
  else if (!q_out_dev) why = "sdx_solve_ik: q_out_dev is NULL";
  else if (attr->task_mask == 0u || (attr->task_mask >> 5)) why = "sdx_solve_ik: task_mask must select at least one of the tasks 0..4 and nothing above them";
  else if ((attr->task_mask & 1u) && (!base_pos_dev || !base_quat_dev)) why = "sdx_solve_ik: task_mask selects the hand base, base_pos_dev or base_quat_dev is NULL";
  else if ((attr->task_mask & 0x1eu) && !tip_pos_dev) why = "sdx_solve_ik: task_mask selects a fingertip, tip_pos_dev is NULL";
  else if (attr->max_iters < 1 || attr->max_iters > 256) why = "sdx_solve_ik: max_iters must lie in 1..256";
  else {
    const auto ok = [](float v) { return std::isfinite(v) && v >= 0.0f; };
    bool all = ok(attr->damping_arm) && ok(attr->damping_finger) && ok(attr->max_step) && ok(attr->pos_tol) && ok(attr->rot_tol), offsets = true;
    for (int f = 0; f < 4; ++f)
      for (int c = 0; c < 3; ++c) offsets = offsets && std::isfinite(attr->tip_offset[f][c]);
    if (!all) why = "sdx_solve_ik: damping_arm, damping_finger, max_step, pos_tol and rot_tol must be finite and not negative";
    else if (!offsets) why = "sdx_solve_ik: tip_offset must be finite";
    else if (!(attr->max_step > 0.0f)) why = "sdx_solve_ik: max_step must be > 0";
    else {   // the shape of the robot that k_solve_ik walks with static indices
      const sdx_scene_desc& sc = h->h_const.sc;
      bool shape = sc.hand_base_body == 7;
      for (int k = 1; k <= 7; ++k) shape = shape && sc.parent[k] == k - 1;
      for (int f = 0; f < 4; ++f) {
        shape = shape && sc.parent[8 + 4 * f] == 7 && sc.fingertip_body[f] == 11 + 4 * f;
        for (int i = 1; i < 4; ++i) shape = shape && sc.parent[8 + 4 * f + i] == 7 + 4 * f + i;
      }
      if (!shape) why = "sdx_solve_ik: the scene's robot is not a 7-link arm chain carrying four 4-link finger chains that end in fingertip_body";
    }
  }
  if (why) { h->err = why; return SDX_ERR_INVALID; }
  sdxk_solve_ik(h->d_const, &h->buf, attr, q0_dev, base_pos_dev, base_quat_dev, tip_pos_dev, q_out_dev, err_out_dev, info_out_dev, (hipStream_t)stream);
  return check_launch(h, "sdx_solve_ik");
}
extern "C" int sdx_set_contact_report(sdx_handle h, const sdx_contact_report* report, void* stream) {
  if (!h) return SDX_ERR_INVALID;
  (void)stream;
  if (!report) { h->report = sdx_contact_report{}; return SDX_OK; }
  if (!report->count) { h->err = "sdx_set_contact_report: report->count is NULL (pass report = NULL to disarm)"; return SDX_ERR_INVALID; }
  h->report = *report;
  return SDX_OK;
}
extern "C" int sdx_contact_wrenches(sdx_handle h, const sdx_contact_report* report, float* net_dev, const sdx_contact_pairs* pairs, float* pair_dev,
                                    void* stream) {
  if (!h) return SDX_ERR_INVALID;
  const char* why = nullptr;
  if (!report) why = "sdx_contact_wrenches: report is NULL";
  else if (!report->count || !report->body || !report->point || !report->force) why = "sdx_contact_wrenches: the report's count, body, point and force must not be NULL";
  else if (!net_dev && !pair_dev) why = "sdx_contact_wrenches: net_dev and pair_dev are both NULL";
  else if (pair_dev && !pairs) why = "sdx_contact_wrenches: pair_dev without pairs";
  else if (pairs) {
    if (pairs->n_sensor < 0 || pairs->n_sensor > 32 || pairs->n_filter < 0 || pairs->n_filter > 32) why = "sdx_contact_wrenches: n_sensor and n_filter must lie in 0..32";
    else
      for (int i = 0; i < pairs->n_sensor; ++i)
        if (pairs->sensor_body[i] < 0 || pairs->sensor_body[i] >= SDX_BODIES) why = "sdx_contact_wrenches: a sensor body is not a row of SDX_T_RB in [0, SDX_BODIES)";
  }
  if (why) { h->err = why; return SDX_ERR_INVALID; }
  sdxk_contact_wrenches(&h->buf, report, net_dev, pairs, pair_dev, (hipStream_t)stream);
  return check_launch(h, "sdx_contact_wrenches");
}
extern "C" int sdx_set_force_perturbation(sdx_handle h, const sdx_force_perturb_attr* attr, float* rb_forces_dev, float* prob_dev, void* stream) {
  if (!h) return SDX_ERR_INVALID;
  if (!attr || !(attr->force_scale > 0.0f || std::isnan(attr->force_scale))) {   // off (a NaN scale is an error, below)
    if (h->fp_forces && h->ext_force == h->fp_forces) h->ext_force = nullptr;
    h->fp_forces = h->fp_prob = nullptr;
    return SDX_OK;
  }
  const sdx_force_perturb_attr& a = *attr;
  const char* why = nullptr;
  if (!std::isfinite(a.force_scale) || !std::isfinite(a.prob_lo) || !std::isfinite(a.prob_hi) || !std::isfinite(a.decay) || !std::isfinite(a.decay_interval))
    why = "force_scale, the probability range, decay and decay_interval must be finite";
  else if (!(a.prob_lo > 0.0f && a.prob_lo <= a.prob_hi && a.prob_hi <= 1.0f)) why = "the probability range needs 0 < lo <= hi <= 1";
  else if (!(a.decay > 0.0f && a.decay <= 1.0f)) why = "decay must lie in (0, 1]";
  else if (!(a.decay_interval > 0.0f)) why = "decay_interval must be > 0";
  else if (!rb_forces_dev || !prob_dev) why = "rb_forces_dev and prob_dev must not be NULL";
  else if ((uintptr_t)rb_forces_dev % 16 != 0) why = "rb_forces_dev must be 16-byte aligned";
  if (why) { h->err = std::string("sdx_set_force_perturbation: ") + why; return SDX_ERR_INVALID; }
  h->fp = a;
  h->fp_factor = (float)std::pow((double)a.decay, (double)h->h_const.sc.dt / (double)a.decay_interval);
  h->fp_forces = rb_forces_dev;
  h->fp_prob = prob_dev;
  sdxk_force_perturb(h->d_const, &h->buf, &h->fp, h->fp_factor, h->fp_forces, h->fp_prob, nullptr, SDX_FP_DRAW, (hipStream_t)stream);
  return check_launch(h, "sdx_set_force_perturbation");
}

extern "C" int sdx_pre_physics(sdx_handle h, const float* actions_dev, void* stream) {
  if (!h || !actions_dev) return SDX_ERR_INVALID;
  int flags = 1 | 4;
  const float* act = noise_actions(h, actions_dev, &flags, (hipStream_t)stream);
  if (h->buf.dr_on) sdxk_dr_sample(h->d_const, &h->buf, &h->dr, 0, nullptr, (hipStream_t)stream);   // before this step's resets (BT:229-260 runs inside reset_idx)
  force_perturb_step(h, (hipStream_t)stream);   // (after the sampler: a push is scaled by the brick's mass factor of this step)
  sdxk_pre_physics(h->d_const, &h->buf, act, nullptr, nullptr, flags, (hipStream_t)stream);
  return check_launch(h, "sdx_pre_physics");
}
extern "C" int sdx_simulate(sdx_handle h, void* stream) {
  if (!h) return SDX_ERR_INVALID;
  physics_step(h, (hipStream_t)stream);
  return check_launch(h, "sdx_simulate");
}
extern "C" int sdx_post_physics(sdx_handle h, void* stream) {
  if (!h) return SDX_ERR_INVALID;
  post_physics_step(h, (hipStream_t)stream);
  return check_launch(h, "sdx_post_physics");
}
extern "C" int sdx_compute_observations(sdx_handle h, void* stream) {
  if (!h) return SDX_ERR_INVALID;
  sdxk_post_physics(h->d_const, &h->buf, 0, (hipStream_t)stream);
  return check_launch(h, "sdx_compute_observations");
}
// The shared opening of Orient's and Search's reset events: the reset flags are read on the host (as reset_buf.nonzero() does), with
// progress_buf[0] in the same round trip when `progress0` is given; when some env resets, *mask holds the flags as 0 / 1 and its
// device copy is h->orient_mask; when none does, *mask comes back empty.
static int reset_mask_from_flags(sdx_handle h, hipStream_t st, std::vector<uint8_t>* mask, int64_t* progress0) {
  const int N = h->buf.N;
  std::vector<int64_t> flags(N);
  HIPCHK(h, hipMemcpyAsync(flags.data(), h->buf.reset, sizeof(int64_t) * N, hipMemcpyDeviceToHost, st));
  if (progress0) HIPCHK(h, hipMemcpyAsync(progress0, h->buf.progress, sizeof(int64_t), hipMemcpyDeviceToHost, st));
  HIPCHK(h, hipStreamSynchronize(st));
  mask->assign(N, 0);
  int any = 0;
  for (int i = 0; i < N; ++i) { (*mask)[i] = flags[i] != 0; any |= (*mask)[i]; }
  if (!any) { mask->clear(); return SDX_OK; }
  if (!h->orient_mask) { HIPCHK(h, hipMalloc((void**)&h->orient_mask, N)); h->allocs.push_back(h->orient_mask); }
  HIPCHK(h, hipMemcpyAsync(h->orient_mask, mask->data(), N, hipMemcpyHostToDevice, st));
  return SDX_OK;
}
// BlockAssemblyOrient reset (OR:1390-1695).  Like the reference (reset_buf.nonzero()) this reads the reset flags on the host; a reset
// event costs 50 (only when steps have been taken) + 2 + 1 + 50 simulator steps of ALL envs, during which the resetting envs' arms
// are scripted by the tracking IK.  The shipped task only resets on time-out, so all envs reset together every episodeLength steps.
static int orient_reset_if_needed(sdx_handle h, hipStream_t st) {
  std::vector<uint8_t> mask;
  const int rc = reset_mask_from_flags(h, st, &mask, nullptr);
  if (rc != SDX_OK || mask.empty()) return rc;
  uint32_t steps = 0;
  HIPCHK(h, hipMemcpyAsync(&steps, h->buf.step_count, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  HIPCHK(h, hipStreamSynchronize(st));
  if (steps > 0)
    for (int i = 0; i < 50; ++i) { sdxk_orient_pregrasp(h->d_const, &h->buf, h->orient_mask, 0, i, st); sdxk_physics(h->d_const, &h->buf, st); }
  if (steps > 0) sdxk_post_physics(h->d_const, &h->buf, 0, st);                        // self.compute_observations() before the harvest, OR:1464-1465
  sdxk_pre_physics(h->d_const, &h->buf, nullptr, h->orient_mask, nullptr, 2, st);      // harvest, restore piles, hand to the prepare pose, counters
  sdxk_physics(h->d_const, &h->buf, st);
  sdxk_physics(h->d_const, &h->buf, st);                                               // OR:1618-1620
  sdxk_orient_post_reset(h->d_const, &h->buf, h->orient_mask, st);
  sdxk_physics(h->d_const, &h->buf, st);                                               // OR:1653
  for (int i = 0; i < 50; ++i) { sdxk_orient_pregrasp(h->d_const, &h->buf, h->orient_mask, 1, i, st); sdxk_physics(h->d_const, &h->buf, st); }
  return check_launch(h, "sdx_step(orient reset)");
}

// BlockAssemblySearch: reset_idx + post_reset (SE:1274-1538) for the envs whose reset flag is set (read on the host, as
// reset_buf.nonzero() does): outcome / harvest / lattice restore on the device, 60 settling steps of all envs, a segmentation render
// (emergence bookkeeping), hand to the prepare pose.  *progress0 = progress_buf[0] before this step (the end-of-episode render keys
// on it, SE:992).
static int search_reset_if_needed(sdx_handle h, hipStream_t st, int64_t* progress0) {
  std::vector<uint8_t> mask;
  const int rc = reset_mask_from_flags(h, st, &mask, progress0);
  if (rc != SDX_OK || mask.empty()) return rc;
  sdxk_pre_physics(h->d_const, &h->buf, nullptr, h->orient_mask, nullptr, 2, st);      // outcome, harvest, lattice + noise, target drop, default pose
  for (int i = 0; i < 60; ++i) sdxk_physics(h->d_const, &h->buf, st);                  // SE:1437-1439
  sdxk_seg_camera(h->d_const, &h->buf, st);                                            // SE:1444-1455
  sdxk_search_set_hand(h->d_const, &h->buf, h->orient_mask, 0, st);                    // SE:1482-1495
  if (mask[0]) *progress0 = 0;
  return check_launch(h, "sdx_step(search reset)");
}

extern "C" int sdx_step(sdx_handle h, const float* actions_dev, void* stream) {
  if (!h || !actions_dev) return SDX_ERR_INVALID;
  hipStream_t st = (hipStream_t)stream;
  int targets = 4;                          // k_pre_physics flags of the action -> targets launch
  const float* act = noise_actions(h, actions_dev, &targets, st);
  if (h->buf.dr_on) sdxk_dr_sample(h->d_const, &h->buf, &h->dr, 0, nullptr, st);   // before any reset physics of this step, Orient's / Search's settling launches included
  force_perturb_step(h, st);
  // the kind's reset event: Orient and Search run theirs here, on the host's reading of the reset flags; GraspSim and InsertSim reset
  // inside the k_pre_physics launch below (flag 1)
  const int kind = h->h_const.sc.task_kind;
  int64_t p0 = 0;                           // Search: progress_buf[0] before this step
  int rc = SDX_OK;
  if (kind == SDX_TASK_SEARCH) rc = search_reset_if_needed(h, st, &p0);
  else if (kind == SDX_TASK_ORIENT) rc = orient_reset_if_needed(h, st);
  else targets |= 1;
  if (rc != SDX_OK) return rc;
  sdxk_pre_physics(h->d_const, &h->buf, act, nullptr, nullptr, targets, st);
  physics_step(h, st);   // controlFrequencyInv = 1 (EG:18); with the pending external wrench, if any
  if (kind == SDX_TASK_SEARCH && (float)(p0 + 1) >= h->h_const.sc.max_episode_length - 1.0f) {   // SE:992-1019: park the hand, one more step, render
    sdxk_search_set_hand(h->d_const, &h->buf, nullptr, 1, st);
    physics_step(h, st);   // (nothing is pending any more; an armed contact report describes this launch, as SDX_T_CONTACT does)
    sdxk_seg_camera(h->d_const, &h->buf, st);
  }
  post_physics_step(h, st);
  return check_launch(h, "sdx_step");
}
// Not part of include/seqdex.h: the scripted stand-in for a trained grasp policy that the chain benchmark and its tests drive the grasp
// stage with (seqdex_amd/scripts/evaluation.py), as one launch instead of ~40 torch operations per env step.
extern "C" int sdxk_scripted_grasp_actions(sdx_handle h, float* close_state_dev, float* actions_out_dev, void* stream) {
  if (!h || !close_state_dev || !actions_out_dev) return SDX_ERR_INVALID;
  sdxk_scripted_grasp(h->d_const, &h->buf, close_state_dev, actions_out_dev, (hipStream_t)stream);
  return check_launch(h, "sdxk_scripted_grasp_actions");
}
extern "C" int sdx_reset_idx(sdx_handle h, const uint8_t* env_mask_dev, const int32_t* pile_choice_dev, void* stream) {
  if (!h || !env_mask_dev) return SDX_ERR_INVALID;
  if (h->buf.dr_on) sdxk_dr_sample(h->d_const, &h->buf, &h->dr, 0, env_mask_dev, (hipStream_t)stream);   // reset_idx -> apply_randomizations (GS:1395-1396)
  if (h->fp_forces) sdxk_force_perturb(h->d_const, &h->buf, &h->fp, h->fp_factor, h->fp_forces, h->fp_prob, env_mask_dev, SDX_FP_RESET, (hipStream_t)stream);
  sdxk_pre_physics(h->d_const, &h->buf, nullptr, env_mask_dev, pile_choice_dev, 2, (hipStream_t)stream);
  return check_launch(h, "sdx_reset_idx");
}
extern "C" int sdx_render_segmentation(sdx_handle h, void* stream) {
  if (!h) return SDX_ERR_INVALID;
  if (h->h_const.sc.task_kind != SDX_TASK_SEARCH) { h->err = "sdx_render_segmentation: the segmentation camera belongs to BlockAssemblySearch (task_kind 3)"; return SDX_ERR_STATE; }
  sdxk_seg_camera(h->d_const, &h->buf, (hipStream_t)stream);
  return check_launch(h, "sdx_render_segmentation");
}
extern "C" int sdx_render_view(sdx_handle h, const sdx_view_desc* v, const int32_t* env_ids_dev, int32_t n, float* depth_out_dev,
                               int16_t* label_out_dev, uint8_t* rgb_out_dev, void* stream) {
  if (!h) return SDX_ERR_INVALID;
  if (!v || n < 0 || (n > 0 && !env_ids_dev)) { h->err = "sdx_render_view: view / env_ids NULL or n < 0"; return SDX_ERR_INVALID; }
  if (v->width < 1 || v->width > 2048 || v->height < 1 || v->height > 2048) { h->err = "sdx_render_view: width and height must lie in 1..2048"; return SDX_ERR_INVALID; }
  if (v->attach_body < -1 || v->attach_body >= SDX_NLINK) { h->err = "sdx_render_view: attach_body must be -1 or a link in [0, SDX_NLINK)"; return SDX_ERR_INVALID; }
  if (v->geometry != SDX_VIEW_BOUNDS && v->geometry != SDX_VIEW_COLLISION) { h->err = "sdx_render_view: geometry must be SDX_VIEW_BOUNDS or SDX_VIEW_COLLISION"; return SDX_ERR_INVALID; }
  if (!(v->hfov_deg > 0.0f && v->hfov_deg < 180.0f)) { h->err = "sdx_render_view: hfov_deg must lie in (0, 180)"; return SDX_ERR_INVALID; }
  double f[3], c[3], f2 = 0.0, c2 = 0.0, u2 = 0.0;
  bool finite = true;
  for (int a = 0; a < 3; ++a) {
    finite = finite && std::isfinite(v->pos[a]) && std::isfinite(v->target[a]) && std::isfinite(v->up[a]);
    f[a] = (double)v->target[a] - (double)v->pos[a];
  }
  if (!finite) { h->err = "sdx_render_view: pos / target / up must be finite"; return SDX_ERR_INVALID; }
  c[0] = f[1] * v->up[2] - f[2] * v->up[1]; c[1] = f[2] * v->up[0] - f[0] * v->up[2]; c[2] = f[0] * v->up[1] - f[1] * v->up[0];
  for (int a = 0; a < 3; ++a) { f2 += f[a] * f[a]; c2 += c[a] * c[a]; u2 += (double)v->up[a] * v->up[a]; }
  if (!(f2 > 0.0)) { h->err = "sdx_render_view: pos == target (no view direction)"; return SDX_ERR_INVALID; }
  if (!(c2 > 1e-12 * f2 * u2)) { h->err = "sdx_render_view: up is zero or parallel to the view direction"; return SDX_ERR_INVALID; }
  const long long tiles = (long long)((v->width + 15) / 16) * ((v->height + 15) / 16);
  if (tiles * n > 0x7fffffffLL) { h->err = "sdx_render_view: too many tiles for one launch (n x ceil(width / 16) x ceil(height / 16) >= 2^31)"; return SDX_ERR_INVALID; }
  if (n == 0 || (!depth_out_dev && !label_out_dev && !rgb_out_dev)) return SDX_OK;
  sdxk_render_view(h->d_const, &h->buf, v, env_ids_dev, n, depth_out_dev, label_out_dev, rgb_out_dev, (hipStream_t)stream);
  return check_launch(h, "sdx_render_view");
}
extern "C" int sdx_refresh_kinematics(sdx_handle h, void* stream) {
  if (!h) return SDX_ERR_INVALID;
  sdxk_kinematics(h->d_const, &h->buf, (hipStream_t)stream);
  return check_launch(h, "sdx_refresh_kinematics");
}
extern "C" int sdx_set_indexed(sdx_handle h, int32_t id, const float* src_dev, const int32_t* actor_ids_dev, int32_t n, void* stream) {
  if (!h) return SDX_ERR_INVALID;
  if (!src_dev || !actor_ids_dev || n < 0 || (id != SDX_T_ROOT && id != SDX_T_DOF && id != SDX_T_TARGETS)) {
    h->err = "sdx_set_indexed: id must be SDX_T_ROOT, SDX_T_DOF or SDX_T_TARGETS, src / ids non-NULL"; return SDX_ERR_INVALID;
  }
  hipStream_t st = (hipStream_t)stream;
  if (n > 0) sdxk_set_indexed(&h->buf, id, src_dev, actor_ids_dev, n, st);
  if (id == SDX_T_DOF && n > 0) sdxk_kinematics(h->d_const, &h->buf, st);
  return check_launch(h, "sdx_set_indexed");
}
extern "C" int sdx_num_envs(sdx_handle h) { return h ? h->buf.N : SDX_ERR_INVALID; }
extern "C" const char* sdx_last_error(sdx_handle h) { return h ? h->err.c_str() : g_create_err.c_str(); }
#ifdef HIPEMU   // the CPU emulator (tests/hipemu) builds the simulator from four units, sdx_capi / task / physics / camera: there, and only there, the samplers are part of this one
#include "sdx_randomize.hip"
#endif
