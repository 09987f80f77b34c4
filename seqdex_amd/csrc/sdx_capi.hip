// sdx_capi.hip — host side of the sdx_* C ABI declared in include/seqdex.h (simulator + task seam).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "sdx_common.h"
#include "sdx_const_build.h"
#include "sdx_state.h"

extern "C" {
void sdxk_pre_physics(const SdxConst*, const SdxBuf*, const float*, const uint8_t*, const int32_t*, int, hipStream_t);
void sdxk_post_physics(const SdxConst*, const SdxBuf*, int, hipStream_t);
void sdxk_physics(const SdxConst*, const SdxBuf*, hipStream_t);
void sdxk_kinematics(const SdxConst*, const SdxBuf*, hipStream_t);
extern "C" void sdxk_seg_camera(const SdxConst*, const SdxBuf*, hipStream_t);
void sdxk_render_view(const SdxConst*, const SdxBuf*, const sdx_view_desc*, const int32_t*, int, float*, int16_t*, uint8_t*, hipStream_t);
void sdxk_orient_pregrasp(const SdxConst*, const SdxBuf*, const uint8_t*, int, int, hipStream_t);
void sdxk_orient_post_reset(const SdxConst*, const SdxBuf*, const uint8_t*, hipStream_t);
}

struct sdx_sim {
  int device = 0;
  SdxConst* d_const = nullptr;
  SdxConst h_const;
  SdxBuf buf;
  uint8_t* orient_mask = nullptr;   // device copy of the reset flags of an Orient reset event
  std::vector<void*> allocs;
  struct TensorInfo { void* ptr; int64_t shape[4]; int ndim; int dtype; } tinfo[SDX_T_COUNT];
  bool has_piles = false;
  sdx_dr_desc dr{};           // the randomization in force (meaningful while buf.dr_on != nullptr)
  sdx_noise_attr noise_obs{}, noise_act{};   // sdx_set_noise: distribution SDX_DR_NONE = off (always off while randomization is off)
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

static void qrot_host(const float q[4], const float v[3], float out[3]) {
  float u[3] = {q[0], q[1], q[2]};
  float t[3] = {2 * (u[1] * v[2] - u[2] * v[1]), 2 * (u[2] * v[0] - u[0] * v[2]), 2 * (u[0] * v[1] - u[1] * v[0])};
  out[0] = v[0] + q[3] * t[0] + (u[1] * t[2] - u[2] * t[1]);
  out[1] = v[1] + q[3] * t[1] + (u[2] * t[0] - u[0] * t[2]);
  out[2] = v[2] + q[3] * t[2] + (u[0] * t[1] - u[1] * t[0]);
}

// ---------------------------------------------------------------- domain randomization (include/seqdex.h sdx_set_randomization,
// DESIGN.md section 18).  Samples are pure functions of (seed, env, slot, draw): sdx_hash(seed ^ SDX_DR_TAG, env * SDX_DR_SLOTS + slot, draw).
#define SDX_DR_TAG 0xD0A1ull
#define SDX_DR_SLOT_LINK (4 * SDX_NDOF)                        // 92: 24 link masses, then 24 link frictions
#define SDX_DR_SLOT_BRICK (SDX_DR_SLOT_LINK + 2 * SDX_NLINK)   // 140: 72 brick masses, then 72 brick frictions
#define SDX_DR_SLOT_GRAV (SDX_DR_SLOT_BRICK + 2 * SDX_NFREE)   // 284..286: gravity (env 0's row)
__device__ __forceinline__ float dr_u(uint64_t hs, int which) {   // uniform in (0, 1): 24 bits of the hash, +0.5
  const uint32_t b = which ? (uint32_t)(hs >> 16) & 0xffffffu : (uint32_t)(hs >> 40);
  return ((float)b + 0.5f) * (1.0f / 16777216.0f);
}
__device__ __forceinline__ float dr_sched(int schedule, int steps, long long frame) {
  if (schedule == SDX_DR_SCHED_LINEAR) return (float)(frame < steps ? frame : (long long)steps) / (float)steps;
  if (schedule == SDX_DR_SCHED_CONSTANT) return frame < steps ? 0.0f : 1.0f;
  return 1.0f;
}
__device__ __forceinline__ float dr_sched(const sdx_dr_attr& a, long long frame) { return dr_sched(a.schedule, a.schedule_steps, frame); }
__device__ __forceinline__ float dr_bucket(float lo, float hi, int k, int nb) { return lo + (hi - lo) * (float)k / (float)nb; }
// the randomized value of a quantity whose scene value is v0 (s > 0; s == 0 leaves v0)
__device__ float dr_value(const sdx_dr_attr& a, float s, uint64_t hs, float v0) {
#pragma clang fp contract(off)
  const bool scaling = a.operation == SDX_DR_SCALING;
  const float lo = a.range[0], hi = a.range[1];
  float x;
  if (a.distribution == SDX_DR_GAUSSIAN) {
    const float mu = scaling ? lo * s + (1.0f - s) : lo * s, sig = hi * s;
    const float z = sqrtf(-2.0f * logf(dr_u(hs, 0))) * cosf(6.28318530718f * dr_u(hs, 1));
    x = mu + sig * z;
  } else {
    const float a0 = scaling ? lo * s + (1.0f - s) : lo * s, a1 = scaling ? hi * s + (1.0f - s) : hi * s;
    const float u = dr_u(hs, 0);
    if (a.distribution == SDX_DR_UNIFORM) x = a0 + (a1 - a0) * u;
    else x = a0 == a1 ? a0 : expf(logf(a0) + (logf(a1) - logf(a0)) * u);
  }
  if (a.num_buckets > 0) {   // snap down to lo + (hi - lo) k / nb of the untransformed range (gaussian: mu -+ 2 sqrt(sigma))
    const float blo = a.distribution == SDX_DR_GAUSSIAN ? lo - 2.0f * sqrtf(hi) : lo;
    const float bhi = a.distribution == SDX_DR_GAUSSIAN ? lo + 2.0f * sqrtf(hi) : hi;
    const int nb = a.num_buckets;
    int k = (int)floorf((x - blo) / (bhi - blo) * (float)nb);
    k = k < 0 ? 0 : (k > nb - 1 ? nb - 1 : k);
    while (k > 0 && dr_bucket(blo, bhi, k, nb) > x) --k;
    while (k + 1 < nb && dr_bucket(blo, bhi, k + 1, nb) <= x) ++k;
    x = dr_bucket(blo, bhi, k, nb);
  }
  return scaling ? v0 * x : v0 + x;
}
// rows <- the scene's values (factors 1)
__global__ void k_dr_defaults(const SdxConst* __restrict__ C, SdxBuf B) {
  const int e = blockIdx.x, t = threadIdx.x;
  const sdx_scene_desc& sc = C->sc;
  for (int i = t; i < 4 * SDX_NDOF; i += blockDim.x) {
    const int r = i / SDX_NDOF, j = i % SDX_NDOF;
    B.dr_dof[(size_t)e * 4 * SDX_NDOF + i] = r == 0 ? sc.kp[j] : r == 1 ? sc.kd[j] : r == 2 ? sc.lower[j] : sc.upper[j];
  }
  for (int i = t; i < 2 * SDX_NLINK; i += blockDim.x) B.dr_link[(size_t)e * 2 * SDX_NLINK + i] = i < SDX_NLINK ? 1.0f : sc.friction;
  for (int i = t; i < 2 * SDX_NFREE; i += blockDim.x) B.dr_brick[(size_t)e * 2 * SDX_NFREE + i] = i < SDX_NFREE ? 1.0f : sc.friction;
  if (e == 0 && t < 3) B.dr_grav[t] = sc.gravity[t];
}
// gravity ("non-env", BT:241,248): on the first randomization, else when some env resets and frame - last_rand_frame >= frequency
// mask: the envs being reset (sdx_reset_idx's env mask), nullptr = reset_buf (sdx_step / sdx_pre_physics)
__global__ __launch_bounds__(256) void k_dr_gravity(const SdxConst* __restrict__ C, SdxBuf B, sdx_dr_desc d, int first, const uint8_t* mask) {
  __shared__ int any;
  const int t = threadIdx.x;
  if (t == 0) any = first;
  __syncthreads();
  for (int e = t; e < B.N && !first; e += 256) if (mask ? mask[e] != 0 : B.reset[e] != 0) any = 1;
  __syncthreads();
  const long long frame = B.dr_frame[0];
  if (!any || (!first && frame - B.dr_frame[1] < d.frequency)) return;
  const uint64_t draw = (uint64_t)B.dr_draw[B.N];
  __syncthreads();
  if (t < 3 && d.gravity.distribution != SDX_DR_NONE) {
    const float s = dr_sched(d.gravity, frame);
    const uint64_t hs = sdx_hash(B.seed ^ SDX_DR_TAG, (uint64_t)(SDX_DR_SLOT_GRAV + t), draw);
    B.dr_grav[t] = s > 0.0f ? dr_value(d.gravity, s, hs, C->sc.gravity[t]) : C->sc.gravity[t];
  }
  if (t == 0) { B.dr_frame[1] = frame; B.dr_draw[B.N] = (int32_t)(draw + 1); }
}
// per env (BT:238-245): every env on the first randomization, else the envs that reset now with randomize_buf >= frequency (-> 0)
__global__ __launch_bounds__(128) void k_dr_sample(const SdxConst* __restrict__ C, SdxBuf B, sdx_dr_desc d, int first, const uint8_t* mask) {
  const int e = blockIdx.x, t = threadIdx.x;
  if (!first && !((mask ? mask[e] != 0 : B.reset[e] != 0) && B.randomize[e] >= d.frequency)) return;
  const sdx_scene_desc& sc = C->sc;
  const long long frame = B.dr_frame[0];
  const uint64_t draw = (uint64_t)B.dr_draw[e];
  __syncthreads();
  for (int k = t; k < SDX_DR_SLOT_GRAV; k += blockDim.x) {
    const sdx_dr_attr* a;
    float v0;
    float* out;
    bool factor = false;
    if (k < SDX_DR_SLOT_LINK) {
      const int r = k / SDX_NDOF, j = k % SDX_NDOF;
      a = r == 0 ? &d.dof_stiffness : r == 1 ? &d.dof_damping : r == 2 ? &d.dof_lower : &d.dof_upper;
      v0 = r == 0 ? sc.kp[j] : r == 1 ? sc.kd[j] : r == 2 ? sc.lower[j] : sc.upper[j];
      out = &B.dr_dof[(size_t)e * 4 * SDX_NDOF + k];
    } else if (k < SDX_DR_SLOT_BRICK) {
      const int i = k - SDX_DR_SLOT_LINK, l = i % SDX_NLINK;
      factor = i < SDX_NLINK;
      a = factor ? &d.link_mass : &d.link_friction;
      v0 = factor ? sc.link_mass[l] : sc.friction;
      out = &B.dr_link[(size_t)e * 2 * SDX_NLINK + i];
    } else {
      const int i = k - SDX_DR_SLOT_BRICK, b = i % SDX_NFREE;
      factor = i < SDX_NFREE;
      a = factor ? &d.brick_mass : &d.brick_friction;
      v0 = factor ? sc.brick_mass[sc.brick_type[b]] : sc.friction;
      out = &B.dr_brick[(size_t)e * 2 * SDX_NFREE + i];
    }
    if (a->distribution == SDX_DR_NONE) continue;   // not randomized: the row keeps what it holds
    // masses are stored as factors of the scene's mass (inertia scales with them): a scaling sample IS the factor
    const bool scaled = a->operation == SDX_DR_SCALING;
    const float base = factor && scaled ? 1.0f : v0;
    const float s = dr_sched(*a, frame);
    float v = base;
    if (s > 0.0f) v = dr_value(*a, s, sdx_hash(B.seed ^ SDX_DR_TAG, (uint64_t)e * SDX_DR_SLOTS + k, draw), base);
    *out = factor && !scaled ? (v0 != 0.0f ? v / v0 : 1.0f) : v;
  }
  __syncthreads();
  if (t == 0) {
    B.dr_draw[e] = (int32_t)(draw + 1);
    if (!first) B.randomize[e] = 0;
  }
}
static void dr_sample(sdx_sim* h, int first, hipStream_t st, const uint8_t* mask = nullptr) {
  hipLaunchKernelGGL(k_dr_gravity, dim3(1), dim3(256), 0, st, h->d_const, h->buf, h->dr, first, mask);
  hipLaunchKernelGGL(k_dr_sample, dim3(h->buf.N), dim3(128), 0, st, h->d_const, h->buf, h->dr, first, mask);
}

// ---------------------------------------------------------------- observation / action noise (include/seqdex.h sdx_set_noise,
// DESIGN.md section 18).  The operand of (env, column) is a pure function of the seed and three counters the randomization path keeps:
// dr_frame[1] (schedule), dr_draw[N] (correlated part) and step_count (white part).  Column pair p = column / 2 shares one hash per part:
// sdx_hash(seed ^ tag, env * SDX_NOISE_PAIRS + p, counter).
#define SDX_NOISE_TAG_OBS 0x0B50ull   // | SDX_NOISE_CORR / SDX_NOISE_WHITE
#define SDX_NOISE_TAG_ACT 0xAC70ull
#define SDX_NOISE_CORR 0xCull
#define SDX_NOISE_WHITE 0x7ull
#define SDX_NOISE_PAIRS 256           // streams per env (the widest row has 396 / 2 pairs)
// The sampler's Box-Muller (dr_value) on the two uniforms of one hash, both outputs: the pair's first (cos) or second (sin) standard
// normal.  log, cos and sin are rounded ONCE from double precision here: with the device's float versions 0.4 % of the draws lay 3 ulp
// (2 in 47 000: 4 ulp) from the float32 restatement the noise is held to within 2 ulp of.
__device__ __forceinline__ float noise_normal(uint64_t hs, int second) {
#pragma clang fp contract(off)
  const float r = sqrtf(-2.0f * (float)log((double)dr_u(hs, 0))), th = 6.28318530718f * dr_u(hs, 1);
  return r * (float)(second ? sin((double)th) : cos((double)th));
}
// the scaled numbers the reference freezes at a non-env randomization (BT:279-291,309-318): p[0..1] white, p[2..3] correlated
__device__ __forceinline__ void noise_scaled(const sdx_noise_attr& a, float s, float p[4]) {
#pragma clang fp contract(off)
  const bool scaling = a.operation == SDX_DR_SCALING, gauss = a.distribution == SDX_DR_GAUSSIAN;
  for (int k = 0; k < 2; ++k) {
    const float* r = k ? a.range_correlated : a.range;
    p[2 * k] = scaling ? r[0] * s + (1.0f - s) : r[0] * s;
    p[2 * k + 1] = scaling && !gauss ? r[1] * s + (1.0f - s) : r[1] * s;   // a sigma is only ever scaled
  }
}
// corr + white of one column (BT:299-301,326-327); the correlated part is a NORMAL draw for the uniform distribution too
__device__ __forceinline__ float noise_operand(bool gauss, const float p[4], uint64_t hc, uint64_t hw, int odd) {
#pragma clang fp contract(off)
  const float zc = noise_normal(hc, odd);
  const float corr = gauss ? p[2] + p[3] * zc : p[2] + (p[3] - p[2]) * zc;
  const float white = gauss ? p[0] + p[1] * noise_normal(hw, odd) : p[0] + (p[1] - p[0]) * dr_u(hw, odd);
  return corr + white;
}
// One thread per (env, group of 4 columns) = two column pairs.  W % 4 == 0 (GraspSim's 396 columns): one 16-byte load and one 16-byte
// store per thread; the other widths (186, 75, the 23 action columns) go column by column and the last group of a row is partial.
// act == 0: dst = clamp(op(src, operand), +-clip_obs) (src = obs, dst = obs_c, which k_post_physics has filled with clamp(obs));
// act == 1: dst = op(clamp(src, +-clip_actions), operand) (src = the caller's actions, dst = the buffer k_pre_physics then reads).
// An additive block whose scaled numbers are all zero changes nothing: x + 0 would turn a -0 into +0.
__global__ __launch_bounds__(256) void k_noise(const SdxConst* __restrict__ C, SdxBuf B, sdx_noise_attr a, const float* __restrict__ src,
                                               float* __restrict__ dst, int W, int act) {
#pragma clang fp contract(off)
  const int G = (W + 3) >> 2;
  const int tid = blockIdx.x * 256 + threadIdx.x;
  if (tid >= B.N * G) return;
  const int e = tid / G, c0 = (tid - e * G) * 4;
  float p[4];
  noise_scaled(a, dr_sched(a.schedule, a.schedule_steps, B.dr_frame[1]), p);
  const bool additive = a.operation == SDX_DR_ADDITIVE, gauss = a.distribution == SDX_DR_GAUSSIAN;
  const bool zero = additive && p[0] == 0.0f && p[1] == 0.0f && p[2] == 0.0f && p[3] == 0.0f;   // wave-uniform
  if (zero && !act) return;
  const float clip = act ? C->sc.clip_actions : C->sc.clip_obs;
  const bool vec = (W & 3) == 0;
  const int n = W - c0 < 4 ? W - c0 : 4;
  const size_t at = (size_t)e * W + c0;
  float x[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  if (vec) {
    const f4v v = *reinterpret_cast<const f4v*>(src + at);
    x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w;
  } else {
    for (int k = 0; k < n; ++k) x[k] = src[at + k];
  }
  if (act) for (int k = 0; k < 4; ++k) x[k] = clampf(x[k], -clip, clip);
  if (!zero) {
    const uint64_t tag = B.seed ^ (act ? SDX_NOISE_TAG_ACT : SDX_NOISE_TAG_OBS);
    const uint64_t ccorr = (uint64_t)B.dr_draw[B.N], cwhite = (uint64_t)B.step_count[0];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      if (2 * q >= n) break;
      const uint64_t stream = (uint64_t)e * SDX_NOISE_PAIRS + (uint64_t)((c0 >> 1) + q);
      const uint64_t hc = sdx_hash(tag ^ SDX_NOISE_CORR, stream, ccorr), hw = sdx_hash(tag ^ SDX_NOISE_WHITE, stream, cwhite);
#pragma unroll
      for (int odd = 0; odd < 2; ++odd) {
        const int k = 2 * q + odd;
        if (k >= n) break;
        const float o = noise_operand(gauss, p, hc, hw, odd);
        x[k] = additive ? x[k] + o : x[k] * o;
      }
    }
    if (!act) for (int k = 0; k < 4; ++k) x[k] = clampf(x[k], -clip, clip);
  }
  if (vec) {
    f4v v;
    v.x = x[0]; v.y = x[1]; v.z = x[2]; v.w = x[3];
    *reinterpret_cast<f4v*>(dst + at) = v;
  } else {
    for (int k = 0; k < n; ++k) dst[at + k] = x[k];
  }
}
static void noise_launch(sdx_sim* h, const sdx_noise_attr& a, const float* src, float* dst, int W, int act, hipStream_t st) {
  const long long threads = (long long)h->buf.N * ((W + 3) / 4);
  hipLaunchKernelGGL(k_noise, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, st, h->d_const, h->buf, a, src, dst, W, act);
}
// the actions k_pre_physics takes.  With action noise on: h->act_pre, already clamped and noised (flag 8), computed here - before this
// step's re-sampling, from the blocks and counters in force until now.  The caller's buffer is only read.
static const float* noise_actions(sdx_sim* h, const float* actions_dev, int* flags, hipStream_t st) {
  if (h->noise_act.distribution == SDX_DR_NONE) return actions_dev;
  noise_launch(h, h->noise_act, actions_dev, h->act_pre, SDX_NDOF, 1, st);
  *flags |= 8;
  return h->act_pre;
}
// post_physics_step, then the observation noise of BaseTask.step (BT:149-150) on the policy's row
static void post_physics_step(sdx_sim* h, hipStream_t st) {
  sdxk_post_physics(h->d_const, &h->buf, 1, st);
  if (h->noise_obs.distribution != SDX_DR_NONE) noise_launch(h, h->noise_obs, h->buf.obs, h->buf.obs_c, h->buf.obs_w, 0, st);
}

// ---------------------------------------------------------------- sim snapshots (include/seqdex.h sdx_state_*)
// The segment table: every per-env buffer of SdxBuf that a later call reads before it writes.  This list is the one place that says what
// an env's state is; the logs (harvest / pile / T-value rings with their counts and keys, cstats, dbg), the scheduling hints (order,
// cost), scratch (cscratch, tvt_h, orient_mask) and configuration (piles, tv_w, tvt_w, the randomization descriptor, dr_on) are not in it.
static int state_table_build(sdx_sim* h) {
  SdxBuf& B = h->buf;
  SdxStateTab& S = h->st_tab;
  const sdx_scene_desc& sc = h->h_const.sc;
  const int N = B.N;
  const bool search = sc.task_kind == SDX_TASK_SEARCH, warm = sc.warm_start > 0.0f;
  S.N = N;
  S.var3 = (sc.static_var_slot >= 0 || sc.task_kind == SDX_TASK_INSERT) ? 1 : 0;   // the base plate / the insertion site depend on env % 3
  S.row_bytes = 16;   // the row header: source env, warm count, SDX_ST_MAGIC, 0
  S.wcount = B.wcount;
  bool ok = true;
#define SEG(field, per_env) ok = ok && sdx_state_add(&S, B.field, (size_t)(per_env) * sizeof(*B.field), (size_t)(per_env) * sizeof(*B.field), 0)
  SEG(root, SDX_ACTORS * 13); SEG(dof, SDX_NDOF * 2); SEG(rb, SDX_BODIES * 13); SEG(contact, SDX_BODIES * 3);
  SEG(jac, 42); SEG(jac_full, (SDX_NLINK - 1) * 6 * SDX_NDOF); SEG(targets, SDX_NDOF); SEG(prev_targets, SDX_NDOF);
  SEG(obs, B.obs_w); SEG(states, SDX_NUM_STATES); SEG(obs_c, B.obs_w); SEG(states_c, SDX_NUM_STATES);
  SEG(rew, 1); SEG(reset, 1); SEG(progress, 1); SEG(randomize, 1); SEG(actions, SDX_NDOF);
  SEG(init_pos, 3); SEG(init_rot, 4); SEG(successes, 1); SEG(meta_rew, 1); SEG(finger_dist, 1); SEG(tvalue, 1);
  SEG(arm_contacts, 6); SEG(student_obs, 30); SEG(success_buf, 1); SEG(pile_choice, 1); SEG(ncontacts, 1);
  SEG(cam_rot, 4); SEG(insert_aux, 8); SEG(seg_stats, 4); SEG(seg_pix, 4); SEG(emergence, 1);
  if (search) { SEG(seg_image, 128 * 128); SEG(tvt_buf, 652); }
  SEG(dr_dof, 4 * SDX_NDOF); SEG(dr_link, 2 * SDX_NLINK); SEG(dr_brick, 2 * SDX_NFREE); SEG(dr_draw, 1);
#undef SEG
  if (warm) {   // wcount[e] travels in the row header; of the key row and the three impulse rows only the first wcount[e] entries are state
    ok = ok && sdx_state_add(&S, B.wkey, (size_t)SDX_MAXC * 4, (size_t)SDX_MAXC * 4, 1);
    for (int r = 0; r < 3; ++r) ok = ok && sdx_state_add(&S, B.wlam + (size_t)r * SDX_MAXC, (size_t)3 * SDX_MAXC * 4, (size_t)SDX_MAXC * 4, 1);
  }
  if (!ok) { h->err = "sdx_create: state segment table (a buffer is missing, misaligned or not a multiple of 4 bytes per env)"; return SDX_ERR_INVALID; }
  S.nunits = (int32_t)(S.row_bytes / 16);
  void* globs[SDX_ST_NGLOB] = {B.step_count, B.stat, B.cons, B.dr_grav, B.dr_frame, B.dr_draw + N};
  const uint32_t gb[SDX_ST_NGLOB] = {4, 16, 4, 12, 16, 4};
  for (int g = 0; g < SDX_ST_NGLOB; ++g) { S.glob[g] = (char*)globs[g]; S.glob_bytes[g] = gb[g]; }
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

extern "C" int sdx_create(const sdx_scene_desc* scene, int32_t num_envs, int32_t device, uint64_t seed, sdx_handle* out) {
  if (!scene || !out || num_envs <= 0) { g_create_err = "sdx_create: bad argument"; return SDX_ERR_INVALID; }
  if (scene->abi_version != SDX_ABI_VERSION) { g_create_err = "sdx_create: scene.abi_version mismatch"; return SDX_ERR_INVALID; }
  {   // the shape tables k_physics indexes without further checks
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
    if (!ok) { g_create_err = "sdx_create: scene shape tables out of range (n_static, n_rbox, brick / static compounds)"; return SDX_ERR_INVALID; }
    // the warm start's contact age is a 4-bit saturating counter in the cache key (k_physics solve()): a ramp longer than 16 solves would never end
    if (!(scene->warm_age >= 0.0f && scene->warm_age <= 16.0f)) { g_create_err = "sdx_create: warm_age must lie in [0, 16] (the contact age saturates at 16 solves)"; return SDX_ERR_INVALID; }
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
    g_create_err = "sdx_create: no HIP device visible; libseqdex_hip has no CPU fallback";
    return SDX_ERR_NO_DEVICE;
  }
  if (device < 0 || device >= ndev) { g_create_err = "sdx_create: bad device index"; return SDX_ERR_INVALID; }
  sdx_sim* h = new sdx_sim();
  h->device = device;
  sdx_sim* none = nullptr;
  (void)none;
  HIPCHK(h, hipSetDevice(device));
  const int N = num_envs;
  // ---- constants + derived tables
  SdxConst& K = h->h_const;
  sdx_build_const(scene, &K);
  int rc;
  if ((rc = dalloc(h, &h->d_const, 1)) != SDX_OK) { g_create_err = h->err; delete h; return rc; }
  HIPCHK(h, hipMemcpy(h->d_const, &K, sizeof(K), hipMemcpyHostToDevice));

  // ---- buffers
  SdxBuf& B = h->buf;
  memset(&B, 0, sizeof(B));
  B.N = N;
  B.task_kind = scene->task_kind;
  B.orient_gate = scene->orient_tvalue_gate;
  B.obs_w = task_obs_width(scene->task_kind);
  B.K = 1;
  B.seed = seed;
#define ALLOC(field, count) if ((rc = dalloc(h, &B.field, (size_t)(count))) != SDX_OK) { g_create_err = h->err; sdx_destroy(h); return rc; }
  ALLOC(root, (size_t)N * SDX_ACTORS * 13);
  ALLOC(dof, (size_t)N * SDX_NDOF * 2);
  ALLOC(rb, (size_t)N * SDX_BODIES * 13);
  ALLOC(contact, (size_t)N * SDX_BODIES * 3);
  ALLOC(jac, (size_t)N * 42);
  ALLOC(jac_full, (size_t)N * (SDX_NLINK - 1) * 6 * SDX_NDOF);
  ALLOC(targets, (size_t)N * SDX_NDOF);
  ALLOC(prev_targets, (size_t)N * SDX_NDOF);
  ALLOC(obs, (size_t)N * SDX_NUM_OBS);
  ALLOC(states, (size_t)N * SDX_NUM_STATES);
  ALLOC(obs_c, (size_t)N * SDX_NUM_OBS);
  ALLOC(states_c, (size_t)N * SDX_NUM_STATES);
  ALLOC(rew, N);
  ALLOC(reset, N);
  ALLOC(progress, N);
  ALLOC(randomize, N);
  ALLOC(actions, (size_t)N * SDX_NDOF);
  ALLOC(init_pos, (size_t)N * 3);
  ALLOC(init_rot, (size_t)N * 4);
  ALLOC(successes, N);
  ALLOC(meta_rew, N);
  ALLOC(cons, 1);
  ALLOC(finger_dist, N);
  ALLOC(tvalue, N);
  ALLOC(arm_contacts, (size_t)N * 6);
  ALLOC(student_obs, (size_t)N * 30);
  ALLOC(success_buf, N);
  ALLOC(pile_choice, N);
  ALLOC(ncontacts, N);
  ALLOC(piles, (size_t)8 * SDX_NBRICK * 13);
  ALLOC(tv_w, SDX_TV_PARAMS);
  ALLOC(cam_rot, (size_t)N * 4);
  ALLOC(cscratch, 4);   // (contact rows now live in LDS / registers)
  ALLOC(stat, 4);
  ALLOC(step_count, 1);
  ALLOC(dbg, 64 + 2 * (size_t)N);
  { const char* de = getenv("SDX_DEBUG_ENV"); B.dbg_env = de ? atoi(de) : 0; }
  ALLOC(harvest_hand, (size_t)8 * SDX_HARVEST_SLOTS * SDX_NDOF * 2);
  ALLOC(harvest_obj, (size_t)8 * SDX_HARVEST_SLOTS * 13);
  ALLOC(harvest_count, 8);
  ALLOC(insert_aux, (size_t)N * 8);
  ALLOC(tv_succ, (size_t)SDX_TV_LOG_SLOTS * 4);
  ALLOC(tv_fail, (size_t)SDX_TV_LOG_SLOTS * 4);
  ALLOC(tv_count, 2);
  ALLOC(tv_key, (size_t)2 * SDX_TV_LOG_SLOTS);
  ALLOC(harvest_key, (size_t)8 * SDX_HARVEST_SLOTS);
  B.pile_slots = task_pile_slots(scene->task_kind);
  ALLOC(pile_harvest, (size_t)8 * B.pile_slots * SDX_NBRICK * 13);
  ALLOC(pile_harvest_count, 8);
  ALLOC(pile_key, (size_t)8 * B.pile_slots);
  ALLOC(seg_stats, (size_t)N * 4);
  ALLOC(seg_image, scene->task_kind == SDX_TASK_SEARCH ? (size_t)N * 128 * 128 : 1);
  ALLOC(seg_pix, (size_t)N * 4);
  ALLOC(emergence, N);
  ALLOC(cstats, 4);
  ALLOC(order, N);
  ALLOC(cost, N);
  { std::vector<int32_t> iota((size_t)N); for (int i = 0; i < N; ++i) iota[i] = i; HIPCHK(h, hipMemcpy(B.order, iota.data(), (size_t)N * sizeof(int32_t), hipMemcpyHostToDevice)); }
  ALLOC(wcount, N);
  // the solver's impulse cache (24.5 KB per env) only exists when the scene asks for the warm start; k_physics<.., false> never reads it
  ALLOC(wkey, scene->warm_start > 0.0f ? (size_t)N * SDX_MAXC : 1);
  ALLOC(wlam, scene->warm_start > 0.0f ? (size_t)N * 3 * SDX_MAXC : 1);
  ALLOC(dr_dof, (size_t)N * 4 * SDX_NDOF);
  ALLOC(dr_link, (size_t)N * 2 * SDX_NLINK);
  ALLOC(dr_brick, (size_t)N * 2 * SDX_NFREE);
  ALLOC(dr_grav, 3);
  ALLOC(dr_frame, 2);
  ALLOC(dr_draw, (size_t)N + 1);
  B.dr_on = nullptr;
  if (scene->task_kind == SDX_TASK_SEARCH) {
    ALLOC(tvt_buf, (size_t)N * 652);
    ALLOC(tvt_w, (size_t)1024 * 652 + 1024 + 512 * 1024 + 512 + 128 * 512 + 128 + 2 * 128 + 2);
    ALLOC(tvt_h, (size_t)N * (1024 + 512 + 128 + 4));
  }
#undef ALLOC
  if ((rc = dalloc(h, &h->act_pre, (size_t)N * SDX_NDOF)) != SDX_OK) { g_create_err = h->err; sdx_destroy(h); return rc; }
  set_tensor(h, SDX_T_ROOT, B.root, SDX_F32, {(int64_t)N * SDX_ACTORS, 13});
  set_tensor(h, SDX_T_DOF, B.dof, SDX_F32, {(int64_t)N * SDX_NDOF, 2});
  set_tensor(h, SDX_T_RB, B.rb, SDX_F32, {N, SDX_BODIES, 13});
  set_tensor(h, SDX_T_CONTACT, B.contact, SDX_F32, {N, SDX_BODIES * 3});
  set_tensor(h, SDX_T_JAC_EEF, B.jac, SDX_F32, {N, 6, 7});
  set_tensor(h, SDX_T_TARGETS, B.targets, SDX_F32, {N, SDX_NDOF});
  set_tensor(h, SDX_T_PREV_TARGETS, B.prev_targets, SDX_F32, {N, SDX_NDOF});
  set_tensor(h, SDX_T_OBS, B.obs, SDX_F32, {N, B.obs_w});
  set_tensor(h, SDX_T_STATES, B.states, SDX_F32, {N, SDX_NUM_STATES});
  set_tensor(h, SDX_T_OBS_CLAMPED, B.obs_c, SDX_F32, {N, B.obs_w});
  set_tensor(h, SDX_T_STATES_CLAMPED, B.states_c, SDX_F32, {N, SDX_NUM_STATES});
  set_tensor(h, SDX_T_REW, B.rew, SDX_F32, {N});
  set_tensor(h, SDX_T_RESET, B.reset, SDX_I64, {N});
  set_tensor(h, SDX_T_PROGRESS, B.progress, SDX_I64, {N});
  set_tensor(h, SDX_T_RANDOMIZE, B.randomize, SDX_I64, {N});
  set_tensor(h, SDX_T_ACTIONS, B.actions, SDX_F32, {N, SDX_NDOF});
  set_tensor(h, SDX_T_INIT_POS, B.init_pos, SDX_F32, {N, 3});
  set_tensor(h, SDX_T_INIT_ROT, B.init_rot, SDX_F32, {N, 4});
  set_tensor(h, SDX_T_SUCCESSES, B.successes, SDX_F32, {N});
  set_tensor(h, SDX_T_META_REW, B.meta_rew, SDX_F32, {N});
  set_tensor(h, SDX_T_CONS_SUCCESSES, B.cons, SDX_F32, {1});
  set_tensor(h, SDX_T_FINGER_DIST, B.finger_dist, SDX_F32, {N});
  set_tensor(h, SDX_T_TVALUE, B.tvalue, SDX_F32, {N});
  set_tensor(h, SDX_T_ARM_CONTACTS, B.arm_contacts, SDX_F32, {N, 6});
  set_tensor(h, SDX_T_STUDENT_OBS, B.student_obs, SDX_F32, {N, 30});
  set_tensor(h, SDX_T_SUCCESS_BUF, B.success_buf, SDX_I64, {N});
  set_tensor(h, SDX_T_PILE_CHOICE, B.pile_choice, SDX_I32, {N});
  set_tensor(h, SDX_T_NCONTACTS, B.ncontacts, SDX_I32, {N});
  set_tensor(h, SDX_T_DEBUG, B.dbg, SDX_I64, {64 + 2 * (int64_t)N});
  set_tensor(h, SDX_T_HARVEST_HAND, B.harvest_hand, SDX_F32, {8, SDX_HARVEST_SLOTS, SDX_NDOF, 2});
  set_tensor(h, SDX_T_HARVEST_OBJ, B.harvest_obj, SDX_F32, {8, SDX_HARVEST_SLOTS, 13});
  set_tensor(h, SDX_T_HARVEST_COUNT, B.harvest_count, SDX_I32, {8});
  set_tensor(h, SDX_T_INSERT_AUX, B.insert_aux, SDX_F32, {N, 8});
  set_tensor(h, SDX_T_TV_SUCCESS, B.tv_succ, SDX_F32, {SDX_TV_LOG_SLOTS, 4});
  set_tensor(h, SDX_T_TV_FAILURE, B.tv_fail, SDX_F32, {SDX_TV_LOG_SLOTS, 4});
  set_tensor(h, SDX_T_TV_COUNT, B.tv_count, SDX_I32, {2});
  set_tensor(h, SDX_T_PILE_HARVEST, B.pile_harvest, SDX_F32, {8, B.pile_slots, SDX_NBRICK, 13});
  set_tensor(h, SDX_T_PILE_HARVEST_COUNT, B.pile_harvest_count, SDX_I32, {8});
  set_tensor(h, SDX_T_TV_KEYS, B.tv_key, SDX_I64, {2, SDX_TV_LOG_SLOTS});
  set_tensor(h, SDX_T_HARVEST_KEYS, B.harvest_key, SDX_I64, {8, SDX_HARVEST_SLOTS});
  set_tensor(h, SDX_T_PILE_HARVEST_KEYS, B.pile_key, SDX_I64, {8, B.pile_slots});
  if (scene->task_kind == SDX_TASK_SEARCH) set_tensor(h, SDX_T_SEG_IMAGE, B.seg_image, SDX_I16, {N, 128, 128});
  else set_tensor(h, SDX_T_SEG_IMAGE, B.seg_image, SDX_I16, {1, 1, 1});   // placeholder: the camera belongs to Search
  set_tensor(h, SDX_T_SEG_PIXELS, B.seg_pix, SDX_F32, {N, 4});
  set_tensor(h, SDX_T_EMERGENCE, B.emergence, SDX_F32, {N});
  set_tensor(h, SDX_T_CONTACT_STATS, B.cstats, SDX_I32, {4});
  set_tensor(h, SDX_T_WARM_COUNT, B.wcount, SDX_I32, {N});
  if (scene->warm_start > 0.0f) {
    set_tensor(h, SDX_T_WARM_KEYS, B.wkey, SDX_I32, {N, SDX_MAXC});
    set_tensor(h, SDX_T_WARM_LAMBDA, B.wlam, SDX_F32, {N, 3, SDX_MAXC});
  } else {
    set_tensor(h, SDX_T_WARM_KEYS, B.wkey, SDX_I32, {1});
    set_tensor(h, SDX_T_WARM_LAMBDA, B.wlam, SDX_F32, {1});
  }
  set_tensor(h, SDX_T_CAM_ROT, B.cam_rot, SDX_F32, {N, 4});
  set_tensor(h, SDX_T_DR_DOF, B.dr_dof, SDX_F32, {N, 4, SDX_NDOF});
  set_tensor(h, SDX_T_DR_LINK, B.dr_link, SDX_F32, {N, 2, SDX_NLINK});
  set_tensor(h, SDX_T_DR_BRICK, B.dr_brick, SDX_F32, {N, 2, SDX_NFREE});
  set_tensor(h, SDX_T_DR_GRAVITY, B.dr_grav, SDX_F32, {3});
  set_tensor(h, SDX_T_DR_FRAME, B.dr_frame, SDX_I64, {2});
  set_tensor(h, SDX_T_JACOBIAN, B.jac_full, SDX_F32, {N, SDX_NLINK - 1, 6, SDX_NDOF});
  if (scene->task_kind == SDX_TASK_SEARCH) set_tensor(h, SDX_T_TVALUE_OBS, B.tvt_buf, SDX_F32, {N, 652});
  else set_tensor(h, SDX_T_TVALUE_OBS, B.seg_pix, SDX_F32, {1, 1});   // placeholder: the temporal buffer belongs to Search

  // ---- initial actor states (what create_actor's start poses give, GS:897-1000)
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
  {  // default saved piles: K=1, the spawn lattice for every type group (replaced by sdx_load_initial_states)
    std::vector<float> p8;
    for (int t = 0; t < 8; ++t) p8.insert(p8.end(), pile0.begin(), pile0.end());
    HIPCHK(h, hipMemcpy(B.piles, p8.data(), p8.size() * 4, hipMemcpyHostToDevice));
  }
  {
    std::vector<int64_t> ones(N, 1);  // reset_buf = ONES: every env resets on the first step (BT:63)
    HIPCHK(h, hipMemcpy(B.reset, ones.data(), (size_t)N * 8, hipMemcpyHostToDevice));
  }
  if ((rc = state_table_build(h)) != SDX_OK) { g_create_err = h->err; sdx_destroy(h); return rc; }
  hipLaunchKernelGGL(k_dr_defaults, dim3(N), dim3(128), 0, 0, h->d_const, B);   // the randomization rows hold the scene's values
  sdxk_kinematics(h->d_const, &h->buf, 0);  // first refresh (GS:243-246)
  HIPCHK(h, hipDeviceSynchronize());
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
  h->has_piles = true;
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
    hipLaunchKernelGGL(k_dr_defaults, dim3(h->buf.N), dim3(128), 0, st, h->d_const, h->buf);
    return check_launch(h, "sdx_set_randomization");
  }
  const sdx_dr_attr* at[9] = {&desc->gravity, &desc->dof_stiffness, &desc->dof_damping, &desc->dof_lower, &desc->dof_upper,
                              &desc->link_mass, &desc->link_friction, &desc->brick_mass, &desc->brick_friction};
  bool ok = desc->frequency >= 1;
  for (int i = 0; i < 9; ++i) ok = ok && dr_attr_ok(*at[i]);
  if (!ok) { h->err = "sdx_set_randomization: bad desc (frequency >= 1, known distribution / operation / schedule, schedule_steps > 0, finite ranges)"; return SDX_ERR_INVALID; }
  h->dr = *desc;
  h->buf.dr_on = h->buf.dr_draw;
  dr_sample(h, 1, st);
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

extern "C" int sdx_pre_physics(sdx_handle h, const float* actions_dev, void* stream) {
  if (!h || !actions_dev) return SDX_ERR_INVALID;
  int flags = 1 | 4;
  const float* act = noise_actions(h, actions_dev, &flags, (hipStream_t)stream);
  if (h->buf.dr_on) dr_sample(h, 0, (hipStream_t)stream);   // before this step's resets (BT:229-260 runs inside reset_idx)
  sdxk_pre_physics(h->d_const, &h->buf, act, nullptr, nullptr, flags, (hipStream_t)stream);
  return check_launch(h, "sdx_pre_physics");
}
extern "C" int sdx_simulate(sdx_handle h, void* stream) {
  if (!h) return SDX_ERR_INVALID;
  sdxk_physics(h->d_const, &h->buf, (hipStream_t)stream);
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

extern "C" void sdxk_search_set_hand(const SdxConst*, const SdxBuf*, const uint8_t*, int, hipStream_t);

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
  if (h->buf.dr_on) dr_sample(h, 0, st);   // before any reset physics of this step, Orient's / Search's settling launches included
  if (h->h_const.sc.task_kind == SDX_TASK_SEARCH) {
    int64_t p0 = 0;
    const int rc = search_reset_if_needed(h, st, &p0);
    if (rc != SDX_OK) return rc;
    sdxk_pre_physics(h->d_const, &h->buf, act, nullptr, nullptr, targets, st);
    sdxk_physics(h->d_const, &h->buf, st);
    if ((float)(p0 + 1) >= h->h_const.sc.max_episode_length - 1.0f) {                  // SE:992-1019: park the hand, one more step, render
      sdxk_search_set_hand(h->d_const, &h->buf, nullptr, 1, st);
      sdxk_physics(h->d_const, &h->buf, st);
      sdxk_seg_camera(h->d_const, &h->buf, st);
    }
    post_physics_step(h, st);
    return check_launch(h, "sdx_step");
  }
  if (h->h_const.sc.task_kind == SDX_TASK_ORIENT) {
    const int rc = orient_reset_if_needed(h, st);
    if (rc != SDX_OK) return rc;
    sdxk_pre_physics(h->d_const, &h->buf, act, nullptr, nullptr, targets, st);
    sdxk_physics(h->d_const, &h->buf, st);
    post_physics_step(h, st);
    return check_launch(h, "sdx_step");
  }
  sdxk_pre_physics(h->d_const, &h->buf, act, nullptr, nullptr, 1 | targets, st);
  sdxk_physics(h->d_const, &h->buf, st);   // controlFrequencyInv = 1 (EG:18)
  post_physics_step(h, st);
  return check_launch(h, "sdx_step");
}
// Not part of include/seqdex.h: the scripted stand-in for a trained grasp policy that the chain benchmark and its tests drive the grasp
// stage with (seqdex_amd/scripts/evaluation.py), as one launch instead of ~40 torch operations per env step.
extern "C" void sdxk_scripted_grasp(const SdxConst*, const SdxBuf*, float*, float*, hipStream_t);
extern "C" int sdxk_scripted_grasp_actions(sdx_handle h, float* close_state_dev, float* actions_out_dev, void* stream) {
  if (!h || !close_state_dev || !actions_out_dev) return SDX_ERR_INVALID;
  sdxk_scripted_grasp(h->d_const, &h->buf, close_state_dev, actions_out_dev, (hipStream_t)stream);
  return check_launch(h, "sdxk_scripted_grasp_actions");
}
extern "C" int sdx_reset_idx(sdx_handle h, const uint8_t* env_mask_dev, const int32_t* pile_choice_dev, void* stream) {
  if (!h || !env_mask_dev) return SDX_ERR_INVALID;
  if (h->buf.dr_on) dr_sample(h, 0, (hipStream_t)stream, env_mask_dev);   // reset_idx -> apply_randomizations (GS:1395-1396)
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
// one thread per (listed actor, column)
// src may BE the library's own tensor (the documented use: edit SDX_T_ROOT / SDX_T_DOF in place, then name the rows that changed): no __restrict__ on it
__global__ void k_set_indexed(SdxBuf B, int id, const float* src, const int32_t* __restrict__ ids, int n) {
  const int i = blockIdx.x, t = threadIdx.x;
  if (i >= n) return;
  const int actor = ids[i];
  if (actor < 0 || actor >= B.N * SDX_ACTORS) return;
  const int e = actor / SDX_ACTORS, slot = actor % SDX_ACTORS;
  if (id == SDX_T_ROOT) {
    if (slot == 0 || t >= 13) return;                       // the hand actor has a fixed base: its root state is not settable
    const float v = src[(size_t)actor * 13 + t];
    B.root[(size_t)actor * 13 + t] = v;
    B.rb[((size_t)e * SDX_BODIES + SDX_NLINK + slot - 1) * 13 + t] = v;
    if (t == 0) B.wcount[e] = 0;                            // a teleported body invalidates the env's cached contact impulses (warm start)
  } else if (slot == 0) {
    if (id == SDX_T_DOF) { if (t < SDX_NDOF * 2) B.dof[(size_t)e * SDX_NDOF * 2 + t] = src[(size_t)e * SDX_NDOF * 2 + t]; }
    else if (t < SDX_NDOF) B.targets[(size_t)e * SDX_NDOF + t] = src[(size_t)e * SDX_NDOF + t];
  }
}
extern "C" int sdx_set_indexed(sdx_handle h, int32_t id, const float* src_dev, const int32_t* actor_ids_dev, int32_t n, void* stream) {
  if (!h) return SDX_ERR_INVALID;
  if (!src_dev || !actor_ids_dev || n < 0 || (id != SDX_T_ROOT && id != SDX_T_DOF && id != SDX_T_TARGETS)) {
    h->err = "sdx_set_indexed: id must be SDX_T_ROOT, SDX_T_DOF or SDX_T_TARGETS, src / ids non-NULL"; return SDX_ERR_INVALID;
  }
  hipStream_t st = (hipStream_t)stream;
  if (n > 0) hipLaunchKernelGGL(k_set_indexed, dim3(n), dim3(64), 0, st, h->buf, id, src_dev, actor_ids_dev, n);
  if (id == SDX_T_DOF && n > 0) sdxk_kinematics(h->d_const, &h->buf, st);
  return check_launch(h, "sdx_set_indexed");
}
extern "C" int sdx_num_envs(sdx_handle h) { return h ? h->buf.N : SDX_ERR_INVALID; }
extern "C" const char* sdx_last_error(sdx_handle h) { return h ? h->err.c_str() : g_create_err.c_str(); }
