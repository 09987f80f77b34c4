// sdx_randomize.hip — the samplers of domain randomization and of observation / action noise (include/seqdex.h sdx_set_randomization,
// sdx_set_noise) and of the random pushes on the target brick (sdx_set_force_perturbation; section 21): kernels with
// pinned numerics and their launchers.  Argument checks and call order: sdx_capi.hip.
#include "sdx_kernels.h"

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
extern "C" void sdxk_dr_defaults(const SdxConst* C, const SdxBuf* B, hipStream_t st) {
  hipLaunchKernelGGL(k_dr_defaults, dim3(B->N), dim3(128), 0, st, C, *B);
}
extern "C" void sdxk_dr_sample(const SdxConst* C, const SdxBuf* B, const sdx_dr_desc* desc, int first, const uint8_t* mask, hipStream_t st) {
  hipLaunchKernelGGL(k_dr_gravity, dim3(1), dim3(256), 0, st, C, *B, *desc, first, mask);
  hipLaunchKernelGGL(k_dr_sample, dim3(B->N), dim3(128), 0, st, C, *B, *desc, first, mask);
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
extern "C" void sdxk_noise(const SdxConst* C, const SdxBuf* B, const sdx_noise_attr* attr, const float* src, float* dst, int W, int act, hipStream_t st) {
  const long long threads = (long long)B->N * ((W + 3) / 4);
  hipLaunchKernelGGL(k_noise, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, st, C, *B, *attr, src, dst, W, act);
}

// ---------------------------------------------------------------- random pushes on the target brick (include/seqdex.h
// sdx_set_force_perturbation): the reference's rule (morb.py:1495-1516) on the caller's rb_forces [N, SDX_BODIES, 3] and
// prob [N].  Stateless draws: sdx_hash(seed ^ SDX_FORCE_TAG, env * 256 + slot, step_count); slot 0 the push decision, 1 z_x / z_y, 2 z_z,
// 3 the probability.
#define SDX_FORCE_TAG 0xF0CEull
#define SDX_FORCE_ROW (SDX_BODIES * 3)
__device__ __forceinline__ uint64_t force_hash(uint64_t seed, int e, int slot, uint64_t step) {
  return sdx_hash(seed ^ SDX_FORCE_TAG, (uint64_t)e * 256 + (uint64_t)slot, step);
}
// exp((log lo - log hi) u + log hi) (GS:1519-1520), in double, rounded once
__device__ __forceinline__ float force_prob(const sdx_force_perturb_attr& a, uint64_t seed, int e, uint64_t step) {
#pragma clang fp contract(off)
  const double llo = log((double)a.prob_lo), lhi = log((double)a.prob_hi);
  const double t = (llo - lhi) * (double)dr_u(force_hash(seed, e, 3, step), 0);
  return (float)exp(t + lhi);
}
// One thread per group of 4 consecutive floats of the flat tensor (a group may span two envs: 495 floats per env): one 16-byte load and
// store per thread, the last group of an N x 495 that is no multiple of 4 goes float by float.  Per element, in the rule's order: reset
// (-> 0), decay (x factor), push (the three elements of the target brick's row: the decision is the same hash for all three).  The
// element (e, 0) also writes prob[e] when env e draws a new one; only envs that do NOT draw read prob[e].
__global__ __launch_bounds__(256) void k_force_perturb(const SdxConst* __restrict__ C, SdxBuf B, sdx_force_perturb_attr a, float factor,
                                                       float* __restrict__ F, float* __restrict__ prob, const uint8_t* __restrict__ mask, int mode) {
#pragma clang fp contract(off)
  const long long total = (long long)B.N * SDX_FORCE_ROW;
  const long long i0 = ((long long)blockIdx.x * 256 + threadIdx.x) * 4;
  if (i0 >= total) return;
  const int n = total - i0 < 4 ? (int)(total - i0) : 4;
  const uint64_t step = (uint64_t)B.step_count[0];
  const sdx_scene_desc& sc = C->sc;
  float x[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  if (mode != SDX_FP_DRAW) {
    if (n == 4) {
      const f4v v = *reinterpret_cast<const f4v*>(F + i0);
      x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w;
    } else {
      for (int k = 0; k < n; ++k) x[k] = F[i0 + k];
    }
  }
  for (int k = 0; k < n; ++k) {
    const int e = (int)((i0 + k) / SDX_FORCE_ROW), c = (int)((i0 + k) - (long long)e * SDX_FORCE_ROW);
    const bool reset = mode == SDX_FP_STEP ? B.reset[e] != 0 : (mode == SDX_FP_RESET && (mask ? mask[e] != 0 : true));
    if (reset) x[k] = 0.0f;
    if (mode == SDX_FP_STEP) {
      x[k] *= factor;
      const int segb = seg_actor(e) - SDX_ACTOR_BRICK0;
      if (c / 3 == SDX_BODY_BRICK0 + segb) {
        const float p = reset ? force_prob(a, B.seed, e, step) : prob[e];
        if (dr_u(force_hash(B.seed, e, 0, step), 0) < p) {
          const int r = c % 3;
          const float z = noise_normal(force_hash(B.seed, e, r < 2 ? 1 : 2, step), r == 1);
          float m = sc.brick_mass[sc.brick_type[segb]] * sc.seg_mass_scale;   // the mass k_physics gives this brick (load_constants)
          if (B.dr_on) m *= B.dr_brick[(size_t)e * 2 * SDX_NFREE + segb];
          x[k] = z * m * a.force_scale;
        }
      }
    }
    if (c == 0 && (reset || mode == SDX_FP_DRAW)) prob[e] = force_prob(a, B.seed, e, step);
  }
  if (mode == SDX_FP_DRAW) return;
  if (n == 4) {
    f4v v;
    v.x = x[0]; v.y = x[1]; v.z = x[2]; v.w = x[3];
    *reinterpret_cast<f4v*>(F + i0) = v;
  } else {
    for (int k = 0; k < n; ++k) F[i0 + k] = x[k];
  }
}
extern "C" void sdxk_force_perturb(const SdxConst* C, const SdxBuf* B, const sdx_force_perturb_attr* attr, float factor, float* rb_forces, float* prob,
                                   const uint8_t* mask, int mode, hipStream_t st) {
  const long long groups = ((long long)B->N * SDX_FORCE_ROW + 3) / 4;
  hipLaunchKernelGGL(k_force_perturb, dim3((unsigned)((groups + 255) / 256)), dim3(256), 0, st, C, *B, *attr, factor, rb_forces, prob, mask, mode);
}
