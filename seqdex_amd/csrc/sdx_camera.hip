// sdx_camera.hip — segmentation "camera" of BlockAssemblySearch (SE = tasks/block_assembly/allegro_hand_block_assembly_search.py).
// The reference renders IMAGE_SEGMENTATION with Isaac Gym's camera sensor (128 x 128, fixed pose, SE:755-757,873-878) and uses only two
// things of the image: how many pixels carry the target brick's segmentation id and where their centroid is (SE:1232-1241,1640-1646).
// Here the image is ray-cast against the scene's boxes (bricks = their bounding boxes with segmentation id brick index + 1 (SE:840),
// table / bin / robot = id 0): one thread per pixel, boxes of the env staged in LDS as (centre, rotation matrix, half extents, ray
// origin in the box frame), nearest hit wins.  Box geometry instead of the studded meshes is the approximation of this whole build
// (DESIGN.md section 3); the pixel counts are therefore NOT comparable digit by digit with Isaac Gym's renderer (parity unpinned) -
// the kernel is checked against oracle/camera_oracle.py, a numpy ray caster of the same boxes.
#include "sdx_kernels.h"   // (includes sdx_common.h)

#define CAM_W 128
#define CAM_H 128
#define CAM_MAXBOX (SDX_NBRICK + SDX_MAX_STATIC + SDX_MAX_RBOX)

struct CamBox { float c[3]; float m[9]; float h[3]; float o[3]; int id; };   // m: rows = box axes in world coordinates; o = ray origin in the box frame

__device__ __forceinline__ void quat_rows(f4 q, float* m) {
  const f3 x = qrot(q, F3(1, 0, 0)), y = qrot(q, F3(0, 1, 0)), z = qrot(q, F3(0, 0, 1));
  m[0] = x.x; m[1] = x.y; m[2] = x.z; m[3] = y.x; m[4] = y.y; m[5] = y.z; m[6] = z.x; m[7] = z.y; m[8] = z.z;
}

// grid (CAM_H * CAM_W / 256, N); stats[e] = {count, sum of rows, sum of columns, 0} of the pixels showing the target brick
__global__ __launch_bounds__(256) void k_seg_camera(const SdxConst* __restrict__ C, SdxBuf B, int32_t* __restrict__ stats, int16_t* __restrict__ image) {
  __shared__ CamBox s_box[CAM_MAXBOX];
  __shared__ int s_acc[3];
  const sdx_scene_desc& sc = C->sc;
  const int e = blockIdx.y, tid = threadIdx.x;
  const float* root_e = B.root + (size_t)e * SDX_ACTORS * 13;
  const float* rb_e = B.rb + (size_t)e * SDX_BODIES * 13;
  const int ns = sc.n_static, nr = sc.n_rbox, nbox = SDX_NBRICK + ns + nr;
  const f3 cam = ld3(sc.seg_cam_pos);
  for (int i = tid; i < nbox; i += 256) {
    CamBox& b = s_box[i];
    f3 c, h;
    f4 q = {0.0f, 0.0f, 0.0f, 1.0f};
    int id = 0;
    if (i < SDX_NBRICK) {
      const float* r = root_e + (SDX_ACTOR_BRICK0 + i) * 13;
      const int t = sc.brick_type[i];
      q = ld4(r + 3);
      c = ld3(r) + qrot(q, ld3(sc.brick_center[t]));
      h = ld3(sc.brick_half[t]);
      id = i + 1;                                                               // segmentationId = lego_i + 1, SE:840
    } else if (i < SDX_NBRICK + ns) {
      c = ld3(sc.static_center[i - SDX_NBRICK]); h = ld3(sc.static_half[i - SDX_NBRICK]);
    } else {
      const int k = i - SDX_NBRICK - ns, l = sc.rbox_link[k];
      const f4 ql = ld4(rb_e + l * 13 + 3);
      c = ld3(rb_e + l * 13) + qrot(ql, ld3(sc.rbox_center[k]));
      q = qmul(ql, ld4(sc.rbox_quat[k]));
      h = ld3(sc.rbox_half[k]);
    }
    b.c[0] = c.x; b.c[1] = c.y; b.c[2] = c.z;
    quat_rows(q, b.m);
    b.h[0] = h.x; b.h[1] = h.y; b.h[2] = h.z;
    const f3 d = cam - c;
    b.o[0] = b.m[0] * d.x + b.m[1] * d.y + b.m[2] * d.z;
    b.o[1] = b.m[3] * d.x + b.m[4] * d.y + b.m[5] * d.z;
    b.o[2] = b.m[6] * d.x + b.m[7] * d.y + b.m[8] * d.z;
    b.id = id;
  }
  if (tid < 3) s_acc[tid] = 0;
  __syncthreads();
  // pinhole camera looking from seg_cam_pos at seg_cam_target, world z up; row 0 is the top of the image
  const f3 tgt = ld3(sc.seg_cam_target);
  f3 f = tgt - cam;
  f = f * (1.0f / sqrtf(dot(f, f)));
  f3 r = cross(f, F3(0.0f, 0.0f, 1.0f));
  r = r * (1.0f / sqrtf(dot(r, r)));
  const f3 u = cross(r, f);
  const float th = tanf(0.5f * sc.seg_cam_hfov_deg * 0.017453292519943295f);
  const int pix = blockIdx.x * 256 + tid, row = pix / CAM_W, col = pix % CAM_W;
  const float px = (2.0f * ((float)col + 0.5f) / (float)CAM_W - 1.0f) * th;
  const float py = (1.0f - 2.0f * ((float)row + 0.5f) / (float)CAM_H) * th;    // square image: the vertical extent equals the horizontal one
  const f3 d = f + r * px + u * py;
  float best = 3.0e38f;
  int best_id = 0;
  for (int i = 0; i < nbox; ++i) {
    const CamBox& b = s_box[i];
    float tmin = 0.0f, tmax = 3.0e38f;
    bool hit = true;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const float da = b.m[3 * a] * d.x + b.m[3 * a + 1] * d.y + b.m[3 * a + 2] * d.z;
      const float oa = b.o[a], ha = b.h[a];
      if (fabsf(da) < 1e-12f) { if (fabsf(oa) > ha) hit = false; }
      else {
        const float inv = 1.0f / da;
        float t0 = (-ha - oa) * inv, t1 = (ha - oa) * inv;
        if (t0 > t1) { const float tt = t0; t0 = t1; t1 = tt; }
        tmin = fmaxf(tmin, t0); tmax = fminf(tmax, t1);
      }
    }
    if (hit && tmin <= tmax && tmin < best) { best = tmin; best_id = b.id; }
  }
  if (image) image[((size_t)e * CAM_H + row) * CAM_W + col] = (int16_t)best_id;
  const int target = seg_actor(e) - SDX_ACTOR_BRICK0 + 1;                       // segmentation_id_list[i], SE:846-847
  if (best_id == target) { atomicAdd(&s_acc[0], 1); atomicAdd(&s_acc[1], row); atomicAdd(&s_acc[2], col); }
  __syncthreads();
  if (tid < 3 && s_acc[tid]) atomicAdd(&stats[(size_t)e * 4 + tid], s_acc[tid]);
}

// pixel statistics (SE:1232-1241) and the emergence reward (SE:1640-1646) from the accumulated sums
__global__ void k_seg_finalize(SdxBuf B, const int32_t* __restrict__ stats) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= B.N) return;
  const int n = stats[(size_t)e * 4];
  int cx = 0, cy = 0;
  if (n > 0) { cx = (int)((float)stats[(size_t)e * 4 + 1] / (float)n); cy = (int)((float)stats[(size_t)e * 4 + 2] / (float)n); }
  B.seg_pix[(size_t)e * 4 + 0] = (float)n;
  B.seg_pix[(size_t)e * 4 + 1] = (float)cx;
  B.seg_pix[(size_t)e * 4 + 2] = (float)cy;
  const float last = B.seg_pix[(size_t)e * 4 + 3];
  B.emergence[e] = ((float)n - last) * 5.0f;                                    // SE:1645
  B.seg_pix[(size_t)e * 4 + 3] = (float)n;                                      // last_emergence_pixel, SE:1646
}

extern "C" void sdxk_seg_camera(const SdxConst* C, const SdxBuf* B, hipStream_t st) {
  (void)hipMemsetAsync(B->seg_stats, 0, (size_t)B->N * 4 * sizeof(int32_t), st);
  hipLaunchKernelGGL(k_seg_camera, dim3(CAM_H * CAM_W / 256, B->N), dim3(256), 0, st, C, *B, B->seg_stats, B->seg_image);
  hipLaunchKernelGGL(k_seg_finalize, dim3((B->N + 255) / 256), dim3(256), 0, st, *B, B->seg_stats);
}

// ---------------------------------------------------------------- view camera (include/seqdex.h sdx_render_view)
// A general pinhole camera of k_seg_camera's model (any pose, any size, optionally riding on a robot link) that renders depth, labels
// and a shaded class colour of a list of envs, for looking at the engine: nothing in the step path launches it.
// One workgroup = one 16 x 16 pixel tile of one env.  Stage 1 (collective): every box of the env - bounding boxes (SDX_VIEW_BOUNDS, the
// boxes of k_seg_camera in its order) or the boxes k_physics collides (SDX_VIEW_COLLISION) - is placed by one lane, its bounding sphere
// is tested against the four side planes of the tile's pyramid and against "behind the camera", and the survivors are compacted into LDS
// in ASCENDING box order (ballot + prefix popcount per wave, waves in order): coplanar faces tie, and ties go to the lower box index as
// in the brute-force loop the result is defined by.  Stage 2: every pixel walks its tile's list only.
// The arithmetic of this section is not contracted into FMAs (the pragma holds to the end of the file; sdx_common.h's vector helpers were
// compiled before it, hence the v* copies): tests/helpers/view_oracle.py restates it operation by operation in numpy.
#pragma clang fp contract(off)
__device__ __forceinline__ f3 vadd(f3 a, f3 b) { return F3(a.x + b.x, a.y + b.y, a.z + b.z); }
__device__ __forceinline__ f3 vsub(f3 a, f3 b) { return F3(a.x - b.x, a.y - b.y, a.z - b.z); }
__device__ __forceinline__ f3 vscale(f3 a, float s) { return F3(a.x * s, a.y * s, a.z * s); }
__device__ __forceinline__ float vdot(f3 a, f3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ f3 vcross(f3 a, f3 b) { return F3(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x); }
__device__ __forceinline__ f3 vqrot(f4 q, f3 v) {
  const f3 u = F3(q.x, q.y, q.z), t = vscale(vcross(u, v), 2.0f);
  return vadd(vadd(v, vscale(t, q.w)), vcross(u, t));
}
__device__ __forceinline__ f4 vqmul(f4 a, f4 b) {
  f4 r;
  r.x = a.w * b.x + a.x * b.w + a.y * b.z - a.z * b.y;
  r.y = a.w * b.y - a.x * b.z + a.y * b.w + a.z * b.x;
  r.z = a.w * b.z + a.x * b.y - a.y * b.x + a.z * b.w;
  r.w = a.w * b.w - a.x * b.x - a.y * b.y - a.z * b.z;
  return r;
}
__device__ __forceinline__ void vquat_rows(f4 q, float* m) {
  const f3 x = vqrot(q, F3(1, 0, 0)), y = vqrot(q, F3(0, 1, 0)), z = vqrot(q, F3(0, 0, 1));
  m[0] = x.x; m[1] = x.y; m[2] = x.z; m[3] = y.x; m[4] = y.y; m[5] = y.z; m[6] = z.x; m[7] = z.y; m[8] = z.z;
}
#define VIEW_TILE 16
#define VIEW_MAX_STATIC_SEEN SDX_MAX_STATIC_SUB
#define VIEW_MAXBOX (SDX_NFREE * SDX_MAX_SUB + SDX_MAX_SUB_HOLLOW + (SDX_NBRICK - SDX_NFREE) + VIEW_MAX_STATIC_SEEN + SDX_MAX_RBOX)
// classes of the colour table: kept here, in this one place
enum { VC_BACKGROUND = 0, VC_TARGET = 1, VC_TYPE0 = 2, VC_FIXED = 10, VC_ARM = 11, VC_HAND = 12, VC_TABLE = 13, VC_BIN = 14, VC_FLOOR = 15, VC_PLATE = 16, VC_COUNT = 17 };
__constant__ float c_view_color[VC_COUNT][3] = {
    {24, 26, 32},                                                                                     // background
    {255, 48, 48},                                                                                    // the env's target brick
    {66, 135, 245}, {60, 180, 75}, {255, 225, 25}, {245, 130, 48}, {145, 30, 180}, {70, 240, 240}, {240, 50, 230}, {170, 110, 40},   // brick types 0..7
    {128, 128, 140},                                                                                  // fixed bricks
    {200, 200, 210}, {250, 190, 150},                                                                 // robot: arm links, hand links
    {120, 90, 60}, {90, 110, 130}, {150, 150, 120}, {0, 128, 128}};                                   // table, bin, floor slab, base plate

struct ViewParams {
  float pos[3], target[3], up[3];
  int32_t attach;          // -1 or a link
  float hfov_deg;
  int32_t W, H, geometry, n, tiles_x, tiles_y;
};
// a staged survivor: 20 words = 5 x 16 bytes (a lane-uniform row read is a broadcast ds_read_b128 each)
struct __attribute__((aligned(16))) ViewBox { float m[9]; float h[3]; float o[3]; int32_t label; int32_t cls; float pad[3]; };

// box i of env e in the chosen geometry: centre, orientation, half extents, label, class.  Returns false past the last box.
// BOUNDS:    132 brick bounding boxes, n_static static bounding boxes, n_rbox robot boxes.
// COLLISION: per brick (index order) its slabs / the hollow compound of the target / the bounding box of a fixed brick, then per static
//            slot its boxes (slot static_var_slot shows row static_var_row[e % 3]), then the robot boxes.
// The enumeration is a closed form of i (no prefix sums): free bricks have brick_nsub boxes EACH BY TYPE, so the index -> (brick, sub)
// map walks the 72 free bricks once; the lanes do it independently (<= 72 short iterations, once per tile).
__device__ __forceinline__ bool view_box(const sdx_scene_desc& sc, const float* root_e, const float* rb_e, int e, int geometry, int i,
                                         f3* c, f4* q, f3* h, int* label, int* cls) {
  const int segb = seg_actor(e) - SDX_ACTOR_BRICK0;
  const int ns = sc.n_static, nr = sc.n_rbox;
  f4 qq = {0.0f, 0.0f, 0.0f, 1.0f};
  int brick = -1, sub = -1, slot = -1, srow = 0, k = -1;    // which kind i is
  if (geometry == SDX_VIEW_BOUNDS) {
    if (i < SDX_NBRICK) brick = i;
    else if (i < SDX_NBRICK + ns) { slot = i - SDX_NBRICK; sub = -1; }
    else if (i < SDX_NBRICK + ns + nr) k = i - SDX_NBRICK - ns;
    else return false;
  } else {
    int j = i;
    for (int b = 0; b < SDX_NFREE && brick < 0; ++b) {
      const int nb = (sc.seg_hollow && b == segb) ? sc.hollow_nsub[sc.brick_type[b]] : sc.brick_nsub[sc.brick_type[b]];
      if (j < nb) { brick = b; sub = j; }
      else j -= nb;
    }
    if (brick < 0) {
      if (j < SDX_NBRICK - SDX_NFREE) brick = SDX_NFREE + j;
      else {
        j -= SDX_NBRICK - SDX_NFREE;
        for (int s = 0; s < ns && slot < 0; ++s) {
          const int row = s == sc.static_var_slot ? sc.static_var_row[e % 3] : s;
          const int nb = sc.static_sub_n[row];
          if (j < nb) { slot = s; srow = sc.static_sub_first[row] + j; sub = j; }
          else j -= nb;
        }
        if (slot < 0) {
          if (j < nr) k = j;
          else return false;
        }
      }
    }
  }
  if (brick >= 0) {
    const float* r = root_e + (SDX_ACTOR_BRICK0 + brick) * 13;
    const int t = sc.brick_type[brick];
    qq = ld4(r + 3);
    f3 off = ld3(sc.brick_center[t]), hh = ld3(sc.brick_half[t]);
    if (sub >= 0 && brick < SDX_NFREE) {
      const bool hol = sc.seg_hollow && brick == segb;
      off = hol ? ld3(sc.hollow_sub_center[t][sub]) : ld3(sc.brick_sub_center[t][sub]);
      hh = hol ? ld3(sc.hollow_sub_half[t][sub]) : ld3(sc.brick_sub_half[t][sub]);
    }
    *c = vadd(ld3(r), vqrot(qq, off));
    *h = hh;
    *label = brick + 1;                                                           // segmentationId = lego_i + 1, SE:840
    *cls = brick == segb ? VC_TARGET : (brick < SDX_NFREE ? VC_TYPE0 + t : VC_FIXED);
  } else if (slot >= 0) {
    if (sub < 0) { *c = ld3(sc.static_center[slot]); *h = ld3(sc.static_half[slot]); }
    else { *c = ld3(sc.static_sub_center[srow]); *h = ld3(sc.static_sub_half[srow]); }
    *label = -100 - slot;
    *cls = slot == 0 ? VC_TABLE : (slot < 6 ? VC_BIN : (slot == 6 ? VC_FLOOR : VC_PLATE));   // table, 5 bin boxes, merged brick floor, base plate
  } else {
    const int l = sc.rbox_link[k];
    const f4 ql = ld4(rb_e + l * 13 + 3);
    *c = vadd(ld3(rb_e + l * 13), vqrot(ql, ld3(sc.rbox_center[k])));
    qq = vqmul(ql, ld4(sc.rbox_quat[k]));
    *h = ld3(sc.rbox_half[k]);
    *label = -1 - l;
    *cls = l < sc.hand_base_body ? VC_ARM : VC_HAND;
  }
  *q = qq;
  return true;
}

// grid (tiles_x * tiles_y * n); any of depth / label / rgb may be nullptr.  An env id outside [0, N) leaves its images untouched.
__global__ __launch_bounds__(256) void k_view_render(const SdxConst* __restrict__ C, SdxBuf B, ViewParams P, const int32_t* __restrict__ env_ids,
                                                     float* __restrict__ depth, int16_t* __restrict__ label, uint8_t* __restrict__ rgb) {
  __shared__ ViewBox s_box[VIEW_MAXBOX];
  __shared__ int s_wcnt[(VIEW_MAXBOX + 255) / 256][4];
  const sdx_scene_desc& sc = C->sc;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int tiles = P.tiles_x * P.tiles_y;
  const int k_img = blockIdx.x / tiles, tile = blockIdx.x % tiles, ty = tile / P.tiles_x, tx = tile % P.tiles_x;
  const int e = env_ids[k_img];
  if (e < 0 || e >= B.N) return;                                                  // (uniform over the workgroup)
  const float* root_e = B.root + (size_t)e * SDX_ACTORS * 13;
  const float* rb_e = B.rb + (size_t)e * SDX_BODIES * 13;
  // the camera: k_seg_camera's model; pos / target / up are in the frame of link `attach` when attach >= 0
  f3 cam = ld3(P.pos), tgt = ld3(P.target), up = ld3(P.up);
  if (P.attach >= 0) {
    const f3 lp = ld3(rb_e + P.attach * 13);
    const f4 lq = ld4(rb_e + P.attach * 13 + 3);
    cam = vadd(lp, vqrot(lq, cam)); tgt = vadd(lp, vqrot(lq, tgt)); up = vqrot(lq, up);
  }
  f3 f = vsub(tgt, cam);
  f = vscale(f, 1.0f / sqrtf(vdot(f, f)));
  f3 r = vcross(f, up);
  r = vscale(r, 1.0f / sqrtf(vdot(r, r)));
  const f3 u = vcross(r, f);
  const float th = tanf(0.5f * P.hfov_deg * 0.017453292519943295f);
  const float tv = th * (float)P.H / (float)P.W;                                  // square pixels
  // the tile's pyramid: pixel centres of its first / last column and row, widened by half a pixel
  const float x_lo = (2.0f * (float)(tx * VIEW_TILE) / (float)P.W - 1.0f) * th, x_hi = (2.0f * (float)(tx * VIEW_TILE + VIEW_TILE) / (float)P.W - 1.0f) * th;
  const float y_hi = (1.0f - 2.0f * (float)(ty * VIEW_TILE) / (float)P.H) * tv, y_lo = (1.0f - 2.0f * (float)(ty * VIEW_TILE + VIEW_TILE) / (float)P.H) * tv;
  const float nx_lo = sqrtf(1.0f + x_lo * x_lo), nx_hi = sqrtf(1.0f + x_hi * x_hi), ny_lo = sqrtf(1.0f + y_lo * y_lo), ny_hi = sqrtf(1.0f + y_hi * y_hi);
  // ---- stage 1: place, cull, compact (every lane takes part, also those of an edge tile that lie outside the image)
  int total = 0;
  for (int chunk = 0; chunk < (VIEW_MAXBOX + 255) / 256; ++chunk) {
    const int i = chunk * 256 + tid;
    f3 c = F3(0, 0, 0), h = F3(0, 0, 0);
    f4 q = {0.0f, 0.0f, 0.0f, 1.0f};
    int lab = 0, cls = 0;
    bool keep = i < VIEW_MAXBOX && view_box(sc, root_e, rb_e, e, P.geometry, i, &c, &q, &h, &lab, &cls);
    float m[9];
    f3 o = F3(0, 0, 0);
    if (keep) {
      vquat_rows(q, m);
      const f3 d = vsub(cam, c);
      o.x = m[0] * d.x + m[1] * d.y + m[2] * d.z;
      o.y = m[3] * d.x + m[4] * d.y + m[5] * d.z;
      o.z = m[6] * d.x + m[7] * d.y + m[8] * d.z;
      // the bounding sphere in camera coordinates (x right, y up, z along the optical axis), 1e-4 R + 1e-5 m wider than it is: the
      // camera basis is orthonormal to fp32 rounding only
      const f3 g = vsub(c, cam);
      const float gx = vdot(g, r), gy = vdot(g, u), gz = vdot(g, f);
      const float R = sqrtf(vdot(h, h)) * 1.0001f + 1e-5f;
      const bool out = gz < -R || gx - x_lo * gz < -R * nx_lo || x_hi * gz - gx < -R * nx_hi || gy - y_lo * gz < -R * ny_lo || y_hi * gz - gy < -R * ny_hi;
      const bool inside = fabsf(o.x) < h.x && fabsf(o.y) < h.y && fabsf(o.z) < h.z;   // the wrist camera sits inside its own link's box
      keep = !out && !inside;
    }
    const unsigned long long mask = __ballot(keep);
    if (lane == 0) s_wcnt[chunk][wave] = __popcll(mask);
    __syncthreads();
    int at = total + __popcll(mask & ((1ull << lane) - 1ull));
    for (int w = 0; w < 4; ++w) { const int n = s_wcnt[chunk][w]; if (w < wave) at += n; total += n; }
    if (keep) {
      ViewBox& b = s_box[at];
#pragma unroll
      for (int a = 0; a < 9; ++a) b.m[a] = m[a];
      b.h[0] = h.x; b.h[1] = h.y; b.h[2] = h.z;
      b.o[0] = o.x; b.o[1] = o.y; b.o[2] = o.z;
      b.label = lab; b.cls = cls;
    }
  }
  __syncthreads();
  // ---- stage 2: each wave renders a 16 x 4 strip (64 contiguous bytes of depth per row)
  const int row = ty * VIEW_TILE + wave * 4 + (lane >> 4), col = tx * VIEW_TILE + (lane & 15);
  const float px = (2.0f * ((float)col + 0.5f) / (float)P.W - 1.0f) * th;
  const float py = (1.0f - 2.0f * ((float)row + 0.5f) / (float)P.H) * tv;
  const f3 d = vadd(vadd(f, vscale(r, px)), vscale(u, py));
  float best = 3.0e38f, best_nd = 0.0f;
  int best_i = -1;
  for (int i = 0; i < total; ++i) {
    const ViewBox& b = s_box[i];
    float tmin = 0.0f, tmax = 3.0e38f, nd = -1.0f;
    bool hit = true;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const float da = b.m[3 * a] * d.x + b.m[3 * a + 1] * d.y + b.m[3 * a + 2] * d.z;
      const float oa = b.o[a], ha = b.h[a];
      if (fabsf(da) < 1e-12f) { if (fabsf(oa) > ha) hit = false; }
      else {
        const float inv = 1.0f / da;
        float t0 = (-ha - oa) * inv, t1 = (ha - oa) * inv;
        if (t0 > t1) { const float tt = t0; t0 = t1; t1 = tt; }
        if (t0 > tmin) { tmin = t0; nd = fabsf(da); }                            // the entering face so far: axis a (its sign does not enter |n . d|)
        tmax = fminf(tmax, t1);
      }
    }
    if (hit && tmin <= tmax && tmin < best) { best = tmin; best_i = i; best_nd = nd; }
  }
  if (row >= P.H || col >= P.W) return;                                           // edge tiles: masked after the collective stages
  const size_t pix = ((size_t)k_img * P.H + row) * P.W + col;
  if (depth) depth[pix] = best_i >= 0 ? best : __int_as_float(0x7f800000);        // +inf: nothing hit
  if (label) label[pix] = (int16_t)(best_i >= 0 ? s_box[best_i].label : 0);
  if (rgb) {
    const float* cc = c_view_color[best_i >= 0 ? s_box[best_i].cls : VC_BACKGROUND];
    float shade = 1.0f;                                                           // background, or a ray that starts on the box's surface
    if (best_i >= 0 && best_nd >= 0.0f) shade = 0.35f + 0.65f * (best_nd / sqrtf(vdot(d, d)));   // headlight: |n . d| / |d|, n the entering face's normal
#pragma unroll
    for (int a = 0; a < 3; ++a) rgb[pix * 3 + a] = (uint8_t)(int)(cc[a] * shade + 0.5f);
  }
}

extern "C" void sdxk_render_view(const SdxConst* C, const SdxBuf* B, const sdx_view_desc* v, const int32_t* env_ids, int n, float* depth,
                                 int16_t* label, uint8_t* rgb, hipStream_t st) {
  ViewParams P;
  for (int a = 0; a < 3; ++a) { P.pos[a] = v->pos[a]; P.target[a] = v->target[a]; P.up[a] = v->up[a]; }
  P.attach = v->attach_body; P.hfov_deg = v->hfov_deg; P.W = v->width; P.H = v->height; P.geometry = v->geometry; P.n = n;
  P.tiles_x = (v->width + VIEW_TILE - 1) / VIEW_TILE; P.tiles_y = (v->height + VIEW_TILE - 1) / VIEW_TILE;
  hipLaunchKernelGGL(k_view_render, dim3((unsigned)(P.tiles_x * P.tiles_y * n)), dim3(256), 0, st, C, *B, P, env_ids, depth, label, rgb);
}
