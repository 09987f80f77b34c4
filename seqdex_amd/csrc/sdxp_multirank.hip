// sdxp_multirank.hip — the multi-rank optimiser step from the exchange on: the gradient rebuilt from every rank's factors, the bit-reproducible squared
// norm, clip + Adam on flat gradients (all-reduced, rebuilt, or left by the GEMM step of sdxp_bigmb.hip: sdxpk_apply_flat) and the one-launch apply.  What
// precedes the exchange (k_grad_layer / k_grad_heads, k_pack_factors) stays in sdxp_update.hip beside k_layer: in a unit that calls layer_input with cur = true only, the constant is propagated into it before inlining and their code changes.
// Where a parameter lives is sdxp_device.h's to say (trunk_slot, head_row); the rebuild from fact_all is stated once (rebuild_row, head_elem)
// for the kernels that store the flat gradient and for the one-launch apply that keeps it in registers; the grid both forms of the apply
// share is apply_job; the words of the one-launch apply's meeting are sdxp_tagged_words.h's.
#include "sdxp_device.h"
#include "sdxp_launch.h"
#include "sdxp_ppo_terms.h"
#include "sdxp_tagged_words.h"
#include <cstddef>

// block-level sum of the squared-gradient contributions of this workgroup, written (no atomics) to the slot of this workgroup:
// part[slot] for the actor-critic buffer, part[SDXP_SQN_STRIDE + slot] for the central value.  Every thread of the 256 calls it.
__device__ __forceinline__ void write_sqn_partials(float ss_ac, float ss_cv, float* part, int slot) {
  __shared__ float s_sq[2][4];
  const int tid = threadIdx.x;
  ss_ac = wave_sum(ss_ac); ss_cv = wave_sum(ss_cv);
  if ((tid & 63) == 0) { s_sq[0][tid >> 6] = ss_ac; s_sq[1][tid >> 6] = ss_cv; }
  __syncthreads();
  if (tid == 0) {
    part[slot] = (s_sq[0][0] + s_sq[0][1]) + (s_sq[0][2] + s_sq[0][3]);
    part[SDXP_SQN_STRIDE + slot] = (s_sq[1][0] + s_sq[1][1]) + (s_sq[1][2] + s_sq[1][3]);
  }
}

// ---- the SUM over ranks of the minibatch gradients rebuilt from fact_all, stated once: the kernels of the three-launch apply store what
// these functions yield to the flat gradient, the one-launch apply keeps it in registers for its Adam.  Ranks in ascending order on every
// rank, samples in ascending order within a rank: identical sums everywhere and in both forms.
// Trunk layers: a workgroup has four rows of layer l of one network, a wave one row n, a lane its columns lane + 64 j (K <= 1024: 16 per lane)
struct RowJob { int net, n; bool valid; TrunkSlot t; };
__device__ __forceinline__ RowJob row_job(const SdxpDev& D, int l, int bidx) {   // workgroup bidx of the trunk_row_blocks(D, l) of layer l
  const int blocks_per_net = (D.units[l] + 3) / 4;
  const int net = bidx / blocks_per_net, n = (bidx % blocks_per_net) * 4 + ((int)threadIdx.x >> 6);
  return {net, n, n < D.units[l], trunk_slot(D, net, l)};
}
// the accumulation: g[j] the gradient of weight (n, lane + 64 j), sb of the row's bias.  Every thread of the 256 calls it (LDS image of the input).
template <int MB>
__device__ __forceinline__ void rebuild_row(const SdxpDev& D, int l, const RowJob& r, float (&g)[16], float& sb) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int tid = threadIdx.x, lane = tid & 63, K = r.t.K, Nl = r.t.N;
  sb = 0.0f;
#pragma unroll
  for (int j = 0; j < 16; ++j) g[j] = 0.0f;
  for (int rk = 0; rk < D.world; ++rk) {
    const float* F = D.fact_all + (size_t)rk * D.foff.total;
    const float* gx = F + D.foff.x[r.net][l];
    for (int i = tid; i < MB * K; i += 256) sm[i] = gx[i];
    __syncthreads();
    if (r.valid) {
      float dyn[MB];
#pragma unroll
      for (int s = 0; s < MB; ++s) { dyn[s] = F[D.foff.dy[r.net][l] + s * Nl + r.n]; sb += dyn[s]; }
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const int k = lane + 64 * j;
        if (k < K) {
#pragma unroll
          for (int s = 0; s < MB; ++s) g[j] += dyn[s] * sm[s * K + k];
        }
      }
    }
    __syncthreads();
  }
}
// this lane's share of the squared norm of the rank AVERAGE of the row
__device__ __forceinline__ float row_sqn_share(const SdxpDev& D, const RowJob& r, const float (&g)[16], float sb) {
  const int lane = threadIdx.x & 63;
  const float sc = 1.0f / (float)D.world;
  float ss = 0.0f;
  if (r.valid) {
#pragma unroll
    for (int j = 0; j < 16; ++j) { if (lane + 64 * j < r.t.K) ss += (g[j] * sc) * (g[j] * sc); }
    if (lane == 0) ss += (sb * sc) * (sb * sc);
  }
  return ss;
}
__device__ __forceinline__ void row_store(const RowJob& r, const float (&g)[16], float sb) {
  const int lane = threadIdx.x & 63;
  if (!r.valid) return;
#pragma unroll
  for (int j = 0; j < 16; ++j) { const int k = lane + 64 * j; if (k < r.t.K) r.t.G[r.t.woff + (size_t)r.n * r.t.K + k] = g[j]; }
  if (lane == 0) r.t.G[r.t.boff + r.n] = sb;
}
template <int MB>
__device__ __forceinline__ void grad_layer_w_body(const SdxpDev& D, int l, int bidx, float* part = nullptr, int slot = 0) {
  const RowJob r = row_job(D, l, bidx);
  float g[16], sb;
  rebuild_row<MB>(D, l, r, g, sb);
  row_store(r, g, sb);
  if (!part) return;
  const float ss = row_sqn_share(D, r, g, sb);
  write_sqn_partials(r.net == 2 ? 0.0f : ss, r.net == 2 ? ss : 0.0f, part, slot);
}
template <int MB>
__global__ __launch_bounds__(256) void k_grad_layer_w(SdxpDev D, int l) { grad_layer_w_body<MB>(D, l, blockIdx.x); }
// Heads: this thread's element of the head gradient.  i: an index into the main slice [A + 2 rows][units[2]], or past it; t: the thread's
// place among the tails that the last heads block adds (0 .. A + 1 the rows' biases, 64 .. 64 + A - 1 logstd, 128 the SUM of the ranks'
// minibatch KL - no parameter: it goes where sdxp_apply(0, -INFINITY) and the LR rule look for it), -1 elsewhere
struct HeadElem { int buf; bool kl; size_t idx; float g; };   // buf: HeadRow::buf, -1: this thread has none; idx: into the buffer's flat gradient
template <int MB>
__device__ __forceinline__ HeadElem head_elem(const SdxpDev& D, int i, int t) {
  const int U = D.units[2], A = D.act_dim, W = D.world;
  const size_t T = D.foff.total;
  HeadElem e = {-1, false, 0, 0.0f};
  if (i < (A + 2) * U) {
    const HeadRow hr = head_row(D, i / U);
    const int k = i % U;
    for (int r = 0; r < W; ++r) {
      const float* F = D.fact_all + r * T;
      const float* dh = F + D.foff.dh;
      const float* h = F + D.foff.h[hr.net];
      for (int s = 0; s < MB; ++s) e.g += dh[s * 34 + hr.col] * h[s * U + k];
    }
    e.buf = hr.buf; e.idx = hr.woff + k;
  } else if (t >= 0 && t < A + 2) {
    const HeadRow hr = head_row(D, t);
    for (int r = 0; r < W; ++r) {
      const float* dh = D.fact_all + r * T + D.foff.dh;
      for (int s = 0; s < MB; ++s) e.g += dh[s * 34 + hr.col];
    }
    e.buf = hr.buf; e.idx = hr.boff;
  } else if (t >= 64 && t < 64 + A) {
    for (int r = 0; r < W; ++r) e.g += D.fact_all[r * T + D.foff.dls + (t - 64)];
    e.buf = 0; e.idx = D.off.logstd + (t - 64);
  } else if (t == 128) {
    for (int r = 0; r < W; ++r) e.g += D.fact_all[r * T + D.foff.kl];
    e.buf = 0; e.kl = true; e.idx = D.g_tail;
  }
  return e;
}
// the element's share of the squared norms of the rank average (write_sqn_partials' two sums)
__device__ __forceinline__ void head_sqn_share(const SdxpDev& D, const HeadElem& e, float& ss_ac, float& ss_cv) {
  const float sc = 1.0f / (float)D.world;
  if (e.buf < 0 || e.kl) return;
  if (e.buf) ss_cv += (e.g * sc) * (e.g * sc); else ss_ac += (e.g * sc) * (e.g * sc);
}
template <int MB>
__device__ __forceinline__ void grad_heads_w_body(const SdxpDev& D, int hb, int nhb, float* part = nullptr, int slot = 0) {   // block hb of nhb; the last one also does the tails
  const int tid = threadIdx.x, n_main = (D.act_dim + 2) * D.units[2];
  float ss_ac = 0.0f, ss_cv = 0.0f;
  auto store = [&](const HeadElem& e) {
    if (e.buf >= 0) (e.buf ? D.cv_g : D.ac_g)[e.idx] = e.g;
    head_sqn_share(D, e, ss_ac, ss_cv);
  };
  for (int i = hb * 256 + tid; i < n_main; i += nhb * 256) store(head_elem<MB>(D, i, -1));
  if (hb == nhb - 1) store(head_elem<MB>(D, n_main, tid));
  if (part) write_sqn_partials(ss_ac, ss_cv, part, slot);
}
template <int MB>
__global__ __launch_bounds__(256) void k_grad_heads_w(SdxpDev D) { grad_heads_w_body<MB>(D, 0, 1); }
// squared norm of the flat gradient, bit-reproducible (every rank must compute the SAME clip scale from the same gradient, or the
// replicas drift apart): fixed block -> slice mapping, in-block tree in a fixed order, second stage sums the 512 block partials
__device__ __forceinline__ void sqnorm_block(const float* __restrict__ g, size_t n, float scale, float* part) {   // part: this block's slot
  __shared__ float sw[4];
  float s = 0.0f;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) { const float v = g[i] * scale; s += v * v; }
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) sw[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) *part = (sw[0] + sw[1]) + (sw[2] + sw[3]);
}
__global__ __launch_bounds__(256) void k_sqnorm(const float* __restrict__ g, size_t n, float scale, float* part) {
  sqnorm_block(g, n, scale, part + blockIdx.x);
}
__global__ __launch_bounds__(512) void k_sqnorm_fin(const float* __restrict__ part, int nparts, float* out) {
  __shared__ float sw[8];
  float s = threadIdx.x < nparts ? part[threadIdx.x] : 0.0f;
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) sw[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) *out = ((sw[0] + sw[1]) + (sw[2] + sw[3])) + ((sw[4] + sw[5]) + (sw[6] + sw[7]));
}
// clip_grad_norm_ + Adam of one flat buffer (which: 0 actor-critic, 1 central value) whose rank-summed gradient has the squared norm gn2
// (of the rank average): grid-stride sweep over P / M / V / G with the element function ADAM (adam1 or adam1x)
typedef float (*AdamFn)(float, float, float&, float&, float, float);
template <AdamFn ADAM>
__device__ __forceinline__ void adam_sweep(const SdxpDev& D, int which, float gn2) {
  const SdxpCtrl* ctl = D.ctrl;
  const size_t n = which ? D.coff.total : D.off.total;
  float* P = which ? D.cv : D.ac; float* M = which ? D.cv_m : D.ac_m; float* V = which ? D.cv_v : D.ac_v;
  const float* G = which ? D.cv_g : D.ac_g;
  const float inv_w = 1.0f / (float)ctl->world;
  const float clip = ppo_clip_scale(D, sqrtf(gn2));
  const PpoAdamScales a = ppo_adam_scales(which ? ctl->cv_lr : ctl->ac_lr, (which ? ctl->cv_t : ctl->ac_t) + 1);
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
    float m = M[i], v = V[i];
    P[i] = ADAM(P[i], G[i] * inv_w * clip, m, v, a.lr_bc1, a.isq_bc2);
    M[i] = m; V[i] = v;
  }
}
__global__ __launch_bounds__(256) void k_adam_explicit(SdxpDev D, int which) {
  adam_sweep<adam1>(D, which, which ? D.ctrl->gn2_cv : D.ctrl->gn2_ac);
}
__global__ void k_apply_fin(SdxpDev D, int which, float kl_host) {
  SdxpCtrl* ctl = D.ctrl;
  ppo_adam_advance(*ctl, which);
  if (which) return;
  // NaN -> device value, all-reduced in place; -inf -> the KL word that travelled with the gradients in ALL_GRADS
  const float kl = (kl_host != kl_host) ? ctl->last_kl / (float)ctl->world
                 : (kl_host == -INFINITY ? D.ac_g[D.g_tail] / (float)ctl->world : kl_host);
  ppo_lr_advance(*ctl, D, kl);
}

// ---- the factor path's "apply" in four launches: every gradient block of the three layers and the heads at once, the squared
// norms of both flat gradients, clip + Adam of both networks, the step counters / LR rule
// The grid of k_grad_all_w / k_apply_factors_fused: the trunk_row_blocks of layers 0, 1, 2, then the heads blocks (one main-slice element
// per thread, + one block for the tails).  Workgroup b is block ApplyJob::b of trunk layer l, or (l = -1) heads block b; heads0: the first heads block
struct ApplyJob { int l, b, heads0; };
__host__ __device__ inline ApplyJob apply_job(const SdxpDev& D, int b) {
  const int heads0 = trunk_row_blocks(D, 0) + trunk_row_blocks(D, 1) + trunk_row_blocks(D, 2);
  int l = 0;
  for (; l < 3 && b >= trunk_row_blocks(D, l); ++l) b -= trunk_row_blocks(D, l);
  return {l < 3 ? l : -1, b, heads0};
}
struct ApplyGrid { int nb, Kmax; };
static ApplyGrid apply_grid(const SdxpDev* D) {
  const int nhb = ((D->act_dim + 2) * D->units[2] + 255) / 256 + 1;
  return {apply_job(*D, 0).heads0 + nhb, D->units[0] > D->state_dim ? D->units[0] : D->state_dim};
}
template <int MB>
__global__ __launch_bounds__(256) void k_grad_all_w(SdxpDev D, int with_norm) {
  float* part = with_norm ? D.sqn_part : nullptr;      // squared-norm contribution of every workgroup (the gradients are still in registers)
  const ApplyJob job = apply_job(D, blockIdx.x);
  if (job.l < 0) grad_heads_w_body<MB>(D, job.b, (int)gridDim.x - job.heads0, part, blockIdx.x);
  else grad_layer_w_body<MB>(D, job.l, job.b, part, blockIdx.x);
}
__global__ __launch_bounds__(256) void k_sqnorm2(SdxpDev D, float scale) {
  const int which = blockIdx.y;
  sqnorm_block(which ? D.cv_g : D.ac_g, which ? D.coff.total : D.off.total, scale, D.sqn_part + which * 512 + blockIdx.x);
}
// the squared norm of buffer `which` from s, this thread's share of its partials: every block folds them in the same fixed order -> the
// same clip scale in every block and on every rank; block 0 publishes the sum in the control block
__device__ __forceinline__ float fold_gn2(SdxpCtrl* ctl, int which, float s) {
  __shared__ float sw[4];
  __shared__ float s_n2;
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) sw[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    s_n2 = (sw[0] + sw[1]) + (sw[2] + sw[3]);
    if (blockIdx.x == 0) { if (which) ctl->gn2_cv = s_n2; else ctl->gn2_ac = s_n2; }
  }
  __syncthreads();
  return s_n2;
}
// the 512 partials of k_sqnorm2, two per thread
__global__ __launch_bounds__(256) void k_adam2(SdxpDev D) {
  const int which = blockIdx.y;
  adam_sweep<adam1>(D, which, fold_gn2(D.ctrl, which, D.sqn_part[which * 512 + threadIdx.x] + D.sqn_part[which * 512 + 256 + threadIdx.x]));
}
// the per-workgroup partials that k_grad_all_w left in sqn_part (nparts slots per buffer); adam1x: bit-identical to the one-launch apply
__global__ __launch_bounds__(256) void k_adam3(SdxpDev D, int nparts) {
  const int which = blockIdx.y;
  float s = 0.0f;
  for (int i = threadIdx.x; i < nparts; i += 256) s += D.sqn_part[which * SDXP_SQN_STRIDE + i];
  adam_sweep<adam1x>(D, which, fold_gn2(D.ctrl, which, s));
}
__global__ void k_apply_fin2(SdxpDev D) {
  SdxpCtrl* ctl = D.ctrl;
  ppo_adam_advance(*ctl, 1);
  ppo_adam_advance(*ctl, 0);
  ppo_lr_advance(*ctl, D, D.ac_g[D.g_tail] / (float)ctl->world);
}
template <int MB>
static void launch_apply_factors(const SdxpDev* D, hipStream_t st) {
  const ApplyGrid g = apply_grid(D);
  // the squared norms ride along with the gradient rebuild (one launch and one 13.4 MB read less than a separate norm pass)
  hipLaunchKernelGGL(k_grad_all_w<MB>, dim3(g.nb), dim3(256), (size_t)MB * g.Kmax * sizeof(float), st, *D, 1);
  hipLaunchKernelGGL(k_adam3, dim3(512, 2), dim3(256), 0, st, *D, g.nb);
  hipLaunchKernelGGL(k_apply_fin2, dim3(1), dim3(1), 0, st, *D);
}
// ---- the apply phase of the multi-rank step as ONE launch (round 6).  The three-launch form above rebuilds the summed
// gradient (k_grad_all_w: 13.4 MB written), reads it back beside weights and moments (k_adam3) and advances the control block from a
// single thread (k_apply_fin2): three dependent graph nodes of 7-10 us each.  Here every workgroup keeps the gradient elements it rebuilt
// in registers, publishes its share of the squared norm, meets the other workgroups at ONE grid-wide ticket (all of them are resident: the
// host checks the occupancy before it picks this form), folds the published shares in the fixed order of k_adam3 - the same clip scale
// in every workgroup and on every rank - and sends its elements through Adam.  The flat gradient is never materialised (only the KL word
// is); workgroup 0 advances the control block behind the ticket (every workgroup read what it needs of it BEFORE it arrived).
// Exchange discipline (MI355X guide, cross-XCD hand-off): shares and KL word leave as write-through (sc1) stores, the producer drains its
// stores (vmcnt(0)) before the relaxed agent-scope ticket increment, consumers read them with agent-scope loads after the ticket completes.
// A workgroup that waits too long raises the fail flag (bar[SDXP_BAR_APPLY_FAIL]) and every later launch returns at once: sdxp_update_status reports it
// and the handle goes back to the three-launch form.
// The meeting's words are (share_ac, share_cv, 0, tag) in the buffer Q.  Wave-uniform retry until every word idx0 + i * stride < limit carries
// `tag`; x / y: the words' payloads added in ascending i.  false (and *failflag set) if they do not arrive.
__device__ __forceinline__ bool tw_gather_sum(__amdgpu_buffer_rsrc_t Q, unsigned idx0, unsigned stride, unsigned limit, unsigned tag, float& x, float& y, unsigned* failflag) {
  unsigned spins = 0;
  for (;;) {
    u32x4 w[SDXP_SQN_STRIDE / 256];
#pragma unroll
    for (int i = 0; i < SDXP_SQN_STRIDE / 256; ++i) { const unsigned idx = idx0 + i * stride; w[i] = load16(Q, idx < limit ? idx : idx0); }
    bool good = true;
    x = 0.0f; y = 0.0f;
#pragma unroll
    for (int i = 0; i < SDXP_SQN_STRIDE / 256; ++i) {
      const bool act = idx0 + i * stride < limit;
      good = good && (!act || lq_ok(w[i], tag));
      if (act) { x += __uint_as_float(w[i].x); y += __uint_as_float(w[i].y); }
    }
    if (__builtin_amdgcn_ballot_w64(!good) == 0) return true;
    SDX_POLL_SLEEP_OR_GIVE_UP(spins, failflag)
  }
}
template <int MB>
__global__ __launch_bounds__(256, 6) void k_apply_factors_fused(SdxpDev D, unsigned* __restrict__ gen, unsigned* __restrict__ failflag) {
  __shared__ float s_sq[2][4], s_n2[2];
  __shared__ int s_ok;
  __shared__ unsigned s_gen;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  SdxpCtrl* ctl = D.ctrl;
  if (tid == 0) { s_ok = __hip_atomic_load(failflag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0; s_gen = __hip_atomic_load(gen, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
  __syncthreads();
  const unsigned tag = s_gen + 1u;   // s_gen: launches of this handle so far (device counter: launches replayed from a hipGraph see it grow); workgroup 0 advances it behind the meeting
  if (!s_ok) return;   // an earlier launch timed out at its ticket: nothing is applied until the host has looked (sdxp_update_status)
  // ---- what this launch needs of the control block (read before the ticket: workgroup 0 advances the block behind it)
  const float inv_w = 1.0f / (float)ctl->world;
  const PpoAdamScales sa = ppo_adam_scales(ctl->ac_lr, ctl->ac_t + 1), sv = ppo_adam_scales(ctl->cv_lr, ctl->cv_t + 1);
  const float ac_lr_bc1 = sa.lr_bc1, ac_isq = sa.isq_bc2, cv_lr_bc1 = sv.lr_bc1, cv_isq = sv.isq_bc2;
  // ---- the job of this workgroup: four rows of a trunk layer of one network (g, sb), or a slice of the heads (at most one element per thread)
  const ApplyJob job = apply_job(D, blockIdx.x);
  float g[16], sb = 0.0f, ss_ac = 0.0f, ss_cv = 0.0f;
  RowJob row = {};
  HeadElem he = {-1, false, 0, 0.0f};
  if (job.l >= 0) {
    row = row_job(D, job.l, job.b);
    rebuild_row<MB>(D, job.l, row, g, sb);
    const float ss = row_sqn_share(D, row, g, sb);
    if (row.net == 2) ss_cv = ss; else ss_ac = ss;
  } else {
    he = head_elem<MB>(D, job.b * 256 + tid, job.b == (int)gridDim.x - job.heads0 - 1 ? tid : -1);
    if (he.kl) __hip_atomic_store(&D.ac_g[he.idx], he.g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    head_sqn_share(D, he, ss_ac, ss_cv);
  }
  // ---- this workgroup's shares of the two squared norms (write_sqn_partials' order), then the grid-wide meeting: NO atomics.
  // (First versions: one device-scope counter - 1 380 arrivals served one after the other at the memory side: 105 us per optimiser step
  // against 68 with three launches; 64 counters: 87 us, the kernel alone 46.5 us against 7.8 + 18.4 + 4.7 for the three.)  The meeting is
  // two hops of tagged 16-byte words, the persistent kernel's exchange discipline (sdxp_tagged_words.h: write-through store, polling
  // agent-scope loads, a torn word polled again), laid out so that the sums are k_adam3's to the bit: every workgroup publishes
  // (share_ac, share_cv); workgroup w < 4 plays wave w of k_adam3's fold - lane l adds the shares 64 w + l + 256 k in ascending k, then
  // wave_sum - and publishes that wave's sum; every workgroup gathers the four sums and adds them as (s0 + s1) + (s2 + s3).
  ss_ac = wave_sum(ss_ac); ss_cv = wave_sum(ss_cv);
  if (lane == 0) { s_sq[0][wave] = ss_ac; s_sq[1][wave] = ss_cv; }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the KL word of thread 128 has left before the barrier that precedes this workgroup's word
  __syncthreads();
  if (wave == 0) {
    const __amdgpu_buffer_rsrc_t Q = __builtin_amdgcn_make_buffer_rsrc(D.sqn_part + SDXP_TW_OFF, 0, (SDXP_SQN_STRIDE + 64) * 16, 0x00020000);
    const unsigned nwg = gridDim.x;
    bool ok = true;
    if (lane == 0) lq_store(Q, blockIdx.x, (s_sq[0][0] + s_sq[0][1]) + (s_sq[0][2] + s_sq[0][3]), (s_sq[1][0] + s_sq[1][1]) + (s_sq[1][2] + s_sq[1][3]), 0.0f, tag);
    if (blockIdx.x < 4) {   // wave blockIdx.x of k_adam3's fold
      float x, y;
      const unsigned t = 64u * blockIdx.x + lane;
      ok = tw_gather_sum(Q, t < nwg ? t : 0u, 256u, t < nwg ? nwg : 0u, tag, x, y, failflag);
      x = wave_sum(x); y = wave_sum(y);
      if (ok && lane == 0) lq_store(Q, SDXP_SQN_STRIDE + blockIdx.x, x, y, 0.0f, tag);
    }
    float x = 0.0f, y = 0.0f;
    ok = ok && tw_gather_sum(Q, SDXP_SQN_STRIDE + (lane < 4 ? lane : 0), 64u, SDXP_SQN_STRIDE + 4u, tag, x, y, failflag);   // (one word per lane: 0.0f + the sum, exact)
    const float x0 = lane0(x), y0 = lane0(y);
    const float x1 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, x), 1)), y1 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, y), 1));
    const float x2 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, x), 2)), y2 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, y), 2));
    const float x3 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, x), 3)), y3 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, y), 3));
    if (lane == 0) { s_ok = ok; s_n2[0] = (x0 + x1) + (x2 + x3); s_n2[1] = (y0 + y1) + (y2 + y3); }
  }
  __syncthreads();
  if (!s_ok) return;
  const float n2_ac = s_n2[0], n2_cv = s_n2[1];
  const float clip_ac = ppo_clip_scale(D, sqrtf(n2_ac)), clip_cv = ppo_clip_scale(D, sqrtf(n2_cv));
  // ---- Adam of the elements this workgroup holds (k_adam3's arithmetic: adam1x(P, G * inv_w * clip, ...))
  if (job.l >= 0) {
    if (row.valid) {
      float *P = row.t.P, *M = row.t.M, *V = row.t.V;
      const int net = row.net, n = row.n, K = row.t.K;
      const size_t boff = row.t.boff;
      const float clip = net == 2 ? clip_cv : clip_ac, lr_bc1 = net == 2 ? cv_lr_bc1 : ac_lr_bc1, isq = net == 2 ? cv_isq : ac_isq;
      const size_t row0 = row.t.woff + (size_t)n * K;
#pragma unroll
      for (int hf = 0; hf < 2; ++hf) {   // eight columns per pass: their 24 loads in flight together, 80 VGPRs without a spill
        if (512 * hf >= K) break;
        float p[8], m[8], v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int kk = lane + 64 * (8 * hf + j);
          const int k = kk < K ? kk : K - 1;    // clamped address instead of a branch around the load
          p[j] = P[row0 + k]; m[j] = M[row0 + k]; v[j] = V[row0 + k];
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int k = lane + 64 * (8 * hf + j);
          if (k < K) {
            P[row0 + k] = adam1x(p[j], g[8 * hf + j] * inv_w * clip, m[j], v[j], lr_bc1, isq);
            M[row0 + k] = m[j]; V[row0 + k] = v[j];
          }
        }
      }
      if (lane == 0) {
        float bm = M[boff + n], bv = V[boff + n];
        P[boff + n] = adam1x(P[boff + n], sb * inv_w * clip, bm, bv, lr_bc1, isq);
        M[boff + n] = bm; V[boff + n] = bv;
      }
    }
  } else if (he.buf >= 0 && !he.kl) {
    const int c = he.buf;
    float* P = c ? D.cv : D.ac; float* M = c ? D.cv_m : D.ac_m; float* V = c ? D.cv_v : D.ac_v;
    float hm = M[he.idx], hv = V[he.idx];
    P[he.idx] = adam1x(P[he.idx], he.g * inv_w * (c ? clip_cv : clip_ac), hm, hv, c ? cv_lr_bc1 : ac_lr_bc1, c ? cv_isq : ac_isq);
    M[he.idx] = hm; V[he.idx] = hv;
  }
  // ---- k_apply_fin2's work, behind the ticket
  if (blockIdx.x == 0 && tid == 0) {
    __hip_atomic_store(gen, tag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    ctl->gn2_ac = n2_ac; ctl->gn2_cv = n2_cv;
    ppo_adam_advance(*ctl, 1);
    ppo_adam_advance(*ctl, 0);
    ppo_lr_advance(*ctl, D, __hip_atomic_load(&D.ac_g[D.g_tail], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) / (float)ctl->world);
  }
}
// 1 when the shapes fit the one-launch apply's tables and every workgroup can be resident at once on the current device (its grid-wide ticket)
extern "C" int sdxpk_apply_fused_prepare(const SdxpDev* D, int mb_size) {
  const ApplyGrid g = apply_grid(D);
  if (g.nb > SDXP_SQN_STRIDE || g.Kmax > 1024 || D->obs_dim > 1024 || (mb_size != 2 && mb_size != 4)) return 0;
  int per_cu = 0, dev = 0, cus = 0;
  return hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, mb_size == 2 ? k_apply_factors_fused<2> : k_apply_factors_fused<4>, 256,
                                                      (size_t)mb_size * g.Kmax * sizeof(float)) == hipSuccess &&
         hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && (long long)per_cu * cus >= g.nb;
}
extern "C" void sdxpk_apply_factors_fused(const SdxpDev* D, int mb_size, unsigned* bar, hipStream_t st) {
  const ApplyGrid g = apply_grid(D);
  hipLaunchKernelGGL((mb_size == 2 ? k_apply_factors_fused<2> : k_apply_factors_fused<4>), dim3(g.nb), dim3(256), (size_t)mb_size * g.Kmax * sizeof(float), st, *D,
                     bar + SDXP_BAR_APPLY_GEN, bar + SDXP_BAR_APPLY_FAIL);
}
// clip_grad_norm_ + Adam + LR schedule on the flat gradients already sitting in ac_g / cv_g (KL word in ac_g[g_tail])
extern "C" void sdxpk_apply_flat(const SdxpDev* D, hipStream_t st) {
  hipLaunchKernelGGL(k_sqnorm2, dim3(512, 2), dim3(256), 0, st, *D, 1.0f / (float)D->world);
  hipLaunchKernelGGL(k_adam2, dim3(512, 2), dim3(256), 0, st, *D);
  hipLaunchKernelGGL(k_apply_fin2, dim3(1), dim3(1), 0, st, *D);
}
extern "C" int sdxpk_apply_factors(const SdxpDev* D, int mb_size, hipStream_t st) {
  return sdxp_for_minibatch(mb_size, [&](auto m) { launch_apply_factors<decltype(m)::value>(D, st); });
}
extern "C" int sdxpk_grads_from_factors(const SdxpDev* D, int mb_size, hipStream_t st) {
  return sdxp_for_minibatch(mb_size, [&](auto m) {
    constexpr int MB = decltype(m)::value;
    for (int l = 0; l < 3; ++l)
      hipLaunchKernelGGL(k_grad_layer_w<MB>, dim3(trunk_row_blocks(*D, l)), dim3(256), (size_t)MB * trunk_kmax(D, l) * sizeof(float), st, *D, l);
    hipLaunchKernelGGL(k_grad_heads_w<MB>, dim3(1), dim3(256), 0, st, *D);
  });
}
extern "C" void sdxpk_apply_explicit(const SdxpDev* D, int which, float kl, int world, hipStream_t st) {
  const size_t n = which ? D->coff.total : D->off.total;
  float* acc = which ? &D->ctrl->gn2_cv : &D->ctrl->gn2_ac;
  hipLaunchKernelGGL(k_sqnorm, dim3(512), dim3(256), 0, st, which ? D->cv_g : D->ac_g, n, 1.0f / (float)world, D->sqn_part);
  hipLaunchKernelGGL(k_sqnorm_fin, dim3(1), dim3(512), 0, st, D->sqn_part, 512, acc);
  hipLaunchKernelGGL(k_adam_explicit, dim3(1024), dim3(256), 0, st, *D, which);
  hipLaunchKernelGGL(k_apply_fin, dim3(1), dim3(1), 0, st, *D, which, kl);
}
