// sdxp_bigmb_heads.h — the head section of the large-minibatch PPO step: everything between the last trunk layer's outputs and the
// trunk's backward pass.  Included by sdxp_bigmb.hip only (its includes come first).  Two forms, chosen per handle (big_heads):
//   * the 13-launch section for any units[2] / act_dim <= 32: k_gemm for the policy head's three products, the small kernels below
//     for the value heads, k_big_head / k_big_fin for the losses;
//   * the fused section k_big_heads + k_big_heads_reduce for units[2] == 256, act_dim <= 23.
// Both leave dLoss/d(pre-activation of trunk layer 2) in dy[net][2], the heads' weight gradients and d logstd in the flat gradients,
// and the control block advanced (big_minibatch_done).  The layouts of their partials in ws->part stand beside the kernels that
// write them: HeadParts (13 launches), the HP_* offsets (fused).
#pragma once

// ------------------------------------------------------------------------------------------------ 13 launches: value heads, reductions
// value heads: v[m] = H[m] . w + b (wave per row, U = 256: one float4 per lane)
__global__ __launch_bounds__(256) void k_rowdot(const float* __restrict__ H, int U, int M, const float* __restrict__ w, const float* __restrict__ b,
                                                float* __restrict__ v) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= M) return;
  float a = 0.0f;
  for (int k = lane; k < U; k += 64) a += H[(size_t)row * U + k] * w[k];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o, 64);
  if (lane == 0) v[row] = a + b[0];
}
// dY2[m][k] = dv[m] * w[k] * ELU'(H[m][k])
__global__ __launch_bounds__(256) void k_vhead_back(const float* __restrict__ dv, const float* __restrict__ w, const float* __restrict__ H, int U,
                                                    int M, float* __restrict__ dY) {
  const size_t n = (size_t)M * U;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
    const int m = (int)(i / U), k = (int)(i % U);
    dY[i] = dv[m] * w[k] * belu_grad_from_out(H[i]);
  }
}
// value-head weight gradient partials: out[z][k] = sum_{m in split z} dv[m] H[m][k]; out[z][U] = sum dv
__global__ __launch_bounds__(256) void k_vhead_wgrad(const float* __restrict__ dv, const float* __restrict__ H, int U, int M, int rchunk,
                                                     float* __restrict__ out, size_t oz) {
  const int k = threadIdx.x;            // U == 256
  const int rbeg = blockIdx.x * rchunk, rend = min(M, rbeg + rchunk);
  float a = 0.0f, sb = 0.0f;
  for (int m = rbeg; m < rend; ++m) { const float d = dv[m]; a += d * H[(size_t)m * U + k]; sb += d; }
  out[(size_t)blockIdx.x * oz + k] = a;
  if (k == 0) out[(size_t)blockIdx.x * oz + U] = sb;
}

// out[q][i] = sum_z part[q][z * pz + i] for the two value heads (q = 0, 1): one wave per output element, lanes stride over the VS
// partials, fixed-order wave reduction (deterministic)
__global__ __launch_bounds__(256) void k_vhead_reduce(const float* __restrict__ p0, const float* __restrict__ p1, size_t pz, int VS, int n,
                                                      float* __restrict__ o0, float* __restrict__ o1) {
  const int w = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (w >= 2 * n) return;
  const float* part = w < n ? p0 : p1;
  const int i = w < n ? w : w - n;
  float a = 0.0f;
  for (int z = lane; z < VS; z += 64) a += part[(size_t)z * pz + i];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o, 64);
  if (lane == 0) (w < n ? o0 : o1)[i] = a;
}

// out[i] = sum_z part[z * pz + i], i < n: one wave per output element, lanes stride over the S partials (fixed order: deterministic)
__global__ __launch_bounds__(256) void k_wave_reduce(const float* __restrict__ part, size_t pz, int S, int n, float* __restrict__ out) {
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (i >= n) return;
  float a = 0.0f;
  for (int z = lane; z < S; z += 64) a += part[(size_t)z * pz + i];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o, 64);
  if (lane == 0) out[i] = a;
}

// ------------------------------------------------------------------------------------------------ 13 launches: losses
// thread = sample s of the minibatch (dataset row r0 + s).  The formulas are sdxp_ppo_terms.h's (RC:1796-1830, 2114-2126):
// Gaussian neglogp, clipped surrogate, (clipped) value losses of the critic and the central value, bound loss, KL to the stored
// mu/sigma.  Writes dmu [MB][24] (column 23 = 0), dv [2][MB], the refreshed mu/sigma rows (RC:1358) and block partials
// part[block][40]: 0..22 d logstd, 32..37 the six loss sums.
#define BIGP 40
__global__ __launch_bounds__(256) void k_big_head(SdxpDev D, size_t r0, int MB, const float* __restrict__ mu, const float* __restrict__ vc,
                                                  const float* __restrict__ vcv, float* __restrict__ dmu, float* __restrict__ dv,
                                                  float* __restrict__ part) {
  __shared__ float s_red[4][BIGP];
  const int s = blockIdx.x * 256 + threadIdx.x, A = D.act_dim, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const bool live = s < MB;
  const float invM = 1.0f / (float)MB;
  float nlp = 0.0f, kl = 0.0f, bl = 0.0f, ent = 0.0f, gnlp = 0.0f;
  float stat[6] = {0, 0, 0, 0, 0, 0};
  const float* ls_p = D.ac + D.off.logstd;
  if (live) {
    const size_t r = r0 + s;
    for (int a = 0; a < A; ++a) {
      const float ls = ls_p[a];
      const PpoActionTerms t = ppo_action_terms(ls, expf(ls), mu[(size_t)s * 24 + a], D.mb_actions[r * A + a], D.mb_mus[r * A + a], D.mb_sigmas[r * A + a]);
      nlp += t.nlp; kl += t.kl; bl += t.bl; ent += t.ent;
    }
    const PpoRowTerms t = ppo_row_terms(D, D.adv[r], D.mb_neglogp[r], ppo_neglogp(nlp, A), D.returns[r], D.mb_values[r], vc[s], vcv[s], invM);
    gnlp = t.gnlp;
    dv[s] = t.dv[0]; dv[(size_t)MB + s] = t.dv[1];
    stat[0] = t.a_loss; stat[1] = t.closs[0]; stat[2] = bl; stat[3] = kl; stat[4] = t.closs[1]; stat[5] = ent;
  }
  // head gradients + d logstd partial sums (one wave reduction per action)
  for (int a = 0; a < 24; ++a) {
    float dls = 0.0f;
    if (live) {
      float d = 0.0f;
      if (a < A) {
        const size_t r = r0 + s;
        const float sg = expf(ls_p[a]), m = mu[(size_t)s * 24 + a];
        const PpoActionGrad g = ppo_action_grad(gnlp, ppo_z(D.mb_actions[r * A + a], m, sg), sg, m, D.bounds_coef, invM);
        d = g.dmu; dls = g.dls;
        D.mb_mus[r * A + a] = m;
        D.mb_sigmas[r * A + a] = sg;
      }
      dmu[(size_t)s * 24 + a] = d;
    }
    if (a < A) {
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) dls += __shfl_xor(dls, o, 64);
      if (lane == 0) s_red[wave][a] = dls;
    }
  }
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    float t = stat[j];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) t += __shfl_xor(t, o, 64);
    if (lane == 0) s_red[wave][32 + j] = t;
  }
  __syncthreads();
  if (threadIdx.x < BIGP) {
    const int j = threadIdx.x;
    const bool used = j < A || (j >= 32 && j < 38);
    part[(size_t)blockIdx.x * BIGP + j] = used ? (s_red[0][j] + s_red[1][j]) + (s_red[2][j] + s_red[3][j]) : 0.0f;
  }
}
// one thread: the minibatch's six loss sums into the control block, the KL word behind the gradients (multi-rank all-reduce; read by
// k_apply_fin2), Adam left to the apply kernels, the cursor moved on (what k_ctrl does in explicit mode for the small-minibatch path)
__device__ __forceinline__ void big_minibatch_done(const SdxpDev& D, int MB, const float* sums) {
  SdxpCtrl& c = *D.ctrl;
  for (int q = 0; q < 6; ++q) c.acc[1 + q] = sums[q];
  ppo_account_minibatch(c, 1.0f / (float)MB, &D.ac_g[D.g_tail]);
  ppo_explicit_reset(c);
  ppo_advance_cursor(c, D.num_minibatches, true);
}
// one block: fold the block partials, write d logstd into the flat gradient, then big_minibatch_done
__global__ __launch_bounds__(64) void k_big_fin(SdxpDev D, int nblocks, int MB, const float* __restrict__ part) {
  __shared__ float s_t[BIGP];
  const int j = threadIdx.x;
  if (j < BIGP) {
    float t = 0.0f;
    for (int b = 0; b < nblocks; ++b) t += part[(size_t)b * BIGP + j];
    s_t[j] = t;
  }
  __syncthreads();
  if (j < D.act_dim) D.ac_g[D.off.logstd + j] = ppo_dlogstd(s_t[j], D.entropy_coef);
  if (j == 0) big_minibatch_done(D, MB, &s_t[32]);
}

// What the 13 launches keep in ws->part (offsets and sizes in floats), U2 = units[2], A = act_dim:
//   [0, hb * BIGP)        the loss partials of k_big_head's hb blocks
//   [0, Sh * pz)          Sh splits of the policy head's weight gradient, each [G_mu [A][U2] | b_mu [A]] as the flat layout has it - a
//                         23-row product whose only parallelism is the reduction over the minibatch rows, so it is split 256 rows at a
//                         time (32 .. 128 splits instead of the trunk's 8 .. 16: 94 us -> about 15 at 32 768 rows)
//   [vp0, vp0 + VS * vz)  the 64-row splits of the critic head, each [g_v [U2] | b_v]
//   [vp1, vp1 + VS * vz)  the same for the central value
// The first two regions share their front.  That is sound only in big_heads' launch order: k_big_fin folds the loss partials BEFORE
// the policy head's weight-gradient product overwrites them with its splits.
// `floats` bounds vp1 + VS * vz without reading act_dim (act_dim <= 32 stands for it) and counts the loss partials beside the splits;
// big_part_floats sizes the workspace with it.
static int big_splits(int MB) { int s = (MB + 511) / 512; return s < 1 ? 1 : (s > 16 ? 16 : s); }   // splits of a trunk layer's weight gradient
struct HeadParts { int hb, Sh, VS; size_t pz, vz, vp0, vp1, floats; };
static HeadParts head_parts(const SdxpDev& D, int MB) {
  const int S = big_splits(MB);
  HeadParts p;
  p.hb = (MB + 255) / 256;
  p.Sh = MB / 256 < S ? S : (MB / 256 > 128 ? 128 : MB / 256);
  p.VS = (MB + 63) / 64;
  p.pz = (size_t)D.act_dim * D.units[2] + D.act_dim;
  p.vz = (size_t)D.units[2] + 1;
  p.vp0 = (size_t)p.Sh * p.pz;
  p.vp1 = p.vp0 + (size_t)p.VS * p.vz;
  p.floats = (size_t)p.hb * BIGP + (size_t)2 * p.VS * p.vz + (size_t)p.Sh * (32 * p.vz);
  return p;
}

// ------------------------------------------------------------------------------------------------ fused heads
// The whole head section in ONE launch (+ one reduction): the policy head mu = H_a Wmu^T + b and the two value heads, the per-sample
// losses of k_big_head, the head gradients dmu / dv, the data gradients dY_2 = (dmu Wmu) * ELU'(H_a), dv w * ELU'(H) of the three
// networks, and the heads' weight-gradient partials.  As 13 launches this section took 126 us of a 630 us optimiser step at 2 048
// rows for 1 % of its flops (profiles/r6_bigmb_kernel_stats_mb2048_before.csv).  A workgroup owns HR = 32 consecutive minibatch rows (times
// `nrb` such blocks, one after the other, for large minibatches): the three trunk outputs of those rows (96 KB), Wmu and the value
// weights live in LDS; rows are padded to 260 floats so that 16-byte reads of 8 different rows cover the 32 banks once.
//   phase 1  thread = (row, 3 actions): mu, 16-byte LDS reads along k; wave 0 also does the two value heads
//   phase 2  thread = row (32 lanes): the loss formulas of k_big_head, dmu / dv into LDS, loss sums folded over the 32 lanes
//   phase 3  thread = trunk column k: dY_2 of the three networks for the 32 rows (Wmu's column in registers, dmu broadcast from LDS) and
//            the column's weight-gradient sums, which stay in registers across the workgroup's row blocks
// k_big_heads_reduce folds the workgroups' partial records in index order (deterministic) into the flat gradients and does k_big_fin's
// bookkeeping.
#define HR 32
#define HU 256              // trunk output width the fused kernel is written for (units[2] of both shipped YAMLs); else the 13-launch path
#define HLD 260             // padded LDS row
// One workgroup's partial record in ws->part, [40 | G_mu [23][256] | b_mu [23] | g_v [256], b_v | g_cv [256], b_cv]: offsets in floats.
// The first 40: d logstd sums 0 .. 22, the six loss sums 24 .. 29 (all inside the reduction's first block of 32 elements).  Rows
// a >= act_dim of G_mu / b_mu are zeros.  [G_mu | b_mu], [g_v | b_v] and [g_cv | b_cv] are each contiguous as in the flat layout
constexpr int HP_GMU = BIGP, HP_BMU = HP_GMU + 23 * HU, HP_GV = HP_BMU + 23, HP_BV = HP_GV + HU, HP_GCV = HP_BV + 1, HP_BCV = HP_GCV + HU,
              HPZ = HP_BCV + 1;
struct HeadsLds {
  float H[3][HR][HLD];
  float Wm[23][HLD];
  float wv[2][HU];
  float bmu[24], bv[4];   // (bv padded: mu / dmu rows stay 16-byte aligned)
  float mu[HR][24], dmu[HR][24];
  float v[2][HR], dv[2][HR];
  float red[BIGP], redw[4][BIGP];
};
__global__ __launch_bounds__(512) void k_big_heads(SdxpDev D, size_t r0, int MB, int nrb, const float* __restrict__ Ha, const float* __restrict__ Hc,
                                                   const float* __restrict__ Hcv, float* __restrict__ dYa, float* __restrict__ dYc,
                                                   float* __restrict__ dYcv, float* __restrict__ part) {
  extern __shared__ __attribute__((aligned(16))) char heads_smem[];
  HeadsLds& L = *reinterpret_cast<HeadsLds*>(heads_smem);
  const int t = threadIdx.x, A = D.act_dim;
  const float* Hsrc[3] = {Ha, Hc, Hcv};
  // weights of the heads (once per workgroup)
  constexpr int NTH = 512;   // 8 waves: two per SIMD (one workgroup per CU: 130 KB of LDS)
  for (int i = t; i < 23 * (HU / 4); i += NTH) {
    const int a = i / (HU / 4), k4 = i % (HU / 4);
    float4 w = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (a < A) w = *reinterpret_cast<const float4*>(D.ac + D.off.mu_w + (size_t)a * HU + 4 * k4);
    *reinterpret_cast<float4*>(&L.Wm[a][4 * k4]) = w;
  }
  if (t < HU) { L.wv[0][t] = D.ac[D.off.v_w + t]; L.wv[1][t] = D.cv[D.coff.v_w + t]; }
  if (t < 24) L.bmu[t] = t < A ? D.ac[D.off.mu_b + t] : 0.0f;
  if (t == 32) L.bv[0] = D.ac[D.off.v_b];
  if (t == 33) L.bv[1] = D.cv[D.coff.v_b];
  if (t < BIGP) L.red[t] = 0.0f;
  // phase-3 accumulators of column (t & 255) over the row half (t >> 8) of every block, kept across the row blocks
  float G[23], gv0 = 0.0f, gv1 = 0.0f, bsum = 0.0f;   // bsum: thread a < 23: sum of dmu[.][a]; threads 23, 24: sum of dv[0 / 1][.]
#pragma unroll
  for (int a = 0; a < 23; ++a) G[a] = 0.0f;
  const float invM = 1.0f / (float)MB;
  const float* ls_p = D.ac + D.off.logstd;
  for (int rb = 0; rb < nrb; ++rb) {
    const int s0 = (blockIdx.x * nrb + rb) * HR;
    if (s0 >= MB) break;                                  // block-uniform
    __syncthreads();                                      // the previous block's phase 3 is done with H / dmu / dv
    // ---- phase 0: the three trunk outputs of rows s0 .. s0 + 31 (coalesced 16-byte loads; rows past the minibatch read as zeros)
    for (int i = t; i < 3 * HR * (HU / 4); i += NTH) {
      const int net = i / (HR * (HU / 4)), rr = (i / (HU / 4)) % HR, k4 = i % (HU / 4);
      float4 h = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      if (s0 + rr < MB) h = *reinterpret_cast<const float4*>(Hsrc[net] + (size_t)(s0 + rr) * HU + 4 * k4);
      *reinterpret_cast<float4*>(&L.H[net][rr][4 * k4]) = h;
    }
    __syncthreads();
    // ---- phase 1: heads forward
    {
      const int rr = (t & 255) >> 3, g = t & 7, kh = t >> 8;   // the two halves of k on the two halves of the workgroup
      float acc[3] = {0.0f, 0.0f, 0.0f};
      const int a0 = g, a1 = g + 8, a2 = g + 16 < 23 ? g + 16 : 22;
#pragma unroll 4
      for (int k4 = kh * (HU / 8); k4 < (kh + 1) * (HU / 8); ++k4) {
        const float4 h = *reinterpret_cast<const float4*>(&L.H[0][rr][4 * k4]);
        const float4 w0 = *reinterpret_cast<const float4*>(&L.Wm[a0][4 * k4]), w1 = *reinterpret_cast<const float4*>(&L.Wm[a1][4 * k4]),
                     w2 = *reinterpret_cast<const float4*>(&L.Wm[a2][4 * k4]);
        acc[0] += h.x * w0.x; acc[0] += h.y * w0.y; acc[0] += h.z * w0.z; acc[0] += h.w * w0.w;
        acc[1] += h.x * w1.x; acc[1] += h.y * w1.y; acc[1] += h.z * w1.z; acc[1] += h.w * w1.w;
        acc[2] += h.x * w2.x; acc[2] += h.y * w2.y; acc[2] += h.z * w2.z; acc[2] += h.w * w2.w;
      }
      if (kh == 1) { L.dmu[rr][a0] = acc[0]; L.dmu[rr][a1] = acc[1]; if (g + 16 < 23) L.dmu[rr][a2] = acc[2]; }   // (dmu as staging: phase 2 rewrites it)
      // value heads: (net, row, 8 slices of k) on the upper half's first 512 ... = all 512 threads: 2 x 32 x 8
      float av = 0.0f;
      {
        const int net = t >> 8, r2 = (t & 255) >> 3, ks = t & 7;
#pragma unroll
        for (int k4 = ks * (HU / 32); k4 < (ks + 1) * (HU / 32); ++k4) {
          const float4 h = *reinterpret_cast<const float4*>(&L.H[1 + net][r2][4 * k4]);
          const float4 w = *reinterpret_cast<const float4*>(&L.wv[net][4 * k4]);
          av += h.x * w.x; av += h.y * w.y; av += h.z * w.z; av += h.w * w.w;
        }
#pragma unroll
        for (int o = 1; o < 8; o <<= 1) av += __shfl_xor(av, o, 64);
        if (ks == 0) L.v[net][r2] = av + L.bv[net];
      }
      __syncthreads();
      if (kh == 0) {
        L.mu[rr][a0] = (acc[0] + L.dmu[rr][a0]) + L.bmu[a0];
        L.mu[rr][a1] = (acc[1] + L.dmu[rr][a1]) + L.bmu[a1];
        if (g + 16 < 23) L.mu[rr][a2] = (acc[2] + L.dmu[rr][a2]) + L.bmu[a2];
        if (g == 7) L.mu[rr][23] = 0.0f;
      }
    }
    __syncthreads();
    // ---- phase 2: losses and head gradients (formulas: sdxp_ppo_terms.h).  Thread = (row rr, action group g): the
    // actions g, g + 8, g + 16 of row s0 + rr; the per-row sums over the actions are folded over the 8 lanes of the row (xor 1, 2, 4),
    // the per-action sums over the rows over the wave's 8 rows (xor 8, 16, 32), then over the 4 waves in index order
    if (t < 256) {
      const int rr = t >> 3, g = t & 7, s = s0 + rr, wave = t >> 6;
      const bool live = s < MB;
      const size_t r = r0 + (live ? s : 0);
      float nlp = 0.0f, kl = 0.0f, bl = 0.0f, ent = 0.0f;
      float zq[3], sgq[3], mq[3];
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const int a = g + 8 * j;
        zq[j] = 0.0f; sgq[j] = 1.0f; mq[j] = 0.0f;
        if (live && a < A) {
          const float ls = ls_p[a], sg = expf(ls), m = L.mu[rr][a];
          const PpoActionTerms t = ppo_action_terms(ls, sg, m, D.mb_actions[r * A + a], D.mb_mus[r * A + a], D.mb_sigmas[r * A + a]);
          nlp += t.nlp; kl += t.kl; bl += t.bl; ent += t.ent;
          zq[j] = t.z; sgq[j] = sg; mq[j] = m;
        }
      }
#pragma unroll
      for (int o = 1; o < 8; o <<= 1) { nlp += __shfl_xor(nlp, o, 64); kl += __shfl_xor(kl, o, 64); bl += __shfl_xor(bl, o, 64); ent += __shfl_xor(ent, o, 64); }
      float gnlp = 0.0f;
      float stat[6] = {0, 0, 0, 0, 0, 0};
      if (live) {   // (every lane of the row needs gnlp; lane g = 0 keeps the row's value gradients and statistics)
        const PpoRowTerms t = ppo_row_terms(D, D.adv[r], D.mb_neglogp[r], ppo_neglogp(nlp, A), D.returns[r], D.mb_values[r], L.v[0][rr], L.v[1][rr], invM);
        gnlp = t.gnlp;
        if (g == 0) {
          L.dv[0][rr] = t.dv[0]; L.dv[1][rr] = t.dv[1];
          stat[0] = t.a_loss; stat[1] = t.closs[0]; stat[2] = bl; stat[3] = kl; stat[4] = t.closs[1]; stat[5] = ent;
        }
      } else if (g == 0) { L.dv[0][rr] = 0.0f; L.dv[1][rr] = 0.0f; }
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const int a = g + 8 * j;
        float d = 0.0f, dls = 0.0f;
        if (live && a < A) {
          const PpoActionGrad ag = ppo_action_grad(gnlp, zq[j], sgq[j], mq[j], D.bounds_coef, invM);
          d = ag.dmu; dls = ag.dls;
          D.mb_mus[r * A + a] = mq[j];
          D.mb_sigmas[r * A + a] = sgq[j];
        }
        if (a < 24) L.dmu[rr][a] = d;
#pragma unroll
        for (int o = 8; o < 64; o <<= 1) dls += __shfl_xor(dls, o, 64);
        if (a < 24 && (t & 56) == 0) L.redw[wave][a] = dls;   // lanes 0 .. 7 of the wave hold the sums over its 8 rows
      }
#pragma unroll
      for (int j = 0; j < 6; ++j) {
        float x = stat[j];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
        if ((t & 63) == 0) L.redw[wave][32 + j] = x;
      }
    }
    __syncthreads();
    if (t < BIGP && (t < 24 || (t >= 32 && t < 38))) L.red[t] += (L.redw[0][t] + L.redw[1][t]) + (L.redw[2][t] + L.redw[3][t]);
    // ---- phase 3: thread = trunk column t
    {
      const int col = t & 255, rh = t >> 8;
      float wcol[23];
#pragma unroll
      for (int a = 0; a < 23; ++a) wcol[a] = L.Wm[a][col];
      const float wv0 = L.wv[0][col], wv1 = L.wv[1][col];
      const int nrow = MB - s0 < HR ? MB - s0 : HR;
      const int rbeg = rh * (HR / 2), rend = nrow < (rh + 1) * (HR / 2) ? nrow : (rh + 1) * (HR / 2);
      for (int rr = rbeg; rr < rend; ++rr) {
        float d[24];
#pragma unroll
        for (int q4 = 0; q4 < 6; ++q4) {
          const float4 x = *reinterpret_cast<const float4*>(&L.dmu[rr][4 * q4]);   // every lane reads the same row: LDS broadcast
          d[4 * q4] = x.x; d[4 * q4 + 1] = x.y; d[4 * q4 + 2] = x.z; d[4 * q4 + 3] = x.w;
        }
        const float ha = L.H[0][rr][col], hc = L.H[1][rr][col], hcv = L.H[2][rr][col];
        float x = 0.0f;
#pragma unroll
        for (int a = 0; a < 23; ++a) { x += d[a] * wcol[a]; G[a] += d[a] * ha; }
        const size_t o = (size_t)(s0 + rr) * HU + col;
        dYa[o] = x * belu_grad_from_out(ha);
        const float d0 = L.dv[0][rr], d1 = L.dv[1][rr];
        dYc[o] = d0 * wv0 * belu_grad_from_out(hc);
        dYcv[o] = d1 * wv1 * belu_grad_from_out(hcv);
        gv0 += d0 * hc; gv1 += d1 * hcv;
      }
      if (t < 23) for (int rr = 0; rr < nrow; ++rr) bsum += L.dmu[rr][t];
      else if (t < 25) for (int rr = 0; rr < nrow; ++rr) bsum += L.dv[t - 23][rr];
    }
  }
  __syncthreads();
  // the upper row half's column sums through LDS (the H rows are dead), added to the lower half's in a fixed order
  float* X = &L.H[0][0][0];   // [25][256]
  if (t >= 256) {
#pragma unroll
    for (int a = 0; a < 23; ++a) X[a * HU + (t & 255)] = G[a];
    X[23 * HU + (t & 255)] = gv0; X[24 * HU + (t & 255)] = gv1;
  }
  __syncthreads();
  if (t >= 256) return;
  float* P = part + (size_t)blockIdx.x * HPZ;
  if (t < BIGP) P[t] = t < 24 ? L.red[t] : (t < 30 ? L.red[t + 8] : 0.0f);   // [0..22] d logstd, [24..29] the six loss sums
#pragma unroll
  for (int a = 0; a < 23; ++a) P[HP_GMU + a * HU + t] = G[a] + X[a * HU + t];
  if (t < 23) P[HP_BMU + t] = bsum;
  P[HP_GV + t] = gv0 + X[23 * HU + t];
  P[HP_GCV + t] = gv1 + X[24 * HU + t];
  if (t == 23) P[HP_BV] = bsum;
  if (t == 24) P[HP_BCV] = bsum;
}
// fold of the heads' partial records over the workgroups (index order: deterministic) into the flat gradients, then big_minibatch_done
__global__ __launch_bounds__(256) void k_big_heads_reduce(SdxpDev D, int nblocks, int MB, const float* __restrict__ part) {
  __shared__ float s_t[BIGP];
  // eight lanes per output element: lane l sums the workgroups b = l, l + 8, ... in order, the eight sums are added in a fixed tree
  const int i = blockIdx.x * 32 + (threadIdx.x >> 3), l = threadIdx.x & 7, A = D.act_dim;
  float x = 0.0f;
  if (i < HPZ) for (int b = l; b < nblocks; b += 8) x += part[(size_t)b * HPZ + i];
#pragma unroll
  for (int o = 1; o < 8; o <<= 1) x += __shfl_xor(x, o, 64);
  if (l != 0) { if (blockIdx.x != 0) return; }   // (block 0's helper lanes stay for its barrier)
  const int gi = i - HP_GMU;                     // index into the three gradient blocks; their starts counted from G_mu:
  constexpr int BMU = HP_BMU - HP_GMU, GV = HP_GV - HP_GMU, GCV = HP_GCV - HP_GMU;
  if (l == 0 && i >= HP_GMU && i < HPZ) {
    if (gi < GV) {   // [mu_w | mu_b] is contiguous in the flat layout; rows a >= act_dim of the partials are zeros and have no slot
      const int a = gi < BMU ? gi / HU : gi - BMU;
      if (a < A) D.ac_g[D.off.mu_w + (gi < BMU ? (size_t)gi : (size_t)A * HU + a)] = x;
    } else if (gi < GCV) D.ac_g[D.off.v_w + (gi - GV)] = x;
    else D.cv_g[D.coff.v_w + (gi - GCV)] = x;
  }
  if (blockIdx.x != 0) return;
  if (l == 0 && i < 32) s_t[i] = x;    // block 0 folds elements 0 .. 31: the d logstd sums 0 .. 22 and the six loss sums 24 .. 29
  __syncthreads();
  const int j = threadIdx.x;
  if (j < A) D.ac_g[D.off.logstd + j] = ppo_dlogstd(s_t[j], D.entropy_coef);
  if (j == 0) big_minibatch_done(D, MB, &s_t[24]);
}
static int heads_nrb(int MB) { int n = MB / (HR * 512); return n < 1 ? 1 : n; }
static int heads_blocks(int MB) { const int nrb = heads_nrb(MB); return (MB + HR * nrb - 1) / (HR * nrb); }
