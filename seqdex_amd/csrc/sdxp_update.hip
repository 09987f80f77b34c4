// sdxp_update.hip — the rank-MB optimiser step of the small-minibatch update as a sequence of kernels: the hipGraph path, and the
// multi-rank steps up to what leaves the rank (flat gradients or packed factors; sdxp_multirank.hip has what follows the exchange).
// sdxp_persist.hip is the same step as one persistent launch.  Where a trunk layer or a head row lives in the flat parameter, moment and
// gradient buffers is sdxp_device.h's to say (trunk_slot, head_row), and so is the launch shape of a row-per-wave kernel (trunk_kmax, trunk_row_blocks).
// Update with the shipped minibatch_size 4 (YG:50,75): a minibatch gradient of a Linear layer is the rank-MB
// product dY^T X, so it is never materialised:
//   * the optimiser step of minibatch i is applied LAZILY inside the forward of minibatch i+1: the layer
//     kernel streams each weight row ONCE (w, m, v in; w, m, v out), rebuilds g[n][k] = sum_s dY[s][n] X[s][k]
//     from the rank-MB factors kept in LDS, applies clip-scale + Adam and immediately uses the new row for
//     the forward dot products (wave per row, lanes along K -> coalesced, wave reduction);
//   * the global gradient norm (clip_grad_norm_, RC:1859-1877) comes from the MB x MB Gram matrices of the
//     factors: |dY^T X|_F^2 = sum_{s,s'} (dY_s . dY_s')(X_s . X_s');
//   * actor, critic and central-value networks advance in the SAME launches (they are independent given the
//     dataset; rl_games runs train_central_value first, RC:1323-1324 - interleaving is arithmetically identical).
// Per optimiser step: L1, L2, L3, HEAD(+loss +backward of the heads), B3, B2, CTRL = 7 launches for all three nets (factor buffers: sdxp_device.h).
#include "sdxp_device.h"
#include "sdxp_launch.h"
#include "sdxp_ppo_terms.h"
#include <cstddef>

#define MAXG 64   // MB*MB for MB <= 8
#define STAMP(i) do { if (threadIdx.x == 0) D.dbg[i] = (long long)__builtin_readcyclecounter(); } while (0)

// block-wide symmetric Gram of MB vectors of length K living in LDS (v[s*K+k]); result (MB*MB floats) to out (global)
template <int MB>
__device__ void block_gram(const float* v, int K, float* out, float* s_scr /*>= MB*MB floats of LDS*/) {
  const int tid = threadIdx.x, nt = blockDim.x;
  float g[MB][MB];
#pragma unroll
  for (int a = 0; a < MB; ++a)
#pragma unroll
    for (int b = 0; b < MB; ++b) g[a][b] = 0.0f;
  for (int k = tid; k < K; k += nt) {
    float x[MB];
#pragma unroll
    for (int a = 0; a < MB; ++a) x[a] = v[a * K + k];
#pragma unroll
    for (int a = 0; a < MB; ++a)
#pragma unroll
      for (int b = 0; b <= a; ++b) g[a][b] += x[a] * x[b];
  }
  if (tid < MB * MB) s_scr[tid] = 0.0f;
  __syncthreads();
#pragma unroll
  for (int a = 0; a < MB; ++a)
#pragma unroll
    for (int b = 0; b <= a; ++b) {
      const float r = wave_sum(g[a][b]);
      if ((tid & 63) == 0) atomicAdd(&s_scr[a * MB + b], r);
    }
  __syncthreads();
  if (tid < MB * MB) { const int a = tid / MB, b = tid % MB; out[tid] = a >= b ? s_scr[a * MB + b] : s_scr[b * MB + a]; }
}

// L-kernel: lazy Adam of the previous minibatch + forward of the current one for trunk layer `l` of all three nets.
// block = 256 threads = 4 waves; a wave owns RPW consecutive weight rows; lanes run along K with float4 accesses.
// All global loads of a wave (RPW rows x KI float4 columns x {w,m,v}) are issued before any arithmetic so that the
// kernel is bandwidth- rather than latency-bound.
template <int MB, int RPW, int KI>
__global__ __launch_bounds__(256) void k_layer(SdxpDev D, int l) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  __shared__ float s_scr[MAXG];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  SdxpCtrl* ctl = D.ctrl;
  const int par = ctl->step & 1;
  const int Nl = D.units[l];
  constexpr int rows_per_block = 4 * RPW;
  const int blocks_per_net = (Nl + rows_per_block - 1) / rows_per_block;
  const int net = blockIdx.x / blocks_per_net, blk = blockIdx.x % blocks_per_net;
  const TrunkSlot t = trunk_slot(D, net, l);
  const int K = t.K, K4 = K >> 2;
  const bool pend = (net == 2 ? ctl->cv_pending : ctl->ac_pending) != 0;
  float *P = t.P, *Mo = t.M, *Vo = t.V;
  const size_t woff = t.woff, boff = t.boff;
  const float lr = net == 2 ? ctl->cv_lr_applied : ctl->ac_lr_applied;
  const float gs = net == 2 ? ctl->cv_gscale : ctl->ac_gscale;          // grad clip scale of the pending step
  const float bc1 = net == 2 ? ctl->cv_bc1 : ctl->ac_bc1, bc2 = net == 2 ? ctl->cv_bc2 : ctl->ac_bc2;
  const float lr_bc1 = lr / bc1, isq_bc2 = 1.0f / sqrtf(bc2);
  const int n0 = blk * rows_per_block + wave * RPW;
  // ---- issue this wave's weight / moment loads first
  float4 w[RPW][KI], m[RPW][KI], v[RPW][KI];
#pragma unroll
  for (int r = 0; r < RPW; ++r)
#pragma unroll
    for (int i = 0; i < KI; ++i) {
      const int k4 = lane + 64 * i, n = n0 + r;
      if (k4 < K4 && n < Nl) {
        const size_t o = woff + (size_t)n * K;
        w[r][i] = reinterpret_cast<const float4*>(P + o)[k4];
        if (pend) { m[r][i] = reinterpret_cast<const float4*>(Mo + o)[k4]; v[r][i] = reinterpret_cast<const float4*>(Vo + o)[k4]; }
      } else w[r][i] = make_float4(0, 0, 0, 0);
    }
  float dyn[RPW][MB], bias[RPW], bm[RPW], bv[RPW];
#pragma unroll
  for (int r = 0; r < RPW; ++r) {
    const int n = n0 + r;
    bias[r] = n < Nl ? P[boff + n] : 0.0f;
    bm[r] = (pend && n < Nl) ? Mo[boff + n] : 0.0f;
    bv[r] = (pend && n < Nl) ? Vo[boff + n] : 0.0f;
#pragma unroll
    for (int s = 0; s < MB; ++s) dyn[r][s] = (pend && n < Nl) ? dy_at<MB>(D, net, l, par ^ 1, s, n) * gs : 0.0f;
  }
  // ---- stage the rank-MB factors of the inputs
  float* xc = sm;                 // [MB][K] current input
  float* xp = sm + MB * K;        // [MB][K] previous input (factor of the pending gradient)
  {
    const float4* gc = reinterpret_cast<const float4*>(layer_input<MB>(D, ctl, net, l, true));
    const float4* gp = reinterpret_cast<const float4*>(layer_input<MB>(D, ctl, net, l, false));
    float4* c4 = reinterpret_cast<float4*>(xc);
    float4* p4 = reinterpret_cast<float4*>(xp);
    for (int i = tid; i < MB * K4; i += 256) { c4[i] = gc[i]; if (pend) p4[i] = gp[i]; }
  }
  __syncthreads();
  if (blk == 0) block_gram<MB>(xc, K, ctl->gx[net][l], s_scr);   // Gram of this layer's input, for the grad norm
  float* xn = D.x[net][l + 1] + (size_t)par * MB * Nl;            // output = next layer's input
#pragma unroll
  for (int r = 0; r < RPW; ++r) {
    const int n = n0 + r;
    float acc[MB];
#pragma unroll
    for (int s = 0; s < MB; ++s) acc[s] = 0.0f;
#pragma unroll
    for (int i = 0; i < KI; ++i) {
      const int k4 = lane + 64 * i;
      if (k4 < K4 && n < Nl) {
        float4 ww = w[r][i];
        if (pend) {
          float4 mm = m[r][i], vv = v[r][i];
          float4 g = make_float4(0, 0, 0, 0);
#pragma unroll
          for (int s = 0; s < MB; ++s) {
            const float4 x = reinterpret_cast<const float4*>(xp + s * K)[k4];
            g.x += dyn[r][s] * x.x; g.y += dyn[r][s] * x.y; g.z += dyn[r][s] * x.z; g.w += dyn[r][s] * x.w;
          }
          ww.x = adam1(ww.x, g.x, mm.x, vv.x, lr_bc1, isq_bc2); ww.y = adam1(ww.y, g.y, mm.y, vv.y, lr_bc1, isq_bc2);
          ww.z = adam1(ww.z, g.z, mm.z, vv.z, lr_bc1, isq_bc2); ww.w = adam1(ww.w, g.w, mm.w, vv.w, lr_bc1, isq_bc2);
          const size_t o = woff + (size_t)n * K;
          reinterpret_cast<float4*>(Mo + o)[k4] = mm; reinterpret_cast<float4*>(Vo + o)[k4] = vv;
          reinterpret_cast<float4*>(P + o)[k4] = ww;
        }
#pragma unroll
        for (int s = 0; s < MB; ++s) {
          const float4 x = reinterpret_cast<const float4*>(xc + s * K)[k4];
          acc[s] += ww.x * x.x + ww.y * x.y + ww.z * x.z + ww.w * x.w;
        }
      }
    }
    float b = bias[r];
    if (pend && n < Nl) {
      float g = 0.0f;
#pragma unroll
      for (int s = 0; s < MB; ++s) g += dyn[r][s];
      float mm = bm[r], vv = bv[r];
      b = adam1(b, g, mm, vv, lr_bc1, isq_bc2);
      if (lane == 0) { Mo[boff + n] = mm; Vo[boff + n] = vv; P[boff + n] = b; }
    }
#pragma unroll
    for (int s = 0; s < MB; ++s) {
      const float y = wave_sum(acc[s]) + b;
      if (lane == 0 && n < Nl) xn[s * Nl + n] = elu(y);
    }
  }
}

// HEAD kernel (one block of 1024 threads): lazy Adam of the head parameters, head forward, PPO losses (R7), gradients
// of the heads' pre-activations, backward through the heads into dY of trunk layer 2, KL + statistics, mu/sigma
// write-back (dataset.update_mu_sigma, RC:1358), and the gradient-norm contributions of the heads and of layer 2.
// flush != 0: only the lazy Adam part (end of an epoch).
template <int MB>
__global__ __launch_bounds__(1024) void k_head(SdxpDev D, int flush) {
  __shared__ float s_h[3][MB][256];      // head inputs of the current minibatch
  __shared__ float s_hp[3][MB][256];     // ... of the previous one (factor of the pending gradient)
  __shared__ float s_w[26][256];         // head weight rows after the lazy Adam (23 mu rows, critic V, central V)
  __shared__ float s_dy2[3][MB][256];
  __shared__ float s_mu[MB][32], s_dmu[MB][32], s_dmu_p[MB][32], s_z[MB][32], s_act[MB][32], s_omu[MB][32], s_osg[MB][32];
  __shared__ float s_v[2][MB], s_dv[2][MB], s_dv_p[2][MB], s_gnlp[MB], s_ls[32];
  __shared__ float s_stat[MB][8], s_gh[3][MAXG], s_gd[3][MAXG], s_n2[3], s_n2p[3], s_dls[32], s_term[3 * MAXG], s_bterm[32];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  __shared__ SdxpCtrl s_ctl;               // read-mostly snapshot of the control block
  SdxpCtrl* gctl = D.ctrl;
  for (int i = tid; i < (int)(sizeof(SdxpCtrl) / 4); i += 1024) reinterpret_cast<uint32_t*>(&s_ctl)[i] = reinterpret_cast<const uint32_t*>(gctl)[i];
  __syncthreads();
  const SdxpCtrl* ctl = &s_ctl;
  STAMP(0);
  const int par = ctl->step & 1, U = D.units[2], A = D.act_dim;
  const size_t r0 = (size_t)ctl->mb_index * MB;   // first dataset row of this minibatch: contiguous, unshuffled (App. C)
  const bool apend = ctl->ac_pending != 0, cpend = ctl->cv_pending != 0;
  for (int i = tid; i < 3 * MB * U; i += 1024) {
    const int net = i / (MB * U), r = i % (MB * U);
    s_h[net][r / U][r % U] = D.x[net][3][(size_t)par * MB * U + r];
    s_hp[net][r / U][r % U] = D.x[net][3][(size_t)(par ^ 1) * MB * U + r];
  }
  if (tid < MB * 32) {
    const int s = tid / 32, a = tid % 32;
    s_dmu_p[s][a] = (a < A) ? D.dhead[(size_t)(par ^ 1) * MB * 34 + s * 34 + a] : 0.0f;
    s_act[s][a] = (a < A) ? D.mb_actions[(r0 + s) * A + a] : 0.0f;
    s_omu[s][a] = (a < A) ? D.mb_mus[(r0 + s) * A + a] : 0.0f;
    s_osg[s][a] = (a < A) ? D.mb_sigmas[(r0 + s) * A + a] : 1.0f;
  }
  if (tid < 2 * MB) s_dv_p[tid / MB][tid % MB] = D.dhead[(size_t)(par ^ 1) * MB * 34 + (tid % MB) * 34 + 32 + tid / MB];
  if (tid < 3) s_n2[tid] = 0.0f;
  __syncthreads();
  STAMP(1);
  // ---- lazy Adam + forward of the head rows: rows 0..A-1 = mu, row A = critic value, row A+1 = central value.
  // U = 256: one float4 per lane and row; both rows of a wave are loaded before any arithmetic.
  {
    const float ac_lr_bc1 = ctl->ac_lr_applied / ctl->ac_bc1, ac_isq = 1.0f / sqrtf(ctl->ac_bc2), ac_gs = ctl->ac_gscale;
    const float cv_lr_bc1 = ctl->cv_lr_applied / ctl->cv_bc1, cv_isq = 1.0f / sqrtf(ctl->cv_bc2), cv_gs = ctl->cv_gscale;
    float4 w[2], m[2], v[2];
    float bias[2], bm[2], bv[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int row = wave + 16 * j;
      w[j] = make_float4(0, 0, 0, 0); m[j] = w[j]; v[j] = w[j]; bias[j] = bm[j] = bv[j] = 0.0f;
      if (row < A + 2) {
        const HeadRow hr = head_row(D, row);
        const float* P = hr.buf ? D.cv : D.ac;
        const float* Mo = hr.buf ? D.cv_m : D.ac_m;
        const float* Vo = hr.buf ? D.cv_v : D.ac_v;
        w[j] = reinterpret_cast<const float4*>(P + hr.woff)[lane];
        bias[j] = P[hr.boff];
        if (hr.buf ? cpend : apend) {
          m[j] = reinterpret_cast<const float4*>(Mo + hr.woff)[lane]; v[j] = reinterpret_cast<const float4*>(Vo + hr.woff)[lane];
          bm[j] = Mo[hr.boff]; bv[j] = Vo[hr.boff];
        }
      }
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int row = wave + 16 * j;
      if (row >= A + 2) continue;
      const HeadRow hr = head_row(D, row);
      const int net = hr.net;
      float* P = hr.buf ? D.cv : D.ac;
      float* Mo = hr.buf ? D.cv_m : D.ac_m;
      float* Vo = hr.buf ? D.cv_v : D.ac_v;
      const size_t woff = hr.woff, boff = hr.boff;
      const bool pend = net == 2 ? cpend : apend;
      const float lr_bc1 = net == 2 ? cv_lr_bc1 : ac_lr_bc1, isq_bc2 = net == 2 ? cv_isq : ac_isq;
      const float gs = net == 2 ? cv_gs : ac_gs;
      float dyn[MB], acc[MB];
#pragma unroll
      for (int s = 0; s < MB; ++s) dyn[s] = pend ? gs * (row < A ? s_dmu_p[s][row] : s_dv_p[row - A][s]) : 0.0f;
      float4 ww = w[j];
      const int k = 4 * lane;
      if (pend) {
        float4 g = make_float4(0, 0, 0, 0), mm = m[j], vv = v[j];
#pragma unroll
        for (int s = 0; s < MB; ++s) {
          g.x += dyn[s] * s_hp[net][s][k]; g.y += dyn[s] * s_hp[net][s][k + 1];
          g.z += dyn[s] * s_hp[net][s][k + 2]; g.w += dyn[s] * s_hp[net][s][k + 3];
        }
        ww.x = adam1(ww.x, g.x, mm.x, vv.x, lr_bc1, isq_bc2); ww.y = adam1(ww.y, g.y, mm.y, vv.y, lr_bc1, isq_bc2);
        ww.z = adam1(ww.z, g.z, mm.z, vv.z, lr_bc1, isq_bc2); ww.w = adam1(ww.w, g.w, mm.w, vv.w, lr_bc1, isq_bc2);
        reinterpret_cast<float4*>(Mo + woff)[lane] = mm; reinterpret_cast<float4*>(Vo + woff)[lane] = vv;
        reinterpret_cast<float4*>(P + woff)[lane] = ww;
      }
      s_w[row][k] = ww.x; s_w[row][k + 1] = ww.y; s_w[row][k + 2] = ww.z; s_w[row][k + 3] = ww.w;
#pragma unroll
      for (int s = 0; s < MB; ++s)
        acc[s] = ww.x * s_h[net][s][k] + ww.y * s_h[net][s][k + 1] + ww.z * s_h[net][s][k + 2] + ww.w * s_h[net][s][k + 3];
      float b = bias[j];
      if (pend) {
        float g = 0.0f;
#pragma unroll
        for (int s = 0; s < MB; ++s) g += dyn[s];
        float mm = bm[j], vv = bv[j];
        b = adam1(b, g, mm, vv, lr_bc1, isq_bc2);
        if (lane == 0) { Mo[boff] = mm; Vo[boff] = vv; P[boff] = b; }
      }
#pragma unroll
      for (int s = 0; s < MB; ++s) {
        const float y = wave_sum(acc[s]) + b;
        if (lane == 0) { if (row < A) s_mu[s][row] = y; else s_v[row - A][s] = y; }
      }
    }
  }
  if (tid >= 512 && tid < 512 + 32) {   // logstd parameter (fixed_sigma: a free Parameter, YG:18-21)
    const int a = tid - 512;
    float ls = 0.0f;
    if (a < A) {
      const size_t o = D.off.logstd + a;
      ls = D.ac[o];
      if (apend) {
        const float g = D.dlogstd[(size_t)(par ^ 1) * 32 + a] * ctl->ac_gscale;
        float m = D.ac_m[o], v = D.ac_v[o];
        ls = adam1(ls, g, m, v, ctl->ac_lr_applied / ctl->ac_bc1, 1.0f / sqrtf(ctl->ac_bc2));
        D.ac_m[o] = m; D.ac_v[o] = v; D.ac[o] = ls;
      }
    }
    s_ls[a] = ls;
  }
  __syncthreads();
  if (flush) {
    if (tid == 0) { gctl->ac_pending = 0; gctl->cv_pending = 0; }
    return;
  }
  const float invM = 1.0f / (float)MB;
  STAMP(2);
  // ---- per-sample scalars (sdxp_ppo_terms.h): lanes (s, a) reduce over the 32-lane half-wave of sample s; z stays in LDS for dmu / dlogstd
  float r_nlp = 0.0f, r_kl = 0.0f, r_bl = 0.0f, r_ent = 0.0f;
  if (tid < MB * 32) {
    const int s = tid / 32, a = tid % 32;
    float z = 0.0f;
    if (a < A) {
      const float ls = s_ls[a];
      const PpoActionTerms t = ppo_action_terms(ls, expf(ls), s_mu[s][a], s_act[s][a], s_omu[s][a], s_osg[s][a]);
      z = t.z; r_nlp = t.nlp; r_kl = t.kl; r_bl = t.bl; r_ent = t.ent;
    }
    s_z[s][a] = z;
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) {
      r_nlp += __shfl_xor(r_nlp, o, 64); r_kl += __shfl_xor(r_kl, o, 64);
      r_bl += __shfl_xor(r_bl, o, 64); r_ent += __shfl_xor(r_ent, o, 64);
    }
  }
  if (tid < MB * 32 && (tid % 32) == 0) {
    const int s = tid / 32;
    const PpoRowTerms t = ppo_row_terms(D, D.adv[r0 + s], D.mb_neglogp[r0 + s], ppo_neglogp(r_nlp, A), D.returns[r0 + s], D.mb_values[r0 + s],
                                        s_v[0][s], s_v[1][s], invM);
    s_gnlp[s] = t.gnlp;
    s_dv[0][s] = t.dv[0]; s_dv[1][s] = t.dv[1];
    s_stat[s][1] = t.a_loss; s_stat[s][2] = t.closs[0]; s_stat[s][3] = r_bl; s_stat[s][4] = r_kl;
    s_stat[s][5] = t.closs[1]; s_stat[s][6] = r_ent;
  }
  __syncthreads();
  if (tid < MB * 32) {
    const int s = tid / 32, a = tid % 32;
    float dmu = 0.0f;
    if (a < A) {
      const float sg = expf(s_ls[a]), mu = s_mu[s][a];
      dmu = ppo_action_grad(s_gnlp[s], s_z[s][a], sg, mu, D.bounds_coef, invM).dmu;
      D.mb_mus[(r0 + s) * A + a] = mu;                                                            // RC:1358
      D.mb_sigmas[(r0 + s) * A + a] = sg;
    }
    s_dmu[s][a] = dmu;
    D.dhead[(size_t)par * MB * 34 + s * 34 + a] = dmu;
    if (a < 2) D.dhead[(size_t)par * MB * 34 + s * 34 + 32 + a] = s_dv[a][s];
  }
  if (tid >= 512 && tid < 512 + A) {
    const int a = tid - 512;
    float dls = 0.0f;
    for (int s = 0; s < MB; ++s) dls += ppo_dlogstd_term(s_gnlp[s], s_z[s][a], invM);
    dls = ppo_dlogstd(dls, D.entropy_coef);   // the norm below sees this value
    D.dlogstd[(size_t)par * 32 + a] = dls;
    s_dls[a] = dls;
  }
  if (tid == 0) {
    for (int j = 1; j <= 6; ++j) {
      float t = 0.0f;
      for (int s = 0; s < MB; ++s) t += s_stat[s][j];
      gctl->acc[j] = t;
    }
  }
  __syncthreads();
  STAMP(3);
  // ---- backward through the heads: dY2[net][s][k] = (sum_rows dhead * W_head[row][k]) * elu'(h[net][s][k])
  for (int i = tid; i < 3 * MB * U; i += 1024) {
    const int net = i / (MB * U), s = (i / U) % MB, k = i % U;
    float d = 0.0f;
    if (net == 0) { for (int a = 0; a < A; ++a) d += s_dmu[s][a] * s_w[a][k]; }
    else d = s_dv[net - 1][s] * s_w[A + net - 1][k];
    const float v = d * elu_grad_from_out(s_h[net][s][k]);
    s_dy2[net][s][k] = v;
    D.dy2[net][(size_t)par * MB * U + s * U + k] = v;
  }
  __syncthreads();
  STAMP(4);
  // ---- gradient-norm pieces available here: heads (dhead x h) and trunk layer 2 (dy2 x x[net][2], Gram from k_layer).
  // Six Gram matrices (h and dy2 of the three nets, K = 256): one wave each, 4 elements per lane, DPP reductions,
  // results written by lane 0 (no atomics).  Waves 6..8 do the bias-gradient norms of layer 2.
  if (wave < 6) {
    const int net = wave % 3;
    const float* v = wave < 3 ? &s_h[net][0][0] : &s_dy2[net][0][0];
    float* out = wave < 3 ? s_gh[net] : s_gd[net];
    float x[MB][4];
#pragma unroll
    for (int a = 0; a < MB; ++a)
#pragma unroll
      for (int j = 0; j < 4; ++j) x[a][j] = v[a * 256 + lane + 64 * j];
#pragma unroll
    for (int a = 0; a < MB; ++a)
#pragma unroll
      for (int b2 = 0; b2 <= a; ++b2) {
        const float r = wave_sum(x[a][0] * x[b2][0] + x[a][1] * x[b2][1] + x[a][2] * x[b2][2] + x[a][3] * x[b2][3]);
        if (lane == 0) { out[a * MB + b2] = r; out[b2 * MB + a] = r; }
      }
  } else if (wave < 9) {
    const int net = wave - 6;
    float bs = 0.0f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float sb = 0.0f;
#pragma unroll
      for (int s2 = 0; s2 < MB; ++s2) sb += s_dy2[net][s2][lane + 64 * j];
      bs += sb * sb;
    }
    bs = wave_sum(bs);
    if (lane == 0) s_n2[net] = bs;
  }
  __syncthreads();
  // n2 of heads + layer 2: thread (net, a, b) forms one term, 3 threads add them up
  if (tid < 3 * MB * MB) {
    const int net = tid / (MB * MB), a = (tid / MB) % MB, b2 = tid % MB;
    float dd = 0.0f;
    if (net == 0) { for (int j = 0; j < A; ++j) dd += s_dmu[a][j] * s_dmu[b2][j]; }
    else dd = s_dv[net - 1][a] * s_dv[net - 1][b2];
    s_term[tid] = dd * s_gh[net][a * MB + b2] + s_gd[net][a * MB + b2] * ctl->gx[net][2][a * MB + b2];
  } else if (tid >= 256 && tid < 256 + 32) {   // head bias gradients (mu biases, the two value biases) and logstd
    const int j = tid - 256;
    float t = 0.0f;
    if (j < A) { float sb = 0; for (int a = 0; a < MB; ++a) sb += s_dmu[a][j]; t = sb * sb + s_dls[j] * s_dls[j]; }
    s_bterm[j] = t;
  }
  __syncthreads();
  if (tid < 3) {
    const int net = tid;
    float n2 = 0.0f;
    for (int i = 0; i < MB * MB; ++i) n2 += s_term[net * MB * MB + i];
    if (net == 0) { for (int j = 0; j < A; ++j) n2 += s_bterm[j]; }
    else { float sb = 0; for (int a = 0; a < MB; ++a) sb += s_dv[net - 1][a]; n2 += sb * sb; }
    s_n2p[net] = n2;
  }
  __syncthreads();
  if (tid < 3) gctl->n2_part[tid] = s_n2p[tid] + s_n2[tid];
  STAMP(5);
}

// B-kernel: backward of trunk layer l+1 into dxacc of layer l for all nets:
//   dxacc_l[s][k] += sum_{n in split} dY_{l+1}[s][n] W_{l+1}[n][k]; thread per k, block per (net, k-chunk, n-split).
template <int MB>
__global__ __launch_bounds__(256) void k_back(SdxpDev D, int l) {   // l = layer whose output gradient is produced (1 or 0)
  const SdxpCtrl* ctl = D.ctrl;
  const int par = ctl->step & 1;
  const int Nn = D.units[l + 1], K = D.units[l];
  const int kchunks = (K + 255) / 256, splits = D.bsplit;
  const int per_net = kchunks * splits;
  const int net = blockIdx.x / per_net, rem = blockIdx.x % per_net, kc = rem / splits, sp = rem % splits;
  const int k = kc * 256 + threadIdx.x;
  __shared__ float s_dy[MB][64];
  const int n_per = (Nn + splits - 1) / splits, n0 = sp * n_per, n1 = min(Nn, n0 + n_per);
  const TrunkSlot t = trunk_slot(D, net, l + 1);
  const float* P = t.P;
  const size_t woff = t.woff;
  float acc[MB];
#pragma unroll
  for (int s = 0; s < MB; ++s) acc[s] = 0.0f;
  for (int nb = n0; nb < n1; nb += 64) {
    __syncthreads();
    for (int i = threadIdx.x; i < MB * 64; i += 256) {
      const int s = i / 64, n = nb + (i % 64);
      s_dy[s][i % 64] = n < n1 ? dy_at<MB>(D, net, l + 1, par, s, n) : 0.0f;
    }
    __syncthreads();
    if (k < K) {
      const int cnt = min(64, n1 - nb);
      for (int j = 0; j < cnt; ++j) {
        const float w = P[woff + (size_t)(nb + j) * K + k];
#pragma unroll
        for (int s = 0; s < MB; ++s) acc[s] += s_dy[s][j] * w;
      }
    }
  }
  if (k < K) {
    float* out = D.dxacc[net][l] + (size_t)par * MB * K;
#pragma unroll
    for (int s = 0; s < MB; ++s) atomicAdd(&out[s * K + k], acc[s]);
  }
}

// CTRL kernel (one block of 1024 threads): finishes the gradient norms (layers 0 and 1 from dxacc*elu' and the stored
// input Grams; layer 2 + heads from k_head), clip scales, Adam bias corrections, legacy adaptive LR (PS:306-312),
// statistics, advances the minibatch cursor and clears the other parity's dxacc.
// advance bits: 1 = a minibatch was just back-propagated; 2 = move the cursor; 8 = explicit-gradient (multi-rank) mode.
template <int MB>
__global__ __launch_bounds__(1024) void k_ctrl(SdxpDev D, int advance) {
  __shared__ float s_gd[3][2][MAXG];
  __shared__ float s_b[3];
  __shared__ float s_part[16][MAXG + 1];
  __shared__ SdxpCtrl s_ctl;               // snapshot: the single-thread bookkeeping below runs on LDS, not on HBM
  SdxpCtrl* gctl = D.ctrl;
  const int tid = threadIdx.x;
  for (int i = tid; i < (int)(sizeof(SdxpCtrl) / 4); i += 1024) reinterpret_cast<uint32_t*>(&s_ctl)[i] = reinterpret_cast<const uint32_t*>(gctl)[i];
  if (tid < 3 * 2 * MAXG) (&s_gd[0][0][0])[tid] = 0.0f;
  if (tid < 3) s_b[tid] = 0.0f;
  __syncthreads();
  SdxpCtrl* ctl = &s_ctl;
  const int par = ctl->step & 1;
  if (threadIdx.x == 0) D.dbg[8] = (long long)__builtin_readcyclecounter();
  if (advance & 1) {
    // (net, l) groups of dY vectors: l = 0 groups (units[0] long) get 3 waves each, l = 1 groups 2 waves each; a wave
    // accumulates lane-wise over its 64-neuron chunks and reduces ONCE (11 DPP sums), partials go to LDS.
    const int wave = tid >> 6, lane = tid & 63;
    if (wave < 15) {
      const int l = wave < 9 ? 0 : 1;
      const int net = wave < 9 ? wave / 3 : (wave - 9) / 2;
      const int sub = wave < 9 ? wave % 3 : (wave - 9) % 2, nsub = wave < 9 ? 3 : 2;
      const int C = D.units[l] / 64;
      float g[MB][MB], bs = 0.0f;
#pragma unroll
      for (int a = 0; a < MB; ++a)
#pragma unroll
        for (int b2 = 0; b2 < MB; ++b2) g[a][b2] = 0.0f;
      for (int c = sub; c < C; c += nsub) {
        const int n = c * 64 + lane;
        float v[MB], sb = 0.0f;
#pragma unroll
        for (int a = 0; a < MB; ++a) { v[a] = dy_at<MB>(D, net, l, par, a, n); sb += v[a]; }
        bs += sb * sb;
#pragma unroll
        for (int a = 0; a < MB; ++a)
#pragma unroll
          for (int b2 = 0; b2 <= a; ++b2) g[a][b2] += v[a] * v[b2];
      }
#pragma unroll
      for (int a = 0; a < MB; ++a)
#pragma unroll
        for (int b2 = 0; b2 <= a; ++b2) {
          const float r = wave_sum(g[a][b2]);
          if (lane == 0) { s_part[wave][a * MB + b2] = r; s_part[wave][b2 * MB + a] = r; }
        }
      const float rb = wave_sum(bs);
      if (lane == 0) s_part[wave][MAXG] = rb;
    }
    __syncthreads();
    if (threadIdx.x == 0) D.dbg[9] = (long long)__builtin_readcyclecounter();
    // n2[net] = n2_part[net] + sum_l sum_ab Gd[net][l][ab] * Gx[net][l][ab] + bias terms: thread (net, l, ab)
    if (tid < 3 * 2 * MB * MB) {
      const int net = tid / (2 * MB * MB), l = (tid / (MB * MB)) % 2, ab = tid % (MB * MB);
      float gd = 0.0f;
      if (l == 0) { for (int w = 0; w < 3; ++w) gd += s_part[net * 3 + w][ab]; }
      else { for (int w = 0; w < 2; ++w) gd += s_part[9 + net * 2 + w][ab]; }
      s_gd[net][l][ab] = gd * ctl->gx[net][l][ab];
    }
    __syncthreads();
    if (tid == 0) {
      float n2[3];
      for (int net = 0; net < 3; ++net) {
        float s = ctl->n2_part[net];
        for (int w = 0; w < 3; ++w) s += s_part[net * 3 + w][MAXG];
        for (int w = 0; w < 2; ++w) s += s_part[9 + net * 2 + w][MAXG];
        for (int l = 0; l < 2; ++l)
          for (int i = 0; i < MB * MB; ++i) s += s_gd[net][l][i];
        n2[net] = s;
      }
      const float ac_norm = sqrtf(n2[0] + n2[1]), cv_norm = sqrtf(n2[2]);
      ctl->ac_gnorm = ac_norm; ctl->cv_gnorm = cv_norm;
      ctl->ac_gscale = ppo_clip_scale(D, ac_norm);
      ctl->cv_gscale = ppo_clip_scale(D, cv_norm);
      const bool explicit_mode = (advance & 8) != 0;   // multi-rank: Adam/LR happen in sdxp_apply after the all-reduce
      if (!explicit_mode) {
        ctl->ac_t += 1; ctl->cv_t += 1;
        ctl->ac_b1pow *= 0.9; ctl->ac_b2pow *= 0.999; ctl->cv_b1pow *= 0.9; ctl->cv_b2pow *= 0.999;
        ctl->ac_bc1 = (float)(1.0 - ctl->ac_b1pow); ctl->ac_bc2 = (float)(1.0 - ctl->ac_b2pow);
        ctl->cv_bc1 = (float)(1.0 - ctl->cv_b1pow); ctl->cv_bc2 = (float)(1.0 - ctl->cv_b2pow);
        ctl->ac_lr_applied = ctl->ac_lr; ctl->cv_lr_applied = ctl->cv_lr;
        ctl->ac_pending = 1; ctl->cv_pending = 1;
      } else ppo_explicit_reset(*ctl);
      // explicit mode: this rank's minibatch KL rides with factors / gradients, and the learning rate moves in the apply
      const float kl = ppo_account_minibatch(*ctl, 1.0f / (float)MB, explicit_mode ? &D.ac_g[D.g_tail] : nullptr);
      if (explicit_mode) D.fact[D.foff.kl] = kl;
      else ppo_lr_advance(*ctl, D, kl);
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) D.dbg[10] = (long long)__builtin_readcyclecounter();
  if (advance & 2) {
    if (tid == 0) ppo_advance_cursor(*ctl, D.num_minibatches, (advance & 1) != 0);
    // the split-N accumulators of the parity that the NEXT step will write must start from zero
    const int npar = (advance & 1) ? (par ^ 1) : par;
    for (int net = 0; net < 3; ++net)
      for (int l = 0; l < 2; ++l) {
        float* a = D.dxacc[net][l] + (size_t)npar * MB * D.units[l];
        for (int i = tid; i < MB * D.units[l]; i += 1024) a[i] = 0.0f;
      }
  }
  __syncthreads();
  // write the header of the control block back (the Gram area gx is owned by the L kernels and left untouched)
  for (int i = tid; i < (int)(offsetof(SdxpCtrl, gx) / 4); i += 1024) reinterpret_cast<uint32_t*>(gctl)[i] = reinterpret_cast<const uint32_t*>(&s_ctl)[i];
  for (int i = (int)(offsetof(SdxpCtrl, rms_count) / 4) + tid; i < (int)(sizeof(SdxpCtrl) / 4); i += 1024) reinterpret_cast<uint32_t*>(gctl)[i] = reinterpret_cast<const uint32_t*>(&s_ctl)[i];
  if (threadIdx.x == 0) D.dbg[11] = (long long)__builtin_readcyclecounter();
}

// central-value input normalisation for the whole epoch, hoisted out of the minibatch loop: thread = feature, sequential
// over the minibatches exactly like RunningMeanStd in train mode (update with the minibatch, then normalise it) during
// mini-epoch 0 -> cvx0; statistics frozen afterwards (App. C) -> cvx1 for mini-epochs >= 1.
template <int MB>
__global__ void k_cv_prenorm(SdxpDev D) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= D.state_dim) return;
  const int S = D.state_dim;
  const float* __restrict__ src = D.mb_states;
  float* __restrict__ dst = D.cvx0;
  double mean = D.rms_mean[k], var = D.rms_var[k], cnt = D.ctrl->rms_count;
  // the running statistics form a serial chain over the minibatches; the rows of the next minibatch are fetched while the
  // chain of the current one runs, so that the chain, not the HBM latency, sets the time per minibatch
  float xn[MB];
#pragma unroll
  for (int s = 0; s < MB; ++s) xn[s] = src[(size_t)s * S + k];
  for (int mb = 0; mb < D.num_minibatches; ++mb) {
    float x[MB];
#pragma unroll
    for (int s = 0; s < MB; ++s) x[s] = xn[s];
    if (mb + 1 < D.num_minibatches) {
#pragma unroll
      for (int s = 0; s < MB; ++s) xn[s] = src[((size_t)(mb + 1) * MB + s) * S + k];
    }
    if (D.cv_normalize_input) {
      double bm = 0.0, bv = 0.0;
#pragma unroll
      for (int s = 0; s < MB; ++s) bm += x[s];
      bm /= MB;
#pragma unroll
      for (int s = 0; s < MB; ++s) { const double d = x[s] - bm; bv += d * d; }
      bv = MB > 1 ? bv / (MB - 1) : 0.0;
      const double delta = bm - mean, tot = cnt + MB;
      const double m2 = var * cnt + bv * MB + delta * delta * cnt * MB / tot;
      mean = mean + delta * MB / tot;
      var = m2 / tot;
      cnt = tot;
    }
    const float fm = (float)mean, rs = sqrtf((float)var + 1e-5f);
#pragma unroll
    for (int s = 0; s < MB; ++s)
      dst[((size_t)mb * MB + s) * S + k] = D.cv_normalize_input ? clampf((x[s] - fm) / rs, -5.0f, 5.0f) : x[s];
  }
  D.rms_mean[k] = mean; D.rms_var[k] = var;
  // rms_count is advanced by k_cv_rms_count AFTER this launch: every block of this grid reads the starting count above, and no
  // ordering exists between the blocks of one launch
}
__global__ void k_cv_rms_count(SdxpDev D, int rows) { if (D.cv_normalize_input) D.ctrl->rms_count += (double)rows; }
// mini-epochs >= 1: statistics frozen at their end-of-mini-epoch-0 values -> cvx1 (one thread per element)
__global__ __launch_bounds__(256) void k_cv_prenorm_frozen(SdxpDev D) {
  const int S = D.state_dim;
  const size_t total = (size_t)D.N * D.horizon * S;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int k = (int)(i % S);
    const float x = D.mb_states[i];
    const float fm = (float)D.rms_mean[k], rs = sqrtf((float)D.rms_var[k] + 1e-5f);
    D.cvx1[i] = D.cv_normalize_input ? clampf((x - fm) / rs, -5.0f, 5.0f) : x;
  }
}

// ------------------------------------------------------------------------------------------------ explicit gradients
// world_size > 1: the minibatch gradient is materialised into the flat *_GRADS buffers (same layout as the
// parameters) so that the caller can all-reduce it with RCCL; then sq-norm, clip and Adam run elementwise.
template <int MB>
__global__ __launch_bounds__(256) void k_grad_layer(SdxpDev D, int l) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const SdxpCtrl* ctl = D.ctrl;
  const int par = ctl->step & 1, Nl = D.units[l];
  const int blocks_per_net = (Nl + 3) / 4;
  const int net = blockIdx.x / blocks_per_net, n = (blockIdx.x % blocks_per_net) * 4 + wave;
  const TrunkSlot t = trunk_slot(D, net, l);
  const int K = t.K;
  float* G = t.G;
  const size_t woff = t.woff, boff = t.boff;
  const float* gx = layer_input<MB>(D, ctl, net, l, true);
  for (int i = tid; i < MB * K; i += 256) sm[i] = gx[i];
  __syncthreads();
  if (n >= Nl) return;
  float dyn[MB], sb = 0.0f;
#pragma unroll
  for (int s = 0; s < MB; ++s) { dyn[s] = dy_at<MB>(D, net, l, par, s, n); sb += dyn[s]; }
  for (int k = lane; k < K; k += 64) {
    float g = 0.0f;
#pragma unroll
    for (int s = 0; s < MB; ++s) g += dyn[s] * sm[s * K + k];
    G[woff + (size_t)n * K + k] = g;
  }
  if (lane == 0) G[boff + n] = sb;
}
template <int MB>
__global__ __launch_bounds__(256) void k_grad_heads(SdxpDev D) {
  const int tid = threadIdx.x, par = D.ctrl->step & 1, U = D.units[2], A = D.act_dim;
  const float* dh = D.dhead + (size_t)par * MB * 34;
  for (int i = tid; i < (A + 2) * U; i += 256) {
    const int row = i / U, k = i % U;
    const HeadRow hr = head_row(D, row);
    const float* h = D.x[hr.net][3] + (size_t)par * MB * U;
    float g = 0.0f;
    for (int s = 0; s < MB; ++s) g = fmaf(dh[s * 34 + hr.col], h[s * U + k], g);   // (spelled out: left to the compiler the products are paired and added unfused)
    (hr.buf ? D.cv_g : D.ac_g)[hr.woff + k] = g;
  }
  if (tid < A + 2) {
    const HeadRow hr = head_row(D, tid);
    float g = 0.0f;
    for (int s = 0; s < MB; ++s) g += dh[s * 34 + hr.col];
    (hr.buf ? D.cv_g : D.ac_g)[hr.boff] = g;
  }
  if (tid < A) D.ac_g[D.off.logstd + tid] = D.dlogstd[(size_t)par * 32 + tid];
}
// ---- multi-rank path, factor exchange: instead of all-reducing 13.4 MB of materialised gradients per optimiser step the ranks
// all-gather the rank-MB factors (194 KB each) and every rank rebuilds the SUM over ranks of dY^T X locally.
template <int MB>
__global__ __launch_bounds__(256) void k_pack_factors(SdxpDev D) {
  const SdxpCtrl* ctl = D.ctrl;
  const int par = ctl->step & 1, seg = blockIdx.y;
  float* F = D.fact;
  const int stride = gridDim.x * 256, t0 = blockIdx.x * 256 + threadIdx.x;
  if (seg < 9) {
    const int net = seg / 3, l = seg % 3;
    const int K = trunk_slot(D, net, l).K;
    const float* src = layer_input<MB>(D, ctl, net, l, true);
    for (int i = t0; i < MB * K; i += stride) F[D.foff.x[net][l] + i] = src[i];
  } else if (seg < 18) {
    const int net = (seg - 9) / 3, l = (seg - 9) % 3, Nl = D.units[l];
    for (int i = t0; i < MB * Nl; i += stride) F[D.foff.dy[net][l] + i] = dy_at<MB>(D, net, l, par, i / Nl, i % Nl);
  } else if (seg < 21) {
    const int net = seg - 18, U = D.units[2];
    const float* src = D.x[net][3] + (size_t)par * MB * U;
    for (int i = t0; i < MB * U; i += stride) F[D.foff.h[net] + i] = src[i];
  } else if (seg == 21) {
    for (int i = t0; i < MB * 34; i += stride) F[D.foff.dh + i] = D.dhead[(size_t)par * MB * 34 + i];
  } else {
    for (int i = t0; i < 32; i += stride) F[D.foff.dls + i] = D.dlogstd[(size_t)par * 32 + i];
  }
}

template <int MB, int RPW, int KI>
static void launch_layer(const SdxpDev* D, int l, int Kmax, hipStream_t st) {
  const int blocks = 3 * ((D->units[l] + 4 * RPW - 1) / (4 * RPW));
  hipLaunchKernelGGL((k_layer<MB, RPW, KI>), dim3(blocks), dim3(256), (size_t)2 * MB * Kmax * sizeof(float), st, *D, l);
}
template <int MB>
static void launch_layers(const SdxpDev* D, hipStream_t st) {
  for (int l = 0; l < 3; ++l) {
    const int Kmax = trunk_kmax(D, l);
    const int ki = (Kmax / 4 + 63) / 64;   // float4 columns per lane
    const bool two = (3 * D->units[l]) / 4 >= 512;   // 2 rows per wave when there are plenty of rows
    if (ki <= 1) { if (two) launch_layer<MB, 2, 1>(D, l, Kmax, st); else launch_layer<MB, 1, 1>(D, l, Kmax, st); }
    else if (ki == 2) { if (two) launch_layer<MB, 2, 2>(D, l, Kmax, st); else launch_layer<MB, 1, 2>(D, l, Kmax, st); }
    else if (ki == 3) { if (two) launch_layer<MB, 2, 3>(D, l, Kmax, st); else launch_layer<MB, 1, 3>(D, l, Kmax, st); }
    else { if (two) launch_layer<MB, 2, 4>(D, l, Kmax, st); else launch_layer<MB, 1, 4>(D, l, Kmax, st); }
  }
}
template <int MB>
static void launch_fwd_bwd(const SdxpDev* D, hipStream_t st) {
  launch_layers<MB>(D, st);
  hipLaunchKernelGGL(k_head<MB>, dim3(1), dim3(1024), 0, st, *D, 0);
  for (int l = 1; l >= 0; --l) {
    const int K = D->units[l];
    hipLaunchKernelGGL(k_back<MB>, dim3(3 * ((K + 255) / 256) * D->bsplit), dim3(256), 0, st, *D, l);
  }
}
template <int MB>
static void launch_step(const SdxpDev* D, hipStream_t st) {
  launch_fwd_bwd<MB>(D, st);
  hipLaunchKernelGGL(k_ctrl<MB>, dim3(1), dim3(1024), 0, st, *D, 1 | 2);
}
__global__ void k_ctrl_begin_epoch(SdxpCtrl* c) {
  c->mb_index = 0; c->mini_epoch = 0; c->n_mb = 0; c->prev_mb = 0; c->prev_mini_epoch = 0;
  c->sum_a_loss = c->sum_c_loss = c->sum_b_loss = c->sum_kl = c->sum_cv_loss = c->sum_entropy = 0.0f;
  for (int i = 0; i < 8; ++i) c->acc[i] = 0.0f;
}
// cursor and loss sums of the control block back to the start of an epoch's update phase (every update path)
extern "C" void sdxpk_begin_epoch(const SdxpDev* D, hipStream_t st) { hipLaunchKernelGGL(k_ctrl_begin_epoch, dim3(1), dim3(1), 0, st, D->ctrl); }
extern "C" int sdxpk_update_step(const SdxpDev* D, int mb_size, hipStream_t st) {
  return sdxp_for_minibatch(mb_size, [&](auto m) { launch_step<decltype(m)::value>(D, st); });
}
// multi-rank steps: forward/backward of the minibatch under the cursor, then what leaves this rank - the flat gradients for an
// all-reduce (explicit) or the packed rank-MB factors for an all-gather; sdxp_multirank.hip has what follows the exchange
static int launch_backward(const SdxpDev* D, int mb_size, bool factors, hipStream_t st) {
  return sdxp_for_minibatch(mb_size, [&](auto m) {
    constexpr int M = decltype(m)::value;
    launch_fwd_bwd<M>(D, st);
    if (factors) hipLaunchKernelGGL(k_pack_factors<M>, dim3(8, 23), dim3(256), 0, st, *D);
    for (int l = 0; l < 3 && !factors; ++l)
      hipLaunchKernelGGL(k_grad_layer<M>, dim3(trunk_row_blocks(*D, l)), dim3(256), (size_t)M * trunk_kmax(D, l) * sizeof(float), st, *D, l);
    if (!factors) hipLaunchKernelGGL(k_grad_heads<M>, dim3(1), dim3(256), 0, st, *D);
    hipLaunchKernelGGL(k_ctrl<M>, dim3(1), dim3(1024), 0, st, *D, 1 | 2 | 8);
  });
}
extern "C" int sdxpk_backward_explicit(const SdxpDev* D, int mb_size, hipStream_t st) { return launch_backward(D, mb_size, false, st); }
extern "C" int sdxpk_backward_factors(const SdxpDev* D, int mb_size, hipStream_t st) { return launch_backward(D, mb_size, true, st); }
// central-value pre-normalisation for all minibatches of the epoch
extern "C" int sdxpk_prenorm(const SdxpDev* D, int mb_size, hipStream_t st) {
  return sdxp_for_minibatch(mb_size, [&](auto m) {
    constexpr int M = decltype(m)::value;
    hipLaunchKernelGGL(k_cv_prenorm<M>, dim3((D->state_dim + 63) / 64), dim3(64), 0, st, *D);
    hipLaunchKernelGGL(k_cv_rms_count, dim3(1), dim3(1), 0, st, *D, D->num_minibatches * M);
    hipLaunchKernelGGL(k_cv_prenorm_frozen, dim3(1024), dim3(256), 0, st, *D);
  });
}
// begin of an epoch's update phase on the multi-kernel paths: the pre-normalisation, then the cursor move that clears the accumulators
extern "C" int sdxpk_update_begin(const SdxpDev* D, int mb_size, hipStream_t st) {
  if (sdxpk_prenorm(D, mb_size, st)) return -1;
  return sdxp_for_minibatch(mb_size, [&](auto m) { hipLaunchKernelGGL(k_ctrl<decltype(m)::value>, dim3(1), dim3(1024), 0, st, *D, 2); });
}
// flush: apply the last pending optimiser step (the L/HEAD kernels run once more on the staged minibatch; their forward outputs are discarded)
extern "C" int sdxpk_update_flush_layers(const SdxpDev* D, int mb_size, hipStream_t st) {
  return sdxp_for_minibatch(mb_size, [&](auto m) {
    constexpr int M = decltype(m)::value;
    launch_layers<M>(D, st);
    hipLaunchKernelGGL(k_head<M>, dim3(1), dim3(1024), 0, st, *D, 1);
  });
}
