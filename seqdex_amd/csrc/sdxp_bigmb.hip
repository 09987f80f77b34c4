// sdxp_bigmb.hip — large-minibatch PPO optimiser step (minibatch_size > 8) for gfx950.
//
// The reference trains the insert policy with minibatch_size 4096 (cfg/lego/ppo_continuous_insert.yaml:50,75) and BASELINE.md asks
// for a labelled large-minibatch variant next to the shipped minibatch of 4.  With thousands of samples per step the update is
// GEMM-shaped, not the rank-MB weight streaming of sdxp_update.hip / sdxp_persist.hip: forward Y = ELU(X W^T + b), data gradient
// dX = (dY W) * ELU'(H), weight gradient G = dY^T X, all three on the f32-input matrix cores (v_mfma_f32_32x32x2_f32: exact fp32,
// k-ordered fma chain), LDS-tiled 128x128x32 per 256-thread workgroup (4 waves of 64x64; 64x64x16 for small problems), the
// same layer of the three networks in one launch.  rl_games' calc_gradients
// (a2c_continuous.py / RC:1796-1877) + CentralValueTrain.train_net for all three networks of one minibatch:
//
//   forward 3 nets x 3 trunk layers (NT GEMM, bias + ELU fused) -> mu head (NT GEMM) + two value heads (row dots)
//   k_big_head: per-sample PPO losses and their head gradients (the formulas of sdxp_ppo_terms.h), block partials
//   k_big_fin:  statistics, d logstd, KL word, minibatch bookkeeping of the control block
//   backward: head data gradients, then per net  G_l = dY_l^T X_l (TN GEMM, split over the minibatch rows, partials reduced in a
//   fixed order: deterministic), b_l = column sums of dY_l, dY_{l-1} = (dY_l W_l) * ELU'(H_{l-1}) (NN GEMM, fused)
//   -> flat gradients in ac_g / cv_g (parameter layout), then the explicit clip + Adam of sdxp_multirank.hip (k_sqnorm2 / k_adam2).
//
// The central-value input normalisation (RunningMeanStd in train mode: update with the minibatch, then normalise it, during
// mini-epoch 0; frozen afterwards) is hoisted out of the loop as in the small-minibatch path, with column statistics reduced in fp64.
//
// This file is the host side: set-up, the per-epoch pre-normalisation, the three phases of a step (big_forward, big_heads,
// big_backward) and the test hooks.  The kernels are in sdx_gemm.h / sdx_gemm_nt.h (trunk products, with the functions that describe a
// product by the role of its operands), sdxp_bigmb_heads.h (head section and the layouts of its partials) and sdxp_bigmb_stats.h
// (input statistics).  The trunk products take one of three paths, fixed per handle by sdxpk_big_setup: k_gemm (any shape), k_gemm_nt
// on staged operands with transposed copies (ws->nt), or k_gemm_nt with k_gemm_tt for the weight gradients (ws->nt && ws->tt, fp32).
#include "sdx_common.h"
#include "sdxp_launch.h"
#include "sdxp_ppo_terms.h"
#include <cstddef>
#include <cstdint>
#include <cstdlib>

#include "sdx_gemm.h"
#include "sdx_gemm_nt.h"
#include "sdxp_bigmb_heads.h"   // head kernels, BIGP / HPZ, HeadsLds, HeadParts, big_splits, heads_nrb / heads_blocks
#include "sdxp_bigmb_stats.h"   // k_big_colstats, k_big_rms_update, k_big_rms_count, k_big_normalise

// ------------------------------------------------------------------------------------------------ set-up
// floats of ws->part per network (the workspace holds three such regions): the largest of the trunk's weight-gradient splits
// (nsplit x [W_l | b_l]), the 13-launch head section's partials and a third of the fused head kernel's records, which span the three regions
static size_t big_part_floats(const SdxpDev* D, const SdxpBigWs& w) {
  size_t mx = 0;
  for (int net = 0; net < 3; ++net)
    for (int l = 0; l < 3; ++l) {
      const size_t pz = (size_t)D->units[l] * w.layer[net][l].K + D->units[l];
      if (pz > mx) mx = pz;
    }
  const size_t need = (size_t)w.nsplit * mx, hp = head_parts(*D, w.MB).floats, hf = ((size_t)heads_blocks(w.MB) * HPZ + 2) / 3;
  const size_t m1 = need > hp ? need : hp;
  return m1 > hf ? m1 : hf;
}
// lowers the large-minibatch options to what shapes and device allow, sets the LDS attributes of the kernels that stay (NT path: 16-byte aligned windows)
static void big_prepare(const SdxpDev* D, int MB, SdxpOpts* o) {
  int dev = 0, lds = 0;
  if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&lds, hipDeviceAttributeMaxSharedMemoryPerBlock, dev) != hipSuccess) lds = 0;
  o->bigmb_fused_heads = o->bigmb_fused_heads && D->units[2] == HU && D->act_dim <= 23;
  if (o->bigmb_fused_heads && (lds < (int)sizeof(HeadsLds) || hipFuncSetAttribute(reinterpret_cast<const void*>(k_big_heads),
                                                                   hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(HeadsLds)) != hipSuccess)) {
    fprintf(stderr, "libseqdex_hip: k_big_heads cannot have %zu bytes of LDS on device %d: this handle uses the 13-launch head section\n", sizeof(HeadsLds), dev);
    o->bigmb_fused_heads = 0;
  }
  o->bigmb_nt = o->bigmb_nt && MB % 8 == 0 && D->units[0] % 128 == 0 && D->units[1] % 128 == 0 && D->units[2] % 128 == 0 && D->obs_dim % 4 == 0 &&
                D->state_dim % 4 == 0;
  o->bigmb_tt = o->bigmb_tt && o->bigmb_nt && !D->bf16;
  if (o->bigmb_nt && !(D->bf16 ? gemm_nt_prepare<1, EPI_FWD>() && gemm_nt_prepare<1, EPI_NN>() && gemm_nt_prepare<1, EPI_TN>()
                               : gemm_nt_prepare<0, EPI_FWD>() && gemm_nt_prepare<0, EPI_NN>() && gemm_nt_prepare<0, EPI_TN>() && (!o->bigmb_tt || gemm_tt_prepare()))) {
    fprintf(stderr, "libseqdex_hip: k_gemm_nt / k_gemm_tt cannot have their LDS on device %d: this handle's trunk products use k_gemm\n", dev);
    o->bigmb_nt = o->bigmb_tt = 0;
  }
  (void)hipGetLastError();
}
// The workspace of one large minibatch (SdxpBigWs): activations and pre-activation gradients, split partials of the weight gradients and,
// on the NT path, the staged operands of sdx_gemm_nt.h.  Every buffer comes zero-filled from `alloc`: the padding the kernels never write stays zero
extern "C" int sdxpk_big_setup(const SdxpDev* D, int MB, SdxpOpts* o, SdxpAllocFn alloc, void* ctx, SdxpBigWs* ws) {
  big_prepare(D, MB, o);
  SdxpBigWs& w = *ws;
  int rc = 0;
  auto get = [&](auto*& p, size_t count, size_t elem) {
    void* q = nullptr;
    if (rc == 0) rc = alloc(ctx, &q, count * elem);
    p = static_cast<std::remove_reference_t<decltype(p)>>(q);
  };
  const int* units = D->units;
  const size_t BM = (size_t)MB, R = (size_t)D->N * D->horizon;
  w.MB = MB; w.nsplit = big_splits(MB);
  w.nt = o->bigmb_nt; w.tt = o->bigmb_tt; w.nt_tile = o->nt_tile; w.fused_heads = o->bigmb_fused_heads;
  if (w.nt) { w.KC = D->bf16 ? 64 : 32; w.MBp = (MB + w.KC - 1) / w.KC * w.KC; w.Rp = (int)R + 64; }
  for (int l = 0; l < 3; ++l) {
    const size_t woff[3] = {D->off.a_w[l], D->off.c_w[l], D->coff.w[l]}, boff[3] = {D->off.a_b[l], D->off.c_b[l], D->coff.b[l]};
    for (int net = 0; net < 3; ++net) {
      const int K = l == 0 ? (net == 2 ? D->state_dim : D->obs_dim) : units[l - 1];
      w.layer[net][l] = {K, w.nt ? (K + w.KC - 1) / w.KC * w.KC : K, woff[net], boff[net]};
    }
  }
  for (int net = 0; net < 3; ++net)
    for (int l = 0; l < 3; ++l) { get(w.h[net][l], BM * units[l], 4); get(w.dy[net][l], BM * units[l], 4); }
  get(w.mu, BM * 24, 4); get(w.dmu, BM * 24, 4); get(w.v, 2 * BM, 4); get(w.dv, 2 * BM, 4);
  w.part_region = big_part_floats(D, w);
  get(w.part, 3 * w.part_region, 4);
  get(w.dpart, (size_t)w.nsplit * D->state_dim * 2, 8);
  w.zeros = nullptr; if (w.tt) get(w.zeros, 64, 4);
  if (w.nt) {   // every operand of the NT products k-contiguous in the element type of the run
    const size_t ES = D->bf16 ? 2 : 4;
    for (int i = 0; i < 3; ++i) {
      const int kp0 = w.layer[i == 0 ? 0 : 2][0].kp;
      get(w.xn[i], R * kp0, ES); get(w.xt[i], (size_t)kp0 * w.Rp, ES);
    }
    for (int net = 0; net < 3; ++net)
      for (int l = 0; l < 3; ++l) {
        const int kp = w.layer[net][l].kp;
        get(w.wn[net][l], (size_t)units[l] * kp, ES);
        w.wt[net][l] = nullptr;
        if (l > 0) get(w.wt[net][l], (size_t)kp * units[l], ES);
        get(w.dyt[net][l], (size_t)units[l] * w.MBp, ES);
        w.dyn[net][l] = nullptr;
        if (l == 2 && !D->bf16) w.dyn[net][l] = w.dy[net][l];
        else if (l > 0) get(w.dyn[net][l], BM * units[l], ES);
        if (l < 2) {
          get(w.ht[net][l], (size_t)units[l] * w.MBp, ES);
          if (D->bf16) get(w.hn[net][l], BM * units[l], ES); else w.hn[net][l] = w.h[net][l];
        }
      }
  }
  return rc;
}
template <int BF>
static void stage_launch(const StageArgs* a, int count, hipStream_t st) {
  StageBatch sb;
  int Rx = 0, Kx = 0;
  for (int q = 0; q < 9; ++q) {
    sb.a[q] = a[q < count ? q : 0];
    if (q < count) { Rx = a[q].R > Rx ? a[q].R : Rx; Kx = a[q].Kp > Kx ? a[q].Kp : Kx; }
  }
  hipLaunchKernelGGL((k_stage<BF>), dim3((Kx + 63) / 64, (Rx + 63) / 64, count), dim3(256), 0, st, sb);
}
static void stage(const SdxpDev& D, const StageArgs* a, int count, hipStream_t st) {
  if (D.bf16) stage_launch<1>(a, count, st); else stage_launch<0>(a, count, st);
}

// central-value inputs of the whole epoch: cvx0 (statistics updated minibatch by minibatch, mini-epoch 0), cvx1 (frozen)
extern "C" void sdxpk_big_prenorm(const SdxpDev* D, const SdxpBigWs* ws, hipStream_t st) {
  const int MB = ws->MB, S = D->state_dim, nsplit = ws->nsplit, rchunk = (MB + nsplit - 1) / nsplit;
  for (int mb = 0; mb < D->num_minibatches; ++mb) {
    const size_t r0 = (size_t)mb * MB;
    if (D->cv_normalize_input) {
      hipLaunchKernelGGL(k_big_colstats, dim3((S + 63) / 64, nsplit), dim3(256), 0, st, *D, r0, MB, rchunk, ws->dpart);
      hipLaunchKernelGGL(k_big_rms_update, dim3((S + 255) / 256), dim3(256), 0, st, *D, MB, nsplit, ws->dpart);
      hipLaunchKernelGGL(k_big_rms_count, dim3(1), dim3(1), 0, st, *D, MB);
    }
    hipLaunchKernelGGL(k_big_normalise, dim3(1024), dim3(256), 0, st, *D, r0, (size_t)MB, D->cvx0);
  }
  hipLaunchKernelGGL(k_big_normalise, dim3(1024), dim3(256), 0, st, *D, (size_t)0, (size_t)D->N * D->horizon, D->cvx1);
  if (ws->nt) {   // the epoch's layer-0 inputs in the element type of the run, both orientations (sdx_gemm_nt.h): once per epoch
    const int R = D->N * D->horizon, kpo = ws->layer[0][0].kp, kps = ws->layer[2][0].kp;
    const StageArgs a[3] = {stage_args(D->mb_obs, R, D->obs_dim, kpo, ws->xn[0], ws->xt[0], ws->Rp),
                            stage_args(D->cvx0, R, D->state_dim, kps, ws->xn[1], ws->xt[1], ws->Rp),
                            stage_args(D->cvx1, R, D->state_dim, kps, ws->xn[2], ws->xt[2], ws->Rp)};
    stage(*D, a, 3, st);
  }
}

// ------------------------------------------------------------------------------------------------ one optimiser step
struct BigStep {   // what the three parts of one optimiser step share, per net (actor and critic share buffers and input rows)
  size_t r0;                                       // first dataset row of the minibatch
  const float* P[3]; float* G[3];                  // parameter / gradient buffer: ws->layer's woff / boff count from these
  const float* X0[3]; const void *Xn[3], *Xt[3];   // the minibatch's layer-0 input rows: fp32; staged (ws->xn), and staged transposed (ws->xt: row stride ws->Rp), on the NT path
};
static BigStep big_step_ctx(const SdxpDev& D, const SdxpBigWs* ws, int mb, int me) {
  const size_t r0 = (size_t)mb * ws->MB, ES = D.bf16 ? 2 : 4;   // ES: bytes per staged element
  const float* obs = D.mb_obs + r0 * D.obs_dim;
  BigStep c = {r0, {D.ac, D.ac, D.cv}, {D.ac_g, D.ac_g, D.cv_g}, {obs, obs, (me == 0 ? D.cvx0 : D.cvx1) + r0 * D.state_dim}, {}, {}};
  for (int net = 0; net < 3 && ws->nt; ++net) {
    const int sel = net < 2 ? 0 : (me == 0 ? 1 : 2);
    c.Xn[net] = (const char*)ws->xn[sel] + r0 * ws->layer[net][0].kp * ES;
    c.Xt[net] = (const char*)ws->xt[sel] + r0 * ES;
  }
  return c;
}

// forward: layer l of the three networks in one launch
static void big_forward(const SdxpDev& D, const SdxpBigWs* ws, const BigStep& c, hipStream_t st) {
  const int MB = ws->MB;
  if (ws->nt) {   // this step's weights in the element type, [out][in padded] and (layers 1, 2) transposed [in][out]
    StageArgs a[9];
    for (int net = 0; net < 3; ++net)
      for (int l = 0; l < 3; ++l) {
        const SdxpBigLayer& L = ws->layer[net][l];
        a[net * 3 + l] = stage_args(c.P[net] + L.woff, D.units[l], L.K, L.kp, ws->wn[net][l], ws->wt[net][l], D.units[l]);
      }
    stage(D, a, 9, st);
  }
  for (int l = 0; l < 3; ++l) {
    const int Nl = D.units[l];
    GemmArgs g[3];
    NtArgs n[3];
    for (int net = 0; net < 3; ++net) {
      const SdxpBigLayer& L = ws->layer[net][l];
      const float* b = c.P[net] + L.boff;
      if (!ws->nt) { g[net] = gemm_forward(l == 0 ? c.X0[net] : ws->h[net][l - 1], c.P[net] + L.woff, b, ws->h[net][l], Nl, MB, Nl, L.K); continue; }
      // bf16 runs keep the outputs of layers 0 and 1 in bf16 only (both orientations): the next layer, the weight gradient and the
      // ELU' of the backward pass read those; the last trunk layer stays fp32 for the fp32 heads.  Only the transposed-copy form of
      // the weight gradient reads a transposed layer output
      const bool elem = D.bf16 && l < 2;
      n[net] = nt_forward(l == 0 ? c.Xn[net] : ws->hn[net][l - 1], ws->wn[net][l], L.kp, b, MB, Nl, elem ? nullptr : ws->h[net][l],
                          elem ? ws->hn[net][l] : nullptr, (l < 2 && !ws->tt) ? ws->ht[net][l] : nullptr, ws->MBp);
    }
    if (!ws->nt) gemm<0, 0, 1>(g, 3, 1, st, D.bf16 != 0);
    else if (D.bf16) gemm_nt<1, EPI_FWD>(n, 3, 1, st, ws->nt_tile);
    else gemm_nt<0, EPI_FWD>(n, 3, 1, st, ws->nt_tile);
  }
}

// heads, losses, head backward: data gradients into dy[net][2], weight gradients into the flat buffers, control block advanced
static void big_heads(const SdxpDev& D, const SdxpBigWs* ws, const BigStep& c, hipStream_t st) {
  const int MB = ws->MB, A = D.act_dim, U2 = D.units[2];
  if (ws->fused_heads) {
    const int nrb = heads_nrb(MB), nb = heads_blocks(MB);
    hipLaunchKernelGGL(k_big_heads, dim3(nb), dim3(512), sizeof(HeadsLds), st, D, c.r0, MB, nrb, ws->h[0][2], ws->h[1][2], ws->h[2][2], ws->dy[0][2], ws->dy[1][2],
                       ws->dy[2][2], ws->part);
    hipLaunchKernelGGL(k_big_heads_reduce, dim3((HPZ + 31) / 32), dim3(256), 0, st, D, nb, MB, ws->part);
    return;
  }
  // The order matters to ws->part (HeadParts, sdxp_bigmb_heads.h): k_big_fin has folded k_big_head's loss partials before the policy
  // head's weight-gradient product writes its splits over them
  const HeadParts hp = head_parts(D, MB);
  const float *mu_w = D.ac + D.off.mu_w, *v_w = D.ac + D.off.v_w, *cv_w = D.cv + D.coff.v_w;
  float *vp0 = ws->part + hp.vp0, *vp1 = ws->part + hp.vp1;
  const GemmArgs gm = gemm_forward(ws->h[0][2], mu_w, D.ac + D.off.mu_b, ws->mu, 24, MB, A, U2);
  gemm<0, 0, 2>(&gm, 1, 1, st);
  hipLaunchKernelGGL(k_rowdot, dim3((MB + 3) / 4), dim3(256), 0, st, ws->h[1][2], U2, MB, v_w, D.ac + D.off.v_b, ws->v);
  hipLaunchKernelGGL(k_rowdot, dim3((MB + 3) / 4), dim3(256), 0, st, ws->h[2][2], U2, MB, cv_w, D.cv + D.coff.v_b, ws->v + MB);
  hipLaunchKernelGGL(k_big_head, dim3(hp.hb), dim3(256), 0, st, D, c.r0, MB, ws->mu, ws->v, ws->v + MB, ws->dmu, ws->dv, ws->part);
  hipLaunchKernelGGL(k_big_fin, dim3(1), dim3(64), 0, st, D, hp.hb, MB, ws->part);
  const GemmArgs gd = gemm_data_grad(ws->dmu, 24, mu_w, ws->h[0][2], ws->dy[0][2], MB, A, U2);
  gemm<0, 1, 3>(&gd, 1, 1, st);                                         // dY2 = (dmu Wmu) * ELU'(h3)
  hipLaunchKernelGGL(k_vhead_back, dim3(512), dim3(256), 0, st, ws->dv, v_w, ws->h[1][2], U2, MB, ws->dy[1][2]);
  hipLaunchKernelGGL(k_vhead_back, dim3(512), dim3(256), 0, st, ws->dv + MB, cv_w, ws->h[2][2], U2, MB, ws->dy[2][2]);
  // mu head: G[A][U2] = dmu^T h3, bias = row sums of dmu^T; the partials are summed by one wave per output
  const GemmArgs gw = gemm_weight_grad(ws->dmu, 24, ws->h[0][2], ws->part, hp.pz, MB, (MB + hp.Sh - 1) / hp.Sh, A, U2);
  gemm<1, 1, 4>(&gw, 1, hp.Sh, st);
  hipLaunchKernelGGL(k_vhead_wgrad, dim3(hp.VS), dim3(256), 0, st, ws->dv, ws->h[1][2], U2, MB, 64, vp0, hp.vz);
  hipLaunchKernelGGL(k_vhead_wgrad, dim3(hp.VS), dim3(256), 0, st, ws->dv + MB, ws->h[2][2], U2, MB, 64, vp1, hp.vz);
  hipLaunchKernelGGL(k_wave_reduce, dim3(((int)hp.pz + 3) / 4), dim3(256), 0, st, ws->part, hp.pz, hp.Sh, (int)hp.pz, D.ac_g + D.off.mu_w);
  hipLaunchKernelGGL(k_vhead_reduce, dim3((2 * (U2 + 1) + 3) / 4), dim3(256), 0, st, vp0, vp1, hp.vz, hp.VS, U2 + 1, D.ac_g + D.off.v_w,
                     D.cv_g + D.coff.v_w);
}

// Splits of layer l's weight-gradient product over the minibatch rows on the NT / TT path: as few as still give the 512 workgroup slots
// about a round and a half of 128 x 64-or-wider tiles (every split costs a pass over [W | b] in the partial reduction), at least 4 chunks
// each, never more than the workspace has room for (ws->nsplit)
static int nt_wgrad_splits(const SdxpDev& D, const SdxpBigWs* ws, int l) {
  int Kmax = 0;
  for (int net = 0; net < 3; ++net) Kmax = ws->layer[net][l].K > Kmax ? ws->layer[net][l].K : Kmax;
  const int tiles = 3 * ((D.units[l] + 127) / 128) * ((Kmax + 127) / 128);
  int Sl = (768 + tiles - 1) / tiles;
  const int smax = ws->MBp / (4 * ws->KC) > 0 ? ws->MBp / (4 * ws->KC) : 1;
  if (Sl > smax) Sl = smax;
  if (Sl > ws->nsplit) Sl = ws->nsplit;
  return Sl < 1 ? 1 : Sl;
}
// trunk backward, layer by layer for the three networks at once: G_l = dY_l^T X_l with b_l = row sums of dY_l^T as split partials,
// their reduction into the flat gradients, then dY_{l-1} = (dY_l W_l) * ELU'(H_{l-1})
static void big_backward(const SdxpDev& D, const SdxpBigWs* ws, const BigStep& c, hipStream_t st) {
  const int MB = ws->MB, MBp = ws->MBp;
  if (ws->nt && !ws->tt) {   // the head kernels left dLoss/d(pre-activation of trunk layer 2) in fp32: element-type copy + transpose
    const int U2 = D.units[2];
    StageArgs a[3];
    for (int net = 0; net < 3; ++net) a[net] = stage_args(ws->dy[net][2], MB, U2, U2, D.bf16 ? ws->dyn[net][2] : nullptr, ws->dyt[net][2], MBp);
    stage(D, a, 3, st);
  }
  for (int l = 2; l >= 0; --l) {
    const int Nl = D.units[l], S = ws->nt ? nt_wgrad_splits(D, ws, l) : ws->nsplit;
    // reduction rows per split; NT / TT: a whole number of chunks
    const int rchunk = ws->nt ? (((MBp + S - 1) / S) + ws->KC - 1) / ws->KC * ws->KC : (MB + S - 1) / S;
    GemmArgs gw[3], gx[3];
    NtArgs nw[3], nx[3];
    ReduceBatch rb;
    rb.S = S;
    for (int net = 0; net < 3; ++net) {
      const SdxpBigLayer& L = ws->layer[net][l];
      const size_t pz = (size_t)Nl * L.K + Nl;                            // [W_l | b_l] contiguous in the flat layout
      float* part = ws->part + (size_t)net * ws->part_region;
      rb.part[net] = part; rb.pz[net] = pz; rb.n[net] = pz; rb.out[net] = c.G[net] + L.woff;
      if (!ws->nt) {
        gw[net] = gemm_weight_grad(ws->dy[net][l], Nl, l == 0 ? c.X0[net] : ws->h[net][l - 1], part, pz, MB, rchunk, Nl, L.K);
        if (l > 0) gx[net] = gemm_data_grad(ws->dy[net][l], Nl, c.P[net] + L.woff, ws->h[net][l - 1], ws->dy[net][l - 1], MB, Nl, L.K);
      } else if (ws->tt) {   // fp32: dY_l and the layer input as the other products leave them; one image of dY_{l-1} (layer 0 included:
                             // its weight gradient reads it), ELU' from the layer output itself
        nw[net] = tt_weight_grad(ws->dy[net][l], l == 0 ? c.Xn[net] : ws->h[net][l - 1], L.kp, part, pz, MB, rchunk, Nl, L.K);
        if (l > 0) nx[net] = nt_data_grad(ws->dy[net][l], ws->wt[net][l], ws->h[net][l - 1], nullptr, MB, Nl, L.K, ws->dy[net][l - 1], nullptr, 0);
      } else {               // transposed copies: layer 0's gradient is read transposed only
        nw[net] = nt_weight_grad(ws->dyt[net][l], MBp, l == 0 ? c.Xt[net] : ws->ht[net][l - 1], l == 0 ? ws->Rp : MBp, part, pz, MBp, rchunk, Nl, L.K);
        if (l > 0) nx[net] = nt_data_grad(ws->dyn[net][l], ws->wt[net][l], ws->hn[net][l - 1], ws->ht[net][l - 1], MB, Nl, L.K,
                                          l > 1 ? ws->dyn[net][l - 1] : nullptr, ws->dyt[net][l - 1], MBp);
      }
    }
    if (!ws->nt) gemm<1, 1, 4>(gw, 3, S, st, D.bf16 != 0);
    else if (ws->tt) gemm_tt(nw, 3, S, ws->zeros, st, ws->nt_tile);
    else if (D.bf16) gemm_nt<1, EPI_TN>(nw, 3, S, st, ws->nt_tile);
    else gemm_nt<0, EPI_TN>(nw, 3, S, st, ws->nt_tile);
    hipLaunchKernelGGL(k_reduce_parts3, dim3(256, 3), dim3(256), 0, st, rb);
    if (l == 0) break;
    if (!ws->nt) gemm<0, 1, 3>(gx, 3, 1, st, D.bf16 != 0);
    else if (D.bf16) gemm_nt<1, EPI_NN>(nx, 3, 1, st, ws->nt_tile);
    else gemm_nt<0, EPI_NN>(nx, 3, 1, st, ws->nt_tile);
  }
}

// forward + losses + backward of minibatch `mb` (mini-epoch `me`) for all three networks; leaves the flat gradients in ac_g / cv_g,
// the KL word in ac_g[g_tail] and the control block advanced.  The caller follows with the explicit clip + Adam.
extern "C" void sdxpk_big_step(const SdxpDev* D, const SdxpBigWs* ws, int mb, int me, hipStream_t st) {
  const BigStep c = big_step_ctx(*D, ws, mb, me);
  big_forward(*D, ws, c, st);
  big_heads(*D, ws, c, st);
  big_backward(*D, ws, c, st);
}

// ---- timing / test hook (not part of include/seqdex.h): one batched NT product on caller-owned operands (tools/time_gemm_nt.py); tile as SdxpOpts::nt_tile
template <int BF, int EPI>
static bool nt_prepare_and_launch(const NtArgs* gs, int count, int splits, int tile, hipStream_t st) {
  const bool ok = gemm_nt_prepare<BF, EPI>();
  if (ok) gemm_nt<BF, EPI>(gs, count, splits, st, tile);
  return hipGetLastError() == hipSuccess && ok;   // (also clears what a refused attribute left behind)
}
extern "C" int sdxpk_gemm_nt_launch(int bf, int epi, const NtArgs* gs, int count, int splits, int tile, hipStream_t st) {
  if (count < 1 || count > 3 || splits < 1) return -1;
  if (epi == EPI_FWD) return (bf ? nt_prepare_and_launch<1, EPI_FWD> : nt_prepare_and_launch<0, EPI_FWD>)(gs, count, splits, tile, st) ? 0 : -1;
  if (epi == EPI_NN) return (bf ? nt_prepare_and_launch<1, EPI_NN> : nt_prepare_and_launch<0, EPI_NN>)(gs, count, splits, tile, st) ? 0 : -1;
  if (epi == EPI_TN) return (bf ? nt_prepare_and_launch<1, EPI_TN> : nt_prepare_and_launch<0, EPI_TN>)(gs, count, splits, tile, st) ? 0 : -1;
  return -1;
}
// ---- test hooks: one batched k_gemm_tt / k_gemm product on caller-owned operands (tests/test_gpu_gemm_products.py).  tile of
// sdxpk_gemm_tt_launch as above; of sdxpk_gemm_launch as gemm<>() of sdx_gemm.h takes it.  Only the (AT, BT, EPI) products the step
// and the T-value trainer instantiate exist: anything else is refused
extern "C" int sdxpk_gemm_tt_launch(const NtArgs* gs, int count, int splits, const float* zeros, int tile, hipStream_t st) {
  if (count < 1 || count > 3 || splits < 1 || !zeros || tile < 0 || tile > 2) return -1;
  const bool ok = gemm_tt_prepare();
  if (ok) gemm_tt(gs, count, splits, zeros, st, tile);
  return hipGetLastError() == hipSuccess && ok ? 0 : -1;
}
extern "C" int sdxpk_gemm_launch(int at, int bt, int epi, int bf, const GemmArgs* gs, int count, int splits, int tile, hipStream_t st) {
  if (count < 1 || count > 3 || splits < 1 || tile < 0 || tile > 3) return -1;
  if (at == 0 && bt == 0 && epi == 1) gemm<0, 0, 1>(gs, count, splits, st, bf != 0, tile);
  else if (at == 0 && bt == 0 && epi == 2) gemm<0, 0, 2>(gs, count, splits, st, bf != 0, tile);
  else if (at == 0 && bt == 1 && epi == 3) gemm<0, 1, 3>(gs, count, splits, st, bf != 0, tile);
  else if (at == 1 && bt == 1 && epi == 4) gemm<1, 1, 4>(gs, count, splits, st, bf != 0, tile);
  else return -1;
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
