// sdxp_persist.hip — the PPO update phase of one epoch (all mini-epochs x minibatches, three networks) as ONE persistent
// kernel on MI355X: 256 workgroups (one per CU) x 512 threads.  Every weight and its Adam moments stay in the VGPR file of the
// CU that owns them for the whole epoch (~132 resident registers per lane of 241), activations / gradient factors of the
// current minibatch live in LDS (147 KiB), and the only inter-CU traffic per optimiser step is the rank-MB factors, exchanged
// as (value, step tag) words - no grid barrier (replaces PS:294-326 / RC:1339-1365 of the reference loop):
//
//   A  dY0 -> Gram -> |g|^2 -> clip scale, Adam of layer 0, forward L0 of own rows                       -> x1  | shadow: Adam L1
//   B  gather x1, forward L1 of own rows                                                                 -> x2  | shadow: Gram x1, Adam L2/heads/biases
//   C  gather x2, forward L2 of own row                                                                  -> x3  | shadow: Gram x2
//   D  gather x3 + heads, PPO losses (replicated on every CU, bit-identical), backward heads and L2      -> dY1 | shadow: stats, LR rule, Gram x3, head norms
//   E  gather dY1, backward L1 (column copy)                                                             -> dY0 | shadow: Grams dY1, dY2
// (Phase A's shadow holds Adam of layer 1 alone.  The Gram of the layer-0 inputs, which stood in it, does not depend on the step - the
// inputs are dataset rows: k_input_grams at the end of this file forms every minibatch's once per epoch, behind the pre-normalisation,
// and the step fetches its 32 floats with its rows.)
// (What closes a phase on one wave or one thread while the other waves stand at its barrier - the publish tails of forward L0 / L1 / L2 on wave 0,
// the value rows and the bias tail of the head forward on waves 7 and 0, the statistics / learning-rate thread of the dY1 shadow - asks LDS for
// all its operands in ONE round trip, and a publish tail forms one (network, sample, row) per lane, the three networks of a word meeting in the
// storing lane by cross-lane moves: sdxp_persist_tails.h.)
//
// Ownership (shipped network 396/564 -> 1024 -> 512 -> 256 -> 23/1, minibatch 4):
//   W0 rows      : CU g, wave w owns half (w&1) of row 4g+(w>>1) of actor, critic and central value
//   W1 rows      : wave w owns quarter (w&3) of row 2g+(w>>2) of the three nets     (forward)
//   W1 columns   : CU g owns columns 4g..4g+3 of the three nets, thread = row       (backward; duplicate copy, same Adam)
//   W2 rows      : wave w owns eighth w of row g of the three nets                  (forward)
//   W2 columns   : CU g owns columns 2g, 2g+1: lanes l / l ^ 32 of wave w = row 32w + (l & 31) of the two columns (backward; duplicate copy)
//   heads        : CU g runs Adam for 25 of the 6 400 head weights - rows (g >> 5) + {0, 8, 16} of columns 8 (g & 31) .. + 7, column g of row 24 - and
//                  publishes them, three rows of a column per 16-byte word (head_owned / head_publish); every CU reads the matrix back in phase D
// Row and column copies receive the same gradient g[n][k] = sum_s dY_s[n] X_s[k] (same operands, same order), so they
// stay bit-identical without communication.  The multi-kernel path (sdxp_update.hip) remains the fallback for other shapes
// and the explicit-gradient multi-rank path.
#include <cstddef>
#include <cstdlib>

#include "sdx_common.h"
#include "sdxp_device.h"   // elu, dpp_add, wave_sum
#include "sdxp_launch.h"
#include "sdxp_persist_lds.h"        // shape constants, PLds, names of its slots and of the recurring thread windows
#include "sdxp_persist_exchange.h"   // lq_* / ll_* tagged words between the CUs
#include "sdxp_persist_sums.h"       // row / wave / block sums, Gram accumulators
#include "sdxp_persist_adam.h"       // adam1, adam1p, opaque, SDX_PIN*
#include "sdxp_persist_tails.h"      // fwd_tail, stats_lr_once: the one-wave / one-thread pieces that close a phase
#include "sdxp_persist_phase_d.h"    // loss_request / loss_front / loss_back, head_backward: the on-chain pieces of phase D behind the head forward

// dataset-row helpers
__device__ __forceinline__ const float* obs_rows(const SdxpDev& D, int mb) { return D.mb_obs + (size_t)mb * MB * D.obs_dim; }
__device__ __forceinline__ const float* cvx_rows(const SdxpDev& D, int mb, int mini_epoch) {
  return (mini_epoch == 0 ? D.cvx0 : D.cvx1) + (size_t)mb * MB * ST;
}

// SINGLE = false: the whole update phase of an epoch (above).  SINGLE = true: forward + backward of ONE minibatch (the one the
// device cursor SdxpCtrl.mb_index points at) with the current parameters; no optimiser state is touched, the rank-MB factors
// are written to D.fact for the multi-rank exchange and the cursor / loss statistics advance as k_ctrl does in explicit mode.
template <bool SINGLE>
__global__ __launch_bounds__(NTH, 2) void k_update_persistent(SdxpDev D, int total_steps, const float* gx0_tab, unsigned* failflag, int stamps, int fault) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  PLds& S = *reinterpret_cast<PLds*>(smem_raw);
  // Thread coordinates are re-derived from an opaque copy of threadIdx/blockIdx at the start of every phase (refresh()):
  // otherwise every LDS address and ownership index of the step loop is hoisted into the loop preheader and the ~150 hoisted
  // values, on top of the resident weights and moments, push the kernel far over the 256-VGPR budget.
  int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, g = blockIdx.x;
  int r0w, h0, n0, r1w, q1, r1, c2c, c2n, he, hrow, hk;
  auto refresh = [&]() {
    int t = threadIdx.x, b = blockIdx.x;
    asm volatile("" : "+v"(t));
    asm volatile("" : "+s"(b));
    tid = t; lane = t & 63; wave = __builtin_amdgcn_readfirstlane(t >> 6); g = b;
    r0w = wave >> 1; h0 = wave & 1; n0 = 4 * g + r0w;
    r1w = wave >> 2; q1 = wave & 3; r1 = 2 * g + r1w;
    c2c = (t >> 5) & 1; c2n = 32 * (t >> 6) + (t & 31);   // column c2n: lanes l and l ^ 32 of one wave hold its two row halves
    head_owned(b, t, he, hrow, hk);   // this CU's HPC head elements: three rows of eight columns and one column of row 24
  };
  refresh();
#define TS(i) if (stamps && g == (stamps >> 8) && tid == 0) { const long long t_ = __builtin_amdgcn_s_memtime(); S.tacc[i] += t_ - S.tlast; S.tlast = t_; }
  if (tid < 32) S.tacc[tid] = 0;
  if (tid == 0) S.fail = 0;
  if (tid == 0) S.tlast = __builtin_amdgcn_s_memtime();
  const int A = ACT;
  u64* const LL = D.ll;   // 8-byte exchange words of the head matrix's row 24 (LL_H24)
  const __amdgpu_buffer_rsrc_t LQ = lq_rsrc(D.ll);   // 16-byte packed words of the chain edges, layout LQ_*: [s][unit], the three networks per word

  // ------------------------------------------------------------------ resident parameters
  // layer 0 rows: row n0 = 4g + (wave>>1), half h0 = wave&1 of K; net 0/1: K = OBS, net 2: K = ST
  float w0a[I0A], m0a[I0A], v0a[I0A], w0c[I0A], m0c[I0A], v0c[I0A], w0v[I0V], m0v[I0V], v0v[I0V];
  // layer 1 rows: row r1 = 2g + (wave>>2), quarter q1 = wave&3: k = q1*256 + lane + 64 i (i<4), three nets
  float w1[3][4], m1[3][4], v1[3][4];
  // layer 1 columns: cols 4g+c, row n = tid
  float c1[3][4], cm1[3][4], cv1[3][4];
  // layer 2 rows: row g, eighth = wave: k = wave*64 + lane
  float w2[3], m2[3], v2[3];
  // layer 2 columns: col 2g + c2c, row n = c2n (c2c = lane >> 5, c2n = 32 wave + (lane & 31): refresh())
  float c2[3], cm2[3], cv2[3];
  // heads ((A+2) x U2 = 6400 weights): CU g runs Adam for HPC elements (hrow, hk) on its first HPC threads (head_owned, sdxp_persist_exchange.h) and
  // publishes the new weights as exchange words; phase D of every CU reads the whole head matrix back through L2.
  float hw = 0.0f, hm = 0.0f, hv = 0.0f;

  auto ldm = [&](const float* p, size_t o) -> float { return SINGLE ? 0.0f : p[o]; };   // Adam moments: not needed for one forward/backward
  auto P_of = [&](int net) -> float* { return net == 2 ? D.cv : D.ac; };
  auto M_of = [&](int net) -> float* { return net == 2 ? D.cv_m : D.ac_m; };
  auto V_of = [&](int net) -> float* { return net == 2 ? D.cv_v : D.ac_v; };
  auto woff = [&](int net, int l) -> size_t { return net == 0 ? D.off.a_w[l] : net == 1 ? D.off.c_w[l] : D.coff.w[l]; };
  auto boff = [&](int net, int l) -> size_t { return net == 0 ? D.off.a_b[l] : net == 1 ? D.off.c_b[l] : D.coff.b[l]; };
  auto head_woff = [&](int row) -> size_t { return row < A ? D.off.mu_w + (size_t)row * U2 : (row == A ? D.off.v_w : D.coff.v_w); };
  auto head_boff = [&](int row) -> size_t { return row < A ? D.off.mu_b + row : (row == A ? D.off.v_b : D.coff.v_b); };
  auto head_net = [&](int row) -> int { return row < A ? 0 : (row == A ? 1 : 2); };
  // column of element i of this lane's layer-1 row quarter (o_w1 and forward L1; the Adam shadow forms its own through opaque())
  auto k_w1 = [&](int i) -> int { return q1 * 256 + lane + 64 * i; };
  // flat offset, in the network's parameter and moment arrays, of elements this lane owns: prologue and epilogue use the same names.  (The central
  // value's layer-0 half row and the layer-2 row eighth stay spelled out in both: named, the one-minibatch prologue forms its addresses differently.)
  auto o_w0 = [&](int net, int k) -> size_t { return woff(net, 0) + (size_t)n0 * D.obs_dim + k; };   // actor / critic (net 0 / 1)
  auto o_w1 = [&](int net, int i) -> size_t { return woff(net, 1) + (size_t)r1 * U0 + q1 * 256 + lane + 64 * i; };   // (k_w1(i), added term by term in 64 bits)
  auto o_hw = [&]() -> size_t { return head_woff(hrow) + hk; };

#pragma unroll
  for (int i = 0; i < I0A; ++i) {
    const int kk = lane + 64 * i, k = h0 * H0A + kk;
    const bool ok = kk < H0A && k < D.obs_dim;
    const size_t oa = o_w0(0, k), oc = o_w0(1, k);
    w0a[i] = ok ? D.ac[oa] : 0.0f; m0a[i] = ok ? ldm(D.ac_m, oa) : 0.0f; v0a[i] = ok ? ldm(D.ac_v, oa) : 0.0f;
    w0c[i] = ok ? D.ac[oc] : 0.0f; m0c[i] = ok ? ldm(D.ac_m, oc) : 0.0f; v0c[i] = ok ? ldm(D.ac_v, oc) : 0.0f;
  }
#pragma unroll
  for (int i = 0; i < I0V; ++i) {
    const int kk = lane + 64 * i, k = h0 * H0V + kk;
    const bool ok = kk < H0V;
    const size_t o = woff(2, 0) + (size_t)n0 * ST + k;
    w0v[i] = ok ? D.cv[o] : 0.0f; m0v[i] = ok ? ldm(D.cv_m, o) : 0.0f; v0v[i] = ok ? ldm(D.cv_v, o) : 0.0f;
  }
#pragma unroll
  for (int net = 0; net < 3; ++net) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const size_t o = o_w1(net, i);
      w1[net][i] = P_of(net)[o]; m1[net][i] = ldm(M_of(net), o); v1[net][i] = ldm(V_of(net), o);
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const size_t o = woff(net, 1) + (size_t)tid * U0 + 4 * g + c;
      c1[net][c] = P_of(net)[o]; cm1[net][c] = ldm(M_of(net), o); cv1[net][c] = ldm(V_of(net), o);
    }
    {
      const size_t o = woff(net, 2) + (size_t)g * U1 + wave * 64 + lane;
      w2[net] = P_of(net)[o]; m2[net] = ldm(M_of(net), o); v2[net] = ldm(V_of(net), o);
    }
    {
      const size_t o = woff(net, 2) + (size_t)c2n * U1 + 2 * g + c2c;
      c2[net] = P_of(net)[o]; cm2[net] = ldm(M_of(net), o); cv2[net] = ldm(V_of(net), o);
    }
  }
  if (tid < HPC) {
    const int net = head_net(hrow);
    const size_t o = o_hw();
    hw = P_of(net)[o]; hm = ldm(M_of(net), o); hv = ldm(V_of(net), o);
  }
  // biases + logstd (LDS, one thread each)
  __shared__ float s_b2[3][32];     // logstd value, m, v
  auto bias_load = [&](int net, size_t o) { S.bias[tid] = P_of(net)[o]; S.bias_m[tid] = ldm(M_of(net), o); S.bias_v[tid] = ldm(V_of(net), o); };
  // (the slot map of S.bias, BIAS_*; the epilogue walks the same ladder: stated once for both, it changes thousands of lines of both instantiations)
  if (tid < BIAS_L1) { const int net = (tid - BIAS_L0) / 4, w = (tid - BIAS_L0) % 4; bias_load(net, boff(net, 0) + 4 * g + w); }
  else if (tid < BIAS_L2) { const int net = (tid - BIAS_L1) / 2, r = (tid - BIAS_L1) % 2; bias_load(net, boff(net, 1) + 2 * g + r); }
  else if (tid < BIAS_HEAD) { const int net = tid - BIAS_L2; bias_load(net, boff(net, 2) + g); }
  else if (tid < BIAS_HEAD + A + 2) { const int row = tid - BIAS_HEAD; bias_load(head_net(row), head_boff(row)); }
  else if (tid >= T_LOGSTD && tid < T_LOGSTD + A) {
    const int a = tid - T_LOGSTD;
    const size_t o = D.off.logstd + a;
    s_b2[0][a] = D.ac[o]; s_b2[1][a] = ldm(D.ac_m, o); s_b2[2][a] = ldm(D.ac_v, o);
  }
  // replicated control state (every CU runs the same state machine on identical inputs)
  SdxpCtrl* gctl = D.ctrl;
  // first exchange tag of this launch minus one: read from the device control block (CU 0 advances it at the end of the launch, when
  // every CU has long read it: nobody finishes a step without everybody's words) - so launches replayed from a hipGraph keep growing tags
  const unsigned tag_base = gctl->ll_tag;
  if (tid == 0) {
    PLds::Ctl& C = S.ctl;
    C.ac_lr = gctl->ac_lr; C.ac_lr_applied = C.ac_lr; C.cv_lr = gctl->cv_lr; C.ac_t = gctl->ac_t; C.cv_t = gctl->cv_t;
    C.ac_b1 = gctl->ac_b1pow; C.ac_b2 = gctl->ac_b2pow; C.cv_b1 = gctl->cv_b1pow; C.cv_b2 = gctl->cv_b2pow;
    C.sum_a = C.sum_c = C.sum_b = C.sum_kl = C.sum_cv = C.sum_ent = C.last_kl = C.ac_gn = C.cv_gn = 0.0f;
  }
  bool pending = false;
  // layer-0 gradient elements of this lane (sum_s dY0_s[row] x0_s[k], before the clip scale), formed in the dY0 shadow of the step that
  // produced them - the LDS round trips of the rebuild are off the chain, Adam of layer 0 runs on registers (round 6)
  float g0a[I0A], g0c[I0A], g0v[I0V];
#pragma unroll
  for (int i = 0; i < I0A; ++i) { g0a[i] = 0.0f; g0c[i] = 0.0f; }
#pragma unroll
  for (int i = 0; i < I0V; ++i) g0v[i] = 0.0f;
  // columns of the layer-0 input image past obs_dim stay zero for the whole launch (the row loads below never touch them)
  for (int i = tid; i < MB * OBS; i += NTH) (&S.obs[0][0])[i] = 0.0f;
  __syncthreads();

    // This step's layer-0 inputs (dataset rows mb*MB .. +MB) go STRAIGHT into LDS (global_load_lds_dword: lane tid of a wave fetches element
  // wave 64 + lane of a row, the wave's 64 dwords land behind one wave-uniform LDS address; no VGPR round trip, no ds_write, no barrier in
  // front of the copy).  The old rows were last read by the dY0 shadow (the layer-0 gradient rebuild), which every wave finished before the
  // barrier at the top of the step; the loads fly under the norm gather and Adam of layer 0 and are waited for in front of forward L0.
  auto load_rows = [&](int mb_, int me_) {
    // row pointers are wave-uniform (scalar registers), the lane adds its 32-bit offset: ONE address VGPR for the twelve loads (twelve 64-bit
    // per-lane pointers formed up front were 24 VGPRs - the kernel has none to spare - and spilled the first looks of the x2 / dY1 words)
    // (the "+s" asm keeps each pointer in a scalar register pair and in place: hoisted out of the step loop as per-lane 64-bit values they
    // cost VGPR pairs for the whole step)
    auto uni = [](const float* q) -> const float* { unsigned long long a = (unsigned long long)q; asm volatile("" : "+s"(a)); return (const float*)a; };
    const float* o = uni(obs_rows(D, mb_));
    const float* c = uni(cvx_rows(D, mb_, me_));
    const unsigned odim = D.obs_dim;
    if constexpr (!SINGLE) {
      // the Grams of these rows, from the table the pre-pass formed for the epoch (k_input_grams): 32 lanes of the last wave - it has one piece
      // fewer than the others below - fetch the observation block and the central value's block of this mini-epoch's class into S.gx0.  The
      // reader is wave 0 at the end of phase E; the previous step's read lies three barriers in front of this request
      const float* gt = uni(gx0_tab + (size_t)mb_ * GX0_STRIDE);
      if (wave == NWV - 1 && lane < 32)
        __builtin_amdgcn_global_load_lds(SDX_AS_GLOBAL(gt + (lane < 16 ? GX0_OBS + lane : (me_ == 0 ? GX0_CVX0 : GX0_CVX1) + (lane - 16))), SDX_AS_LDS(&S.gx0[0][0]), 4, 0, 0);
    }
    if (odim == OBS) {
      // full-width observations: the MB rows are contiguous in the dataset AND in LDS (S.obs, then S.cvx): 960 pieces of 16 bytes, two
      // global_load_lds_dwordx4 per lane (twelve dword loads with their exec masks and M0 writes cost phase A 0.4 us of issue)
      static_assert(offsetof(PLds, cvx) == sizeof(float) * MB * OBS && (MB * OBS) % 4 == 0 && (MB * ST) % 4 == 0, "obs and cvx images are adjacent 16-byte runs");
      constexpr int PO = MB * OBS / 4, PA = PO + MB * ST / 4;
      char* l0 = reinterpret_cast<char*>(&S.obs[0][0]);
#pragma unroll
      for (int j = 0; j < (PA + NTH - 1) / NTH; ++j) {
        const int pc = tid + NTH * j;
        if (pc < PA) {
          const float* src = pc < PO ? o + 4 * pc : c + 4 * (pc - PO);
          __builtin_amdgcn_global_load_lds(SDX_AS_GLOBAL(src), SDX_AS_LDS(l0 + (wave + NWV * j) * 1024), 16, 0, 0);
        }
      }
      return;
    }
#pragma unroll
    for (int s = 0; s < MB; ++s) {
      const float* orow = uni(o + s * odim);
      const float* crow = uni(c + s * ST);
      if ((unsigned)tid < odim) __builtin_amdgcn_global_load_lds(SDX_AS_GLOBAL(orow + (unsigned)tid), SDX_AS_LDS(&S.obs[s][wave * 64]), 4, 0, 0);
      __builtin_amdgcn_global_load_lds(SDX_AS_GLOBAL(crow + (unsigned)tid), SDX_AS_LDS(&S.cvx[s][wave * 64]), 4, 0, 0);
      if (tid + NTH < ST) __builtin_amdgcn_global_load_lds(SDX_AS_GLOBAL(crow + NTH + (unsigned)tid), SDX_AS_LDS(&S.cvx[s][NTH]), 4, 0, 0);
    }
  };
  if (total_steps > 0) load_rows(SINGLE ? gctl->mb_index : 0, SINGLE ? gctl->mini_epoch : 0);   // rows of the first minibatch
  // first look at the gradient-norm words (round 6): every CU published its word at the end of phase E, 1.6 us before the top of the next
  // step, so the words are there when the dY0 shadow ends - what the gather at the top of the step paid for was its own round trip
  // (0.9 us of the 1.2: all 256 CUs show the same 1.2 us, there is no late producer).  The loads are requested behind the shadow's second
  // barrier and taken at the top of the next step; a miss falls back to the polling gather.
  u32x4 pg0[4];
  bool pg0_issued = false;
  for (int step = 0; step <= total_steps; ++step) {
    SDX_LDS_BARRIER();   // LDS only: the next step's row loads (requested in the dY0 shadow) stay in flight across it
    if (S.fail) return;   // an exchange word never arrived (not all CUs resident?): the host sees *failflag and reports it
    if (fault && g == NWG - 1 && step == 3) return;   // SDXP_PERSIST_FAULT=1 (tests): one CU goes silent, the others must time out
    refresh();
    const bool last = step == total_steps;   // the extra iteration only applies the optimiser step of the final minibatch
    const int mbi = SINGLE ? gctl->mb_index : step % D.num_minibatches, mini_epoch = SINGLE ? gctl->mini_epoch : step / D.num_minibatches;
    // tag of everything this step produces / of what the previous step produced.  tag_base advances from launch to launch (the
    // exchange buffer is never cleared), so a word left over from an earlier launch can never match
    const unsigned tag = tag_base + (unsigned)step + 1u, tag_prev = tag_base + (unsigned)step;
    // ================================================================== phase A: gradient norm, Adam of layer 0, forward L0
    if (pending) {
      // Squared gradient norm -> clip scale, WITHOUT a workgroup barrier or an LDS pass on the step's dependent chain.  Every CU published
      // ONE word at the end of the previous step: its four columns' share of <G_dY0, G_x0> + |sum_s dY0_s|^2 for the three networks.  Every
      // WAVE gathers the 256 words itself - CUs lane, lane + 64, ... - and adds them in one fixed order (pair sums, then the DPP tree of
      // wave_sum), so all waves of all CUs hold bit-identical scalars and walk into Adam of layer 0 as their own words arrive.  What does not
      // depend on dY0 - the other layers' and the heads' terms (S.n2rest), the bias corrections and the learning-rate scalars
      // (S.scal[SC_AC_LR_BC1 ..]) - was prepared in the shadows of the previous step.
      // (what the scalars below need from LDS is requested in front of the norm words' take: one LDS round trip less behind the DPP sums)
      float nr0 = S.n2rest[0], nr1 = S.n2rest[1], nr2 = S.n2rest[2];
      float ac_lr_bc1 = S.scal[SC_AC_LR_BC1], ac_isq = S.scal[SC_AC_ISQ], cv_lr_bc1 = S.scal[SC_CV_LR_BC1], cv_isq = S.scal[SC_CV_ISQ];
      float w0[4], w1[4], w2[4];
      lq_take_or_gather<4>(pg0_issued, pg0, LQ, LQ_G0 + lane, 64, tag_prev, w0, w1, w2, failflag, S.fail);
      float n2[3];
      n2[0] = (w0[0] + w0[1]) + (w0[2] + w0[3]); n2[1] = (w1[0] + w1[1]) + (w1[2] + w1[3]); n2[2] = (w2[0] + w2[1]) + (w2[2] + w2[3]);
#pragma unroll
      for (int net = 0; net < 3; ++net) n2[net] = wave_sum(n2[net]);     // three independent DPP chains
      SDX_PIN4X(nr0, nr1, nr2, ac_lr_bc1); SDX_PIN3X(ac_isq, cv_lr_bc1, cv_isq);   // (used from here on; requested above)
      n2[0] += nr0; n2[1] += nr1; n2[2] += nr2;
      // v_sqrt_f32 / v_rcp_f32 (1 ulp each, as in the Adam arithmetic) instead of the IEEE sequences: these four sit between the last word of the
      // norm and the first Adam instruction of every lane
      const float ac_gn = __builtin_amdgcn_sqrtf(n2[0] + n2[1]), cv_gn = __builtin_amdgcn_sqrtf(n2[2]);
      const float gs_ac = D.truncate_grads ? fminf(1.0f, D.grad_norm * __builtin_amdgcn_rcpf(ac_gn + 1e-6f)) : 1.0f;
      const float gs_cv = D.truncate_grads ? fminf(1.0f, D.grad_norm * __builtin_amdgcn_rcpf(cv_gn + 1e-6f)) : 1.0f;
      if (tid == 0) { S.ctl.ac_gn = ac_gn; S.ctl.cv_gn = cv_gn; S.scal[SC_AC_GSCALE] = gs_ac; S.scal[SC_CV_GSCALE] = gs_cv; }   // for the shadows' Adam phases (behind the next barrier)
      TS(0)
      // ---- layer 0 rows: gradient elements from registers (g0a / g0c / g0v, dY0 shadow of the previous iteration), scaled by the clip factor
#pragma unroll
      for (int i = 0; i < I0A; ++i) {
        adam1p(w0a[i], g0a[i] * gs_ac, m0a[i], v0a[i], ac_lr_bc1, ac_isq);
        adam1p(w0c[i], g0c[i] * gs_ac, m0c[i], v0c[i], ac_lr_bc1, ac_isq);
      }
#pragma unroll
      for (int i = 0; i < I0V; ++i) adam1p(w0v[i], g0v[i] * gs_cv, m0v[i], v0v[i], cv_lr_bc1, cv_isq);
      if (tid < BIAS_L1) {   // layer-0 biases (bias gradient = sum_s dY_s[row])
        const int net = (tid - BIAS_L0) / 4;
        float gg = 0.0f;
        for (int s = 0; s < MB; ++s) gg += S.dyown[net][s][DY_L0 + (tid - BIAS_L0) % 4];
        adam_bias(S, StepScal{gs_ac, gs_cv, ac_lr_bc1, ac_isq, cv_lr_bc1, cv_isq}, tid, net, gg);
      }
      TS(1)
    }
    // s_waitcnt vmcnt(0) as an instruction the compiler's counter model SEES (the asm one below it does not see): the first look at the norm
    // words is taken only `if (pending)`, so behind that merge the model holds their loads for outstanding, and where their registers are next
    // written - the top of the x1 or the x2 shadow, as the allocation falls - it waits for vmcnt(0) itself: there, wave 0 has just stored its
    // x1 / x2 word and the wait is that store's round trip (0.2 us per shadow on the phase clock).  Here nothing is in flight but the row loads,
    // which are waited for below anyway
    __builtin_amdgcn_s_waitcnt(0x0F70);
    if (!last) {
      // ---- forward L0 of the owned rows (two half-row waves per row, combined through LDS) once this step's rows have landed
      SDX_WAIT_VMCNT0();
      __syncthreads();
      float pa[MB], pc[MB], pv[MB];
#pragma unroll
      for (int s = 0; s < MB; ++s) { pa[s] = 0.0f; pc[s] = 0.0f; pv[s] = 0.0f; }
#pragma unroll
      for (int i = 0; i < I0A; ++i) {
        const int kk = lane + 64 * i, k = h0 * H0A + kk;
        if (kk < H0A) {
#pragma unroll
          for (int s = 0; s < MB; ++s) { const float x = S.obs[s][k]; pa[s] += w0a[i] * x; pc[s] += w0c[i] * x; }
        }
      }
#pragma unroll
      for (int i = 0; i < I0V; ++i) {
        const int kk = lane + 64 * i, k = h0 * H0V + kk;
        if (kk < H0V) {
#pragma unroll
          for (int s = 0; s < MB; ++s) pv[s] += w0v[i] * S.cvx[s][k];
        }
      }
      // (the twelve wave sums as ONE halving butterfly, value net MB + s: lane s < 4 ends with sample s of the three networks and stores them;
      // same pairs as twelve wave_sum trees, bit-identical results)
      {
        float v[3 * MB], u[3];
#pragma unroll
        for (int s = 0; s < MB; ++s) { v[0 * MB + s] = pa[s]; v[1 * MB + s] = pc[s]; v[2 * MB + s] = pv[s]; }
        wave_sums<3 * MB>(v, u, lane);
        fpart_store(S, u, wave, lane);
      }
      __syncthreads();
      if (wave == 0) {   // wave 0: lane (net, sample s, owned row r) < 48 forms one output, lane (s, r) < 16 stores the three networks' in one packed word (fwd_tail)
        float y[3];
        fwd_tail<0>(S, lane, y);
        if (tid < MB * 4) lq_store(LQ, LQ_X1 + (unsigned)(tid / 4) * U0 + 4 * g + tid % 4, y[0], y[1], y[2], tag);
      }
      TS(2)
      // (the Gram of the layer-0 inputs that stood here, in the shadow of the x1 exchange, does not depend on the step: it arrives from the
      // per-epoch table with the rows of the minibatch - k_input_grams, load_rows, S.gx0)
    }
    refresh();
    if (pending) {
      // ---- (shadow of x1) Adam of layer 1: row copy and column copy, operands are last step's S.x1 / S.dy1
      // (one loop over the 24 elements with the next element's operands in flight: adam_l1_ahead)
      const StepScal sc = step_scal(S);
      adam_l1_ahead(S, sc, q1 * 256 + lane, 4 * g, r1w, tid, w1, m1, v1, c1, cm1, cv1, [](int, int, float) {});
      if (tid >= BIAS_L1 && tid < BIAS_L2) {   // layer-1 biases
        const int net = (tid - BIAS_L1) / 2;
        float gg = 0.0f;
        for (int s = 0; s < MB; ++s) gg += S.dyown[net][s][DY_L1 + (tid - BIAS_L1) % 2];
        adam_bias(S, sc, tid, net, gg);
      }
    }
    TS(3)
    if (!last) {
      __syncthreads();   // every wave is done with the old S.x1
      // ================================================================== phase B: gather x1, forward L1
      {
        float v0[8], v1[8], v2[8];   // word tid + NTH j = (sample, unit) s U0 + unit: S.x1[net] is [MB][U0], i.e. the same flat index
        if (!lq_gather<8>(LQ, LQ_X1 + tid, NTH, tag, v0, v1, v2, failflag)) S.fail = 1;
        image_store(S.x1, v0, v1, v2, tid);
      }
      TS(4)
      __syncthreads();
      {
        float q[3 * MB], u[3];   // value net MB + s
#pragma unroll
        for (int net = 0; net < 3; ++net) {
#pragma unroll
          for (int s = 0; s < MB; ++s) q[net * MB + s] = 0.0f;
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const int k = k_w1(i);
#pragma unroll
            for (int s = 0; s < MB; ++s) q[net * MB + s] += w1[net][i] * S.x1[net][s][k];
          }
        }
        wave_sums<3 * MB>(q, u, lane);
        fpart_store(S, u, wave, lane);
      }
      __syncthreads();
      if (wave == 0) {   // wave 0: lane (net, s, r) < 24 forms one output, lane (s, r) < 8 stores the word (fwd_tail)
        float y[3];
        fwd_tail<1>(S, lane, y);
        if (tid < MB * 2) lq_store(LQ, LQ_X2 + (unsigned)(tid / 2) * U1 + 2 * g + tid % 2, y[0], y[1], y[2], tag);
      }
      TS(5)
      // (the Gram of x1 used to sit here: this shadow was 2.7 us against an edge of 2.1; it now shares ONE block reduction with the
      // Gram of x2 in the shadow of x3 - 60 values through the butterfly instead of 2 x 33 through two of them)
    }
    refresh();
    u32x4 px2[4];
    bool px2_issued = false;
    if (pending) {
      // ---- (shadow of x2) Adam of layer 2 (row and column copies), of this CU's head elements, of the remaining biases and logstd
      const StepScal sc = step_scal(S);
      float dep = 0.0f;
#pragma unroll
      for (int net = 0; net < 3; ++net) {
        // first look at this lane's x2 words before the last network's update: the shadow has outlasted the edge by then (2.2 us of
        // its 2.8 against an edge of 2.1), what follows hides the round trip
        if (net == 2 && !last) { lq_peek<4>(LQ, LQ_X2 + tid, NTH, px2); px2_issued = true; }
        const float gs = sc.gs(net), lrb = sc.lrb(net), isq = sc.isq(net);
        float d2r[MB], dn2[MB];
        const int o_n = opaque(c2n, dep);
#pragma unroll
        for (int s = 0; s < MB; ++s) { d2r[s] = S.dyown[net][s][DY_L2] * gs; dn2[s] = S.dy2[net][s][o_n] * gs; }
        {
          const int k = opaque(wave * 64 + lane, dep);
          float gg = 0.0f;
#pragma unroll
          for (int s = 0; s < MB; ++s) gg += d2r[s] * S.x2[net][s][k];
          adam1(w2[net], gg, m2[net], v2[net], lrb, isq); dep = w2[net];
        }
        {
          const int k = opaque(2 * g + c2c, dep);
          float gg = 0.0f;
#pragma unroll
          for (int s = 0; s < MB; ++s) gg += dn2[s] * S.x2[net][s][k];
          adam1(c2[net], gg, cm2[net], cv2[net], lrb, isq); dep = c2[net];
        }
      }
      // heads: this CU's HPC elements; the new weight is published for phase D of every CU (tag == step)
      if (tid < HPC) {
        const int net = head_net(hrow);
        const float gs = sc.gs(net), lrb = sc.lrb(net), isq = sc.isq(net);
        float gg = 0.0f;
#pragma unroll
        for (int s = 0; s < MB; ++s) gg += (hrow < A ? S.dmu[s][hrow] : S.dv[hrow - A][s]) * gs * S.x3[net][s][hk];
        adam1(hw, gg, hm, hv, lrb, isq);
      }
      if (wave == 0) head_publish(LQ, LL, tid, he, hw, tag_prev);   // the three rows of a column meet in one lane: eight packed words and row 24's
      if (tid >= BIAS_L2 && tid < BIAS_HEAD + A + 2) {   // layer-2 and head biases
        int net; float gg = 0.0f;
        if (tid < BIAS_HEAD) { net = tid - BIAS_L2; for (int s = 0; s < MB; ++s) gg += S.dyown[net][s][DY_L2]; }
        else { const int row = tid - BIAS_HEAD; net = head_net(row); for (int s = 0; s < MB; ++s) gg += row < A ? S.dmu[s][row] : S.dv[row - A][s]; }
        adam_bias(S, sc, tid, net, gg);
      } else if (tid >= T_LOGSTD && tid < T_LOGSTD + A) {   // logstd
        const int a = tid - T_LOGSTD;
        float b = s_b2[0][a], bm = s_b2[1][a], bv = s_b2[2][a];
        adam1(b, S.dls[a] * sc.gs(0), bm, bv, sc.lrb(0), sc.isq(0));
        s_b2[0][a] = b; s_b2[1][a] = bm; s_b2[2][a] = bv;
      }
    }
    TS(6)
    if (last) break;
    __syncthreads();   // every wave is done with the old S.x2 / S.x3 / S.dy2 / S.dmu / S.dv
    // ================================================================== phase C: gather x2, forward L2
    const size_t r0 = (size_t)mbi * MB;
    float pf_act = 0.0f, pf_omu = 0.0f, pf_osg = 1.0f;   // this minibatch's actions and old (mu, sigma): needed in phase D
    float pf_adv = 0.0f, pf_nlp = 0.0f, pf_ret = 0.0f, pf_val = 0.0f;   // per-sample scalars, held by the lane that forms the sample's losses
    if (tid < MB * 32 && (tid % 32) == 31) {
      const size_t i = r0 + tid / 32;
      pf_adv = D.adv[i]; pf_nlp = D.mb_neglogp[i];
    }
    if (tid >= T_VLOSS && tid < T_VLOSS + 2 * MB) {   // (the value-head loss lanes (j, s): loss_front)
      const size_t i = r0 + (tid - T_VLOSS) % MB;
      pf_ret = D.returns[i]; pf_val = D.mb_values[i];
    }
    if (tid < MB * 32 && (tid % 32) < A) {
      const size_t i = (r0 + tid / 32) * A + tid % 32;
      pf_act = D.mb_actions[i];
      // (mu, sigma) were rewritten by CU 0 one mini-epoch ago (update_mu_sigma): agent-scope accesses keep them coherent across XCDs
      pf_omu = __hip_atomic_load(&D.mb_mus[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      pf_osg = __hip_atomic_load(&D.mb_sigmas[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    {
      // Word tid + NTH j is (sample j, unit tid) - and unit tid = wave 64 + lane is the element of row g this lane owns: the products of
      // forward L2 are formed from the gathered registers; the S.x2 image (Gram of x2, backward L2's elu', the next step's Adam of layer 2)
      // is stored behind them, under the DPP sums.
      static_assert(NTH == U1 && MB == 4, "word tid + NTH j of the x2 edge is (sample j, unit tid)");
      float x[3][MB], u[3];
      {
        float v0[4], v1[4], v2[4];
        lq_take_or_gather<4>(px2_issued, px2, LQ, LQ_X2 + tid, NTH, tag, v0, v1, v2, failflag, S.fail);
        TS(7)
#pragma unroll
        for (int s = 0; s < MB; ++s) { x[0][s] = v0[s]; x[1][s] = v1[s]; x[2][s] = v2[s]; }
        image_store(S.x2, v0, v1, v2, tid);
      }
      // (no barrier here: the one that stood between the S.x2 stores and their read-back also kept the S.fpart stores below behind forward L1's
      // readers of S.fpart - the barrier in front of phase C does that - and the S.x2 stores in front of their readers, which all sit behind
      // the barrier that follows the S.fpart stores)
      // (the twelve sums of bare products as one butterfly behind an explicit fma level: the bits of the twelve wave_sum trees that stood here,
      // whose first add the compiler contracted with the product per lane - fwd2_sums above)
      fwd2_sums(w2, x, u, lane);
      fwd2_store(S, u, wave, lane);
    }
    __syncthreads();
    if (wave == 0) {   // wave 0: lane (net, s) < 12 forms one output, lane s < 4 stores the word (fwd_tail)
      float y[3];
      fwd_tail<2>(S, lane, y);
      if (tid < MB) lq_store(LQ, LQ_X3 + (unsigned)tid * U2 + g, y[0], y[1], y[2], tag);
    }
    TS(8)
    // (this minibatch's actions and old (mu, sigma) go to LDS before the Grams: three registers fewer across the 60-value reduction)
    if (tid < MB * 32) { S.act[tid / 32][tid % 32] = pf_act; S.omu[tid / 32][tid % 32] = pf_omu; S.osg[tid / 32][tid % 32] = pf_osg; }
    if (tid >= T_LS && tid < T_LS + 32) { const float l_ = (tid - T_LS < A) ? s_b2[0][tid - T_LS] : 0.0f; S.ls[tid - T_LS] = l_; S.sgm[tid - T_LS] = expf(l_); }
    u32x4 ph[4];
    u64 p24[4];
    if constexpr (!SINGLE)
    {   // ---- (shadow of x3) Grams of x2 and x1 (S.x1 stays valid until the next step's gather).  Two butterflies, ONE pass through LDS
        // and its two barriers: out[0..29] = [x2: net][10], out[32..61] = [x1: net][10]
      float ua[8], ub[8];
      {
        float p[30];
#pragma unroll
        for (int i = 0; i < 30; ++i) p[i] = 0.0f;
#pragma unroll
        for (int net = 0; net < 3; ++net) gram_acc10(&p[net * 10], S.x2[net][0][tid], S.x2[net][1][tid], S.x2[net][2][tid], S.x2[net][3][tid]);
        row_butterfly<30>(p, ua, lane);
      }
      rows_store<8>(S, ua, 0, wave, lane);
      {
        float p[30];
#pragma unroll
        for (int i = 0; i < 30; ++i) p[i] = 0.0f;
#pragma unroll
        for (int h = 0; h < U0 / NTH; ++h) {
#pragma unroll
          for (int net = 0; net < 3; ++net) { const int k = tid + NTH * h; gram_acc10(&p[net * 10], S.x1[net][0][k], S.x1[net][1][k], S.x1[net][2][k], S.x1[net][3][k]); }
          // (the first column's terms are ROUNDED products, the second column is accumulated onto them by fma.  A diagonal entry is a sum of two
          // squares, x x + y y, and 0 + x x folds to the bare product, so either square may be the one contracted into the fma: which one the
          // compiler picks moved with code elsewhere in the kernel, and with it the last bit of G_x1[s][s].  The opaque copy keeps the first.)
          if (h == 0) {
#pragma unroll
            for (int i = 0; i < 30; ++i) asm("" : "+v"(p[i]));
          }
        }
        row_butterfly<30>(p, ub, lane);
      }
      rows_store<8>(S, ub, 32, wave, lane);
      // first look at this wave's head rows (phase D's row view): the words left their CUs a phase ago, in the x2 shadow, and what the top of
      // phase D paid for them was the round trip of its own loads.  Four packed words and row 24's four 8-byte words are 24 registers across
      // rows_reduce; the 8-byte form of the whole matrix was 32 + 8 with the x3 words and spilled here.  Unconditional: at step 0 nobody has
      // published, the words are not taken (a first look behind `if (step != 0)` cost 56 bytes of scratch: its registers then meet at a merge)
      head_rows_peek(LQ, wave, lane, ph); head_row24_peek(LL, wave, lane, tag_prev, p24);
      rows_reduce(S, 64, S.part, tid);
      if (tid < 48) S.gx[tid >> 4][2][tid & 15] = S.part[(tid >> 4) * 10 + tri16(tid & 15)];
      else if (tid >= 64 && tid < 64 + 48) { const int t = tid - 64; S.gx[t >> 4][1][t & 15] = S.part[32 + (t >> 4) * 10 + tri16(t & 15)]; }
    }
    TS(9)
    refresh();
    // ================================================================== phase D: gather x3 and the heads, losses, backward to dY1
    float wh[HR][4];   // this wave's head rows for the forward (row = wave + 8 j, columns lane + 64 e)
    // The head words were published a phase ago (shadow of x2), so they are normally all there.  Row view (head forward): the lane's four
    // packed words - rows wave, wave + 8, wave + 16 of columns lane + 64 e - and, on wave 0, row 24's four words were requested inside the x3
    // shadow (above) and are taken here; what this point still waits for is the first look at the lane's two x3 words (round 3: five chained
    // gathers, then the x3 gather: 2.4 us between the x3 publish and the head forward, 0.7 of them the x3 edge itself).  If a word is missing
    // the polling gathers below wait.  The column view is first used by the heads' backward: it is requested after the head forward, under
    // the loss phase.  (One minibatch: no shadow, and only step 0, which takes the weights from the parameter array.)
    bool row_done = false;
    {
      // first look at this lane's two x3 words; if the x3 words of a slow producer are not there yet, the polling gather below continues
      // after the head words have been taken
      u32x4 w3[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) w3[i] = load16(LQ, LQ_X3 + tid + i * NTH);
      if (step != 0) {
        if constexpr (SINGLE) { head_rows_peek(LQ, wave, lane, ph); head_row24_peek(LL, wave, lane, tag_prev, p24); }
        row_done = head_rows_take(ph, p24, tag_prev, wh);
      }
      float v0[2], v1[2], v2[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) { v0[i] = __uint_as_float(w3[i].x); v1[i] = __uint_as_float(w3[i].y); v2[i] = __uint_as_float(w3[i].z); }
      if (__builtin_amdgcn_ballot_w64(!(lq_ok(w3[0], tag) && lq_ok(w3[1], tag))) != 0) {
        if (!lq_gather<2>(LQ, LQ_X3 + tid, NTH, tag, v0, v1, v2, failflag)) S.fail = 1;
      }
      image_store(S.x3, v0, v1, v2, tid);
    }
    if (!row_done) {
      if (step == 0) {   // nothing has been published yet: the weights the launch started from
#pragma unroll
        for (int j = 0; j < HR; ++j) {
          const int row = wave + 8 * j;
#pragma unroll
          for (int e = 0; e < 4; ++e) wh[j][e] = 0.0f;
          if (row < A + 2) {
            const float* hp = P_of(head_net(row)) + head_woff(row) + lane;
#pragma unroll
            for (int e = 0; e < 4; ++e) wh[j][e] = hp[64 * e];
          }
        }
      } else if (!head_rows_gather(LQ, LL, wave, lane, tag_prev, wh, failflag)) S.fail = 1;
    }
    TS(10)
    __syncthreads();
    // head forward: wave per row (head_forward: the value rows' operands and the rows' biases are requested with the actor rows')
    head_forward(S, wh, wave, lane);
    __syncthreads();
    TS(11)
    // Column view of the head words (this lane's column c2n, rows 13 c2c .. 13 c2c + 12; first used by the heads' backward): requested
    // here, under the loss phase.  No tags: between them the row views of the eight waves cover every head word - wave w words 256 w ..
    // 256 w + 255 of LQ_HW, wave 0 also the 256 words of row 24 - each wave has seen its words' tags (first look or polling gather) before
    // the barrier in front of the head forward, and the words are not rewritten before every CU has finished this step - so the values are
    // read as plain agent-scope loads: eight 8-byte pieces of packed words and one dword of row 24, 17 registers (head_cols_load).
    // (the per-sample scalars prefetched in phase C are taken NOW: the loads below sit behind lane-dependent conditions, and after such a
    // merge the compiler's counter model waits for everything outstanding at the next use of any loaded register - that use would be
    // pf_adv in the loss phase, i.e. the column loads' whole round trip: 0.6 us on the chain)
    SDX_OPAQUE(pf_adv); SDX_OPAQUE(pf_nlp); SDX_OPAQUE(pf_ret); SDX_OPAQUE(pf_val);
    // (the z chain's four LDS operands are asked for HERE, in front of the column view's address arithmetic and loads: loss_request)
    ZOps zo;
    loss_request(S, tid, zo);
    __builtin_amdgcn_sched_barrier(0);
    HeadCols hc;       // rows w + 8 c2c and w + 8 + 8 c2c of the column, w < 8, and row 24: head_cols_take picks wc[] out of them behind the loss phase
    if (step == 0) {
#pragma unroll
      for (int w = 0; w < 8; ++w) {
        const int ra = w + 8 * c2c, rb = ra + 8;
        hc.pair[w].x = __float_as_uint(P_of(head_net(ra))[head_woff(ra) + c2n]); hc.pair[w].y = __float_as_uint(P_of(head_net(rb))[head_woff(rb) + c2n]);
      }
      hc.r24 = __float_as_uint(P_of(2)[head_woff(A + 1) + c2n]);
    } else head_cols_load(LQ, c2c, c2n, hc);   // 9 unconditional loads, nothing between them that looks at a loaded value
    const float invM = 1.0f / (float)MB;
    // (the loss phase restates sdxp_ppo_terms.h: loss_front / loss_back, sdxp_persist_phase_d.h.  Only what the gradients need: the KL, bounds and
    // entropy terms of the statistics are formed in the dY1 shadow, on waves 5 and 7)
    {
      const LossCfg lc = {D.e_clip, D.critic_coef, D.bounds_coef, (bool)D.clip_value};
      float q, bt;
      loss_front(S, lc, tid, zo, pf_adv, pf_nlp, pf_ret, pf_val, invM, q, bt);
      SDX_LDS_BARRIER();   // LDS traffic only: the column view's loads stay in flight (a __syncthreads() would wait for them)
      loss_back(S, tid, q, bt, invM);
      if (g == 0 && tid < MB * 32 && tid % 32 < A) {   // update_mu_sigma (RC:1358), CU 0 only
        const int s = tid / 32, a = tid % 32;
        __hip_atomic_store(&D.mb_mus[(r0 + s) * A + a], S.mu[s][a], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&D.mb_sigmas[(r0 + s) * A + a], S.sgm[a], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      SDX_LDS_BARRIER();   // LDS traffic only: the column view's loads stay in flight (a __syncthreads() would wait for them)
    }
    TS(12)
    refresh();   // (c2n / c2c and the addresses formed from them are derived HERE: formed in front of the head forward they were spilled across it)
    // backward through the heads: lane (column k = c2n, row half c2c) forms its part of dX3[.][k]; the two halves of a column are lanes l and
    // l ^ 32 of ONE wave and meet through v_permlane32_swap, elu' is applied in both lanes, and backward L2's products are fed from these
    // registers.  One code path for both halves: rows 13 c2c + j, j < 13 - the upper half's j = 10, 11 are the two value heads (a1, a2) and
    // S.dmu[.][23..25] are zeros (written with the rest of the row), so its a0 takes three exact zeros instead of a branch that every wave
    // would run both sides of.
    // (no barriers here: the two that let the halves meet in S.dy2 ordered nothing else - S.dmu / S.dv / S.x3 were published by the barriers
    // of the loss phase, and the last readers of S.red / S.part, in the x3 shadow, are behind the barriers of the head forward.  The S.dy2
    // stores below sit in front of block_sum's barriers, their readers - the Gram of dY2, dyown[.][.][DY_L2], the next step's Adam of layer 2 -
    // behind them.)
    float d2[3][MB];
    float wc[13];      // (row 25 = 13 + 12 does not exist: its slot repeats row 24 and is never used)
    head_cols_take(hc, c2c, wc);
    head_backward(S, wc, c2c, c2n, d2);   // (its LDS operands requested ahead of the chains: sdxp_persist_phase_d.h)
    TS(13)
    // backward L2 with the column copy: dY1[net][s][2g+c] = (sum_n dY2[net][s][n] W2[n][2g+c]) * elu'(x2[net][s][2g+c])
    {
      // Lane half c2c holds column 2g + c2c only, so the butterfly runs over 12 values per lane, not 24 of which half are zeros: a 16-lane
      // DPP row lies inside one half, and rows 2 c2c, 2 c2c + 1 of every wave are summed for column c.  A DPP row still holds sixteen
      // consecutive rows n of the column in lane order, and the sixteen row sums are still added in ascending n: the sums of the
      // 24-wide reduction over (column = tid >> 8, row = tid & 255), bit for bit.
      float p[12];
#pragma unroll
      for (int net = 0; net < 3; ++net)
#pragma unroll
        for (int s = 0; s < MB; ++s) p[net * MB + s] = d2[net][s] * c2[net];
      // each column's dY2 is stored once, behind the products: lane half c2c stores samples 2 c2c, 2 c2c + 1
#pragma unroll
      for (int net = 0; net < 3; ++net)
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          float lo = d2[net][i], hi = d2[net][2 + i];
          asm volatile("" : "+v"(lo), "+v"(hi));   // (a select of two elements of d2 becomes d2[2 c2c + i]: the array would live in scratch)
          S.dy2[net][2 * c2c + i][c2n] = c2c ? hi : lo;
        }
      {
        float u2[3];
        row_butterfly<12>(p, u2, lane);
        rows_store<3>(S, u2, 0, wave, lane);
      }
      // dY1 leaves from the reducing lanes, in front of the closing barrier: lane (net MB + s) 2 + c < 24 of wave 0 applies elu' to its own sum
      // and stores dyown; lanes l + 8 (the same DPP row) and l + 16 (the next row: v_permlane16_swap) hand networks 1 and 2 of (s, c) to lane
      // l < 8, which publishes the word.  (S.part is not written: the read-back it served is gone.)
      const int bi = tid >> 1, bc = tid & 1, bnet = min(tid >> 3, 2), bs = bi & 3;
      const float eg = tid < 24 ? elu_g(S.x2[bnet][bs][2 * g + bc]) : 0.0f;   // (requested in front of the barrier: it does not wait for the sums)
      SDX_LDS_BARRIER();
      if (wave == 0) {
        float v = 0.0f;
        if (tid < 24) {   // (net MB + s, c)
          // rows 16 j .. 16 j + 15 of the column, j ascending: rows 4 w + 2 bc, 4 w + 2 bc + 1 of S.red, all sixteen requested in front of the first add
          float r[2 * NWV];
#pragma unroll
          for (int w = 0; w < NWV; ++w) { r[2 * w] = S.red[4 * w + 2 * bc][bi]; r[2 * w + 1] = S.red[4 * w + 2 * bc + 1][bi]; }
          asm volatile("" ::: "memory");
          float t = 0.0f;
#pragma unroll
          for (int j = 0; j < 2 * NWV; ++j) t += r[j];
          v = t * eg;
          S.dyown[bnet][bs][DY_L1 + bc] = v;
        }
        const float v1 = dpp_mov<0x108, 0xF>(0.0f, v);                                        // row_shl:8: lane l + 8
        const unsigned y = __builtin_bit_cast(unsigned, v);
        const auto r = __builtin_amdgcn_permlane16_swap(y, y, false, false);                  // r[1]: rows 1, 1, 3, 3 - lane l + 16 for l < 16
        const float v2 = __builtin_bit_cast(float, (unsigned)r[1]);
        if (tid < MB * 2) lq_store(LQ, LQ_DY1 + (unsigned)(tid >> 1) * U1 + 2 * g + (tid & 1), v, v1, v2, tag);
      }
      // (the reduction's closing barrier - S.red read out before its next writer, S.dyown[.][.][DY_L1 ..] published - stands in the dY1 shadow, in front
      // of that shadow's rows_store: the other waves form their parts of the shadow while wave 0 adds and publishes.  One minibatch: the barrier in
      // front of its statistics thread.)
    }
    TS(14)
    u32x4 pdy1[4];
    bool pdy1_issued = false;
    // ---- (shadow of dY1) loss statistics + LR rule, Gram of x3, head / logstd terms of the squared gradient norm.  Spread over the
    // waves: the x3 Gram's per-thread part only occupies threads 0..255, so the serial pieces - the statistics / LR rule, the products
    // dmu_a . dmu_b and the column sums of the head terms - run on waves 4..6 in front of the SAME block reduction instead of in two more
    // barrier-separated phases after it (3.1 -> about 2 us: this shadow was the longest overrun of its edge, section 4b of DESIGN.md).
    // The statistics-only terms of the loss phase (KL, bounds loss, entropy: a logf, two IEEE divisions and three half-wave sums per lane that
    // no gradient uses) are formed HERE, on waves 5 and 7 as lane (sample, action) - S.mu / S.omu / S.osg / S.sgm / S.ls are those of the loss
    // phase - in front of the reduction's first barrier; the statistics thread runs behind that barrier.
    if (wave == 5 || wave == 7) {   // (wave 4 has the heads' 23-term products in front of the same barrier, wave 6 the statistics thread)
      const int s = (wave - 5) + (lane >> 5), a = lane & 31;
      float r_kl = 0.0f, r_bl = 0.0f, r_ent = 0.0f;
      if (a < A) {
        const float ls = S.ls[a], sg = S.sgm[a], mu = S.mu[s][a];
        const float omu = S.omu[s][a], osg = S.osg[s][a];
        r_kl = logf(osg / sg + 1e-5f) + (sg * sg + (omu - mu) * (omu - mu)) / (2.0f * (osg * osg + 1e-5f)) - 0.5f;
        const float hi = fmaxf(mu - 1.1f, 0.0f), lo = fminf(mu + 1.1f, 0.0f);
        r_bl = hi * hi + lo * lo;
        r_ent = 0.5f + 0.5f * 1.8378770664093453f + ls;
      }
      r_kl = half_sum(r_kl); r_bl = half_sum(r_bl); r_ent = half_sum(r_ent);
      if (a == 31) { S.stat[s][STAT_BOUNDS] = r_bl; S.stat[s][STAT_KL] = r_kl; S.stat[s][STAT_ENTROPY] = r_ent; }
    }
    if (tid == T_STATS) {   // what does not wait for the KL stays in front of the barrier
      PLds::Ctl& C = S.ctl;
      C.ac_lr_applied = C.ac_lr;   // the optimiser step of THIS minibatch uses the current lr; the schedule moves it afterwards
      if constexpr (!SINGLE) {
        // Adam step counters / bias corrections of the optimiser step that applies THIS minibatch's gradient (phase A of the next
        // iteration): nothing here depends on the gradient, so it left the chain (round 6; the double-precision powers and the two
        // divisions sat between the norm and the first Adam instruction).  S.scal[SC_AC_LR_BC1 ..] were last read by the Adam shadows of this
        // iteration, which every wave finished before the barrier in front of phase C
        C.ac_t += 1; C.cv_t += 1;
        C.ac_b1 *= 0.9; C.ac_b2 *= 0.999; C.cv_b1 *= 0.9; C.cv_b2 *= 0.999;
        S.scal[SC_AC_LR_BC1] = C.ac_lr_applied / (float)(1.0 - C.ac_b1); S.scal[SC_AC_ISQ] = 1.0f / sqrtf((float)(1.0 - C.ac_b2));
        S.scal[SC_CV_LR_BC1] = C.cv_lr / (float)(1.0 - C.cv_b1); S.scal[SC_CV_ISQ] = 1.0f / sqrtf((float)(1.0 - C.cv_b2));
      }
    }
    // (everything the thread reads from LDS is requested at once, the arithmetic is that of the serial loop: stats_lr_once)
    auto stats_and_lr = [&]() { if (tid == T_STATS) stats_lr_once(S, invM, D.adaptive_lr, D.kl_threshold); };
    if constexpr (SINGLE) { SDX_LDS_BARRIER(); stats_and_lr(); }   // (one minibatch: no reduction here whose barrier the statistics could share)
    if constexpr (!SINGLE) {
      // Round 6: the Gram of x3 (waves 0..3, unit = tid) and the Gram of dY2 (waves 4..7, unit = tid - 256; it used to wait for the dY0 shadow, whose
      // block reduction is on the chain since the norm edge shrank) go through ONE pass: columns 0..29 / 32..61, each summed over its 16 rows.
      // The heads' terms are only STORED here (S.part[PART_HEAD_G ..], [PART_HEAD_B ..]); the serial sums that closed this shadow (16 + 23 dependent LDS reads on
      // three threads, about 1 us after the reduction) are lanes of the DPP sum at the end of the dY0 shadow now.
      float p[30];
#pragma unroll
      for (int i = 0; i < 30; ++i) p[i] = 0.0f;
      if (tid >= T_HEAD_G && tid < T_HEAD_G + 48) {    // thread (net, a, b): the heads' gradient product that multiplies G_x3[a][b]
        const int t = tid - T_HEAD_G, net = t / 16, a = (t / 4) % 4, b = t % 4;
        float dd = 0.0f;
        if (net == 0) { for (int j = 0; j < A; ++j) dd += S.dmu[a][j] * S.dmu[b][j]; }
        else dd = S.dv[net - 1][a] * S.dv[net - 1][b];
        S.part[PART_HEAD_G + t] = dd;
      } else if (tid >= T_HEAD_B && tid < T_HEAD_B + 32) {   // bias of the policy head and logstd: |sum_s dmu_s[j]|^2 + dlogstd[j]^2
        const int j = tid - T_HEAD_B;
        float t = 0.0f;
        if (j < A) { float sb = 0; for (int a = 0; a < MB; ++a) sb += S.dmu[a][j]; t = sb * sb + S.dls[j] * S.dls[j]; }
        S.part[PART_HEAD_B + j] = t;
      }
      if (tid < U2) {
#pragma unroll
        for (int net = 0; net < 3; ++net) gram_acc10(&p[net * 10], S.x3[net][0][tid], S.x3[net][1][tid], S.x3[net][2][tid], S.x3[net][3][tid]);
      } else {
        const int k = tid - U2;
#pragma unroll
        for (int net = 0; net < 3; ++net) gram_acc10(&p[net * 10], S.dy2[net][0][k], S.dy2[net][1][k], S.dy2[net][2][k], S.dy2[net][3][k]);
      }
      {
        float u[8];
        row_butterfly<30>(p, u, lane);
        SDX_LDS_BARRIER();   // backward L2's closing barrier: wave 0 has read S.red out
        rows_store<8>(S, u, tid < U2 ? 0 : 32, wave, lane);
      }
      SDX_LDS_BARRIER();
      if (tid < 64) {                                 // column tid: rows of waves 0..3 (x3) or 4..7 (dY2)
        const int r0 = tid < 32 ? 0 : 2 * NWV;
        const float t = ordered_sum_ahead<2 * NWV, 64>(&S.red[r0][tid]);
        const int c = tid & 31, net = c / 10, e = c - net * 10;
        // entry e of the lower triangle -> both (hi, lo) and (lo, hi) of the 4x4 matrix
        const int hi = e < 1 ? 0 : (e < 3 ? 1 : (e < 6 ? 2 : 3)), lo = e - hi * (hi + 1) / 2;
        if (c < 30) {
          float* dst = tid < 32 ? S.gx[net][3] : S.gd2[net];
          dst[hi * 4 + lo] = t; dst[lo * 4 + hi] = t;
        }
      }
      // first look at this lane's dY1 words (the polling gather of phase E takes over if a producer is late)
      lq_peek<4>(LQ, LQ_DY1 + tid, NTH, pdy1); pdy1_issued = true;
      stats_and_lr();                                  // thread T_STATS, beside the column sums of threads 0..63 and behind its wave's first look; its readers sit behind the barrier below
      SDX_LDS_BARRIER();
    }
    TS(15)
    refresh();
    // ================================================================== phase E: gather dY1, backward L1
    {
      // Word tid + NTH j is (sample j, unit tid), and row tid of the column copy is this lane's: the products of backward L1 are formed from
      // the gathered registers; the S.dy1 image (Gram of dY1, the next step's Adam of layer 1) is stored behind them.
      float p[48];
      {
        float v0[4], v1[4], v2[4];
        lq_take_or_gather<4>(pdy1_issued, pdy1, LQ, LQ_DY1 + tid, NTH, tag, v0, v1, v2, failflag, S.fail);
        TS(16)
#pragma unroll
        for (int s = 0; s < MB; ++s)
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            p[(0 * MB + s) * 4 + c] = v0[s] * c1[0][c]; p[(1 * MB + s) * 4 + c] = v1[s] * c1[1][c]; p[(2 * MB + s) * 4 + c] = v2[s] * c1[2][c];
          }
        image_store(S.dy1, v0, v1, v2, tid);
      }
      // (no barrier here on the epoch's chain: the one that stood between the S.dy1 stores and their read-back also kept block_sum's stores to
      // S.red / S.part behind the dY1 shadow's readers of both - the LDS barrier that closes that shadow does that - and the S.dy1 stores in
      // front of the Gram of dY1, which sits behind block_sum's barriers.  The one-minibatch instantiation has no such shadow: it keeps it.)
      if constexpr (SINGLE) __syncthreads();
      // block_sum<48>, opened up: the 48 reducing lanes (net MB + s) 4 + c = 16 net + 4 s + c of wave 0 - network net is DPP row net - apply
      // elu' to their own 32-term sum and store dyown; what leaves the CU (the norm word; in the one-minibatch instantiation the dY0 words,
      // rows 1 and 2 reaching row 0 through v_permlane16_swap / v_permlane32_swap) goes out in FRONT of the reduction's second barrier, which
      // the shadow's rows_store still needs.  (S.part is not written: the read-back it served is gone.)
      {
        float u2[12];
        row_butterfly<48>(p, u2, lane);
        rows_store<12>(S, u2, 0, wave, lane);
      }
      const int es = (tid >> 2) & 3, ec = tid & 3, enet = min(tid >> 4, 2);
      const float eg = tid < 48 ? elu_g(S.x1[enet][es][4 * g + ec]) : 0.0f;   // (requested in front of the barrier: it does not wait for the sums)
      SDX_LDS_BARRIER();
      if (wave == 0) {
        float v = 0.0f;
        if (tid < 48) {
          const float t = ordered_sum_ahead<4 * NWV, 64>(&S.red[0][tid]);
          v = t * eg;
          S.dyown[enet][es][DY_L0 + ec] = v;
        }
        if constexpr (SINGLE) {
          const unsigned y = __builtin_bit_cast(unsigned, v);
          const auto r16 = __builtin_amdgcn_permlane16_swap(y, y, false, false);   // r16[1]: rows 1, 1, 3, 3 - lane l + 16 for l < 16
          const auto r32 = __builtin_amdgcn_permlane32_swap(y, y, false, false);   // r32[1]: the upper half in both halves - lane l + 32 for l < 32
          if (tid < MB * 4)
            lq_store(LQ, LQ_DY0 + (unsigned)es * U0 + 4 * g + ec, v, __builtin_bit_cast(float, (unsigned)r16[1]), __builtin_bit_cast(float, (unsigned)r32[1]), tag);
        }
      }
      if constexpr (!SINGLE) {
        // the other CUs need dY0 only for the gradient norm: publish this CU's share of the Gram dY0 dY0^T (its four columns).
        // Lanes 0..47 of wave 0 wrote dyown above; the same wave reads it back (LDS keeps program order within a wave)
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        if (wave == 0) {
          // lane (a, b) < 16: entry (a, b) of the CU's 4x4 Gram of dY0 (its four columns) times (G_x0[a][b] + 1): the weight-gradient term
          // <G_dY0, G_x0> and the bias term |sum_s dY0_s|^2 = sum of all entries of the Gram; a DPP row sum, ONE word per CU
          float t[3] = {0.0f, 0.0f, 0.0f};
          if (lane < 16) {
            const int hi = lane >> 2, lo = lane & 3;
#pragma unroll
            for (int net = 0; net < 3; ++net) {
              float gg = 0.0f;
#pragma unroll
              for (int c = 0; c < 4; ++c) gg += S.dyown[net][hi][DY_L0 + c] * S.dyown[net][lo][DY_L0 + c];
              t[net] = gg * S.gx0[net >> 1][lane] + gg;
            }
          }
#pragma unroll
          for (int net = 0; net < 3; ++net) t[net] = row_sum16(t[net]);
          if (lane == 0) lq_store(LQ, LQ_G0 + g, t[0], t[1], t[2], tag);
        }
        // (the reduction's second barrier stands in the dY0 shadow, in front of its rows_store: the other waves form their Gram terms meanwhile)
      }
    }
    TS(17)
    if constexpr (SINGLE) {
      // ---- hand the minibatch over to the multi-rank exchange: rank-MB factors -> D.fact (layout SdxpFactOff), CU g writes slice g
      __syncthreads();
      float* F = D.fact;
      const int i = g * NTH + tid, stride = NWG * NTH;
      for (int j = i; j < MB * D.obs_dim; j += stride) {
        const float v = S.obs[j / D.obs_dim][j % D.obs_dim];
        F[D.foff.x[0][0] + j] = v; F[D.foff.x[1][0] + j] = v;
      }
      for (int j = i; j < MB * ST; j += stride) F[D.foff.x[2][0] + j] = (&S.cvx[0][0])[j];
#pragma unroll
      for (int net = 0; net < 3; ++net) {
        for (int j = i; j < MB * U0; j += stride) F[D.foff.x[net][1] + j] = (&S.x1[net][0][0])[j];
        for (int j = i; j < MB * U1; j += stride) { F[D.foff.x[net][2] + j] = (&S.x2[net][0][0])[j]; F[D.foff.dy[net][1] + j] = (&S.dy1[net][0][0])[j]; }
        for (int j = i; j < MB * U2; j += stride) { F[D.foff.h[net] + j] = (&S.x3[net][0][0])[j]; F[D.foff.dy[net][2] + j] = (&S.dy2[net][0][0])[j]; }
      }
      if (i < MB * U0) {   // dY0: every CU produced four columns of it; the first 8 CUs collect the packed words
        float v0[1], v1[1], v2[1];
        if (!lq_gather<1>(LQ, LQ_DY0 + i, 1, tag, v0, v1, v2, failflag)) S.fail = 1;
        F[D.foff.dy[0][0] + i] = v0[0]; F[D.foff.dy[1][0] + i] = v1[0]; F[D.foff.dy[2][0] + i] = v2[0];
      }
      if (g == 0) {
        if (tid < MB * 34) {
          const int s = tid / 34, c = tid % 34;
          F[D.foff.dh + tid] = c < A ? S.dmu[s][c] : (c == 32 ? S.dv[0][s] : (c == 33 ? S.dv[1][s] : 0.0f));
        }
        if (tid >= 192 && tid < 192 + 32) F[D.foff.dls + tid - 192] = tid - 192 < A ? S.dls[tid - 192] : 0.0f;
        if (tid == 0) {   // what k_ctrl does after a minibatch in explicit (multi-rank) mode: statistics, KL words, cursor
          const PLds::Ctl& C = S.ctl;
          gctl->sum_a_loss += C.sum_a; gctl->sum_c_loss += C.sum_c; gctl->sum_b_loss += C.sum_b; gctl->sum_kl += C.sum_kl;
          gctl->sum_cv_loss += C.sum_cv; gctl->sum_entropy += C.sum_ent; gctl->n_mb += 1; gctl->last_kl = C.last_kl;
          gctl->ac_pending = 0; gctl->cv_pending = 0;
          F[D.foff.kl] = C.last_kl; D.ac_g[D.g_tail] = C.last_kl;
          gctl->prev_mb = gctl->mb_index; gctl->prev_mini_epoch = gctl->mini_epoch;
          int mbn = gctl->mb_index + 1;
          if (mbn >= D.num_minibatches) { mbn = 0; gctl->mini_epoch += 1; }
          gctl->mb_index = mbn;
          gctl->step += 1;
          gctl->ll_tag = tag_base + 3u;
        }
      }
      return;
    }
    if constexpr (!SINGLE)
    {   // ---- (shadow of dY0; on the step's chain since the norm edge shrank to one word per CU) Gram of dY1 - the Gram of dY2 moved into the dY1
        // shadow (round 6) -, this lane's layer-0 gradient elements, the next step's rows, and the part of the squared norm that does not wait for dY0
      {
        float p[30], ua[8];
#pragma unroll
        for (int i = 0; i < 30; ++i) p[i] = 0.0f;
#pragma unroll
        for (int net = 0; net < 3; ++net) gram_acc10(&p[net * 10], S.dy1[net][0][tid], S.dy1[net][1][tid], S.dy1[net][2][tid], S.dy1[net][3][tid]);
        row_butterfly<30>(p, ua, lane);
        SDX_LDS_BARRIER();   // backward L1's second barrier: wave 0 has read S.red out and published, S.dyown[.][.][DY_L0 ..] is there for what follows
        rows_store<8>(S, ua, 0, wave, lane);
      }
      SDX_LDS_BARRIER();          // (rows_reduce, opened up: the stage between its two barriers occupies 32 threads ...)
      lq_peek<4>(LQ, LQ_G0 + lane, 64, pg0); pg0_issued = true;   // (0.7 us into the shadow: the words left their CUs 0.7 + 2.0 (phase E) us ago; the round trip ends with the shadow)
      if (tid < 32) {
        S.part[tid] = ordered_sum_ahead<4 * NWV, 64>(&S.red[0][tid]);
      }
      // ... so this lane's layer-0 gradient elements are formed here, by every wave (dyown[.][.][DY_L0 ..] were published by the barrier above;
      // S.obs / S.cvx still hold this minibatch): 4 + 5 batches of four independent LDS loads instead of 13 dependent round trips on the chain
      {
        float da[MB], dc[MB], dvv[MB];
#pragma unroll
        for (int s = 0; s < MB; ++s) { da[s] = S.dyown[0][s][DY_L0 + r0w]; dc[s] = S.dyown[1][s][DY_L0 + r0w]; dvv[s] = S.dyown[2][s][DY_L0 + r0w]; }
#pragma unroll
        for (int i = 0; i < I0A; ++i) {
          const int kk = lane + 64 * i, k = h0 * H0A + kk;
          const bool ok = kk < H0A && k < D.obs_dim;
          const int kc = ok ? k : 0;
          float ga = 0.0f, gc = 0.0f;
#pragma unroll
          for (int s = 0; s < MB; ++s) { const float x = S.obs[s][kc]; ga += da[s] * x; gc += dc[s] * x; }
          g0a[i] = ok ? ga : 0.0f; g0c[i] = ok ? gc : 0.0f;
          m0a[i] *= 0.9f; v0a[i] *= 0.999f; m0c[i] *= 0.9f; v0c[i] *= 0.999f;   // (adam1p: off the chain)
        }
#pragma unroll
        for (int i = 0; i < I0V; ++i) {
          const int kk = lane + 64 * i, k = h0 * H0V + kk;
          const bool ok = kk < H0V;
          const int kc = ok ? k : 0;
          float gv = 0.0f;
#pragma unroll
          for (int s = 0; s < MB; ++s) gv += dvv[s] * S.cvx[s][kc];
          g0v[i] = ok ? gv : 0.0f;
          m0v[i] *= 0.9f; v0v[i] *= 0.999f;
        }
      }
      SDX_LDS_BARRIER();
      if (step + 1 < total_steps) { const bool wrap = mbi + 1 >= D.num_minibatches; load_rows(wrap ? 0 : mbi + 1, mini_epoch + (wrap ? 1 : 0)); }
      if (wave == 1) {
        // lane (net, i) < 48: entry i of the Grams of dY1 / dY2 against (G_x1 / G_x2 + 1) - weight and bias gradients of trunk layers 1, 2 -, of the
        // Gram of x3 against the heads' gradient products (S.part[PART_HEAD_G ..], dY1 shadow), + the head-bias / logstd terms (32 entries over the 16 lanes
        // of net 0; |sum_s dV_s|^2 on lane 0 of nets 1, 2); a DPP row sum per network
        float t = 0.0f;
        if (lane < 48) {
          const int net = lane >> 4, i = lane & 15;
          t = S.part[net * 10 + tri16(i)] * (S.gx[net][1][i] + 1.0f) + S.gd2[net][i] * (S.gx[net][2][i] + 1.0f) + S.gx[net][3][i] * S.part[PART_HEAD_G + net * 16 + i];
          if (net == 0) t += S.part[PART_HEAD_B + i] + S.part[PART_HEAD_B + 16 + i];
          else if (i == 0) { float sb = 0.0f; for (int a = 0; a < MB; ++a) sb += S.dv[net - 1][a]; t += sb * sb; }
        }
        t = row_sum16(t);
        if (lane < 48 && (lane & 15) == 0) S.n2rest[lane >> 4] = t;
      } else if (tid >= 128 && tid < 128 + 3 * MB) { const int net = (tid - 128) / MB, s = (tid - 128) % MB; S.dyown[net][s][DY_L2] = S.dy2[net][s][g]; }
    }
    TS(18)
    pending = true;
  }

  if (stamps && g == (stamps >> 8) && tid < 32) D.dbg[tid] = S.tacc[tid];
  // ------------------------------------------------------------------ epilogue: resident parameters back to HBM
  refresh();
#pragma unroll
  for (int i = 0; i < I0A; ++i) {
    const int kk = lane + 64 * i, k = h0 * H0A + kk;
    if (kk < H0A && k < D.obs_dim) {
      const size_t oa = o_w0(0, k), oc = o_w0(1, k);
      D.ac[oa] = w0a[i]; D.ac_m[oa] = m0a[i]; D.ac_v[oa] = v0a[i];
      D.ac[oc] = w0c[i]; D.ac_m[oc] = m0c[i]; D.ac_v[oc] = v0c[i];
    }
  }
#pragma unroll
  for (int i = 0; i < I0V; ++i) {
    const int kk = lane + 64 * i, k = h0 * H0V + kk;
    if (kk < H0V) { const size_t o = woff(2, 0) + (size_t)n0 * ST + k; D.cv[o] = w0v[i]; D.cv_m[o] = m0v[i]; D.cv_v[o] = v0v[i]; }
  }
#pragma unroll
  for (int net = 0; net < 3; ++net) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const size_t o = o_w1(net, i);
      P_of(net)[o] = w1[net][i]; M_of(net)[o] = m1[net][i]; V_of(net)[o] = v1[net][i];
    }
    {
      const size_t o = woff(net, 2) + (size_t)g * U1 + wave * 64 + lane;
      P_of(net)[o] = w2[net]; M_of(net)[o] = m2[net]; V_of(net)[o] = v2[net];
    }
  }
  if (tid < HPC) {
    const int net = head_net(hrow);
    const size_t o = o_hw();
    P_of(net)[o] = hw; M_of(net)[o] = hm; V_of(net)[o] = hv;
  }
  auto bias_store = [&](int net, size_t o) { P_of(net)[o] = S.bias[tid]; M_of(net)[o] = S.bias_m[tid]; V_of(net)[o] = S.bias_v[tid]; };
  if (g == 0) {   // head biases and logstd are replicated on every CU: CU 0 writes them
    if (tid >= BIAS_HEAD && tid < BIAS_HEAD + A + 2) {
      const int row = tid - BIAS_HEAD;
      bias_store(head_net(row), head_boff(row));
    }
    if (tid >= T_LOGSTD && tid < T_LOGSTD + A) {
      const int a = tid - T_LOGSTD;
      const size_t o = D.off.logstd + a;
      D.ac[o] = s_b2[0][a]; D.ac_m[o] = s_b2[1][a]; D.ac_v[o] = s_b2[2][a];
    }
    if (tid == 0) {
      const PLds::Ctl& C = S.ctl;
      gctl->ac_lr = C.ac_lr; gctl->ac_t = C.ac_t; gctl->cv_t = C.cv_t;
      gctl->ac_b1pow = C.ac_b1; gctl->ac_b2pow = C.ac_b2; gctl->cv_b1pow = C.cv_b1; gctl->cv_b2pow = C.cv_b2;
      gctl->sum_a_loss = C.sum_a; gctl->sum_c_loss = C.sum_c; gctl->sum_b_loss = C.sum_b; gctl->sum_kl = C.sum_kl;
      gctl->sum_cv_loss = C.sum_cv; gctl->sum_entropy = C.sum_ent; gctl->n_mb = total_steps; gctl->last_kl = C.last_kl;
      gctl->ac_gnorm = C.ac_gn; gctl->cv_gnorm = C.cv_gn; gctl->ac_pending = 0; gctl->cv_pending = 0;
      gctl->mb_index = 0; gctl->mini_epoch = total_steps / D.num_minibatches;
      gctl->ll_tag = tag_base + (unsigned)total_steps + 2u;
    }
  }
  if (tid < BIAS_L1) { const int net = (tid - BIAS_L0) / 4, w = (tid - BIAS_L0) % 4; bias_store(net, boff(net, 0) + 4 * g + w); }
  else if (tid < BIAS_L2) { const int net = (tid - BIAS_L1) / 2, r = (tid - BIAS_L1) % 2; bias_store(net, boff(net, 1) + 2 * g + r); }
  else if (tid < BIAS_HEAD) { const int net = tid - BIAS_L2; bias_store(net, boff(net, 2) + g); }
}

extern "C" size_t sdxpk_persist_lds_bytes() { return sizeof(PLds); }
extern "C" int sdxpk_persist_supported(const SdxpDev* D, int minibatch, int n_cus) {
  return minibatch == MB && D->obs_dim <= OBS && D->obs_dim % 4 == 0 && D->state_dim == ST && D->units[0] == U0 && D->units[1] == U1 &&
         D->units[2] == U2 && D->act_dim == ACT && n_cus >= NWG;
}
// both instances may use their LDS on the current device `dev` (sdxp_create); 0: they cannot, the handle takes the multi-kernel paths
extern "C" int sdxpk_persist_prepare(int dev) {
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(k_update_persistent<false>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(PLds)) == hipSuccess &&
      hipFuncSetAttribute(reinterpret_cast<const void*>(k_update_persistent<true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(PLds)) == hipSuccess) return 1;
  (void)hipGetLastError();
  fprintf(stderr, "libseqdex_hip: k_update_persistent cannot have %zu bytes of LDS on device %d: this handle uses the hipGraph update and the multi-kernel step\n", sizeof(PLds), dev);
  return 0;
}
// The 4x4 Grams of the layer-0 inputs of every minibatch of the epoch: tab[mb][GX0_OBS | GX0_CVX0 | GX0_CVX1][16], one workgroup per
// minibatch.  The rows are dataset rows - mb_obs is fixed for the epoch, cvx0 / cvx1 are written by the pre-normalisation in front of the
// persistent launch - so the epoch kernel, which formed these Grams in the shadow of its x1 edge in every one of the mini-epochs, fetches
// them with the rows instead (load_rows).  The summation order is the one that shadow had, so that the norm words keep their bits: thread
// tid holds column tid of the observations (zero past obs_dim) and columns tid, tid + NTH of the central value's rows; value 0..9 the
// observations' triangle, 11..20 the central value's (10 and 21, |sum_s x_s|^2, had no reader and stay zero: the butterfly keeps its
// numbering); row_butterfly<22> over the 16-lane DPP rows, then the 32 row sums added from 0.0f in ascending (wave, row) order.  Two
// passes, cvx0 and cvx1 (the observations' values of the second are not stored).
__global__ __launch_bounds__(NTH) void k_input_grams(const float* __restrict__ obs, int obs_dim, const float* __restrict__ cvx0, const float* __restrict__ cvx1, float* __restrict__ tab) {
  __shared__ float red[4 * NWV][24];
  __shared__ float part[24];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const size_t mb = blockIdx.x;
  const float* o = obs + mb * MB * obs_dim;
  float xo[MB];
#pragma unroll
  for (int s = 0; s < MB; ++s) xo[s] = tid < obs_dim ? o[(size_t)s * obs_dim + tid] : 0.0f;
  for (int cls = 0; cls < 2; ++cls) {
    const float* c = (cls == 0 ? cvx0 : cvx1) + mb * MB * ST;
    float xa[MB], xb[MB];
#pragma unroll
    for (int s = 0; s < MB; ++s) { xa[s] = c[s * ST + tid]; xb[s] = tid + NTH < ST ? c[s * ST + tid + NTH] : 0.0f; }
    float p[22], u2[6];
#pragma unroll
    for (int i = 0; i < 22; ++i) p[i] = 0.0f;
    if (tid < OBS) gram_acc10(&p[0], xo[0], xo[1], xo[2], xo[3]);
    gram_acc10(&p[11], xa[0], xa[1], xa[2], xa[3]);
    if (tid + NTH < ST) gram_acc10(&p[11], xb[0], xb[1], xb[2], xb[3]);
    row_butterfly<22>(p, u2, lane);
    if ((lane & 15) < 4) {
      float* r = red[wave * 4 + (lane >> 4)];
#pragma unroll
      for (int j = 0; j < 6; ++j) r[4 * j + (lane & 3)] = u2[j];
    }
    __syncthreads();
    if (tid < 22) {
      float t = 0.0f;
#pragma unroll
      for (int w = 0; w < 4 * NWV; ++w) t += red[w][tid];
      part[tid] = t;
    }
    __syncthreads();
    float* out = tab + mb * GX0_STRIDE;
    if (tid < 16) { if (cls == 0) out[GX0_OBS + tid] = part[tri16(tid)]; }
    else if (tid >= 64 && tid < 80) out[(cls == 0 ? GX0_CVX0 : GX0_CVX1) + tid - 64] = part[11 + tri16(tid - 64)];
    __syncthreads();   // part and red are written again by the second pass
  }
}
// obs [4 n_mb][obs_dim], cvx0 / cvx1 [4 n_mb][ST] -> tab [n_mb][GX0_STRIDE]; sdxp_update runs it behind the pre-normalisation of a persistent
// epoch, tests/test_gpu_persist_input_grams.py on rows of its own
extern "C" int sdxpk_input_grams(const float* obs, int obs_dim, const float* cvx0, const float* cvx1, int n_mb, float* tab, hipStream_t st) {
  if (obs_dim < 1 || obs_dim > OBS || n_mb < 1) return -1;
  hipLaunchKernelGGL(k_input_grams, dim3(n_mb), dim3(NTH), 0, st, obs, obs_dim, cvx0, cvx1, tab);
  return 0;
}
extern "C" size_t sdxpk_input_grams_floats(int n_mb) { return (size_t)n_mb * GX0_STRIDE; }
// stamps: SdxpOpts::persist_stamps (phase clock of one CU); fault: SDXP_PERSIST_FAULT=1 (one CU goes silent: the failure-path test); gx0_tab: the
// table k_input_grams wrote for this epoch's rows
extern "C" int sdxpk_update_persistent(const SdxpDev* D, const float* gx0_tab, int total_steps, unsigned* failflag, int stamps, int fault, hipStream_t st) {
  if (hipMemsetAsync(failflag, 0, sizeof(unsigned), st) != hipSuccess) return -1;
  hipLaunchKernelGGL(k_update_persistent<false>, dim3(NWG), dim3(NTH), sizeof(PLds), st, *D, total_steps, gx0_tab, failflag, stamps, fault);
  return 0;
}
// forward + backward of the minibatch under the device cursor -> D.fact (multi-rank path); the fail flag is sticky (not cleared here)
extern "C" int sdxpk_fwd_bwd_persistent(const SdxpDev* D, unsigned* failflag, hipStream_t st) {
  hipLaunchKernelGGL(k_update_persistent<true>, dim3(NWG), dim3(NTH), sizeof(PLds), st, *D, 1, nullptr, failflag, 0, 0);
  return 0;
}
