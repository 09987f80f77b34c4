// sdxp_rollout.hip — the rollout of rl_games' A2CAgent as hand-written HIP for gfx950; the update phase is in
// sdxp_update.hip / sdxp_persist.hip (rank-MB step), sdxp_multirank.hip (after the ranks' exchange) and sdxp_bigmb.hip (GEMM step).
// M = num_envs rows: fp32 MFMA GEMMs  Y = ELU(X W^T + b)  (v_mfma_f32_32x32x2_f32, LDS-tiled, 64x64 block tile, 4 waves of 32x32),
// head kernel = mu / value / Gaussian sample / neglogp (RC:1697-1723,2114-2126), reward bookkeeping, GAE and advantage normalisation.
#include "sdxp_device.h"
#include "sdxp_launch.h"
#include "sdx_mfma.h"

// ------------------------------------------------------------------------------------------------ rollout GEMM
// Y[M,N] = act(X[M,K] W[N,K]^T + b[N]); act = ELU when elu_flag.  X may be normalised on the fly with (mean, rstd)
// (central-value running mean/std, clamp +-5; App. C of SURVEY.md).  K % 4 == 0.
// One launch serves up to TWO such products (blockIdx.z): the same layer of the actor and of the central-value trunk during a rollout.
// 64 x 64 output tile per workgroup (4 waves, one 32 x 32 v_mfma_f32_32x32x2_f32 tile each), reduction chunks of 32.  The operands of chunk
// c + 2 are in flight from HBM / L2 (registers) while chunk c is multiplied out of one LDS buffer and chunk c + 1 is written into the other:
// ONE barrier per chunk and two chunks of load latency hidden.  (Round 2's kernel loaded, stored, synchronised and multiplied one
// 16-wide chunk at a time: 25 dependent round trips for the 396-wide first layer, 35 us per launch, 6 launches per env step.)
#define GT 64
#define SDXP_NORM_K 1024   // widest input that may be normalised on the fly (checked by the launchers)
struct LinArgs { const float* X; const float* W; const float* b; float* Y; int M, N, K, elu; const double* nmean; const double* nvar; };
struct LinBatch { LinArgs a[2]; };
// WTM = 1: 64 x 64 tile (wave = 32 x 32); WTM = 2: 128 x 64 tile (wave = 64 x 32: two MFMAs share one W operand - 21 instead of 16 flops
// per operand byte fetched from L2).  GKc = reduction chunk staged per barrier.  KS = split of every chunk over KS groups of four waves
// (256 KS threads): group g multiplies the k range [g GKc / KS, (g + 1) GKc / KS) of each chunk into its own accumulators and the groups
// are summed through LDS, in group order, at the end.  At M = 1024 the middle and last layers launch only 256 / 128 workgroups, one wave
// per SIMD: every LDS read and every barrier was exposed (matrix pipe 26 % busy, profiles/r3_act_pmc.csv); with KS groups a SIMD holds
// KS waves whose reads and multiplies overlap, and each thread moves 1 / KS of the operands.
template <int WTM, int KS, int GKc>
__global__ __launch_bounds__(256 * KS) void k_linear_mfma(LinBatch lb) {
  constexpr int TM = GT * WTM, NT = 256 * KS, F4R = GKc / 4;       // rows of X per tile, threads, float4 pieces per row and chunk
  constexpr int NX = TM * F4R / NT, NW = GT * F4R / NT, KG = GKc / KS;
  static_assert(NX >= 1 && NW >= 1 && TM * F4R % NT == 0 && GT * F4R % NT == 0 && KG % 2 == 0, "chunk does not divide over the threads");
  constexpr int OPER = 2 * (TM + GT) * (GKc + 1), RED = (KS - 1) * 4 * 16 * 64;
  __shared__ float lds[OPER > RED ? OPER : RED];
  __shared__ float nmu[SDXP_NORM_K], nsd[SDXP_NORM_K];            // mean and sqrt(var + eps) of the normalised input, as floats
  float (*Xs)[TM][GKc + 1] = reinterpret_cast<float (*)[TM][GKc + 1]>(lds);
  float (*Ws)[GT][GKc + 1] = reinterpret_cast<float (*)[GT][GKc + 1]>(lds + 2 * TM * (GKc + 1));
  const LinArgs& g = lb.a[blockIdx.z];
  const int tid = threadIdx.x, wave = (tid >> 6) & 3, kg = tid >> 8, lane = tid & 63;
  // (An XCD-aware workgroup -> tile map - the tiles cut into 8 rectangles, XCD c working through rectangle c so that it pulls 1/4 of X and
  // 1/2 of W through the fabric instead of all of X - was measured at M = 1024: 87.3 us per sdxp_act against 86.2 with the plain map.
  // These layers are not bound by operand traffic.)
  const int m0 = blockIdx.y * TM, n0 = blockIdx.x * GT;
  const int M = g.M, N = g.N, K = g.K;
  if (m0 >= M || n0 >= N) return;                 // the grid covers the larger problem of the batch
  const int wm = (wave >> 1) * 32 * WTM, wn = (wave & 1) * 32;
  f32x16 acc[WTM];
#pragma unroll
  for (int u = 0; u < WTM; ++u)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[u][i] = 0.0f;
  // element e = tid + NT p of a chunk: row e / F4R, k offset 4 (e % F4R): consecutive lanes read consecutive 16-byte pieces of a row.
  // fetch() only issues loads, from clamped (always valid) addresses and without a branch, so that the compiler can count them: with
  // exec-masked loads every wait became vmcnt(0) and the chunk in flight was waited for where it was issued.  stage() zeroes the pieces
  // outside the matrix and applies the running-mean/std normalisation of X from per-k tables built once per workgroup (same arithmetic
  // as normalising at load time)
  float4 xv0[NX], xv1[NX], wv0[NW], wv1[NW];
  auto fetch = [&](int k0, float4 (&xr)[NX], float4 (&wr)[NW]) {
#pragma unroll
    for (int p = 0; p < NX; ++p) {
      const int e = tid + NT * p, r = e / F4R, k = k0 + 4 * (e % F4R);
      const int rr = m0 + r < M ? m0 + r : M - 1, kc = k < K ? k : 0;
      xr[p] = *reinterpret_cast<const float4*>(g.X + (size_t)rr * K + kc);
    }
#pragma unroll
    for (int p = 0; p < NW; ++p) {
      const int e = tid + NT * p, r = e / F4R, k = k0 + 4 * (e % F4R);
      const int rr = n0 + r < N ? n0 + r : N - 1, kc = k < K ? k : 0;
      wr[p] = *reinterpret_cast<const float4*>(g.W + (size_t)rr * K + kc);
    }
  };
  const bool norm = g.nmean != nullptr;
  auto stage = [&](int buf, int k0, const float4 (&xr)[NX], const float4 (&wr)[NW]) {
#pragma unroll
    for (int p = 0; p < NX; ++p) {
      const int e = tid + NT * p, r = e / F4R, k = 4 * (e % F4R);
      const bool in = m0 + r < M && k0 + k < K;
      float xq[4] = {xr[p].x, xr[p].y, xr[p].z, xr[p].w};
      if (norm) {
        const int kt = in ? k0 + k : 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) xq[j] = clampf((xq[j] - nmu[kt + j]) / nsd[kt + j], -5.0f, 5.0f);
      }
      float* dx = &Xs[buf][r][k];
#pragma unroll
      for (int j = 0; j < 4; ++j) dx[j] = in ? xq[j] : 0.0f;
    }
#pragma unroll
    for (int p = 0; p < NW; ++p) {
      const int e = tid + NT * p, r = e / F4R, k = 4 * (e % F4R);
      const bool in = n0 + r < N && k0 + k < K;
      float* dw = &Ws[buf][r][k]; dw[0] = in ? wr[p].x : 0.0f; dw[1] = in ? wr[p].y : 0.0f; dw[2] = in ? wr[p].z : 0.0f; dw[3] = in ? wr[p].w : 0.0f;
    }
  };
  // all LDS operands of the chunk are requested before the first multiply (the rolled form read two, waited, multiplied twice)
  auto mma = [&](int buf) {
    float av[WTM][KG / 2], bv[KG / 2];
#pragma unroll
    for (int j = 0; j < KG / 2; ++j) {
      const int kk = kg * KG + 2 * j + (lane >> 5);
      bv[j] = Ws[buf][wn + (lane & 31)][kk];
#pragma unroll
      for (int u = 0; u < WTM; ++u) av[u][j] = Xs[buf][wm + 32 * u + (lane & 31)][kk];
    }
    __builtin_amdgcn_sched_barrier(0);             // (the scheduler otherwise sinks the reads back between the multiplies)
#pragma unroll
    for (int j = 0; j < KG / 2; ++j)
#pragma unroll
      for (int u = 0; u < WTM; ++u) acc[u] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[u][j], bv[j], acc[u], 0, 0, 0);
  };
  const int nchunk = (K + GKc - 1) / GKc;
  fetch(0, xv0, wv0);
  fetch(GKc, xv1, wv1);
  if (norm) {
    for (int k = tid; k < K; k += NT) { nmu[k] = (float)g.nmean[k]; nsd[k] = sqrtf((float)g.nvar[k] + 1e-5f); }
    __syncthreads();
  }
  stage(0, 0, xv0, wv0);
  __syncthreads();
  // two chunks per trip so that the register slots and LDS buffers are fixed names: chunk c multiplies out of buffer c & 1 while chunk
  // c + 2 is in flight into the slot chunk c came from and chunk c + 1 moves from the other slot into the other buffer; one barrier a chunk
  int c = 0;
  for (; c + 1 < nchunk; c += 2) {
    fetch((c + 2) * GKc, xv0, wv0);
    mma(0);
    stage(1, (c + 1) * GKc, xv1, wv1);
    __syncthreads();
    fetch((c + 3) * GKc, xv1, wv1);
    mma(1);
    stage(0, (c + 2) * GKc, xv0, wv0);
    __syncthreads();
  }
  if (c < nchunk) mma(0);                         // odd number of chunks: the last one sits in buffer 0
  if constexpr (KS > 1) {                          // sum of the k groups, in group order (the operand buffers are reused)
    static_assert(WTM == 1 || KS == 1, "the reduction buffer holds one accumulator tile per wave");
    __syncthreads();                               // an odd last chunk is still being read out of buffer 0
    for (int gsrc = 1; gsrc < KS; ++gsrc) {
      float* red = lds + ((gsrc - 1) * 4 + wave) * 16 * 64;
      if (kg == gsrc)
#pragma unroll
        for (int i = 0; i < 16; ++i) red[i * 64 + lane] = acc[0][i];
    }
    __syncthreads();
    if (kg != 0) return;
    for (int gsrc = 1; gsrc < KS; ++gsrc) {
      const float* red = lds + ((gsrc - 1) * 4 + wave) * 16 * 64;
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[0][i] += red[i * 64 + lane];
    }
  }
  const int col = n0 + wn + (lane & 31);
  if (col < N) {
    const float bias = g.b[col];
#pragma unroll
    for (int u = 0; u < WTM; ++u)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = mfma_cd_row(m0 + wm + 32 * u, r, lane);
        if (row < M) {
          const float v = acc[u][r] + bias;
          g.Y[(size_t)row * N + col] = g.elu ? elu(v) : v;
        }
      }
  }
}
// ---- the same product with the operands staged by LDS-DMA (round 6).  k_linear_mfma above moves every 16-byte piece
// global -> VGPR -> (normalise / zero) -> four ds_write_b32 into a padded [row][33] image and reads it back one dword at a time: per 32-wide
// chunk a wave issues 2 loads, 8 LDS stores and 16 LDS loads around its 8 MFMAs, in three barrier-separated phases (read, multiply, stage), and
// a chunk takes ~0.9 us where its multiplies need 0.5 (2 waves per SIMD).  Here the pieces go straight into LDS (global_load_lds_dwordx4: no
// staging registers, no LDS stores, no stage phase), into an XOR-swizzled image of 16-byte slots - slot(row, q) = 8 row + (q ^ ((row >> 1) & 7)),
// the swizzle applied on the SOURCE address since the DMA writes base + 16 lane - that ds_read_b128 reads without bank conflicts in its four
// 16-lane groups; a lane gets four k values per read, so a wave issues 4 LDS loads per chunk instead of 16 (the k order inside a chunk is
// permuted - lanes 0-31 take piece 2t, lanes 32-63 piece 2t + 1 of the k group - identically for both operands).  NBUF image pairs rotate:
// wait (counted vmcnt) for chunk c, LDS-only barrier, request chunk c + NBUF - 1 into the pair everybody finished reading before that barrier,
// read, multiply.  The normalisation of a first layer's input is applied to the A operand after the read (same arithmetic: (x - mean) / sd,
// clamp); pieces past K of the last chunk are zeroed in LDS by the lanes that would have loaded them.  ALL LDS of the kernel is one array (a
// second __shared__ object makes hipcc wait vmcnt(0) in front of every ds_read of a DMA pipeline).
// Measured (tools/time_linear.py, profiles/r6_linear_layers_lds_dma.txt): 28.2 / 29.0 / 17.1 us for the three layers against 30.5 / 29.4 / 17.0 with
// k_linear_mfma's best shape, and the same again (28.9 / 28.6 / 16.9) with the next chunk's LDS reads requested under this chunk's multiplies
// (the form below).  Neither the staging nor the LDS reads are what these layers wait for: a chunk costs 0.74 us = its 16 multiplies per SIMD at
// 68 % of the nominal fp32 matrix rate, the ceiling the large GEMMs of sdx_gemm_nt.h also sit at; a launch costs 5.2 us beyond its chunks, three
// times per sdxp_act.  sdxp_act as a whole did not move, so the launcher keeps shape 3; this kernel is shape 7
// (SDXP_LINEAR_TILE=7), held to float64 with every other shape by tests/test_gpu_linear_kernel.py.  A fourth image pair (72 KB of LDS: the tables
// then sit above 64 KB) gave wrong sums in normalised launches - LDS addresses above 64 KB through inline-asm ds_read - and 1 % in time: dropped.
// LDS reads of the DMA pipeline as inline asm: hipcc's wait-count pass treats every ds_read it can see as a possible reader of every LDS-DMA
// in flight and puts s_waitcnt vmcnt(0) in front of it (seen in the first build of this kernel: the chunk requested a line earlier was waited
// for at once, the pipeline was serial).  What it cannot see it does not wait for; the waits are spelled out (lds_wait4).
typedef float f4v_t __attribute__((ext_vector_type(4)));
__device__ __forceinline__ f4v_t lds_read128(unsigned byte_addr) {
  f4v_t v;
  asm volatile("ds_read_b128 %0, %1" : "=v"(v) : "v"(byte_addr));
  return v;
}
__device__ __forceinline__ void lds_wait4(f4v_t& a, f4v_t& b, f4v_t& c, f4v_t& d) { asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(a), "+v"(b), "+v"(c), "+v"(d)); }
template <int KS, int NBUF>
__global__ __launch_bounds__(256 * KS) void k_linear_glds(LinBatch lb) {
  static_assert(KS == 2 && NBUF == 3, "512 threads move one 16-byte piece of each operand tile per chunk; everything stays below 64 KB of LDS");
  constexpr int GK = 32, TILE = 64 * 8 * 4, OPER = NBUF * 2 * TILE, RED = (KS - 1) * 4 * 16 * 64, NTAB = SDXP_NORM_K + GK;
  static_assert(RED <= OPER, "the k-group reduction reuses the operand images");
  __shared__ __attribute__((aligned(16))) float lds[OPER + 2 * NTAB];
  float* nmu = lds + OPER;
  float* nsd = nmu + NTAB;
  const LinArgs& g = lb.a[blockIdx.z];
  const int tid = threadIdx.x, wave8 = tid >> 6, wave = wave8 & 3, kg = tid >> 8, lane = tid & 63;
  const int m0 = blockIdx.y * GT, n0 = blockIdx.x * GT;
  const int M = g.M, N = g.N, K = g.K;
  if (m0 >= M || n0 >= N) return;
  const int wm = (wave >> 1) * 32, wn = (wave & 1) * 32;
  const bool norm = g.nmean != nullptr;
  if (norm) {   // ordinary loads: finished (the barrier below) before the first DMA is requested
    for (int k = tid; k < NTAB; k += 256 * KS) { nmu[k] = k < K ? (float)g.nmean[k] : 0.0f; nsd[k] = k < K ? sqrtf((float)g.nvar[k] + 1e-5f) : 1.0f; }
    __syncthreads();
  }
  // loader coordinates: slot tid of an image = (row tid / 8, position tid % 8) holds piece q = position ^ swizzle(row) of that row
  const int lrow = tid >> 3, lq = (tid & 7) ^ ((lrow >> 1) & 7);
  const float* pa = g.X + (size_t)(m0 + lrow < M ? m0 + lrow : M - 1) * K + 4 * lq;
  const float* pb = g.W + (size_t)(n0 + lrow < N ? n0 + lrow : N - 1) * K + 4 * lq;
  const int nchunk = (K + GK - 1) / GK;
  auto request = [&](int c, int buf) {
    float* da = lds + buf * 2 * TILE + wave8 * 256;   // this wave's 64 slots of the A image (wave-uniform: the DMA adds 16 lane)
    float* db = da + TILE;
    if (c * GK + 4 * lq < K) {
      __builtin_amdgcn_global_load_lds(SDX_AS_GLOBAL(pa + c * GK), SDX_AS_LDS(da), 16, 0, 0);
      __builtin_amdgcn_global_load_lds(SDX_AS_GLOBAL(pb + c * GK), SDX_AS_LDS(db), 16, 0, 0);
    } else {                                        // past K (last chunk only): zeros, by the lanes whose pieces these are
      *reinterpret_cast<float4*>(da + 4 * lane) = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      *reinterpret_cast<float4*>(db + 4 * lane) = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
  };
  f32x16 acc;
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = 0.0f;
  // reader coordinates
  const int ra = wm + (lane & 31), rb = wn + (lane & 31), hf = lane >> 5;
  const int sa = ra * 8, xa = (ra >> 1) & 7, sb = rb * 8, xb = (rb >> 1) & 7;
  const unsigned lds_base = (unsigned)(uintptr_t)SDX_AS_LDS(lds);   // byte offset of the array inside the workgroup's LDS
  struct Frag { f4v_t a[2], b[2], mu[2], sd[2]; };
  auto read_chunk = [&](int c, int buf, Frag& f) {   // requests only: the LDS-only barrier of the next trip completes them
    const unsigned A = lds_base + (unsigned)buf * (2 * TILE * 4), B = A + TILE * 4;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int q = 4 * kg + 2 * t + hf;
      f.a[t] = lds_read128(A + 16u * (unsigned)(sa + (q ^ xa)));
      f.b[t] = lds_read128(B + 16u * (unsigned)(sb + (q ^ xb)));
      if (norm) {
        const unsigned k = (unsigned)(c * GK + 4 * q);
        f.mu[t] = lds_read128(lds_base + 4u * (OPER + k));
        f.sd[t] = lds_read128(lds_base + 4u * (OPER + NTAB + k));
      }
    }
  };
  // One trip = chunk c out of registers (its LDS reads were requested a trip ago and ran under the previous chunk's multiplies):
  //   wait (counted) until chunk c + 1 has landed, LDS-only barrier (everybody's reads of chunk c are complete: its image pair is free, and
  //   everybody's pieces of chunk c + 1 are there), request chunk c + NBUF into the freed pair, request the LDS reads of chunk c + 1, multiply chunk c.
  auto trip = [&](int c, int buf, Frag& cur, Frag& nxt) {
    if (c + 1 < nchunk) {
      if (c + NBUF - 1 < nchunk) asm volatile("s_waitcnt vmcnt(%0)" :: "n"(2 * (NBUF - 2)) : "memory");   // chunks c + 2 .. c + NBUF - 1 may still fly
      else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    SDX_LDS_BARRIER();
    lds_wait4(cur.a[0], cur.a[1], cur.b[0], cur.b[1]);            // (already complete: ties the registers to the wait for the compiler)
    if (norm) lds_wait4(cur.mu[0], cur.mu[1], cur.sd[0], cur.sd[1]);
    if (c + NBUF < nchunk) request(c + NBUF, buf);
    if (c + 1 < nchunk) read_chunk(c + 1, buf + 1 == NBUF ? 0 : buf + 1, nxt);
    __builtin_amdgcn_sched_barrier(0);                              // the reads are issued in front of the dependent multiplies, not behind them
    if (norm) {
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int i = 0; i < 4; ++i) cur.a[t][i] = clampf((cur.a[t][i] - cur.mu[t][i]) / cur.sd[t][i], -5.0f, 5.0f);
    }
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int i = 0; i < 4; ++i) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(cur.a[t][i], cur.b[t][i], acc, 0, 0, 0);
  };
#pragma unroll
  for (int c = 0; c < NBUF; ++c)
    if (c < nchunk) request(c, c);
  Frag f0, f1;
  // chunk 0: landed once at most NBUF - 1 younger chunks are outstanding
  if (nchunk >= NBUF) asm volatile("s_waitcnt vmcnt(%0)" :: "n"(2 * (NBUF - 1)) : "memory");
  else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  SDX_LDS_BARRIER();
  read_chunk(0, 0, f0);
  int buf = 0;
  for (int c = 0; c < nchunk; c += 2) {
    trip(c, buf, f0, f1);
    buf = buf + 1 == NBUF ? 0 : buf + 1;
    if (c + 1 < nchunk) {
      trip(c + 1, buf, f1, f0);
      buf = buf + 1 == NBUF ? 0 : buf + 1;
    }
  }
  // sum of the k groups, in group order (the operand images are reused)
  SDX_LDS_BARRIER();
  {
    float* red = lds + wave * 16 * 64;
    if (kg == 1)
#pragma unroll
      for (int i = 0; i < 16; ++i) red[i * 64 + lane] = acc[i];
    SDX_LDS_BARRIER();
    if (kg != 0) return;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] += red[i * 64 + lane];
  }
  const int col = n0 + wn + (lane & 31);
  if (col < N) {
    const float bias = g.b[col];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = mfma_cd_row(m0 + wm, r, lane);
      if (row < M) {
        const float v = acc[r] + bias;
        g.Y[(size_t)row * N + col] = g.elu ? elu(v) : v;
      }
    }
  }
}
template <int WTM, int KS, int GKc>
static void launch_linear_as(const LinBatch& lb, int count, int M, int Nx, hipStream_t st) {
  hipLaunchKernelGGL((k_linear_mfma<WTM, KS, GKc>), dim3((Nx + GT - 1) / GT, (M + WTM * GT - 1) / (WTM * GT), count), dim3(256 * KS), 0, st, lb);
}
#define SDXP_LINEAR_SMALL_M_SHAPE 3     // the automatic shape below M = 2048
static void launch_linear(const LinBatch& lb, int count, int M, int Nx, int shape, hipStream_t st) {
  // shape 0 (automatic): up to 2048 rows 64 x 64 tiles, every chunk split over two groups of four waves; beyond: 128 x 64.  Otherwise one shape
  // (SdxpOpts::linear_tile, timing aid): 1 = 64 x 64, 2 = 128 x 64, 3 = 64 x 64 with 2 k groups, 4 = the same with chunks of 64, 5 = 4 k groups and chunks of
  // 64, 6 = 64 x 64 with chunks of 64.  sdxp_act at M = 1024 (tools/time_act.py, profiles/r3_act_shapes.txt): 87 us with shape 3 or 4, 95 with
  // 1, 96 with 6, 95 with 5, 141 with 2 (round 3 started at 143 with shape 1: exec-masked loads made every wait vmcnt(0), and the LDS operands were
  // read two at a time).  The matrix pipe is about half busy in the middle layer; the rest is the per-chunk barrier and LDS read latency
  for (int i = 0; i < count; ++i)
    if (lb.a[i].nmean && lb.a[i].K > SDXP_NORM_K) { fprintf(stderr, "seqdex: k_linear_mfma normalises at most %d input columns (got %d)\n", SDXP_NORM_K, lb.a[i].K); abort(); }
  if (!shape) shape = M > 2048 ? 2 : SDXP_LINEAR_SMALL_M_SHAPE;
  switch (shape) {
    case 2: launch_linear_as<2, 1, 32>(lb, count, M, Nx, st); break;
    case 3: launch_linear_as<1, 2, 32>(lb, count, M, Nx, st); break;
    case 4: launch_linear_as<1, 2, 64>(lb, count, M, Nx, st); break;
    case 5: launch_linear_as<1, 4, 64>(lb, count, M, Nx, st); break;
    case 6: launch_linear_as<1, 1, 64>(lb, count, M, Nx, st); break;
    case 7: hipLaunchKernelGGL((k_linear_glds<2, 3>), dim3((Nx + GT - 1) / GT, (M + GT - 1) / GT, count), dim3(512), 0, st, lb); break;
    default: launch_linear_as<1, 1, 32>(lb, count, M, Nx, st); break;
  }
}

// counter-based standard normal (Box-Muller on two hashed uniforms)
__device__ __forceinline__ float randn(uint64_t seed, uint64_t a, uint64_t b) {
  const uint64_t h = sdx_hash(seed, a, b);
  const float u1 = ((float)((h >> 40) & 0xFFFFFF) + 1.0f) * (1.0f / 16777217.0f);
  const float u2 = (float)((h >> 8) & 0xFFFFFF) * (1.0f / 16777216.0f);
  return sqrtf(-2.0f * logf(u1)) * cosf(6.28318530718f * u2);
}

// rollout heads: one wave per env.  mu = h3a Wmu^T + b; V = h3v Wv^T + b (central value); a = mu + sigma eps;
// neglogp (RC:2114-2126); writes row (env, t) of the env-major experience buffer (PS:345-352).
__global__ __launch_bounds__(64) void k_act_heads(SdxpDev D, int t, const float* __restrict__ obs,
                                                  const float* __restrict__ states, const int64_t* __restrict__ dones,
                                                  const float* __restrict__ eps_in, float* __restrict__ actions_out,
                                                  uint64_t counter) {
  const int e = blockIdx.x, lane = threadIdx.x;
  const int A = D.act_dim;
  constexpr int U = 256;                            // units[2] (sdxp_create refuses other widths)
  __shared__ float s_h[2][U];
  const size_t row = (size_t)e * D.horizon + t;
  // Everything this workgroup reads that does not depend on its own arithmetic is requested up front - the trunk outputs, the value-head
  // weights and the observation / state rows that are copied into the dataset (16-byte pieces; obs_dim and state_dim are multiples of 4):
  // with 4 waves per CU every dependent load is a full L2 round trip (about 0.7 us), and the rolled copy loops alone were 16 of them
  constexpr int CP = 4;                             // 16-byte pieces per lane and row: rows up to 1024 floats (SDXP_NORM_K)
  float ha[U / 64], hv[U / 64], wvh[U / 64];
  float4 co[CP], cs[CP];
  const float4* osrc = reinterpret_cast<const float4*>(obs + (size_t)e * D.obs_dim);
  const float4* ssrc = reinterpret_cast<const float4*>(states + (size_t)e * D.state_dim);
  const int on4 = D.obs_dim >> 2, sn4 = D.state_dim >> 2;
#pragma unroll
  for (int i = 0; i < U / 64; ++i) {
    ha[i] = D.h_a[2][(size_t)e * U + lane + 64 * i];
    hv[i] = D.h_v[2][(size_t)e * U + lane + 64 * i];
    wvh[i] = D.cv[D.coff.v_w + lane + 64 * i];
  }
  // (lanes past the end of a row repeat its last piece, load and store alike: no branch for the optimiser to sink the loads into)
#pragma unroll
  for (int i = 0; i < CP; ++i) {
    co[i] = osrc[min(lane + 64 * i, on4 - 1)];
    cs[i] = ssrc[min(lane + 64 * i, sn4 - 1)];
  }
  __builtin_amdgcn_sched_barrier(0);               // (keeps the loads above the first use: the scheduler sinks each copy load to its store)
#pragma unroll
  for (int i = 0; i < U / 64; ++i) { s_h[0][lane + 64 * i] = ha[i]; s_h[1][lane + 64 * i] = hv[i]; }
  {
    float4* odst = reinterpret_cast<float4*>(D.mb_obs + row * D.obs_dim);
    float4* sdst = reinterpret_cast<float4*>(D.mb_states + row * D.state_dim);
#pragma unroll
    for (int i = 0; i < CP; ++i) {
      odst[min(lane + 64 * i, on4 - 1)] = co[i];
      sdst[min(lane + 64 * i, sn4 - 1)] = cs[i];
    }
  }
  __syncthreads();
  float nlp_part = 0.0f;
  if (lane < A) {
    const float* w = D.ac + D.off.mu_w + (size_t)lane * U;
    float mu = D.ac[D.off.mu_b + lane];
#pragma unroll 1
    for (int k0 = 0; k0 < U; k0 += 32) {           // 32 weight loads in flight (rolled, every k was its own L2 round trip: 13.7 us per launch);
      float wv[32];                                // the sum still runs over k in ascending order
#pragma unroll
      for (int j = 0; j < 32; ++j) wv[j] = w[k0 + j];
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int j = 0; j < 32; ++j) mu += wv[j] * s_h[0][k0 + j];
    }
    const float ls = D.ac[D.off.logstd + lane], sg = expf(ls);
    const float eps = eps_in ? eps_in[(size_t)e * A + lane] : randn(D.seed, counter, (uint64_t)e * 64 + lane);
    const float a = mu + sg * eps;
    const float z = (a - mu) / sg;
    nlp_part = 0.5f * z * z + ls;
    actions_out[(size_t)e * A + lane] = a;
    D.mb_actions[row * A + lane] = a;
    D.mb_mus[row * A + lane] = mu;
    D.mb_sigmas[row * A + lane] = sg;
  }
  const float nlp = wave_sum(nlp_part) + 0.5f * 1.8378770664093453f * (float)A;
  float vpart = 0.0f;
#pragma unroll
  for (int i = 0; i < U / 64; ++i) vpart += wvh[i] * hv[i];
  const float v = wave_sum(vpart) + D.cv[D.coff.v_b];
  if (lane == 0) {
    D.mb_neglogp[row] = nlp;
    D.mb_values[row] = v;
    D.mb_dones[row] = (dones && dones[e] != 0) ? 1.0f : 0.0f;
  }
}

__global__ void k_store_rewards(SdxpDev D, int t, const float* __restrict__ rew, const int64_t* __restrict__ dones_after) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= D.N) return;
  const float r = rew[e];
  D.mb_rewards[(size_t)e * D.horizon + t] = r;   // reward_shaper scale 1 (YG:32-33)
  // episode statistics (PS:361-373): current_rewards/current_lengths, game_rewards/game_lengths on done
  const float cr = D.cur_rew[e] + r, cl = D.cur_len[e] + 1.0f;
  const bool done = dones_after && dones_after[e] != 0;
  if (done) {
    atomicAdd(&D.ctrl->games_sum_rew, cr);
    atomicAdd(&D.ctrl->games_sum_len, cl);
    atomicAdd(&D.ctrl->games_cnt, 1.0f);
  }
  D.cur_rew[e] = done ? 0.0f : cr;
  D.cur_len[e] = done ? 0.0f : cl;
}

// last value head only (get_values, RC:1725-1752)
__global__ __launch_bounds__(64) void k_value_head(SdxpDev D, float* __restrict__ out) {
  const int e = blockIdx.x, lane = threadIdx.x, U = D.units[2];
  float p = 0.0f;
  for (int k = lane; k < U; k += 64) p += D.cv[D.coff.v_w + k] * D.h_v[2][(size_t)e * U + k];
  const float v = wave_sum(p) + D.cv[D.coff.v_b];
  if (lane == 0) out[e] = v;
}

// GAE (discount_values, PS:331-336) + returns, thread per env, env-major rows
__global__ void k_gae(SdxpDev D, const float* __restrict__ last_values, const int64_t* __restrict__ last_dones) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= D.N) return;
  const int H = D.horizon;
  float lastgae = 0.0f;
  for (int t = H - 1; t >= 0; --t) {
    float nonterminal, nextv;
    if (t == H - 1) { nonterminal = (last_dones && last_dones[e] != 0) ? 0.0f : 1.0f; nextv = last_values[e]; }
    else { nonterminal = 1.0f - D.mb_dones[(size_t)e * H + t + 1]; nextv = D.mb_values[(size_t)e * H + t + 1]; }
    const float v = D.mb_values[(size_t)e * H + t];
    const float delta = D.mb_rewards[(size_t)e * H + t] + D.gamma * nextv * nonterminal - v;
    lastgae = delta + D.gamma * D.tau * nonterminal * lastgae;
    D.returns[(size_t)e * H + t] = lastgae + v;
    D.adv[(size_t)e * H + t] = lastgae;          // advantages = returns - values (RC:1639)
  }
}

// advantage normalisation (RC:1645-1651): (A - mean) / (std_unbiased + 1e-8), one block over N*H values
__global__ __launch_bounds__(1024) void k_adv_norm(SdxpDev D) {
  __shared__ double s_a[16], s_b[16];
  const int n = D.N * D.horizon, tid = threadIdx.x;
  double s = 0.0, s2 = 0.0;
  for (int i = tid; i < n; i += 1024) { const double a = D.adv[i]; s += a; }
  // two-pass for accuracy: mean first
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  if ((tid & 63) == 0) s_a[tid >> 6] = s;
  __syncthreads();
  double tot = 0.0;
  for (int i = 0; i < 16; ++i) tot += s_a[i];
  const double mean = tot / n;
  for (int i = tid; i < n; i += 1024) { const double d = D.adv[i] - mean; s2 += d * d; }
  for (int o = 32; o > 0; o >>= 1) s2 += __shfl_xor(s2, o, 64);
  if ((tid & 63) == 0) s_b[tid >> 6] = s2;
  __syncthreads();
  double tot2 = 0.0;
  for (int i = 0; i < 16; ++i) tot2 += s_b[i];
  const float stdv = (float)sqrt(tot2 / (n - 1));
  const float fm = (float)mean;
  for (int i = tid; i < n; i += 1024) D.adv[i] = (D.adv[i] - fm) / (stdv + 1e-8f);
}
// observation rows narrower than the (4-aligned) network input: zero-padded copy
__global__ __launch_bounds__(256) void k_pad_obs(SdxpDev D, const float* __restrict__ obs) {
  const size_t total = (size_t)D.N * D.obs_dim;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const int c = (int)(i % D.obs_dim);
    D.obs_pad[i] = c < D.obs_cols ? obs[(i / D.obs_dim) * D.obs_cols + c] : 0.0f;
  }
}
__global__ void k_ctrl_begin_rollout(SdxpCtrl* c) { c->games_sum_rew = c->games_sum_len = c->games_cnt = 0.0f; }

// ------------------------------------------------------------------------------------------------ launch helpers
extern "C" void sdxpk_linear_as(const float* X, const float* W, const float* b, float* Y, int M, int N, int K, int elu_flag,
                                const double* nmean, const double* nvar, int shape, hipStream_t st) {
  LinBatch lb;
  lb.a[0] = LinArgs{X, W, b, Y, M, N, K, elu_flag, nmean, nvar};
  lb.a[1] = lb.a[0];
  launch_linear(lb, 1, M, N, shape, st);
}
// handle-less callers (Search's T-value): the automatic shape
extern "C" void sdxpk_linear(const float* X, const float* W, const float* b, float* Y, int M, int N, int K, int elu_flag,
                             const double* nmean, const double* nvar, hipStream_t st) {
  sdxpk_linear_as(X, W, b, Y, M, N, K, elu_flag, nmean, nvar, 0, st);
}
// two independent products in one launch (the same layer of the actor and of the central-value trunk)
extern "C" void sdxpk_linear2_as(const float* X0, const float* W0, const float* b0, float* Y0, int N0, int K0, const double* nmean0, const double* nvar0,
                                 const float* X1, const float* W1, const float* b1, float* Y1, int N1, int K1, const double* nmean1, const double* nvar1,
                                 int M, int elu_flag, int shape, hipStream_t st) {
  LinBatch lb;
  lb.a[0] = LinArgs{X0, W0, b0, Y0, M, N0, K0, elu_flag, nmean0, nvar0};
  lb.a[1] = LinArgs{X1, W1, b1, Y1, M, N1, K1, elu_flag, nmean1, nvar1};
  const int Nx = N0 > N1 ? N0 : N1;
  launch_linear(lb, 2, M, Nx, shape, st);
}
extern "C" void sdxpk_begin_rollout(const SdxpDev* D, hipStream_t st) { hipLaunchKernelGGL(k_ctrl_begin_rollout, dim3(1), dim3(1), 0, st, D->ctrl); }
extern "C" void sdxpk_pad_obs(const SdxpDev* D, const float* obs, hipStream_t st) { hipLaunchKernelGGL(k_pad_obs, dim3(256), dim3(256), 0, st, *D, obs); }
extern "C" void sdxpk_act_heads(const SdxpDev* D, int t, const float* obs, const float* states, const int64_t* dones,
                                const float* eps, float* actions_out, uint64_t counter, hipStream_t st) {
  hipLaunchKernelGGL(k_act_heads, dim3(D->N), dim3(64), 0, st, *D, t, obs, states, dones, eps, actions_out, counter);
}
extern "C" void sdxpk_store_rewards(const SdxpDev* D, int t, const float* rew, const int64_t* dones_after, hipStream_t st) { hipLaunchKernelGGL(k_store_rewards, dim3((D->N + 255) / 256), dim3(256), 0, st, *D, t, rew, dones_after); }
extern "C" void sdxpk_value_head(const SdxpDev* D, float* out, hipStream_t st) { hipLaunchKernelGGL(k_value_head, dim3(D->N), dim3(64), 0, st, *D, out); }
extern "C" void sdxpk_gae_only(const SdxpDev* D, const float* last_values, const int64_t* last_dones, hipStream_t st) { hipLaunchKernelGGL(k_gae, dim3((D->N + 255) / 256), dim3(256), 0, st, *D, last_values, last_dones); }
extern "C" void sdxpk_adv_norm(const SdxpDev* D, hipStream_t st) { if (D->normalize_advantage) hipLaunchKernelGGL(k_adv_norm, dim3(1), dim3(1024), 0, st, *D); }
