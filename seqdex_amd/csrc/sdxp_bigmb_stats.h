// sdxp_bigmb_stats.h — the central-value input normalisation of the large-minibatch PPO step (RunningMeanStd in train mode: update with
// the minibatch, then normalise it), column statistics reduced in fp64.  Included by sdxp_bigmb.hip only (its includes come first);
// sdxpk_big_prenorm launches these once per epoch.
#pragma once

// partial column sums / sums of squares (fp64) of rows [r0 + z * rchunk, ...) of mb_states
__global__ __launch_bounds__(256) void k_big_colstats(SdxpDev D, size_t r0, int MB, int rchunk, double* __restrict__ part) {
  __shared__ double s1[4][64], s2[4][64];
  const int S = D.state_dim, c = blockIdx.x * 64 + (threadIdx.x & 63), rg = threadIdx.x >> 6;
  const int rbeg = blockIdx.y * rchunk, rend = min(MB, rbeg + rchunk);
  double a = 0.0, q = 0.0;
  if (c < S)
    for (int r = rbeg + rg; r < rend; r += 4) { const double x = D.mb_states[(r0 + r) * S + c]; a += x; q += x * x; }
  s1[rg][threadIdx.x & 63] = a; s2[rg][threadIdx.x & 63] = q;
  __syncthreads();
  if (rg == 0 && c < S) {
    const int t = threadIdx.x;
    part[((size_t)blockIdx.y * S + c) * 2 + 0] = (s1[0][t] + s1[1][t]) + (s1[2][t] + s1[3][t]);
    part[((size_t)blockIdx.y * S + c) * 2 + 1] = (s2[0][t] + s2[1][t]) + (s2[2][t] + s2[3][t]);
  }
}
// RunningMeanStd.update with the minibatch statistics (unbiased batch variance, parallel-variance merge), thread = feature
__global__ __launch_bounds__(256) void k_big_rms_update(SdxpDev D, int MB, int nsplit, const double* __restrict__ part) {
  const int k = blockIdx.x * 256 + threadIdx.x, S = D.state_dim;
  if (k >= S) return;
  double a = 0.0, q = 0.0;
  for (int z = 0; z < nsplit; ++z) { a += part[((size_t)z * S + k) * 2]; q += part[((size_t)z * S + k) * 2 + 1]; }
  const double bm = a / MB;
  double bv = MB > 1 ? (q - MB * bm * bm) / (MB - 1) : 0.0;
  if (bv < 0.0) bv = 0.0;
  const double cnt = D.ctrl->rms_count, mean = D.rms_mean[k], var = D.rms_var[k];
  const double delta = bm - mean, tot = cnt + MB;
  const double m2 = var * cnt + bv * MB + delta * delta * cnt * MB / tot;
  D.rms_mean[k] = mean + delta * MB / tot;
  D.rms_var[k] = m2 / tot;
}
__global__ void k_big_rms_count(SdxpDev D, int MB) { D.ctrl->rms_count += (double)MB; }
// dst rows = clamp((x - mean) / sqrt(var + 1e-5), +-5) of mb_states rows [r0, r0 + rows)
__global__ __launch_bounds__(256) void k_big_normalise(SdxpDev D, size_t r0, size_t rows, float* __restrict__ dst) {
  const int S = D.state_dim;
  const size_t base = r0 * S, total = rows * S;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const int k = (int)((base + i) % S);
    const float x = D.mb_states[base + i];
    const float fm = (float)D.rms_mean[k], rs = sqrtf((float)D.rms_var[k] + 1e-5f);
    dst[base + i] = D.cv_normalize_input ? clampf((x - fm) / rs, -5.0f, 5.0f) : x;
  }
}
