// sdxp_launch.h — the one declaration of every sdxpk_* host launcher of the PPO library.  Included by sdxp_capi.hip (the caller) and by
// every unit that defines one of them, so that a definition whose parameters differ from the declaration fails to compile instead
// of linking silently.  SdxpDev goes to a launcher by pointer and to its kernels by value.  (sdxpk_linear, which sdx_task.hip borrows,
// is declared in sdx_kernels.h.)
#pragma once
#include <type_traits>
#include "sdx_kernels.h"
#include "sdxp_types.h"
struct NtArgs;   // sdx_gemm_nt.h
struct GemmArgs; // sdx_gemm.h
// device memory for a unit that sizes its own workspace: `bytes` zero-filled bytes owned by ctx (sdxp_create: the handle); SDX_OK or an error code
typedef int (*SdxpAllocFn)(void* ctx, void** ptr, size_t bytes);
extern "C" {
// sdxp_rollout.hip.  shape: SdxpOpts::linear_tile of the handle, 0 = automatic (launch_linear)
void sdxpk_linear_as(const float* X, const float* W, const float* b, float* Y, int M, int N, int K, int elu_flag, const double* nmean, const double* nvar, int shape, hipStream_t st);
void sdxpk_linear2_as(const float* X0, const float* W0, const float* b0, float* Y0, int N0, int K0, const double* nmean0, const double* nvar0,
                      const float* X1, const float* W1, const float* b1, float* Y1, int N1, int K1, const double* nmean1, const double* nvar1,
                      int M, int elu_flag, int shape, hipStream_t st);
void sdxpk_begin_rollout(const SdxpDev* D, hipStream_t st);
void sdxpk_pad_obs(const SdxpDev* D, const float* obs, hipStream_t st);
void sdxpk_act_heads(const SdxpDev* D, int t, const float* obs, const float* states, const int64_t* dones, const float* eps, float* actions_out, uint64_t counter, hipStream_t st);
void sdxpk_store_rewards(const SdxpDev* D, int t, const float* rew, const int64_t* dones_after, hipStream_t st);
void sdxpk_value_head(const SdxpDev* D, float* out, hipStream_t st);
void sdxpk_gae_only(const SdxpDev* D, const float* last_values, const int64_t* last_dones, hipStream_t st);
void sdxpk_adv_norm(const SdxpDev* D, hipStream_t st);
// sdxp_update.hip: the rank-MB step (minibatch_size 2 / 4 / 8; -1 for any other); parameter addressing: trunk_slot / head_row of sdxp_device.h
void sdxpk_begin_epoch(const SdxpDev* D, hipStream_t st);
int sdxpk_prenorm(const SdxpDev* D, int mb_size, hipStream_t st);
int sdxpk_update_begin(const SdxpDev* D, int mb_size, hipStream_t st);
int sdxpk_update_step(const SdxpDev* D, int mb_size, hipStream_t st);
int sdxpk_update_flush_layers(const SdxpDev* D, int mb_size, hipStream_t st);
int sdxpk_backward_explicit(const SdxpDev* D, int mb_size, hipStream_t st);
int sdxpk_backward_factors(const SdxpDev* D, int mb_size, hipStream_t st);
// sdxp_multirank.hip: what follows the exchange.  The rebuild from all ranks' factors is rebuild_row / head_elem there, stored by the first two
// launchers' kernels and kept in registers by the fused one, whose grid-wide meeting is built from sdxp_tagged_words.h
int sdxpk_grads_from_factors(const SdxpDev* D, int mb_size, hipStream_t st);
int sdxpk_apply_factors(const SdxpDev* D, int mb_size, hipStream_t st);
int sdxpk_apply_fused_prepare(const SdxpDev* D, int mb_size);
void sdxpk_apply_factors_fused(const SdxpDev* D, int mb_size, unsigned* bar, hipStream_t st);
void sdxpk_apply_flat(const SdxpDev* D, hipStream_t st);
void sdxpk_apply_explicit(const SdxpDev* D, int which, float kl, int world, hipStream_t st);
// sdxp_persist.hip
size_t sdxpk_persist_lds_bytes();
int sdxpk_persist_supported(const SdxpDev* D, int minibatch, int n_cus);
int sdxpk_persist_prepare(int dev);
// the 4x4 Grams of the layer-0 inputs of n_mb minibatches of 4 rows (obs [4 n_mb][obs_dim], cvx0 / cvx1 [4 n_mb][564]) -> tab, sdxpk_input_grams_floats(n_mb) floats
int sdxpk_input_grams(const float* obs, int obs_dim, const float* cvx0, const float* cvx1, int n_mb, float* tab, hipStream_t st);
size_t sdxpk_input_grams_floats(int n_mb);
int sdxpk_update_persistent(const SdxpDev* D, const float* gx0_tab, int total_steps, unsigned* failflag, int stamps, int fault, hipStream_t st);
int sdxpk_fwd_bwd_persistent(const SdxpDev* D, unsigned* failflag, hipStream_t st);
// sdxp_persist_checks.hip
int sdxpk_wave_sums_check(const float* in, float* ref, float* got, int n, hipStream_t st);   // test entry: wave_sums<n> beside n wave_sum trees, n = 12 or 16
int sdxpk_fwd2_sums_check(const float* w, const float* x, float* ref, float* got, hipStream_t st);   // test entry: fwd2_sums beside the twelve trees it replaces
int sdxpk_input_grams_reference(const float* obs, int obs_dim, const float* cvx, int n_mb, float* out, hipStream_t st);   // test entry: the input Grams as the epoch kernel formed them in its x1 shadow
int sdxpk_adam_ahead_check(const float* x1, const float* dy1, const float* dyr, const float* scal, int g, const float* state, float* out, hipStream_t st);   // test entry: adam_l1_ahead beside the serial loops it replaces
int sdxpk_packed_adam_check(const float* x1, const float* dy1, const float* dyr, const float* scal, int g, const float* state, float* out, hipStream_t st);   // test entry: adam_l1_ahead (element pairs, packed f32) beside its one-element form
// sdxp_bigmb.hip.  sdxpk_big_setup lowers the large-minibatch options of `o` to what shapes and device allow, sets the LDS attributes of
// the kernels that stay and lays out the workspace of one minibatch of MB rows in `ws`, every buffer through `alloc`
int sdxpk_big_setup(const SdxpDev* D, int MB, SdxpOpts* o, SdxpAllocFn alloc, void* ctx, SdxpBigWs* ws);
void sdxpk_big_prenorm(const SdxpDev* D, const SdxpBigWs* ws, hipStream_t st);
void sdxpk_big_step(const SdxpDev* D, const SdxpBigWs* ws, int mb, int me, hipStream_t st);
int sdxpk_gemm_nt_launch(int bf, int epi, const NtArgs* gs, int count, int splits, int tile, hipStream_t st);
int sdxpk_gemm_tt_launch(const NtArgs* gs, int count, int splits, const float* zeros, int tile, hipStream_t st);
int sdxpk_gemm_launch(int at, int bt, int epi, int bf, const GemmArgs* gs, int count, int splits, int tile, hipStream_t st);
// sdxp_exbench.hip (the 16-byte words of sdxp_tagged_words.h and the 8-byte words of sdxp_persist_exchange.h, timed bare)
int sdxpk_exchange_bench(void* ll, long long* out, int words, int rounds, int fmt, int src, int pattern, unsigned tag0, hipStream_t st);
int sdxpk_pingpong_bench(void* ll, long long* out, int peer, int rounds, unsigned tag0, hipStream_t st);
}

// The rank-MB kernels are templates on the minibatch size, instantiated for 2, 4 and 8: f(std::integral_constant<int, MB>) for the
// size asked for and 0, or -1 for a size they do not come in
inline bool sdxp_rank_mb(int mb_size) { return mb_size == 2 || mb_size == 4 || mb_size == 8; }
template <typename F>
static int sdxp_for_minibatch(int mb_size, F&& f) {
  switch (mb_size) {
    case 2: f(std::integral_constant<int, 2>()); return 0;
    case 4: f(std::integral_constant<int, 4>()); return 0;
    case 8: f(std::integral_constant<int, 8>()); return 0;
    default: return -1;
  }
}
