// sdxp_persist_lds.h - private to the persistent PPO update (included by sdxp_persist.hip and sdxp_persist_checks.hip only): the shape the kernel is
// built for, its LDS layout, and the names of the slots, columns, regions and thread roles that more than one phase of the kernel refers to
#pragma once
namespace {
// OBS is the LARGEST actor/critic input width (GraspSim, 396); narrower inputs (Orient: 188) run with the tail columns masked off
constexpr int MB = 4, OBS = 396, ST = 564, U0 = 1024, U1 = 512, U2 = 256, ACT = 23;
constexpr int NWG = 256, NTH = 512, NWV = NTH / 64;
constexpr int H0A = OBS / 2, H0V = ST / 2;   // a layer-0 row is split over two waves: 198 / 282 elements each
constexpr int I0A = (H0A + 63) / 64;   // 4 elements per lane of half an actor/critic layer-0 row
constexpr int I0V = (H0V + 63) / 64;   // 5 for half a central-value layer-0 row
constexpr int HR = 4;                  // head rows per wave (25 rows over 8 waves)
constexpr int HPC = (ACT + 2) * U2 / NWG;   // head weights whose Adam state one CU owns (25)
static_assert(HPC * NWG == (ACT + 2) * U2 && U2 == 256, "head ownership split");

// bias / bias_m / bias_v, one thread per slot: the owned rows' biases and their Adam moments.  L0: + net * 4 + row, L1: + net * 2 + row, L2: + net,
// heads: + head row (replicated on every CU).  Threads T_LOGSTD + a run Adam of logstd[a], which lives in the static bank s_b2.
constexpr int BIAS_L0 = 0, BIAS_L1 = 12, BIAS_L2 = 18, BIAS_HEAD = 21, T_LOGSTD = 64;
static_assert(BIAS_L1 == BIAS_L0 + 3 * 4 && BIAS_L2 == BIAS_L1 + 3 * 2 && BIAS_HEAD == BIAS_L2 + 3 && BIAS_HEAD + ACT + 2 <= T_LOGSTD, "bias slots");
enum { SC_AC_GSCALE, SC_CV_GSCALE, SC_AC_LR_BC1, SC_AC_ISQ, SC_CV_LR_BC1, SC_CV_ISQ };   // scal: clip scales (phase A); lr / (1 - b1^t), 1 / sqrt(1 - b2^t) (statistics thread)
enum { STAT_ACTOR = 1, STAT_CRITIC, STAT_BOUNDS, STAT_KL, STAT_CV, STAT_ENTROPY };       // stat[s][.]: per-sample loss statistics
// part past the block sums, stored in the dY1 shadow for the norm at the end of the dY0 shadow: [PART_HEAD_G + net * 16 + a * 4 + b] the heads'
// gradient product that multiplies G_x3[a][b], [PART_HEAD_B + j < 32] |sum_s dmu_s[j]|^2 + dlogstd[j]^2
constexpr int PART_HEAD_G = 128, PART_HEAD_B = 192;
constexpr int DY_L0 = 0, DY_L1 = 4, DY_L2 = 6;   // dyown[net][s][.]: dY of the owned L0 rows 0..3 (per wave), L1 rows 4..5, L2 row 6
// thread windows that recur across phases: + a < 32 logstd / sigma images and dlogstd; + (net, a, b) < 48 the PART_HEAD_G products; + j < 32 the
// PART_HEAD_B terms; the thread of the loss statistics, the learning-rate rule and the Adam bias corrections (wave 6)
constexpr int T_LS = 128, T_HEAD_G = 256, T_HEAD_B = 320, T_STATS = 384;

struct PLds {
  float obs[MB][OBS];        // layer-0 input of actor/critic (dataset rows)
  float cvx[MB][ST];         // layer-0 input of the central value (pre-normalised rows)
  float x1[3][MB][U0];
  float x2[3][MB][U1];
  float x3[3][MB][U2];
  float dy2[3][MB][U2];
  float dy1[3][MB][U1];
  // Gram matrices (MB x MB) of the factors of the minibatch currently held: inputs gx[net][layer 0..3], gradients gd[net][layer 0..2]
  // (round 6: the gradient factors' Grams never leave the reduction that forms them - layer 0's meets G_x0 on the producing CU, layers 1 / 2
  // meet theirs at the end of the dY0 shadow - so only the inputs' Grams and one partial squared norm per network are kept).
  // Layers 1..3 are formed in the step's shadows.  The [layer 0] slice is no longer written or read: the Grams of the dataset rows come
  // from the per-epoch table (k_input_grams) with the rows themselves and land in gx0 below; the slice stays so that every member behind it
  // keeps its offset and the one-minibatch instantiation, which never had these Grams, compiles to the code it had
  float gx[3][4][16];
  float gd2[3][16];          // Gram of dY2 (formed in the dY1 shadow beside the Gram of x3, used at the end of the dY0 shadow)
  float n2rest[4];           // per network: sum over trunk layers 1, 2 of <G_dY, G_x> + their bias terms + the heads' terms (n2h): everything but layer 0
  float part[64 * 4];        // block_sum results; PART_*
  float fpart[3 * MB * NWV];  // cross-wave partial dot products of the forward passes
  float red[4 * NWV][64];    // block_sum: one row per (wave, DPP row)
  float mu[MB][32], dmu[MB][32], z[MB][32], act[MB][32], omu[MB][32], osg[MB][32];
  float val[2][MB], dv[2][MB], gnlp[MB], ls[32], sgm[32], dls[32], stat[MB][8];   // sgm = exp(ls): formed with ls in the x3 shadow (round 6), not three times in the loss phase; stat: STAT_*
  float bias[64], bias_m[64], bias_v[64];   // BIAS_*
  float dyown[3][MB][8];     // DY_*
  float scal[16];            // SC_*
  // control state machine, owned by thread 0 of every CU (every CU runs it on identical inputs, so the copies stay identical)
  struct Ctl {
    double ac_b1, ac_b2, cv_b1, cv_b2;
    float ac_lr, ac_lr_applied, cv_lr, sum_a, sum_c, sum_b, sum_kl, sum_cv, sum_ent, last_kl, ac_gn, cv_gn;
    int ac_t, cv_t;
  } ctl;
  int fail;
  long long tacc[32], tlast;   // phase clock accumulators of CU 0 (SDXP_PERSIST_STAMPS=1)
  // Grams of the layer-0 inputs of the minibatch held, 16-entry form: [0] the observation rows (actor and critic), [1] the central value's
  // normalised rows of this mini-epoch's class.  One 32-lane global_load_lds of load_rows (GX0_*), read by wave 0 at the end of phase E
  float gx0[2][16];
};
// the table k_input_grams writes and load_rows reads: [minibatch][GX0_OBS | GX0_CVX0 | GX0_CVX1][16] floats
constexpr int GX0_OBS = 0, GX0_CVX0 = 16, GX0_CVX1 = 32, GX0_STRIDE = 48;
static_assert(sizeof(PLds) + 512 <= 160 * 1024, "PLds (+ the static logstd bank) must fit the 160 KiB LDS of a gfx950 CU");
}  // namespace
