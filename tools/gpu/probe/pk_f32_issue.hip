// issue cost of packed f32 VALU (v_pk_fma_f32 / v_pk_mul_f32) beside plain v_fma_f32 in a pure VALU stream, at the occupancy of
// k_update_persistent: 256 workgroups x 512 threads, one workgroup per CU (the LDS request sees to that), so two waves per SIMD.
// Every wave brackets LOOPS x BODY instructions of one stream with s_memtime; printed: the median over all waves of elapsed cycles per
// instruction of the wave (both waves of a SIMD run the same stream: the SIMD retires two instructions in that time), and the fastest and
// slowest wave of the last launch.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 tools/gpu/probe/pk_f32_issue.hip -o pk_f32_issue && ./pk_f32_issue
// Break-even for pairing by hand: a packed instruction below twice a plain one.  The Adam streams are the arithmetic of TWO elements of
// adam_l1_ahead (grad4 + adam1x): 28 plain instructions with 2 v_sqrt_f32 and 2 v_rcp_f32 among them, against 16 with the pairs packed.
// Measured (profiles/persist_packed_f32_issue_cost.txt): 7.4 cycles per independent v_fma_f32, 8.8 per v_pk_fma_f32 / v_pk_mul_f32, and the
// packed Adam pair at 0.82 of the plain one.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <vector>
typedef float f2 __attribute__((ext_vector_type(2)));
constexpr int NWG = 256, NTH = 512, LOOPS = 32, LDS_BYTES = 96 * 1024;
enum { FMA_IND, FMA_DEP, PKFMA_IND, PKFMA_DEP, PKMUL_IND, PKMUL_DEP, ADAM_PLAIN, ADAM_PACKED, NKIND };
static const char* const NAMES[NKIND] = {"v_fma_f32 independent (8 chains)", "v_fma_f32 dependent", "v_pk_fma_f32 independent (8 chains)", "v_pk_fma_f32 dependent",
                                         "v_pk_mul_f32 independent (8 chains)", "v_pk_mul_f32 dependent", "Adam element pair, plain (28 instr)", "Adam element pair, packed (16 instr)"};
static const int BODY[NKIND] = {128, 128, 128, 128, 128, 128, 4 * 28, 4 * 16};

// every group is ONE asm statement, so that the compiler puts nothing between the instructions (between dependent asm statements it places
// an s_nop 0 that its own code does not have); behind v_sqrt_f32 / v_rcp_f32 stands the s_nop 0 that hipcc places in front of a direct use
#define I8(OP, T) OP " %0, %8, %9, %0\n\t" OP " %1, %8, %9, %1\n\t" OP " %2, %8, %9, %2\n\t" OP " %3, %8, %9, %3\n\t" \
                  OP " %4, %8, %9, %4\n\t" OP " %5, %8, %9, %5\n\t" OP " %6, %8, %9, %6\n\t" OP " %7, %8, %9, %7" T
#define D8(OP, T) OP " %0, %1, %2, %0\n\t" OP " %0, %1, %2, %0\n\t" OP " %0, %1, %2, %0\n\t" OP " %0, %1, %2, %0\n\t" \
                  OP " %0, %1, %2, %0\n\t" OP " %0, %1, %2, %0\n\t" OP " %0, %1, %2, %0\n\t" OP " %0, %1, %2, %0" T
#define M8(OP) OP " %0, %0, %8\n\t" OP " %1, %1, %8\n\t" OP " %2, %2, %8\n\t" OP " %3, %3, %8\n\t" OP " %4, %4, %8\n\t" OP " %5, %5, %8\n\t" OP " %6, %6, %8\n\t" OP " %7, %7, %8"
#define MD8(OP) OP " %0, %0, %1\n\t" OP " %0, %0, %1\n\t" OP " %0, %0, %1\n\t" OP " %0, %0, %1\n\t" OP " %0, %0, %1\n\t" OP " %0, %0, %1\n\t" OP " %0, %0, %1\n\t" OP " %0, %0, %1"
#define OUT8(x) "+v"(x[0]), "+v"(x[1]), "+v"(x[2]), "+v"(x[3]), "+v"(x[4]), "+v"(x[5]), "+v"(x[6]), "+v"(x[7])
#define R16(X) X; X; X; X; X; X; X; X; X; X; X; X; X; X; X; X

// one element of grad4 + adam1x (14 instructions), every instruction waiting for the one the arithmetic makes it wait for:
// %0 w  %1 m  %2 v  %3 g  %4 t  %5 q  | %6..%9 d  %10..%13 x  %14 0.1  %15 lrb  %16 isq  %17 1e-8
__device__ __forceinline__ void adam_plain1(float& w, float& m, float& v, const float (&d)[4], const float (&x)[4], float c1, float lrb, float isq, float eps) {
  float g, t, q;
  asm volatile(
      "v_mul_f32 %3, %6, %10\n\tv_fma_f32 %3, %7, %11, %3\n\tv_fma_f32 %3, %8, %12, %3\n\tv_fma_f32 %3, %9, %13, %3\n\t"
      "v_mul_f32 %1, 0x3f666666, %1\n\tv_mul_f32 %2, 0x3f7fbe77, %2\n\tv_mul_f32 %4, 0x3a83126f, %3\n\t"
      "v_fma_f32 %1, %14, %3, %1\n\tv_fma_f32 %2, %3, %4, %2\n\tv_mul_f32 %4, %15, %1\n\t"
      "v_sqrt_f32 %5, %2\n\ts_nop 0\n\tv_fma_f32 %5, %16, %5, %17\n\tv_rcp_f32 %5, %5\n\ts_nop 0\n\tv_fma_f32 %0, -%4, %5, %0"
      : "+v"(w), "+v"(m), "+v"(v), "=&v"(g), "=&v"(t), "=&v"(q)
      : "v"(d[0]), "v"(d[1]), "v"(d[2]), "v"(d[3]), "v"(x[0]), "v"(x[1]), "v"(x[2]), "v"(x[3]), "v"(c1), "v"(lrb), "v"(isq), "v"(eps));
}
// the same for a pair of elements (16 instructions): %18 (0.9, 0.9)  %19 (0.999, 0.999)  %20 (0.001, 0.001); v and q stand in fixed
// registers (v[60:61], v[62:63]) so that v_sqrt_f32 / v_rcp_f32 can name their halves
__device__ __forceinline__ void adam_packed1(f2& w, f2& m, f2& v, const f2 (&d)[4], const f2 (&x)[4], f2 c1, f2 lrb, f2 isq, f2 eps, f2 c9, f2 c999, f2 c001) {
  f2 g, t, q;
  asm volatile(
      "v_pk_mul_f32 %3, %6, %10\n\tv_pk_fma_f32 %3, %7, %11, %3\n\tv_pk_fma_f32 %3, %8, %12, %3\n\tv_pk_fma_f32 %3, %9, %13, %3\n\t"
      "v_pk_mul_f32 %1, %18, %1\n\tv_pk_mul_f32 %2, %19, %2\n\tv_pk_mul_f32 %4, %20, %3\n\t"
      "v_pk_fma_f32 %1, %14, %3, %1\n\tv_pk_fma_f32 %2, %3, %4, %2\n\tv_pk_mul_f32 %4, %15, %1\n\t"
      "v_sqrt_f32 v62, v60\n\tv_sqrt_f32 v63, v61\n\ts_nop 0\n\tv_pk_fma_f32 %5, %16, %5, %17\n\t"
      "v_rcp_f32 v62, v62\n\tv_rcp_f32 v63, v63\n\ts_nop 0\n\tv_pk_fma_f32 %0, %4, %5, %0 neg_lo:[1,0,0] neg_hi:[1,0,0]"
      : "+v"(w), "+v"(m), "+{v[60:61]}"(v), "=&v"(g), "=&v"(t), "=&{v[62:63]}"(q)
      : "v"(d[0]), "v"(d[1]), "v"(d[2]), "v"(d[3]), "v"(x[0]), "v"(x[1]), "v"(x[2]), "v"(x[3]), "v"(c1), "v"(lrb), "v"(isq), "v"(eps), "v"(c9), "v"(c999), "v"(c001));
}

template <int KIND>
__global__ __launch_bounds__(NTH) void k_stream(const float* in, unsigned long long* cycles, float* sink) {
  extern __shared__ char lds[];
  const int tid = threadIdx.x;
  if (in[0] == 12345.0f) lds[tid] = 1;   // keeps the LDS request (one workgroup per CU) alive; never taken
  float a[8], b = in[1], c = in[2], eps = in[11];
  f2 a2[8], b2 = {b, b}, c2 = {c, c}, eps2 = {eps, eps};
#pragma unroll
  for (int i = 0; i < 8; ++i) { a[i] = in[3 + i] + tid; a2[i] = f2{a[i], a[i] + 1.0f}; }
  float w[2] = {a[0], a[1]}, m[2] = {a[2], a[3]}, v[2] = {a[4], a[5]}, d[4] = {a[6], a[7], b, c}, x[4] = {a[0], a[2], a[4], a[6]};
  f2 w2 = a2[0], m2 = a2[1], v2 = a2[2], d2[4] = {a2[3], a2[4], a2[5], a2[6]}, x2[4] = {a2[7], a2[0], a2[1], a2[2]};
  const f2 c9 = {0.9f, 0.9f}, c999 = {0.999f, 0.999f}, c001 = {0.001f, 0.001f};
  __syncthreads();
  unsigned long long t0, t1;
  asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t0));
  for (int it = 0; it < LOOPS; ++it) {
    if constexpr (KIND == FMA_IND) { R16(asm volatile(I8("v_fma_f32", "") : OUT8(a) : "v"(b), "v"(c))); }
    if constexpr (KIND == FMA_DEP) { R16(asm volatile(D8("v_fma_f32", "") : "+v"(a[0]) : "v"(b), "v"(c))); }
    if constexpr (KIND == PKFMA_IND) { R16(asm volatile(I8("v_pk_fma_f32", "") : OUT8(a2) : "v"(b2), "v"(c2))); }
    if constexpr (KIND == PKFMA_DEP) { R16(asm volatile(D8("v_pk_fma_f32", "") : "+v"(a2[0]) : "v"(b2), "v"(c2))); }
    if constexpr (KIND == PKMUL_IND) { R16(asm volatile(M8("v_pk_mul_f32") : OUT8(a2) : "v"(b2))); }
    if constexpr (KIND == PKMUL_DEP) { R16(asm volatile(MD8("v_pk_mul_f32") : "+v"(a2[0]) : "v"(b2))); }
    if constexpr (KIND == ADAM_PLAIN) {
#pragma unroll
      for (int r = 0; r < 4; ++r) { adam_plain1(w[0], m[0], v[0], d, x, b, c, b, eps); adam_plain1(w[1], m[1], v[1], d, x, b, c, b, eps); }
    }
    if constexpr (KIND == ADAM_PACKED) {
#pragma unroll
      for (int r = 0; r < 4; ++r) adam_packed1(w2, m2, v2, d2, x2, b2, c2, b2, eps2, c9, c999, c001);
    }
  }
  asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t1));
  float r = w[0] + w[1] + m[0] + m[1] + v[0] + v[1] + w2.x + w2.y + m2.x + m2.y + v2.x + v2.y;
#pragma unroll
  for (int i = 0; i < 8; ++i) r += a[i] + a2[i].x + a2[i].y;
  sink[blockIdx.x * NTH + tid] = r;
  if ((tid & 63) == 0) cycles[blockIdx.x * (NTH / 64) + (tid >> 6)] = t1 - t0;
}

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e_)); return 2; } } while (0)
template <int KIND>
int run(const float* in, unsigned long long* cyc, float* sink) {
  CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(k_stream<KIND>), hipFuncAttributeMaxDynamicSharedMemorySize, LDS_BYTES));
  const int nw = NWG * NTH / 64;
  std::vector<unsigned long long> h(nw);
  double med[3];
  for (int rep = 0; rep < 3; ++rep) {   // the first launch also loads the code object
    hipLaunchKernelGGL(k_stream<KIND>, dim3(NWG), dim3(NTH), LDS_BYTES, 0, in, cyc, sink);
    CHECK(hipGetLastError());
    CHECK(hipDeviceSynchronize());
    CHECK(hipMemcpy(h.data(), cyc, nw * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    std::sort(h.begin(), h.end());
    med[rep] = (double)h[nw / 2] / (LOOPS * BODY[KIND]);
  }
  const double lo = (double)h[0] / (LOOPS * BODY[KIND]), hi = (double)h[nw - 1] / (LOOPS * BODY[KIND]);
  printf("%-40s %6d instr/wave  median cycles/instr %6.2f %6.2f %6.2f  (last launch: min %.2f max %.2f)\n", NAMES[KIND], LOOPS * BODY[KIND], med[0], med[1], med[2], lo, hi);
  return 0;
}
int main() {
  float hin[16] = {0.0f, 0.999f, 1e-3f, 1.0f, 1.5f, 2.0f, 2.5f, 3.0f, 3.5f, 4.0f, 4.5f, 1e-8f};
  float *in, *sink;
  unsigned long long* cyc;
  CHECK(hipMalloc(&in, sizeof hin));
  CHECK(hipMalloc(&sink, NWG * NTH * sizeof(float)));
  CHECK(hipMalloc(&cyc, NWG * (NTH / 64) * sizeof(unsigned long long)));
  CHECK(hipMemcpy(in, hin, sizeof hin, hipMemcpyHostToDevice));
  printf("packed f32 issue cost: %d workgroups x %d threads, two waves per SIMD, s_memtime cycles per instruction of one wave\n", NWG, NTH);
  int rc = run<FMA_IND>(in, cyc, sink) | run<FMA_DEP>(in, cyc, sink) | run<PKFMA_IND>(in, cyc, sink) | run<PKFMA_DEP>(in, cyc, sink) | run<PKMUL_IND>(in, cyc, sink) |
           run<PKMUL_DEP>(in, cyc, sink) | run<ADAM_PLAIN>(in, cyc, sink) | run<ADAM_PACKED>(in, cyc, sink);
  return rc;
}
