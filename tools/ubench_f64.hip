// ubench_f64.hip -- issue rate of the f64 vector instructions the row-distance kernel is made of (rowdist.hip), gfx950.
// Eight independent chains per lane, W waves per SIMD (W x CUs workgroups of 256 threads), no memory traffic.
// Prints, per instruction and W, the wall time, the wave64 instructions per second and SIMD, and the cycles per
// instruction and SIMD by the shader clock the kernel reads itself (s_memtime against the 100 MHz s_memrealtime).
// The rate to read is the wall-clock one.  The last column divides a workgroup's own cycles by W: it understates the cycles
// per instruction whenever fewer than W waves per SIMD are resident at once, and is there for the clock it reports.
// Build: hipcc --offload-arch=gfx950 -O3 -o tools/ubench_f64 tools/ubench_f64.hip ; run on the GPU box.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <vector>

#define CHECK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("HIP error %s at %d\n", hipGetErrorString(e), __LINE__); return 1; } } while (0)

constexpr int ITERS = 1 << 17;  // tens of milliseconds per launch: the start and the tail of a launch do not weigh

#define DECL double a0 = threadIdx.x + seed, a1 = a0 * 3, a2 = a0 * 5, a3 = a0 * 7, a4 = a0 * 11, a5 = a0 * 13, a6 = a0 * 17, a7 = a0 * 19; double k = one
#define REP8(OP) OP(a0) OP(a1) OP(a2) OP(a3) OP(a4) OP(a5) OP(a6) OP(a7)
#define OP_ADD(x) asm volatile("v_add_f64 %0, %0, %1" : "+v"(x) : "v"(k));
#define OP_MUL(x) asm volatile("v_mul_f64 %0, %0, %1" : "+v"(x) : "v"(k));
#define OP_FMA(x) asm volatile("v_fma_f64 %0, %0, %1, %0" : "+v"(x) : "v"(k));
// one step of the kernel's inner loop: d = a - b; sq = d * d; s = s + sq (3 instructions)
#define OP_STEP(x) asm volatile("v_add_f64 %1, %0, -%2\n\tv_mul_f64 %1, %1, %1\n\tv_add_f64 %0, %0, %1" : "+v"(x), "=&v"(t) : "v"(k));

#define KERNEL(name, BODY, PER_ITER)                                                                            \
  __global__ __launch_bounds__(256) void name(double *out, double seed, double one, unsigned long long *stamps) { \
    DECL;                                                                                                       \
    double t = 0;                                                                                               \
    const unsigned long long t0 = __builtin_amdgcn_s_memtime(), r0 = __builtin_amdgcn_s_memrealtime();          \
    for (int it = 0; it < ITERS; ++it) { BODY }                                                                 \
    const unsigned long long t1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();          \
    if (threadIdx.x == 0) { stamps[2 * blockIdx.x] = t1 - t0; stamps[2 * blockIdx.x + 1] = r1 - r0; }           \
    out[blockIdx.x * 256 + threadIdx.x] = a0 + a1 + a2 + a3 + a4 + a5 + a6 + a7 + t;                            \
  }                                                                                                             \
  constexpr int name##_per_iter = PER_ITER;

KERNEL(k_add_f64, REP8(OP_ADD), 8)
KERNEL(k_mul_f64, REP8(OP_MUL), 8)
KERNEL(k_fma_f64, REP8(OP_FMA), 8)
KERNEL(k_step_f64, REP8(OP_STEP), 24)

typedef void (*kernel_t)(double *, double, double, unsigned long long *);

static int run(const char *name, kernel_t kern, int per_iter, int cus, int waves_per_simd, double *d_out, unsigned long long *d_stamps) {
  const int blocks = cus * waves_per_simd;  // a workgroup of 256 threads is one wave per SIMD of a CU
  hipEvent_t e0, e1;
  CHECK(hipEventCreate(&e0));
  CHECK(hipEventCreate(&e1));
  float best = 1e30f;
  for (int rep = 0; rep < 4; ++rep) {  // the first is a warm-up
    CHECK(hipEventRecord(e0));
    hipLaunchKernelGGL(kern, dim3(blocks), dim3(256), 0, 0, d_out, 1.0, 1.0, d_stamps);
    CHECK(hipEventRecord(e1));
    CHECK(hipEventSynchronize(e1));
    float ms = 0;
    CHECK(hipEventElapsedTime(&ms, e0, e1));
    if (rep) best = std::min(best, ms);
  }
  std::vector<unsigned long long> stamps(2 * (size_t)blocks);
  CHECK(hipMemcpy(stamps.data(), d_stamps, stamps.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  std::vector<double> cyc, mhz;
  for (int b = 0; b < blocks; ++b) {
    cyc.push_back((double)stamps[2 * b]);
    mhz.push_back(stamps[2 * b + 1] ? 100.0 * (double)stamps[2 * b] / (double)stamps[2 * b + 1] : 0.0);
  }
  std::sort(cyc.begin(), cyc.end());
  std::sort(mhz.begin(), mhz.end());
  const double instr_per_wave = (double)ITERS * per_iter;
  const double per_simd_per_s = instr_per_wave * waves_per_simd / (best * 1e-3);
  printf("%-12s waves/SIMD %d  best of 3: %8.3f ms  %.3e wave-instr/s/SIMD  median %.2f cycles/instr/SIMD by s_memtime at %.0f MHz\n", name,
         waves_per_simd, best, per_simd_per_s, cyc[cyc.size() / 2] / (instr_per_wave * waves_per_simd), mhz[mhz.size() / 2]);
  CHECK(hipEventDestroy(e0));
  CHECK(hipEventDestroy(e1));
  return 0;
}

int main() {
  hipDeviceProp_t prop;
  CHECK(hipGetDeviceProperties(&prop, 0));
  const int cus = prop.multiProcessorCount;
  printf("%s: %d CUs, clockRate %d kHz\n", prop.name, cus, prop.clockRate);
  double *d_out = nullptr;
  unsigned long long *d_stamps = nullptr;
  CHECK(hipMalloc(&d_out, (size_t)cus * 8 * 256 * sizeof(double)));
  CHECK(hipMalloc(&d_stamps, (size_t)cus * 8 * 2 * sizeof(unsigned long long)));
  for (int w : {1, 2, 4, 8}) {
    if (run("v_add_f64", k_add_f64, k_add_f64_per_iter, cus, w, d_out, d_stamps)) return 1;
    if (run("v_mul_f64", k_mul_f64, k_mul_f64_per_iter, cus, w, d_out, d_stamps)) return 1;
    if (run("v_fma_f64", k_fma_f64, k_fma_f64_per_iter, cus, w, d_out, d_stamps)) return 1;
    if (run("sub,mul,add", k_step_f64, k_step_f64_per_iter, cus, w, d_out, d_stamps)) return 1;
  }
  CHECK(hipFree(d_out));
  CHECK(hipFree(d_stamps));
  return 0;
}
