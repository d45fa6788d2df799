// Diagnostic: what does the fp64 matrix instruction sustain on this device?  A bare loop of v_mfma_f64_16x16x4_f64 over a
// tile that stays resident in LDS, every operand re-read from LDS by ds_read_b64 exactly as csrc/moments.hip reads it
// (fp64 [32 k][80], 2 x 2 accumulator blocks per wave, 2 + 2 fragment reads per 4 MFMAs), 4 waves per workgroup, WG
// workgroups per CU; no global loads, no staging, no barriers inside the loop.  Prints one JSON line with the TFLOP/s.
// tools/fd_rate.py quotes the kernels of csrc/moments.hip against this number, not against a data-sheet peak.
//   hipcc --offload-arch=gfx950 -O3 -o mfma_f64 mfma_f64.hip && ./mfma_f64 [iters] [workgroups per CU]
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <vector>

typedef __attribute__((ext_vector_type(4))) double f64x4;
constexpr int KC = 32, LD = 80;

__global__ __launch_bounds__(256) void k(const double* __restrict__ src, double* __restrict__ out, int iters) {
  __shared__ double sA[KC * LD];
  __shared__ double sB[KC * LD];
  for (int i = threadIdx.x; i < KC * LD; i += blockDim.x) {
    sA[i] = src[i];
    sB[i] = src[KC * LD + i];
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const double* pa = sA + (lane >> 4) * LD + (wave >> 1) * 32 + (lane & 15);
  const double* pb = sB + (lane >> 4) * LD + (wave & 1) * 32 + (lane & 15);
  f64x4 acc[2][2];
  for (int i = 0; i < 2; ++i)
    for (int j = 0; j < 2; ++j) acc[i][j] = f64x4{0.0, 0.0, 0.0, 0.0};
  for (int it = 0; it < iters; ++it) {
#pragma unroll
    for (int ks = 0; ks < KC / 4; ++ks) {
      const double a0 = pa[ks * 4 * LD], a1 = pa[ks * 4 * LD + 16];
      const double b0 = pb[ks * 4 * LD], b1 = pb[ks * 4 * LD + 16];
      acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
    }
    asm volatile("" ::: "memory");   // the operands are read again every pass
  }
  double s = 0.0;
  for (int i = 0; i < 2; ++i)
    for (int j = 0; j < 2; ++j)
      for (int r = 0; r < 4; ++r) s += acc[i][j][r];
  out[(size_t)blockIdx.x * blockDim.x + threadIdx.x] = s;
}

#define CK(x)                                                                   \
  do {                                                                          \
    hipError_t e_ = (x);                                                        \
    if (e_ != hipSuccess) {                                                     \
      fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_));                   \
      return 1;                                                                 \
    }                                                                           \
  } while (0)

int main(int argc, char** argv) {
  const int iters = argc > 1 ? atoi(argv[1]) : 20000;
  const int per_cu = argc > 2 ? atoi(argv[2]) : 2;
  if (iters < 1 || per_cu < 1 || per_cu > 3) {
    fprintf(stderr, "usage: mfma_f64 [iters >= 1] [workgroups per CU, 1..3]\n");
    return 1;
  }
  hipDeviceProp_t prop;
  CK(hipGetDeviceProperties(&prop, 0));
  const int grid = prop.multiProcessorCount * per_cu;
  std::vector<double> h(2 * KC * LD);
  for (size_t i = 0; i < h.size(); ++i) h[i] = (double)((i * 2654435761u) % 17) - 8.0;
  double *src, *out;
  CK(hipMalloc(&src, h.size() * sizeof(double)));
  CK(hipMalloc(&out, (size_t)grid * 256 * sizeof(double)));
  CK(hipMemcpy(src, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice));
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0));
  CK(hipEventCreate(&e1));
  hipLaunchKernelGGL(k, dim3(grid), dim3(256), 0, 0, src, out, iters / 10 + 1);   // warm-up
  CK(hipDeviceSynchronize());
  float best = 1e30f;
  for (int rep = 0; rep < 3; ++rep) {
    CK(hipEventRecord(e0, 0));
    hipLaunchKernelGGL(k, dim3(grid), dim3(256), 0, 0, src, out, iters);
    CK(hipEventRecord(e1, 0));
    CK(hipEventSynchronize(e1));
    float ms = 0.f;
    CK(hipEventElapsedTime(&ms, e0, e1));
    if (ms < best) best = ms;
  }
  const double flops = (double)grid * 4 /*waves*/ * iters * (KC / 4) * 4 /*MFMAs*/ * (2.0 * 16 * 16 * 4);
  printf("{\"instruction\": \"v_mfma_f64_16x16x4_f64\", \"cus\": %d, \"workgroups_per_cu\": %d, \"iters\": %d, \"ms\": %.3f, "
         "\"tflops\": %.2f}\n", prop.multiProcessorCount, per_cu, iters, best, flops / (best * 1e-3) / 1e12);
  CK(hipFree(src));
  CK(hipFree(out));
  return 0;
}
