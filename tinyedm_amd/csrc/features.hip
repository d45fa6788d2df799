// Denoiser activations as features: the spatial mean of an fp32 NHWC map, written into a slice of a feature row.
//
//   out[b, out_offset + c] = (float)((sum_p (double)x[b, p, c]) / (double)HW)
//
// The contract.  Row b of the result has the same bits whatever B is and wherever the row sits in the batch: the sum is
// taken in fp64 in an order that depends on HW alone.  Pixel p belongs to slot p % 32; a slot adds its pixels in
// ascending order; the slots are then added in ascending order.  Neither the channel count, the load path (16-byte
// loads where C % 4 == 0 and x is 16-byte aligned, element loads otherwise) nor the grid enters that order, so the two
// kernel forms below give the same bits for the same column.  No atomics: every output element is one ordinary store.
//
// The shape.  A streaming reduction, bound by HBM.  A workgroup owns 32 channels of one sample (a 128-byte line per
// pixel) and all HW pixels: 32 slots x 8 lanes of four channels, or 32 slots x 32 lanes of one.  The grid is
// (B, ceil(C / 32)), so a single 32x32x192 map still spreads over six workgroups, and B may exceed 65 535 (it rides on
// grid.x).  A thread keeps four pixels' loads in flight; the fp64 adds stay in program order.  The slots meet in 8 KiB of
// LDS and 32 threads finish one channel each.  (k_skip_gate_f32 forms a similar mean in fp32 for its gate MLP, one
// workgroup per sample; that one serves the network and stays as it is.)
#include "common.h"

namespace {

constexpr int POOL_SLOTS = 32;   // pixel p is summed in slot p % POOL_SLOTS
constexpr int POOL_CH = 32;      // channels per workgroup

template <int VEC>
struct PoolVec;
template <>
struct PoolVec<4> {
  typedef f32x4 type;
};
template <>
struct PoolVec<1> {
  typedef float type;
};
__device__ __forceinline__ float pool_elem(const f32x4& v, int e) { return v[e]; }
__device__ __forceinline__ float pool_elem(float v, int) { return v; }

// VEC = 4: 16-byte loads (C % 4 == 0, x 16-byte aligned); VEC = 1: element loads (any C, any alignment)
template <int VEC>
__global__ __launch_bounds__(POOL_SLOTS* POOL_CH / VEC) void k_pool_features(const float* __restrict__ x,
                                                                             float* __restrict__ out, int HW, int C,
                                                                             long out_stride, int out_offset) {
  typedef typename PoolVec<VEC>::type vec_t;
  constexpr int LPR = POOL_CH / VEC;   // lanes per pixel row
  __shared__ double red[POOL_SLOTS][POOL_CH];
  const long b = blockIdx.x;
  const int cl = threadIdx.x % LPR, slot = threadIdx.x / LPR;
  const int c0 = blockIdx.y * POOL_CH + cl * VEC;
  if (c0 < C && slot < HW) {
    const float* xp = x + b * HW * C + c0;
    double a[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) a[e] = 0.0;
    int p = slot;
    for (; p + 3 * POOL_SLOTS < HW; p += 4 * POOL_SLOTS) {   // four loads in flight, the adds in pixel order
      vec_t v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) v[u] = *reinterpret_cast<const vec_t*>(xp + (long)(p + u * POOL_SLOTS) * C);
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int e = 0; e < VEC; ++e) a[e] += (double)pool_elem(v[u], e);
    }
    for (; p < HW; p += POOL_SLOTS) {
      const vec_t v = *reinterpret_cast<const vec_t*>(xp + (long)p * C);
#pragma unroll
      for (int e = 0; e < VEC; ++e) a[e] += (double)pool_elem(v, e);
    }
#pragma unroll
    for (int e = 0; e < VEC; ++e) red[slot][cl * VEC + e] = a[e];
  }
  __syncthreads();
  const int c = blockIdx.y * POOL_CH + threadIdx.x;
  if (threadIdx.x < POOL_CH && c < C) {
    const int nq = HW < POOL_SLOTS ? HW : POOL_SLOTS;   // (slots beyond the last pixel hold nothing)
    double s = red[0][threadIdx.x];
    for (int q = 1; q < nq; ++q) s += red[q][threadIdx.x];
    out[b * out_stride + out_offset + c] = (float)(s / (double)HW);
  }
}

}  // namespace

extern "C" int edm_f32_pool_features(const float* x, float* out, int B, int HW, int C, long out_stride, int out_offset,
                                     hipStream_t st) {
  EDM_REQUIRE(x && out && B > 0 && HW > 0 && C > 0, "f32_pool_features: bad args");
  EDM_REQUIRE(out_offset >= 0 && out_stride >= (long)out_offset + C,
              "f32_pool_features: columns [%d, %ld) do not fit a row of %ld", out_offset, (long)out_offset + C, out_stride);
  const long chunks = ((long)C + POOL_CH - 1) / POOL_CH;
  EDM_REQUIRE(chunks <= 65535, "f32_pool_features: C = %d exceeds %d channels", C, 65535 * POOL_CH);
  const dim3 grid((unsigned)B, (unsigned)chunks);
  if (C % 4 == 0 && (reinterpret_cast<uintptr_t>(x) & 15) == 0)
    hipLaunchKernelGGL(k_pool_features<4>, grid, dim3(POOL_SLOTS * POOL_CH / 4), 0, st, x, out, HW, C, out_stride,
                       out_offset);
  else
    hipLaunchKernelGGL(k_pool_features<1>, grid, dim3(POOL_SLOTS * POOL_CH), 0, st, x, out, HW, C, out_stride, out_offset);
  EDM_CHECK_LAUNCH("f32_pool_features");
  return EDM_OK;
}
