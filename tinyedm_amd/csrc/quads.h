// The toolkit of the per-sample fp32 kernels around the network (solver steps, likelihood, noise-level evaluation, the
// adaptive and the parallel solver, restoration, the gradient guard): ONE definition each of the quad load / store, the
// order-fixed fp64 reduction, the chunk rule that sizes its workspace, the launch helpers, the non-finite check, and the
// Heun step expressions whose bits several kernels promise to share.  Included after common.h.
#pragma once
#include "common.h"
#include "../../include/tinyedm_hip.h"      // EDM_NLL_MAX_CHUNKS

#include <initializer_list>

// ------------------------------------------------------------------ host side of a launch
// (grid_for sits in common.h: the bf16 elementwise kernels use it too)
// a null pointer counts as aligned
inline bool aligned16(std::initializer_list<const void*> ps) {
  for (const void* p : ps)
    if (reinterpret_cast<uintptr_t>(p) & 15) return false;
  return true;
}
// The chunk rule: how many workgroups of 256 quads share a sample of CHW elements, and with it how many entries of a row
// of `part` (EDM_NLL_MAX_CHUNKS doubles) the order-fixed reduction fills.  A function of CHW alone; edm_sample_chunks is
// this value for the Python side, which sizes the workspaces with it.
inline int sample_chunks(long CHW) {
  const long c = ((CHW + 3) / 4 + 255) / 256;
  return (int)(c < EDM_NLL_MAX_CHUNKS ? c : EDM_NLL_MAX_CHUNKS);
}

// ------------------------------------------------------------------ quads of a sample
// VEC: CHW % 4 == 0 and every operand 16-byte aligned -> one dwordx4 per quad; otherwise the same quads element by
// element, the last quad of a sample holding m = quad_len < 4 elements (loads pad with 0, stores skip the padding).
template <bool VEC>
__device__ __forceinline__ int quad_len(long CHW, long q) {
  return VEC ? 4 : (int)(CHW - 4 * q < 4 ? CHW - 4 * q : 4);
}
template <bool VEC>
__device__ __forceinline__ void load4(const float* __restrict__ p, int m, float (&v)[4]) {
  if (VEC) {
    const f32x4 t = *reinterpret_cast<const f32x4*>(p);
    v[0] = t[0]; v[1] = t[1]; v[2] = t[2]; v[3] = t[3];
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = k < m ? p[k] : 0.f;
  }
}
template <bool VEC>
__device__ __forceinline__ void store4(float* __restrict__ p, int m, const float (&v)[4]) {
  if (VEC) {
    *reinterpret_cast<f32x4*>(p) = f32x4{v[0], v[1], v[2], v[3]};
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (k < m) p[k] = v[k];
  }
}

// ------------------------------------------------------------------ the order-fixed fp64 sum of a sample
// Workgroup (chunk, b) sums its quads of sample b thread-serially, then the xor butterfly of whole waves, then the four
// wave totals in index order into part[b][chunk]; chunk_sum adds a sample's chunks in index order.  No atomics on
// floating point, no dependence on arrival order, and a chunking that depends on CHW alone.
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
// EVERY thread of the 256-thread workgroup calls this, after its loop and outside any divergent branch (threads without
// a quad pass 0): the butterfly then never reads an inactive lane
__device__ __forceinline__ void block_partial(double v, double* __restrict__ slot) {
  __shared__ double red[4];
  v = wave_sum_f64(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) *slot = ((red[0] + red[1]) + red[2]) + red[3];
}
__device__ __forceinline__ double chunk_sum(const double* __restrict__ row, int chunks) {
  double s = 0.0;
  for (int c = 0; c < chunks; ++c) s += row[c];
  return s;
}

// ------------------------------------------------------------------ the health word
// NaN, or beyond 3e38
__device__ __forceinline__ bool nonfinite(float v) { return !(fabsf(v) <= 3.0e38f); }
// One atomicOr per wave that saw a bad value.  health is nullable; every lane of the wave runs this, outside any divergent
// branch.  bits 2u: a non-finite sampler state; 1u: the optimizer's.  A macro, not a function: written as a function the
// compiler carries `bad` differently through the callers' loops (k_dpm_multistep: 27 more instructions per kernel).
#define EDM_RAISE_HEALTH(health, bad, bits)                                               \
  do {                                                                                    \
    if ((health) && __any(bad) && (threadIdx.x & 63) == 0) atomicOr((health), (bits));    \
  } while (0)

// ------------------------------------------------------------------ the Heun step, written once
// edm_heun_euler / edm_heun_correct, their guided, _div, per-sample (adaptive) and windowed (picard) forms all evaluate
// these functions, so the bit-equality they promise one another holds by construction.
// D = Dg + w*(Dm - Dg); w == 0 gives exactly Dg
__device__ __forceinline__ float guidance_mix(float w, float Dm, float Dg) { return fmaf(w, Dm - Dg, Dg); }
// the update x + (t1 - t0) * slope, one fma
__device__ __forceinline__ float heun_update(float x, float slope, float t0, float t1) { return fmaf(t1 - t0, slope, x); }
// Euler stage: dx = (x - D) / t0, returns x1 = x + (t1 - t0) * dx
__device__ __forceinline__ float heun_euler_stage(float x, float D, float t0, float t1, float& dx) {
  dx = (x - D) / t0;
  return heun_update(x, dx, t0, t1);
}
// corrector slope: the mean of dx and dx' = (x1 - D1) / t1
__device__ __forceinline__ float heun_slope(float dx, float x1, float D1, float t1) {
  const float dp = (x1 - D1) / t1;
  return 0.5f * dx + 0.5f * dp;
}
