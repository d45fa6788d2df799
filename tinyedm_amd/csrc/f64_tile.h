// The fp64 tile engine shared by moments.hip (moments, polynomial-kernel sums) and neighbors_f32.hip (feature-space
// distances): a 64 x 64 tile of dot products on v_mfma_f64_16x16x4_f64, the contraction staged 32 elements at a time in LDS
// as fp64 [32 k][64 m].  See the head of moments.hip for the tiling, the fragment map and the C/D map.
#pragma once
#include "common.h"

namespace {

typedef __attribute__((ext_vector_type(4))) double f64x4;
typedef __attribute__((ext_vector_type(2))) double f64x2;

constexpr int MOM_TILE = 64;                       // results per workgroup tile, both ways
constexpr int MOM_KC = 32;                         // contraction steps staged at a time (8 MFMAs of k = 4)
constexpr int MOM_LD = 80;                         // doubles per staged k row (64 + 16 of padding)

struct Raw16 {   // 16 elements as loaded: 16 bytes of uint8 in q[0], or 16 floats
  u32x4 q[4];
};

// Elements e0 .. e0 + 15 of one row (dtype 0: uint8, 1: float32).  `row` must be readable even when !ok (the callers pass a
// row that exists).  vec: the row is 16-byte aligned and every aligned 16 bytes of it lie wholly inside or outside the row;
// the load is then unconditional (from element 0 when the chunk is outside) and finish16 zeroes it.  Element path: guarded
// loads, zeros elsewhere.
__device__ __forceinline__ Raw16 load16(const unsigned char* __restrict__ row, int dtype, bool vec, int e0, int D, bool ok) {
  Raw16 r;
#pragma unroll
  for (int q = 0; q < 4; ++q) r.q[q] = u32x4{0u, 0u, 0u, 0u};
  if (dtype == 0) {
    if (vec) {
      r.q[0] = *reinterpret_cast<const u32x4*>(row + (ok && e0 < D ? e0 : 0));
    } else if (ok) {
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        uint32_t x = 0;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          const int e = e0 + 4 * w + b;
          if (e < D) x |= (uint32_t)row[e] << (8 * b);
        }
        r.q[0][w] = x;
      }
    }
  } else {
    const float* f = reinterpret_cast<const float*>(row);
    if (vec) {
#pragma unroll
      for (int q = 0; q < 4; ++q) r.q[q] = *reinterpret_cast<const u32x4*>(f + (ok && e0 + 4 * q < D ? e0 + 4 * q : 0));
    } else if (ok) {
#pragma unroll
      for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int w = 0; w < 4; ++w) {
          const int e = e0 + 4 * q + w;
          if (e < D) r.q[q][w] = __float_as_uint(f[e]);
        }
    }
  }
  return r;
}

// element e (0..15, a constant after unrolling) of a Raw16 as fp64; 0 when the row is missing or the element is past D
__device__ __forceinline__ double finish16(const Raw16& r, int dtype, int e, int e0, int D, bool ok) {
  const double u = (double)(int)((r.q[0][e >> 2] >> (8 * (e & 3))) & 0xFFu);
  const double f = (double)__uint_as_float(r.q[e >> 2][e & 3]);
  return ok && e0 + e < D ? (dtype == 0 ? u : f) : 0.0;
}

// acc += A^T B over one staged step: sA, sB fp64 [32 k][MOM_LD], the wave's block at m = wm .. wm + 31, n = wn .. wn + 31
__device__ __forceinline__ void mma_chunk(const double* __restrict__ sA, const double* __restrict__ sB, int wm, int wn,
                                          int lane, f64x4 (&acc)[2][2]) {
  const double* pa = sA + (lane >> 4) * MOM_LD + wm + (lane & 15);
  const double* pb = sB + (lane >> 4) * MOM_LD + wn + (lane & 15);
#pragma unroll
  for (int ks = 0; ks < MOM_KC / 4; ++ks) {
    const double a0 = pa[ks * 4 * MOM_LD], a1 = pa[ks * 4 * MOM_LD + 16];
    const double b0 = pb[ks * 4 * MOM_LD], b1 = pb[ks * 4 * MOM_LD + 16];
    acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
    acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
    acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
    acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
  }
}

}  // namespace
