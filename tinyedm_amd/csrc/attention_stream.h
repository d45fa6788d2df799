// What the streamed-operand attention kernels share (attention_generic.hip: up to 256 tokens, score row in registers;
// attention_long.hip: any number of tokens, tiled softmax): the geometry of a head_dim, the MFMA fragment reads of a 64-row
// LDS tile (row reads for the score products, transposing reads for the accumulator-as-operand products) and the pixel-norm
// backward fused into the gradient stores.
#pragma once
#include "common.h"

namespace {

typedef __attribute__((ext_vector_type(4))) short short4v;
typedef __attribute__((ext_vector_type(8))) short short8v;
typedef short4v __attribute__((address_space(3))) * lds_s4p;

constexpr int TK = 64;  // rows per streamed tile

template <int D>
struct Geo {
  static constexpr int DT = D / 16;         // k-steps of the score contraction
  static constexpr int DB = (D + 31) / 32;  // 32-row blocks of the O^T / dQ^T / dK^T / dV^T accumulators
  static constexpr int DP = DB * 32;        // padded dims of an LDS image row
  static constexpr int RS = DP * 2 + 16;    // padded LDS row bytes
};

__device__ __forceinline__ bf16x8 tr_frag_g(const char* p0, const char* p1) {
  short4v a = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4p)(p0));
  short4v b = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4p)(p1));
  short8v c = __builtin_shufflevector(a, b, 0, 1, 2, 3, 4, 5, 6, 7);
  return __builtin_bit_cast(bf16x8, c);
}
__device__ __forceinline__ bf16x8 pack8_g(const f32x16& x, int s2) {
  bf16x8 o;
#pragma unroll
  for (int j = 0; j < 8; ++j) o[j] = (bf16)x[8 * s2 + j];
  return o;
}
__device__ __forceinline__ const bf16x8& ld128_g(const char* p) { return *reinterpret_cast<const bf16x8*>(p); }

template <int D>
__device__ __forceinline__ f32x16 score_tile_g(const char* a_rows, const bf16x8 (&b)[Geo<D>::DT]) {
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
  for (int s = 0; s < Geo<D>::DT; ++s)
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ld128_g(a_rows + s * 32), b[s], acc, 0, 0, 0);
  return acc;
}

// dx = (g - xn*<g,xn>*d/(D*(d-eps)))/d for one token per lane; g in O^T-style accumulators, xn re-derived from the raw row
template <int D>
__device__ __forceinline__ void norm_bwd_store_g(f32x16 (&g)[Geo<D>::DB], const bf16* __restrict__ raw, float dn,
                                                 bf16* __restrict__ dst, int lhi, bool valid) {
  using G = Geo<D>;
  const float inv = 1.0f / dn;
  float dot = 0.f;
  if (valid) {
#pragma unroll
    for (int dt = 0; dt < G::DB; ++dt)
#pragma unroll
      for (int gq = 0; gq < 4; ++gq) {
        const int d0 = dt * 32 + 8 * gq + 4 * lhi;
        if (d0 < D) {
          bf16x4 v = *reinterpret_cast<const bf16x4*>(raw + d0);
#pragma unroll
          for (int r = 0; r < 4; ++r) dot += g[dt][4 * gq + r] * (float)(bf16)((float)v[r] * inv);
        }
      }
  }
  dot += __shfl_xor(dot, 32, 64);
  const float s = dn - NORM_EPS;
  const float coef = s > 0.f ? dot * dn / ((float)D * s) : 0.f;
  if (valid) {
#pragma unroll
    for (int dt = 0; dt < G::DB; ++dt)
#pragma unroll
      for (int gq = 0; gq < 4; ++gq) {
        const int d0 = dt * 32 + 8 * gq + 4 * lhi;
        if (d0 < D) {
          bf16x4 v = *reinterpret_cast<const bf16x4*>(raw + d0);
          bf16x4 o;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float xn = (float)(bf16)((float)v[r] * inv);
            o[r] = (bf16)((g[dt][4 * gq + r] - xn * coef) * inv);
          }
          *reinterpret_cast<bf16x4*>(dst + d0) = o;
        }
      }
  }
}

}  // namespace
