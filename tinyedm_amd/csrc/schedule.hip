// Local step errors of every pair of nodes of a recorded teacher trajectory: the costs of the dynamic-programming search
// for a sampling schedule (Watson et al. 2021; Chen et al. 2024, "GITS").  X fp32 [G+1][B][K] are the states at the nodes
// tau_0 > ... > tau_{G-1} > tau_G = 0 of the teacher's grid, S fp32 [G][B][K] the Euler slopes there.  For i < j, in fp64,
//
//   h = tau[j] - tau[i]
//   order 1, and order 2 when j == G:   e_k = x_ik + h * s_ik - x_jk                 (the Euler jump i -> j)
//   order 2 when j < G:                 e_k = x_ik + (h/2) * (s_ik + s_jk) - x_jk    (the trapezoid along the trajectory)
//   d2[b][i][j] = sum_k e_k^2
//
// evaluated as e = fma(c_j h, s_i + s_j', x_i - x_j) with (c_j, s_j') = (1/2, s_j) for the trapezoid and (1, 0) otherwise:
// the two differences of fp32 values are taken first, in fp64, so the small costs at low sigma keep their digits (no Gram
// identity: |x| is up to 80 sqrt(K), e a small difference).
//
// One workgroup of 256 threads per (sample, TI x TJ tile of pairs).  Thread t owns the quads t, t + 256, ... of the K axis:
// it loads that quad of the tile's TI + TJ rows once, keeps the TI * TJ sums in fp64 registers and adds its quads in
// ascending order, elements in ascending order.  Then the xor butterfly of whole waves and the four wave totals in index
// order (the order of block_partial in quads.h).  The order of a pair's sum is therefore a function of K alone, and its bits
// depend on K, the two nodes' rows, tau[i], tau[j] and order: not on B, G, the place in the tile, the other pairs or the
// load path.  No atomics.
#include "common.h"
#include "quads.h"

namespace {

constexpr int TI = 4, TJ = 8;

template <bool VEC>
__global__ __launch_bounds__(256) void k_pair_step_errors(const float* __restrict__ X, const float* __restrict__ S,
                                                          const double* __restrict__ tau, int B, int G, long K, int order,
                                                          int tiles_j, int tiles, double* __restrict__ d2) {
  __shared__ double red[4][TI * TJ];
  const long bid = blockIdx.x;
  const long b = bid / tiles;
  const int tile = (int)(bid - b * tiles);
  const int i0 = (tile / tiles_j) * TI, j0 = (tile % tiles_j) * TJ;
  double* out = d2 + (b * G) * (long)(G + 1);
  const int tid = threadIdx.x;

  if (j0 + TJ - 1 <= i0) {      // the whole tile lies on or under the diagonal: +0.0 (uniform for the workgroup)
    if (tid < TI * TJ) {
      const int i = i0 + tid / TJ, j = j0 + tid % TJ;
      if (i < G && j <= G) out[(long)i * (G + 1) + j] = 0.0;
    }
    return;
  }

  // rows past the grid are clamped to a valid one: their sums are computed and never written
  const float* xi[TI];
  const float* si[TI];
  const float* xj[TJ];
  const float* sj[TJ];
  double ti[TI], tj[TJ], cj[TJ];
  bool trap[TJ];
#pragma unroll
  for (int a = 0; a < TI; ++a) {
    const int i = i0 + a < G ? i0 + a : G - 1;
    xi[a] = X + ((long)i * B + b) * K;
    si[a] = S + ((long)i * B + b) * K;
    ti[a] = tau[i];
  }
#pragma unroll
  for (int c = 0; c < TJ; ++c) {
    const int j = j0 + c <= G ? j0 + c : G;
    trap[c] = order == 2 && j < G;
    xj[c] = X + ((long)j * B + b) * K;
    sj[c] = S + ((long)(j < G ? j : G - 1) * B + b) * K;     // (S has no row G: not read as a slope, see trap)
    tj[c] = tau[j];
    cj[c] = trap[c] ? 0.5 : 1.0;
  }

  double acc[TI][TJ];
#pragma unroll
  for (int a = 0; a < TI; ++a)
#pragma unroll
    for (int c = 0; c < TJ; ++c) acc[a][c] = 0.0;

  const long nq = (K + 3) / 4;
  for (long q = tid; q < nq; q += 256) {
    const int m = quad_len<VEC>(K, q);
    float xiv[TI][4], siv[TI][4];
#pragma unroll
    for (int a = 0; a < TI; ++a) {
      load4<VEC>(xi[a] + 4 * q, m, xiv[a]);
      load4<VEC>(si[a] + 4 * q, m, siv[a]);
    }
#pragma unroll
    for (int c = 0; c < TJ; ++c) {
      float xjv[4], sjv[4];
      load4<VEC>(xj[c] + 4 * q, m, xjv);
      load4<VEC>(sj[c] + 4 * q, m, sjv);
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (!trap[c]) sjv[k] = 0.f;
#pragma unroll
      for (int a = 0; a < TI; ++a) {
        const double hh = cj[c] * (tj[c] - ti[a]);      // (times 1/2 or 1: exact)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const double e = fma(hh, (double)siv[a][k] + (double)sjv[k], (double)xiv[a][k] - (double)xjv[k]);
          if (k < m) acc[a][c] = fma(e, e, acc[a][c]);
        }
      }
    }
  }

  // every thread arrives here (threads without a quad hold 0): whole-wave butterflies, then the wave totals in index order
#pragma unroll
  for (int a = 0; a < TI; ++a)
#pragma unroll
    for (int c = 0; c < TJ; ++c) {
      const double v = wave_sum_f64(acc[a][c]);
      if ((tid & 63) == 0) red[tid >> 6][a * TJ + c] = v;
    }
  __syncthreads();
  if (tid < TI * TJ) {
    const int i = i0 + tid / TJ, j = j0 + tid % TJ;
    if (i < G && j <= G)
      out[(long)i * (G + 1) + j] = j > i ? ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid] : 0.0;
  }
}

}  // namespace

extern "C" int edm_pair_step_errors(const float* X, const float* S, const double* tau, int B, int G, long K, int order,
                                    double* d2, hipStream_t st) {
  EDM_REQUIRE(X && S && tau && d2 && B > 0 && K > 0, "pair_step_errors: bad args");
  EDM_REQUIRE(G >= 1 && G <= EDM_SCHEDULE_MAX_GRID, "pair_step_errors: G must be in 1 .. %d, got %d", EDM_SCHEDULE_MAX_GRID, G);
  EDM_REQUIRE(order == 1 || order == 2, "pair_step_errors: order must be 1 or 2, got %d", order);
  EDM_REQUIRE((reinterpret_cast<uintptr_t>(tau) & 7) == 0 && (reinterpret_cast<uintptr_t>(d2) & 7) == 0,
              "pair_step_errors: tau and d2 must be 8-byte aligned");
  const int tiles_i = (G + TI - 1) / TI, tiles_j = (G + 1 + TJ - 1) / TJ, tiles = tiles_i * tiles_j;
  const long blocks = (long)B * tiles;
  EDM_REQUIRE(blocks <= 0x7fffffffL, "pair_step_errors: B * tiles = %ld exceeds one grid; split the batch", blocks);
  const dim3 grid((unsigned)blocks), block(256);
  if (K % 4 == 0 && aligned16({X, S}))
    hipLaunchKernelGGL(k_pair_step_errors<true>, grid, block, 0, st, X, S, tau, B, G, K, order, tiles_j, tiles, d2);
  else
    hipLaunchKernelGGL(k_pair_step_errors<false>, grid, block, 0, st, X, S, tau, B, G, K, order, tiles_j, tiles, d2);
  EDM_CHECK_LAUNCH("pair_step_errors");
  return EDM_OK;
}
