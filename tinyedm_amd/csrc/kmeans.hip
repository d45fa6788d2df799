// Feature clustering: per-cluster column sums of gathered float32 rows in fp64 -- the update half of a Lloyd iteration
// (the assignment half is the k = 1 case of csrc/neighbors_f32.hip).
//
//   sums[k][d] = sum over the rows r of cluster k of (double)x[r][d]          d2sums[k] = sum over the same rows of d2[r]
//
// The contract (include/tinyedm_hip.h).  The rows of cluster k are listed in ascending row number; the row at position p
// of that list belongs to chunk p / EDM_CLUSTER_BLOCK.  A chunk's partial starts at +0.0 and adds its rows one at a time in
// ascending position; the cluster's sum starts at +0.0 and adds its chunks' partials one at a time in ascending chunk
// number.  Every output element (and d2sums) follows that one sequence, so its bits are a function of the member list
// alone: K, n, the other clusters, the grid, the rows in flight and the load path (16-byte loads where D % 4 == 0 and x is
// 16-byte aligned, element loads otherwise) do not enter.  No atomics: every output element is one ordinary store.
//
// The shape.  A gather of whole rows, bound by HBM.  One wave owns one chunk and 256 columns of it (64 lanes x four
// columns: one 1-KiB wave load per row), keeps CLUSTER_ROWS rows' loads in flight and adds them in program order.  A
// cluster of half the set is cut into chunks like any other, so no wave carries more than EDM_CLUSTER_BLOCK rows.  The
// second pass gives CLUSTER_FINISH_COLS columns of a cluster to a workgroup, one column per thread, and walks the cluster's
// chunk partials with CLUSTER_FINISH_LOADS loads in flight.  That walk is what a cluster of half the set costs: one wave
// per 64 columns reads all of the cluster's partials (measured: 15 us for 391 chunks at D = 256 against 4 us balanced;
// neither more loads in flight nor another column width changed it -- DESIGN.md, "Feature clustering").
// The workspace is (chunks) x (D + 1) doubles with chunks <= n / EDM_CLUSTER_BLOCK + K; nothing of size n x D exists.
#include "common.h"
#include "../../include/tinyedm_hip.h"   // EDM_CLUSTER_BLOCK

namespace {

constexpr int CLUSTER_COLS = 256;   // columns per wave of the partial pass
#ifndef CLUSTER_ROWS
#define CLUSTER_ROWS 8              // rows in flight per wave (how it was chosen: DESIGN.md, "Feature clustering")
#endif
#ifndef CLUSTER_FINISH_LOADS
#define CLUSTER_FINISH_LOADS 16     // chunk partials in flight per thread of the finish pass
#endif
#ifndef CLUSTER_FINISH_COLS
#define CLUSTER_FINISH_COLS 64      // columns (threads) per workgroup of the finish pass
#endif
constexpr long CLUSTER_MAX_N = (1L << 31) - 64;
constexpr int CLUSTER_MAX_D = 32768;
constexpr int CLUSTER_MAX_K = 1 << 20;

// the four columns of lane `lane` in a 256-column block: VEC = 4 (16-byte loads) 4 lane .. 4 lane + 3; VEC = 1 (element
// loads, coalesced) lane, lane + 64, lane + 128, lane + 192
template <int VEC>
__device__ __forceinline__ int cluster_col(int lane, int e) {
  return VEC == 4 ? 4 * lane + e : lane + 64 * e;
}

template <int VEC>
__device__ __forceinline__ f32x4 cluster_load(const float* __restrict__ row, int c0, int lane, int D) {
  if (VEC == 4) {
    const int c = c0 + 4 * lane;
    return c < D ? *reinterpret_cast<const f32x4*>(row + c) : f32x4{0.f, 0.f, 0.f, 0.f};
  }
  f32x4 v;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int c = c0 + lane + 64 * e;
    v[e] = c < D ? row[c] : 0.f;
  }
  return v;
}

// grid (chunks, ceil(D / 256)), one wave each
template <int VEC>
__global__ __launch_bounds__(64) void k_cluster_partial(const float* __restrict__ x, const int* __restrict__ members,
                                                        const int* __restrict__ starts,
                                                        const int* __restrict__ chunk_first,
                                                        const int* __restrict__ chunk_cluster,
                                                        const double* __restrict__ d2, int D,
                                                        double* __restrict__ partial, double* __restrict__ partial_d2) {
  const int chunk = blockIdx.x, lane = threadIdx.x;
  const int c0 = blockIdx.y * CLUSTER_COLS;
  const int k = chunk_cluster[chunk];
  const int lo = starts[k] + (chunk - chunk_first[k]) * EDM_CLUSTER_BLOCK;
  const int end = starts[k + 1];
  const int cnt = end - lo < EDM_CLUSTER_BLOCK ? end - lo : EDM_CLUSTER_BLOCK;
  const int* __restrict__ m = members + lo;
  const bool with_d2 = d2 != nullptr && blockIdx.y == 0;

  double a[4] = {0.0, 0.0, 0.0, 0.0}, ad = 0.0;
  int j = 0;
  for (; j + CLUSTER_ROWS <= cnt; j += CLUSTER_ROWS) {   // CLUSTER_ROWS rows in flight, the adds in list order
    f32x4 v[CLUSTER_ROWS];
    double dd[CLUSTER_ROWS];
#pragma unroll
    for (int u = 0; u < CLUSTER_ROWS; ++u) {
      const long r = m[j + u];
      v[u] = cluster_load<VEC>(x + r * D, c0, lane, D);
      dd[u] = with_d2 ? d2[r] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < CLUSTER_ROWS; ++u) {
#pragma unroll
      for (int e = 0; e < 4; ++e) a[e] += (double)v[u][e];
      ad += dd[u];
    }
  }
  for (; j < cnt; ++j) {
    const long r = m[j];
    const f32x4 v = cluster_load<VEC>(x + r * D, c0, lane, D);
    const double dd = with_d2 ? d2[r] : 0.0;
#pragma unroll
    for (int e = 0; e < 4; ++e) a[e] += (double)v[e];
    ad += dd;
  }

  double* __restrict__ p = partial + (long)chunk * D;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int c = c0 + cluster_col<VEC>(lane, e);
    if (c < D) p[c] = a[e];
  }
  if (with_d2 && lane == 0) partial_d2[chunk] = ad;
}

// ((+0.0 + p[lo * stride]) + p[(lo + 1) * stride]) + ... + p[(hi - 1) * stride]: the loads in flight, the adds in order
__device__ __forceinline__ double cluster_chain(const double* __restrict__ p, long stride, int lo, int hi) {
  double s = 0.0;
  int q = lo;
  for (; q + CLUSTER_FINISH_LOADS <= hi; q += CLUSTER_FINISH_LOADS) {
    double v[CLUSTER_FINISH_LOADS];
#pragma unroll
    for (int u = 0; u < CLUSTER_FINISH_LOADS; ++u) v[u] = p[(q + u) * stride];
#pragma unroll
    for (int u = 0; u < CLUSTER_FINISH_LOADS; ++u) s += v[u];
  }
  for (; q + 4 <= hi; q += 4) {
    double v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) v[u] = p[(q + u) * stride];
#pragma unroll
    for (int u = 0; u < 4; ++u) s += v[u];
  }
  for (; q < hi; ++q) s += p[q * stride];
  return s;
}

// grid (K, ceil(D / CLUSTER_FINISH_COLS) [+ 1 with d2]): thread t adds column CLUSTER_FINISH_COLS blockIdx.y + t of the
// cluster's chunk partials in chunk order; the grid row past the last column block adds the chunks' distance partials
__global__ __launch_bounds__(CLUSTER_FINISH_COLS) void k_cluster_finish(const double* __restrict__ partial,
                                                                 const double* __restrict__ partial_d2,
                                                                 const int* __restrict__ chunk_first, int D, int col_blocks,
                                                                 double* __restrict__ sums, double* __restrict__ d2sums) {
  const int k = blockIdx.x;
  const int lo = chunk_first[k], hi = chunk_first[k + 1];
  if ((int)blockIdx.y == col_blocks) {
    if (threadIdx.x == 0) d2sums[k] = cluster_chain(partial_d2, 1, lo, hi);
    return;
  }
  const int c = blockIdx.y * CLUSTER_FINISH_COLS + threadIdx.x;
  if (c < D) sums[(long)k * D + c] = cluster_chain(partial + c, D, lo, hi);
}

}  // namespace

// EDM_CLUSTER_BLOCK as this library was built: the chunk tables handed to edm_f32_cluster_sums_partial must be cut with it
// (host logic only)
extern "C" int edm_cluster_block(void) { return EDM_CLUSTER_BLOCK; }

// Chunk partials.  x float32 [n][D] row-contiguous (4-byte aligned); members int32 [n]: the rows of cluster 0 in ascending
// row number, then those of cluster 1, ...; starts int32 [K + 1]: cluster k owns members[starts[k] .. starts[k + 1]);
// chunk_first int32 [K + 1]: cluster k owns the chunks chunk_first[k] .. chunk_first[k + 1], ceil(members / EDM_CLUSTER_BLOCK)
// of them; chunk_cluster int32 [n_chunks]: the cluster of each chunk; d2 fp64 [n] or null.  Writes partial fp64 [n_chunks][D]
// and, with d2, partial_d2 fp64 [n_chunks].  The tables are the caller's: every member must be a row number in [0, n).
extern "C" int edm_f32_cluster_sums_partial(const void* x, const int* members, const int* starts, const int* chunk_first,
                                            const int* chunk_cluster, const double* d2, long n, int D, int K, long n_chunks,
                                            double* partial, double* partial_d2, hipStream_t st) {
  EDM_REQUIRE(x && members && starts && chunk_first && chunk_cluster && partial, "f32_cluster_sums_partial: null pointer");
  EDM_REQUIRE(d2 == nullptr || partial_d2 != nullptr, "f32_cluster_sums_partial: d2 needs partial_d2");
  EDM_REQUIRE(n >= 1 && n <= CLUSTER_MAX_N, "f32_cluster_sums_partial: n must be in [1, 2^31 - 64], got %ld", n);
  EDM_REQUIRE(D >= 1 && D <= CLUSTER_MAX_D, "f32_cluster_sums_partial: D must be in [1, %d], got %d", CLUSTER_MAX_D, D);
  EDM_REQUIRE(K >= 1 && K <= CLUSTER_MAX_K, "f32_cluster_sums_partial: K must be in [1, %d], got %d", CLUSTER_MAX_K, K);
  EDM_REQUIRE(n_chunks >= 1 && n_chunks <= n / EDM_CLUSTER_BLOCK + K,
              "f32_cluster_sums_partial: n_chunks must be in [1, n / %d + K], got %ld", EDM_CLUSTER_BLOCK, n_chunks);
  const dim3 grid((unsigned)n_chunks, (unsigned)((D + CLUSTER_COLS - 1) / CLUSTER_COLS));
  if (D % 4 == 0 && (reinterpret_cast<uintptr_t>(x) & 15) == 0)
    hipLaunchKernelGGL(k_cluster_partial<4>, grid, dim3(64), 0, st, (const float*)x, members, starts, chunk_first,
                       chunk_cluster, d2, D, partial, partial_d2);
  else
    hipLaunchKernelGGL(k_cluster_partial<1>, grid, dim3(64), 0, st, (const float*)x, members, starts, chunk_first,
                       chunk_cluster, d2, D, partial, partial_d2);
  EDM_CHECK_LAUNCH("f32_cluster_sums_partial");
  return EDM_OK;
}

// sums fp64 [K][D] (and d2sums fp64 [K] when partial_d2 and d2sums are given) from the chunk partials, every element
// WRITTEN: a cluster without chunks gets +0.0.
extern "C" int edm_f32_cluster_sums_finish(const double* partial, const double* partial_d2, const int* chunk_first, int D,
                                           int K, double* sums, double* d2sums, hipStream_t st) {
  EDM_REQUIRE(partial && chunk_first && sums, "f32_cluster_sums_finish: null pointer");
  EDM_REQUIRE((partial_d2 == nullptr) == (d2sums == nullptr), "f32_cluster_sums_finish: partial_d2 and d2sums go together");
  EDM_REQUIRE(D >= 1 && D <= CLUSTER_MAX_D, "f32_cluster_sums_finish: D must be in [1, %d], got %d", CLUSTER_MAX_D, D);
  EDM_REQUIRE(K >= 1 && K <= CLUSTER_MAX_K, "f32_cluster_sums_finish: K must be in [1, %d], got %d", CLUSTER_MAX_K, K);
  const int col_blocks = (D + CLUSTER_FINISH_COLS - 1) / CLUSTER_FINISH_COLS;
  const dim3 grid((unsigned)K, (unsigned)(col_blocks + (d2sums ? 1 : 0)));
  hipLaunchKernelGGL(k_cluster_finish, grid, dim3(CLUSTER_FINISH_COLS), 0, st, partial, partial_d2, chunk_first, D,
                     col_blocks, sums, d2sums);
  EDM_CHECK_LAUNCH("f32_cluster_sums_finish");
  return EDM_OK;
}
