// Two fp64 reductions over a resident set of rows, for the Frechet distance and the kernel inception distance of sample sets
// (tinyedm_amd/frechet.py): the moments s = sum_i x_i and G = sum_i x_i x_i^T of an [N, D] set, and the polynomial-kernel
// sums sum_ij (gamma x_i . y_j + coef0)^degree between two index lists of rows.  Both run on v_mfma_f64_16x16x4_f64.
//
// Why fp64 for both input types.  A uint8 product is at most 65025 and every sum here stays far below 2^53, so the
// moments and every dot product of uint8 rows are exact integers in fp64 whatever the summation order: the result is unique
// and tested bit for bit.  A float32 product has 24 + 24 significant bits and is exact in fp64 too; only the sums round, in
// an order that is fixed by the tiling and the split count, so two runs give the same bits.  Rows are converted to fp64 as
// they are written to LDS; nobody materialises an fp64 copy of the set.
//
// One tile engine, two loaders.  A workgroup of 256 threads (4 waves as 2 x 2) owns a 64 x 64 tile of results; a wave a
// 32 x 32 block of it as 2 x 2 accumulators (32 VGPRs).  Per step both operand tiles are staged in LDS as fp64 [32 k][64 m]
// (row stride 80 doubles: the four k rows of a fragment read fall on the two halves of the banks) and the wave issues
// 8 k = 4 steps of 2 + 2 fragment reads and 4 MFMAs (mma_chunk).  Fragments: lane l holds A[m = l & 15][k = l >> 4] and
// B[k = l >> 4][n = l & 15], one fp64 each, i.e. the same LDS address pattern for both operands.  The C/D map of the f64
// MFMA is NOT the dtype-independent 16x16 map: col = l & 15, row = (l >> 4) + 4 reg.
//   moments: k walks the rows of the set (split over blockIdx.y), m the 64 columns of the tile's column block; a thread
//            stages 4 consecutive columns of four rows (a dword of uint8, 16 bytes of float32) as 4 consecutive doubles.
//            Only the tiles on and above the diagonal are computed; a diagonal tile stages one operand and also sums its
//            columns (from LDS, in a fixed order).
//   sums:    k walks the D elements of a row, m the 64 gathered rows of a subset's row block; a thread stages 16
//            consecutive elements of one row as a column of the staged tile (consecutive lanes, consecutive m).
// The raw bits of step t + 1 are loaded before the MFMAs of step t and converted when they are written to LDS.  Missing
// rows and elements past D are ZERO operands (selected, never multiplied away) and the stores are masked.  Aligned
// vector loads run when the base is 16-byte aligned and a row is a whole number of them (moments: D % 4 == 0; sums:
// D % 16 == 0 for uint8, D % 4 == 0 for float32), element loads otherwise, with the same results.  No atomics of any
// kind: every partial leaves by an ordinary store and the finish kernels add the partials in index order.
#include "common.h"
#include "f64_tile.h"   // Raw16, load16, finish16, mma_chunk and the tile constants, shared with neighbors_f32.hip

namespace {

constexpr int MOM_MAX_D = 32768;
constexpr int MOM_MAX_SPLITS = 1024;
constexpr long MOM_PARTIAL_BYTES = 256L << 20;     // edm_moments_splits keeps the gram partials below this
constexpr long POLY_MAX_M = 65535L * MOM_TILE;     // one grid row / column per 64 rows of a subset
constexpr int POLY_MAX_S = 65535;
constexpr int POLY_MAX_D = 1 << 24;

// The moments' loader: elements e0 .. e0 + 3 of one row as raw bits (uint8: the four bytes in r[0]; float32: r[0..3]).  vec: the
// base is 16-byte aligned and D % 4 == 0, so the four elements are one aligned load, wholly inside or outside the row.
__device__ __forceinline__ u32x4 load4(const unsigned char* __restrict__ row, int dtype, bool vec, int e0, int D, bool ok) {
  u32x4 r = {0u, 0u, 0u, 0u};
  if (vec) {
    const int e = ok && e0 < D ? e0 : 0;
    if (dtype == 0)
      r[0] = *reinterpret_cast<const uint32_t*>(row + e);
    else
      r = *reinterpret_cast<const u32x4*>(row + 4 * (long)e);
  } else if (ok) {
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const int e = e0 + w;
      if (e < D) {
        if (dtype == 0)
          r[0] |= (uint32_t)row[e] << (8 * w);
        else
          r[w] = __float_as_uint(reinterpret_cast<const float*>(row)[e]);
      }
    }
  }
  return r;
}
__device__ __forceinline__ double finish4(const u32x4& r, int dtype, int w, int e0, int D, bool ok) {
  const double u = (double)(int)((r[0] >> (8 * w)) & 0xFFu);
  const double f = (double)__uint_as_float(r[w]);
  return ok && e0 + w < D ? (dtype == 0 ? u : f) : 0.0;
}

// ---------------------------------------------------------------------------------------------------------- moments
// psum[s][d] = sum over the rows of share s of (x[d] - shift[d]); pgram[s][i][j] the same for the products, written for
// the 64 x 64 tiles with tile(i) <= tile(j) only.  blockIdx.x: the tile, row-major over the upper triangle (sums_only: the
// diagonal tile blockIdx.x, no products); blockIdx.y: the share of the N rows.
__global__ __launch_bounds__(256) void k_moments(const unsigned char* __restrict__ X, int dtype, int vec,
                                                 const long* __restrict__ index, long N, int D,
                                                 const double* __restrict__ shift, int T, int sums_only,
                                                 double* __restrict__ psum, double* __restrict__ pgram) {
  __shared__ __attribute__((aligned(16))) double sA[MOM_KC * MOM_LD];
  __shared__ __attribute__((aligned(16))) double sB[MOM_KC * MOM_LD];
  __shared__ double sShift[2][MOM_TILE];
  __shared__ double sRed[4][MOM_TILE];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int bi = blockIdx.x, bj = blockIdx.x;
  if (!sums_only) {
    int rem = blockIdx.x;
    bi = 0;
    while (rem >= T - bi) {
      rem -= T - bi;
      ++bi;
    }
    bj = bi + rem;
  }
  const bool diag = bi == bj;
  const int S = gridDim.y, s = blockIdx.y;
  const long n_lo = N * s / S, n_hi = N * (s + 1) / S;
  const long rowbytes = (long)D * (dtype == 0 ? 1 : 4);

  // staging: threads 0..127 the row block's columns (A), 128..255 the column block's (B; idle on a diagonal tile); a
  // thread owns 4 columns of rows kk, kk + 8, kk + 16, kk + 24 of the step, so that the 16 lanes of a row read 64 columns
  // side by side from memory and write 512 consecutive bytes of LDS
  const int op = tid >> 7, q = tid & 15, kk = (tid & 127) >> 4;
  const int c0 = (op ? bj : bi) * MOM_TILE + 4 * q;
  const bool active = !(op && diag);   // uniform per wave
  double* const sMine = op ? sB : sA;
  const double* const pB = diag ? sA : sB;

  if (tid < 2 * MOM_TILE) {
    const int c = (tid >> 6 ? bj : bi) * MOM_TILE + (tid & 63);
    sShift[tid >> 6][tid & 63] = shift && c < D ? shift[c] : 0.0;
  }
  __syncthreads();

  f64x4 acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) acc[a][b] = f64x4{0.0, 0.0, 0.0, 0.0};
  double csum = 0.0;
  const int wm = (wave >> 1) * 32, wn = (wave & 1) * 32;

  if (n_lo < n_hi) {   // (an empty share writes zeros)
    const int n_kt = (int)((n_hi - n_lo + MOM_KC - 1) / MOM_KC);
    u32x4 raw[4];
    auto fetch = [&](int kt) {
      if (!active) return;
#pragma unroll
      for (int n = 0; n < 4; ++n) {
        const long r = n_lo + (long)kt * MOM_KC + kk + 8 * n;
        const long rr = r < n_hi ? r : n_lo;   // a missing row reads the share's first row and is zeroed
        const long src = index ? index[rr] : rr;
        raw[n] = load4(X + src * rowbytes, dtype, vec != 0, c0, D, r < n_hi);
      }
    };
    fetch(0);
    for (int kt = 0; kt < n_kt; ++kt) {
      if (active) {
#pragma unroll
        for (int n = 0; n < 4; ++n) {
          const int k = kk + 8 * n;
          const bool ok = n_lo + (long)kt * MOM_KC + k < n_hi;
          double v[4];
#pragma unroll
          for (int w = 0; w < 4; ++w) {
            v[w] = finish4(raw[n], dtype, w, c0, D, ok);
            if (ok && c0 + w < D) v[w] -= sShift[op][4 * q + w];
          }
          *reinterpret_cast<f64x2*>(sMine + k * MOM_LD + 4 * q) = f64x2{v[0], v[1]};
          *reinterpret_cast<f64x2*>(sMine + k * MOM_LD + 4 * q + 2) = f64x2{v[2], v[3]};
        }
      }
      __syncthreads();
      if (kt + 1 < n_kt) fetch(kt + 1);
      if (diag) {   // column sums of the tile's 64 columns: thread (c, quarter) adds its 8 rows of the step in order
        const int c = tid & 63, r0 = (tid >> 6) * (MOM_KC / 4);
#pragma unroll
        for (int r = 0; r < MOM_KC / 4; ++r) csum += sA[(r0 + r) * MOM_LD + c];
      }
      if (!sums_only) mma_chunk(sA, pB, wm, wn, lane, acc);
      __syncthreads();
    }
  }

  if (!sums_only) {   // acc[a][b][r]: row wm + 16 a + (lane >> 4) + 4 r, column wn + 16 b + (lane & 15) of the tile
    double* out = pgram + (long)s * D * D;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int i = bi * MOM_TILE + wm + 16 * a + (lane >> 4) + 4 * r;
          const int j = bj * MOM_TILE + wn + 16 * b + (lane & 15);
          if (i < D && j < D) out[(long)i * D + j] = acc[a][b][r];
        }
  }
  if (diag) {
    sRed[tid >> 6][tid & 63] = csum;
    __syncthreads();
    const int c = bi * MOM_TILE + tid;
    if (tid < MOM_TILE && c < D) psum[(long)s * D + c] = ((sRed[0][tid] + sRed[1][tid]) + sRed[2][tid]) + sRed[3][tid];
  }
}

// sum[d] = sum_s psum[s][d] and gram[i][j] = sum_s pgram[s][i][j], in split order; an entry below the tile diagonal reads
// its mirror image
__global__ __launch_bounds__(256) void k_moments_finish(const double* __restrict__ psum, const double* __restrict__ pgram,
                                                        int S, int D, double* __restrict__ sum, double* __restrict__ gram) {
  const long id = (long)blockIdx.x * 256 + threadIdx.x;
  if (id < D) {
    double a = 0.0;
    for (int s = 0; s < S; ++s) a += psum[(long)s * D + id];
    sum[id] = a;
  }
  if (gram && id < (long)D * D) {
    const int i = (int)(id / D), j = (int)(id - (long)i * D);
    const bool upper = (i / MOM_TILE) <= (j / MOM_TILE);
    const long at = upper ? (long)i * D + j : (long)j * D + i;
    double a = 0.0;
    for (int s = 0; s < S; ++s) a += pgram[(long)s * D * D + at];
    gram[id] = a;
  }
}

// ------------------------------------------------------------------------------------------------- polynomial-kernel sums
// partial[s][ti][tj] = sum over the 64 x 64 tile (ti, tj) of subset s of (gamma a_i . b_j + coef0)^degree, a_i row
// idx_a[s][i] of A and b_j row idx_b[s][j] of B (a null list: row i itself); exclude: pairs of equal row NUMBERS are
// skipped.  grid (tiles of mb, tiles of ma, S).
__global__ __launch_bounds__(256) void k_poly_sums(const unsigned char* __restrict__ A, int dtype_a, int vec_a,
                                                   const long* __restrict__ idx_a, const unsigned char* __restrict__ B,
                                                   int dtype_b, int vec_b, const long* __restrict__ idx_b, long ma, long mb,
                                                   int D, double gamma, double coef0, int degree, int exclude,
                                                   double* __restrict__ partial) {
  __shared__ __attribute__((aligned(16))) double sA[MOM_KC * MOM_LD];
  __shared__ __attribute__((aligned(16))) double sB[MOM_KC * MOM_LD];
  __shared__ long sIdx[2][MOM_TILE];
  __shared__ double sRed[4];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long s = blockIdx.z;
  const long i0 = (long)blockIdx.y * MOM_TILE, j0 = (long)blockIdx.x * MOM_TILE;

  // staging: waves 0, 1 the rows of A, waves 2, 3 the rows of B; a thread owns row m of the tile and 16 of the step's 32
  // elements, and writes them down a column of the staged [k][m] tile
  const int op = tid >> 7, g = (tid >> 6) & 1, m = tid & 63;
  const long m0 = op ? j0 : i0, mcount = op ? mb : ma;
  const bool ok = m0 + m < mcount;
  const long pos = ok ? m0 + m : m0;   // a missing row reads the tile's first row and is zeroed
  const long* const idx = op ? idx_b : idx_a;
  const long src = idx ? idx[s * mcount + pos] : pos;
  const int dtype = op ? dtype_b : dtype_a;
  const bool vec = (op ? vec_b : vec_a) != 0;
  const unsigned char* const row = (op ? B : A) + src * ((long)D * (dtype == 0 ? 1 : 4));
  double* const sMine = op ? sB : sA;
  if (g == 0) sIdx[op][m] = ok ? src : -1 - op;   // (missing rows never compare equal)

  f64x4 acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) acc[a][b] = f64x4{0.0, 0.0, 0.0, 0.0};
  const int wm = (wave >> 1) * 32, wn = (wave & 1) * 32;

  const int n_kt = (D + MOM_KC - 1) / MOM_KC;
  Raw16 raw = load16(row, dtype, vec, 16 * g, D, ok);
  for (int kt = 0; kt < n_kt; ++kt) {
    const int e0 = kt * MOM_KC + 16 * g;
#pragma unroll
    for (int e = 0; e < 16; ++e) sMine[(16 * g + e) * MOM_LD + m] = finish16(raw, dtype, e, e0, D, ok);
    __syncthreads();
    if (kt + 1 < n_kt) raw = load16(row, dtype, vec, e0 + MOM_KC, D, ok);
    mma_chunk(sA, sB, wm, wn, lane, acc);
    __syncthreads();
  }

  // acc[a][b][r]: row wm + 16 a + (lane >> 4) + 4 r of the tile (A side), column wn + 16 b + (lane & 15) (B side)
  double total = 0.0;
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int il = wm + 16 * a + (lane >> 4) + 4 * r, jl = wn + 16 * b + (lane & 15);
        const bool keep = i0 + il < ma && j0 + jl < mb && !(exclude && sIdx[0][il] == sIdx[1][jl]);
        const double v = gamma * acc[a][b][r] + coef0;
        double p = v;
        for (int d = 1; d < degree; ++d) p *= v;
        total += keep ? p : 0.0;
      }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) total += __shfl_xor(total, o, 64);
  if (lane == 0) sRed[wave] = total;
  __syncthreads();
  if (tid == 0)
    partial[(s * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = ((sRed[0] + sRed[1]) + sRed[2]) + sRed[3];
}

// sums[s] = the `tiles` partials of subset s: lane l adds partials l, l + 64, ... in order, then the lanes meet in a butterfly
__global__ __launch_bounds__(64) void k_poly_finish(const double* __restrict__ partial, long tiles,
                                                    double* __restrict__ sums) {
  const int lane = threadIdx.x;
  const double* p = partial + (long)blockIdx.x * tiles;
  double a = 0.0;
  for (long t = lane; t < tiles; t += 64) a += p[t];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o, 64);
  if (lane == 0) sums[blockIdx.x] = a;
}

inline bool rows_vec(const void* p, int dtype, int D) { return ((uintptr_t)p & 15) == 0 && D % (dtype == 0 ? 16 : 4) == 0; }

}  // namespace

// Shares of the N axis the library picks for the moments of an N x D set (host logic only).  The grid is (upper-triangular
// 64 x 64 tiles) x shares and three workgroups fit a CU: aim at about 4096 workgroups so that the last wave of them costs
// little, but give every share at least 512 rows (16 staged steps) and keep the [shares][D][D] fp64 partials below 256 MiB.
extern "C" int edm_moments_splits(long N, int D) {
  if (N < 1 || D < 1) return 1;
  const long T = (D + MOM_TILE - 1) / MOM_TILE, tiles = T * (T + 1) / 2;
  long s = (4096 + tiles - 1) / tiles;
  if (s > N / 512) s = N / 512;
  const long fit = MOM_PARTIAL_BYTES / ((long)D * D * 8);
  if (s > fit) s = fit;
  if (s > MOM_MAX_SPLITS) s = MOM_MAX_SPLITS;
  return (int)(s < 1 ? 1 : s);
}

extern "C" int edm_moments_partial(const void* x, int dtype, const long* index, long N, int D, const double* shift,
                                   int splits, double* psum, double* pgram, hipStream_t st) {
  EDM_REQUIRE(x && psum, "moments_partial: null pointer");
  EDM_REQUIRE(dtype == 0 || dtype == 1, "moments_partial: dtype must be 0 (uint8) or 1 (float32), got %d", dtype);
  EDM_REQUIRE(N >= 1 && N < (1L << 40), "moments_partial: N must be in [1, 2^40), got %ld", N);
  EDM_REQUIRE(D >= 1 && D <= MOM_MAX_D, "moments_partial: D must be in [1, %d], got %d", MOM_MAX_D, D);
  EDM_REQUIRE(splits >= 1 && splits <= MOM_MAX_SPLITS, "moments_partial: splits must be in [1, %d], got %d", MOM_MAX_SPLITS,
              splits);
  const int T = (D + MOM_TILE - 1) / MOM_TILE;
  const int sums_only = pgram ? 0 : 1;
  const dim3 grid((unsigned)(sums_only ? T : (long)T * (T + 1) / 2), (unsigned)splits);
  hipLaunchKernelGGL(k_moments, grid, dim3(256), 0, st, (const unsigned char*)x, dtype, ((uintptr_t)x & 15) == 0 && D % 4 == 0 ? 1 : 0, index,
                     N, D, shift, T, sums_only, psum, pgram);
  EDM_CHECK_LAUNCH("moments_partial");
  return EDM_OK;
}

extern "C" int edm_moments_finish(const double* psum, const double* pgram, int splits, int D, double* sum, double* gram,
                                  hipStream_t st) {
  EDM_REQUIRE(psum && sum, "moments_finish: null pointer");
  EDM_REQUIRE((pgram == nullptr) == (gram == nullptr), "moments_finish: pgram and gram go together");
  EDM_REQUIRE(D >= 1 && D <= MOM_MAX_D && splits >= 1 && splits <= MOM_MAX_SPLITS, "moments_finish: bad args splits=%d D=%d",
              splits, D);
  const long n = gram ? (long)D * D : (long)D;
  hipLaunchKernelGGL(k_moments_finish, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, psum, pgram, splits, D, sum, gram);
  EDM_CHECK_LAUNCH("moments_finish");
  return EDM_OK;
}

extern "C" int edm_poly_sums_partial(const void* a, int dtype_a, const long* idx_a, const void* b, int dtype_b,
                                     const long* idx_b, int S, long ma, long mb, int D, double gamma, double coef0,
                                     int degree, int exclude_equal_index, double* partial, hipStream_t st) {
  EDM_REQUIRE(a && b && partial, "poly_sums_partial: null pointer");
  EDM_REQUIRE((dtype_a == 0 || dtype_a == 1) && (dtype_b == 0 || dtype_b == 1),
              "poly_sums_partial: dtypes must be 0 (uint8) or 1 (float32), got %d and %d", dtype_a, dtype_b);
  EDM_REQUIRE(S >= 1 && S <= POLY_MAX_S, "poly_sums_partial: S must be in [1, %d], got %d", POLY_MAX_S, S);
  EDM_REQUIRE(ma >= 1 && ma <= POLY_MAX_M && mb >= 1 && mb <= POLY_MAX_M,
              "poly_sums_partial: ma and mb must be in [1, %ld], got %ld and %ld", POLY_MAX_M, ma, mb);
  EDM_REQUIRE(D >= 1 && D <= POLY_MAX_D, "poly_sums_partial: D must be in [1, %d], got %d", POLY_MAX_D, D);
  EDM_REQUIRE(degree >= 1 && degree <= 4, "poly_sums_partial: degree must be in [1, 4], got %d", degree);
  const dim3 grid((unsigned)((mb + MOM_TILE - 1) / MOM_TILE), (unsigned)((ma + MOM_TILE - 1) / MOM_TILE), (unsigned)S);
  hipLaunchKernelGGL(k_poly_sums, grid, dim3(256), 0, st, (const unsigned char*)a, dtype_a, rows_vec(a, dtype_a, D) ? 1 : 0,
                     idx_a, (const unsigned char*)b, dtype_b, rows_vec(b, dtype_b, D) ? 1 : 0, idx_b, ma, mb, D, gamma, coef0,
                     degree, exclude_equal_index, partial);
  EDM_CHECK_LAUNCH("poly_sums_partial");
  return EDM_OK;
}

extern "C" int edm_poly_sums_finish(const double* partial, int S, long tiles, double* sums, hipStream_t st) {
  EDM_REQUIRE(partial && sums, "poly_sums_finish: null pointer");
  EDM_REQUIRE(S >= 1 && S <= POLY_MAX_S && tiles >= 1, "poly_sums_finish: bad args S=%d tiles=%ld", S, tiles);
  hipLaunchKernelGGL(k_poly_finish, dim3((unsigned)S), dim3(64), 0, st, partial, tiles, sums);
  EDM_CHECK_LAUNCH("poly_sums_finish");
  return EDM_OK;
}
