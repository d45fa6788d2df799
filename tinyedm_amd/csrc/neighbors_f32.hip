// Feature-space nearest neighbours of float32 rows: for every query row the k reference rows with the smallest key
// (d2, reference index), and the ball membership counts of precision / recall / density / coverage, both on the fp64 tile
// engine of moments.hip (f64_tile.h: v_mfma_f64_16x16x4_f64, a 64 x 64 tile, K staged 32 elements at a time, float32
// rows converted to fp64 as they enter LDS).  The float32 twin of neighbors.hip.
//
// Why fp64.  A float32 product is exact in fp64, so only the sums round.  d2 = |q|^2 + |r|^2 - 2 q.r loses about
// log2(|q|^2 / d2) bits to cancellation: non-negative features with a large common mean (pool activations) can cancel
// most of an fp32 mantissa, and near-duplicates -- the rows a copy check is about -- would vanish.  In fp64 more than 40
// bits survive.
//
// The norm trick.  Identical rows must give d2 == +0.0 exactly, which holds only if |x|^2 has the bits of x.x as the
// distance tile computes it.  k_f32_norms therefore runs the very tile (A = B = the same 64 rows, same MFMA sequence and
// K order) and keeps the diagonal; 64 times the minimal work is negligible beside a search.  An element of the MFMA
// result depends on its own A row, B row and the K order only, never on its position in the tile.
//
// The contract.  The bits of d2(q, r) depend on the two rows and D only: not on the tile position, the split count, the
// chunking of the references, the load path (16-byte loads when a base is 16-byte aligned and D % 4 == 0, element loads
// otherwise) or on which of the two kernels computes them.  Both form d2 in one function (f32_d2) from one tile function
// (f32_dot_tile), so the k-th-neighbour radius of a search is the very number the ball count compares against.
//
// The key.  d2 >= +0.0, so its bit pattern as u64 is monotone; the total order is the pair (bits of d2, reference index),
// ties to the lower index: a 96-bit key kept as two arrays and compared lexicographically.  Empty slots are (all-ones, -1).
//
// Top-k (k_f32_knn).  A workgroup owns 64 queries and walks a contiguous share of the 64-reference tiles (the R axis is
// split over blockIdx.x).  It keeps per query a sorted list of its k best keys in LDS.  After a tile the 64 x 64 distances
// go to LDS (the staging area, free by then; missing and excluded pairs as all-ones) and the thread that owns a query
// walks its row against the k-th key and inserts the survivors.  A tile costs 64 x 64 x D fp64 MACs, far more than the
// int8 kernel's, so this plain insertion stays a small share of it except at very small D.  The lists leave as
// [split][Q][k] by ordinary stores and k_fknn_merge folds them.  No atomics of any kind in this file.
#include "common.h"
#include "f64_tile.h"

namespace {

typedef unsigned long long u64;

constexpr int FKNN_TILE = MOM_TILE;   // queries and references per workgroup tile
constexpr int FKNN_MAX_K = 32;
constexpr int FKNN_MAX_D = 32768;
constexpr int FKNN_MAX_SPLITS = 1024;
constexpr u64 FKNN_EMPTY = ~0ull;
constexpr int FKNN_STAGE_BYTES = 2 * MOM_KC * MOM_LD * 8;   // the two staged operand tiles (40 KB)
constexpr int FKNN_TLD = FKNN_TILE + 1;                     // doubles per query row of the distance tile in LDS (odd)
static_assert(FKNN_TILE * FKNN_TLD * 8 <= FKNN_STAGE_BYTES, "the distance tile reuses the staging area");
constexpr int FBALL_RED_STRIDE = 33;                        // ints per query row of the ball count's final reduction
static_assert(FKNN_TILE * FBALL_RED_STRIDE * 4 <= FKNN_STAGE_BYTES, "the final reduction reuses the staging area");

__host__ __device__ inline int fknn_list_stride(int k) { return k | 1; }   // odd: the 64 owners hit different banks
inline int fknn_lds_bytes(int k) { return FKNN_STAGE_BYTES + FKNN_TILE * fknn_list_stride(k) * (8 + 4); }

// the one place a distance is formed (2 dot is exact, so a fused and an unfused form round alike)
__device__ __forceinline__ double f32_d2(double nq, double nr, double dot) { return fmax((nq + nr) - 2.0 * dot, 0.0); }

// key (ad, ai) before key (bd, bi)
__device__ __forceinline__ bool key_less(u64 ad, int ai, u64 bd, int bi) { return ad < bd || (ad == bd && ai < bi); }

// acc = the 64 x 64 dot products of query rows q0 .. q0 + 63 and reference rows r0 .. r0 + 63 (rows at or past Q / R and
// elements past D are zero operands).  q0 < Q and r0 < R.  k_poly_sums' K loop: waves 0, 1 stage the query rows, waves 2, 3
// the reference rows; a thread owns row m of the tile and 16 of the step's 32 elements; the raw bits of step t + 1 are
// loaded before the MFMAs of step t.  acc[a][b][r]: query wm + 16 a + (lane >> 4) + 4 r, reference wn + 16 b + (lane & 15),
// wm = (wave >> 1) * 32, wn = (wave & 1) * 32.  Ends behind a barrier: sA and sB are free on return.
__device__ __forceinline__ void f32_dot_tile(const float* __restrict__ Qm, bool vec_q, int q0, int Q,
                                             const float* __restrict__ Rm, bool vec_r, int r0, int R, int D,
                                             double* __restrict__ sA, double* __restrict__ sB, f64x4 (&acc)[2][2]) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int op = tid >> 7, g = (tid >> 6) & 1, m = tid & 63;
  const int m0 = op ? r0 : q0, mcount = op ? R : Q;
  const bool ok = m0 + m < mcount;
  const long pos = ok ? m0 + m : m0;   // a missing row reads the tile's first row and is zeroed
  const unsigned char* const row = reinterpret_cast<const unsigned char*>((op ? Rm : Qm) + pos * (long)D);
  const bool vec = op ? vec_r : vec_q;
  double* const sMine = op ? sB : sA;
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) acc[a][b] = f64x4{0.0, 0.0, 0.0, 0.0};
  const int wm = (wave >> 1) * 32, wn = (wave & 1) * 32;

  const int n_kt = (D + MOM_KC - 1) / MOM_KC;
  Raw16 raw = load16(row, 1, vec, 16 * g, D, ok);
  for (int kt = 0; kt < n_kt; ++kt) {
    const int e0 = kt * MOM_KC + 16 * g;
#pragma unroll
    for (int e = 0; e < 16; ++e) sMine[(16 * g + e) * MOM_LD + m] = finish16(raw, 1, e, e0, D, ok);
    __syncthreads();
    if (kt + 1 < n_kt) raw = load16(row, 1, vec, e0 + MOM_KC, D, ok);
    mma_chunk(sA, sB, wm, wn, lane, acc);
    __syncthreads();
  }
}

// norms[row] = |x_row|^2 with the bits of the distance tile's x.x: the diagonal of the tile of 64 rows against themselves
__global__ __launch_bounds__(256) void k_f32_norms(const float* __restrict__ X, int vec, int N, int D,
                                                   double* __restrict__ norms) {
  __shared__ __attribute__((aligned(16))) double sA[MOM_KC * MOM_LD];
  __shared__ __attribute__((aligned(16))) double sB[MOM_KC * MOM_LD];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r0 = blockIdx.x * FKNN_TILE;
  f64x4 acc[2][2];
  f32_dot_tile(X, vec != 0, r0, N, X, vec != 0, r0, N, D, sA, sB, acc);
  if ((wave >> 1) == (wave & 1)) {   // the waves on the tile diagonal
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int il = (wave >> 1) * 32 + 16 * a + (lane >> 4) + 4 * r;
        if ((lane >> 4) + 4 * r == (lane & 15) && r0 + il < N) norms[r0 + il] = acc[a][a][r];
      }
  }
}

__global__ __launch_bounds__(256) void k_f32_knn(const float* __restrict__ Qm, const float* __restrict__ Rm, int vec_q,
                                                 int vec_r, const double* __restrict__ qn, const double* __restrict__ rn,
                                                 int Q, int R, int D, int k, int exclude_self, int ref_base,
                                                 u64* __restrict__ keys_d2, int* __restrict__ keys_idx) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  double* sA = reinterpret_cast<double*>(smem);
  double* sB = sA + MOM_KC * MOM_LD;
  u64* sT = reinterpret_cast<u64*>(smem);   // the distance tile [64][FKNN_TLD], over the staging area between K loops
  const int ls = fknn_list_stride(k);
  u64* Ld = reinterpret_cast<u64*>(smem + FKNN_STAGE_BYTES);
  int* Li = reinterpret_cast<int*>(Ld + FKNN_TILE * ls);

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = (wave >> 1) * 32, wn = (wave & 1) * 32;
  const int S = gridDim.x, s = blockIdx.x;   // this workgroup's share of the reference tiles
  const int q0 = blockIdx.y * FKNN_TILE;
  const int n_rt = (R + FKNN_TILE - 1) / FKNN_TILE;
  const int rt_lo = (int)((long)n_rt * s / S), rt_hi = (int)((long)n_rt * (s + 1) / S);

  for (int i = tid; i < FKNN_TILE * ls; i += 256) {
    Ld[i] = FKNN_EMPTY;
    Li[i] = -1;
  }
  __syncthreads();

  for (int rt = rt_lo; rt < rt_hi; ++rt) {
    const int r0 = rt * FKNN_TILE;
    f64x4 acc[2][2];
    f32_dot_tile(Qm, vec_q != 0, q0, Q, Rm, vec_r != 0, r0, R, D, sA, sB, acc);

    // ---- the tile's keys: acc[a][b][r] is query wm + 16 a + (lane >> 4) + 4 r against reference wn + 16 b + (lane & 15)
    double rnorm[2];
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      const int rr = r0 + wn + 16 * b + (lane & 15);
      rnorm[b] = rr < R ? rn[rr] : 0.0;
    }
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int il = wm + 16 * a + (lane >> 4) + 4 * r, q = q0 + il;
        const double qnorm = q < Q ? qn[q] : 0.0;
#pragma unroll
        for (int b = 0; b < 2; ++b) {
          const int jl = wn + 16 * b + (lane & 15), rr = r0 + jl;
          const bool ok = q < Q && rr < R && !(exclude_self && ref_base + rr == q);
          const double d2 = f32_d2(qnorm, rnorm[b], acc[a][b][r]);
          sT[il * FKNN_TLD + jl] = ok ? (u64)__double_as_longlong(d2) : FKNN_EMPTY;
        }
      }
    __syncthreads();
    if (tid < FKNN_TILE) {   // the owner of query tid: its 64 candidates against its k-th key
      u64* const L = Ld + tid * ls;
      int* const I = Li + tid * ls;
      u64 thr_d = L[k - 1];
      int thr_i = I[k - 1];
#pragma unroll 8
      for (int j = 0; j < FKNN_TILE; ++j) {
        const u64 c = sT[tid * FKNN_TLD + j];
        const int gi = ref_base + r0 + j;
        if (c != FKNN_EMPTY && key_less(c, gi, thr_d, thr_i)) {
          int p = k - 1;
          while (p > 0 && key_less(c, gi, L[p - 1], I[p - 1])) {
            L[p] = L[p - 1];
            I[p] = I[p - 1];
            --p;
          }
          L[p] = c;
          I[p] = gi;
          thr_d = L[k - 1];
          thr_i = I[k - 1];
        }
      }
    }
    __syncthreads();   // (the next K loop overwrites the tile)
  }

  // lists -> keys[s][q][0..k)
  for (int i = tid; i < FKNN_TILE * k; i += 256) {
    const int ql = i / k, e = i - ql * k;
    if (q0 + ql < Q) {
      const long at = ((long)s * Q + q0 + ql) * k + e;
      keys_d2[at] = Ld[ql * ls + e];
      keys_idx[at] = Li[ql * ls + e];
    }
  }
}

// keys [n_lists][Q][k] (each list ascending, empty slots (all-ones, -1)) -> the k smallest keys of each query, ascending,
// as dist fp64 and idx.  k_knn_merge with two-word keys: one wave per query; the running best k (entries 64..95 of a
// 96-entry LDS window) and 64 new candidates are ranked against each other by counting smaller keys; real keys are unique
// (an index occurs once), so ranks below k are too.
__global__ __launch_bounds__(64) void k_fknn_merge(const u64* __restrict__ keys_d2, const int* __restrict__ keys_idx,
                                                   int n_lists, int Q, int k, double* __restrict__ dist,
                                                   int* __restrict__ idx) {
  __shared__ u64 win_d[96];
  __shared__ int win_i[96];
  __shared__ u64 best_d[FKNN_MAX_K];
  __shared__ int best_i[FKNN_MAX_K];
  const int q = blockIdx.x, lane = threadIdx.x;
  if (lane < FKNN_MAX_K) {
    best_d[lane] = FKNN_EMPTY;
    best_i[lane] = -1;
  }
  __syncthreads();
  const long per = (long)n_lists * k;   // candidate c of this query: list c / k, slot c % k
  for (long c0 = 0; c0 < per; c0 += 64) {
    const long c = c0 + lane;
    u64 mine_d = FKNN_EMPTY;
    int mine_i = -1;
    if (c < per) {
      const long sp = c / k, e = c - sp * k;
      mine_d = keys_d2[(sp * Q + q) * k + e];
      mine_i = keys_idx[(sp * Q + q) * k + e];
    }
    win_d[lane] = mine_d;
    win_i[lane] = mine_i;
    const u64 old_d = lane < FKNN_MAX_K ? best_d[lane] : FKNN_EMPTY;
    const int old_i = lane < FKNN_MAX_K ? best_i[lane] : -1;
    if (lane < FKNN_MAX_K) {
      win_d[64 + lane] = old_d;
      win_i[64 + lane] = old_i;
    }
    __syncthreads();
    int rank_new = 0, rank_old = 0;
#pragma unroll 8
    for (int e = 0; e < 96; ++e) {
      const u64 od = win_d[e];
      const int oi = win_i[e];
      rank_new += key_less(od, oi, mine_d, mine_i) ? 1 : 0;
      rank_old += key_less(od, oi, old_d, old_i) ? 1 : 0;
    }
    __syncthreads();
    if (lane < FKNN_MAX_K) {
      best_d[lane] = FKNN_EMPTY;
      best_i[lane] = -1;
    }
    __syncthreads();
    if (mine_i >= 0 && rank_new < k) {
      best_d[rank_new] = mine_d;
      best_i[rank_new] = mine_i;
    }
    if (old_i >= 0 && rank_old < k) {
      best_d[rank_old] = old_d;
      best_i[rank_old] = old_i;
    }
    __syncthreads();
  }
  if (lane < k) {
    dist[(long)q * k + lane] = __longlong_as_double((long long)best_d[lane]);
    idx[(long)q * k + lane] = best_i[lane];
  }
}

// counts[s][q] = the number of references r in share s of the 64-reference tiles with d2(q, r) <= radii[r] (closed, fp64),
// a radius per REFERENCE.  The distance tile and the distance are k_f32_knn's (f32_dot_tile, f32_d2).  A lane holds 8 query
// rows x 2 reference columns of a tile; the 0/1 results add up in 8 per-lane registers that live across the share's tiles.
// After the last tile the 16 lanes that hold a query row and the two waves that share the query half meet in LDS (the
// staging area): red[64][32 (+1 pad)] ints, one thread per query sums its 32 partial counts and stores one int.  Every
// counts[s][q], q < Q, is written by an ordinary store; an empty share writes 0.
__global__ __launch_bounds__(256) void k_f32_ball_count(const float* __restrict__ Qm, const float* __restrict__ Rm,
                                                        int vec_q, int vec_r, const double* __restrict__ qn,
                                                        const double* __restrict__ rn, const double* __restrict__ radii,
                                                        int Q, int R, int D, int exclude_self, int ref_base,
                                                        int* __restrict__ counts) {
  __shared__ __attribute__((aligned(16))) char smem[FKNN_STAGE_BYTES];
  double* sA = reinterpret_cast<double*>(smem);
  double* sB = sA + MOM_KC * MOM_LD;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = (wave >> 1) * 32, wn = (wave & 1) * 32;
  const int S = gridDim.x, s = blockIdx.x;
  const int q0 = blockIdx.y * FKNN_TILE;
  const int n_rt = (R + FKNN_TILE - 1) / FKNN_TILE;
  const int rt_lo = (int)((long)n_rt * s / S), rt_hi = (int)((long)n_rt * (s + 1) / S);

  int cnt[2][4];   // [a][r]: query wm + 16 a + (lane >> 4) + 4 r, over this lane's reference columns of every tile so far
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int r = 0; r < 4; ++r) cnt[a][r] = 0;

  for (int rt = rt_lo; rt < rt_hi; ++rt) {
    const int r0 = rt * FKNN_TILE;
    f64x4 acc[2][2];
    f32_dot_tile(Qm, vec_q != 0, q0, Q, Rm, vec_r != 0, r0, R, D, sA, sB, acc);

    double rnorm[2], rad[2];
    bool col_ok[2];
    int self_q[2];   // the query row that reference column b must skip (-1: none)
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      const int rr = r0 + wn + 16 * b + (lane & 15);
      col_ok[b] = rr < R;
      rnorm[b] = col_ok[b] ? rn[rr] : 0.0;
      rad[b] = col_ok[b] ? radii[rr] : 0.0;
      self_q[b] = exclude_self ? ref_base + rr : -1;
    }
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int q = q0 + wm + 16 * a + (lane >> 4) + 4 * r;
        const bool row_ok = q < Q;
        const double qnorm = row_ok ? qn[q] : 0.0;
        int c = 0;
#pragma unroll
        for (int b = 0; b < 2; ++b)
          c += (col_ok[b] && q != self_q[b] && f32_d2(qnorm, rnorm[b], acc[a][b][r]) <= rad[b]) ? 1 : 0;
        cnt[a][r] += row_ok ? c : 0;
      }
  }

  // the K loop ended behind a barrier (and an empty share never touched the staging area), so the area is free
  int* red = reinterpret_cast<int*>(smem);
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int r = 0; r < 4; ++r)
      red[(wm + 16 * a + (lane >> 4) + 4 * r) * FBALL_RED_STRIDE + (wave & 1) * 16 + (lane & 15)] = cnt[a][r];
  __syncthreads();
  if (tid < FKNN_TILE && q0 + tid < Q) {
    int total = 0;
#pragma unroll
    for (int e = 0; e < 32; ++e) total += red[tid * FBALL_RED_STRIDE + e];
    counts[(long)s * Q + q0 + tid] = total;
  }
}

constexpr long FKNN_MAX_Q = 65535L * FKNN_TILE;           // grid.y
constexpr long FKNN_MAX_INDEX = (1L << 31) - FKNN_TILE;    // the last tile's row numbers (tile base + 63) stay in an int

inline bool f32_rows_vec(const void* p, int D) { return ((uintptr_t)p & 15) == 0 && D % 4 == 0; }

}  // namespace

// Split count the library picks for a Q x R search (host logic only).  Two workgroups fit a CU (512 at a time on the chip)
// and a workgroup's time is proportional to its share of the reference tiles: aim at about 8 waves of workgroups (4096), but
// give every share at least 4 reference tiles (each share leaves a key list per query, which the merge reads).
extern "C" int edm_f32_knn_splits(long Q, long R) {
  if (Q < 1 || R < 1) return 1;
  const long qt = (Q + FKNN_TILE - 1) / FKNN_TILE, rt = (R + FKNN_TILE - 1) / FKNN_TILE;
  long s = (4096 + qt - 1) / qt;
  if (s > rt / 4) s = rt / 4;
  if (s > FKNN_MAX_SPLITS) s = FKNN_MAX_SPLITS;
  return (int)(s < 1 ? 1 : s);
}

// norms fp64 [n_rows] = |x|^2 of the rows of x float32 [n_rows][D], with the bits of the distance tile's x.x: what
// edm_f32_knn_partial and edm_f32_ball_count_partial take as qnorms / rnorms.  Once per set.
extern "C" int edm_f32_norms(const void* x, long n_rows, int D, double* norms, hipStream_t st) {
  EDM_REQUIRE(x && norms, "f32_norms: null pointer");
  EDM_REQUIRE(n_rows >= 1 && n_rows <= FKNN_MAX_INDEX, "f32_norms: n_rows must be in [1, 2^31 - 64], got %ld", n_rows);
  EDM_REQUIRE(D >= 1 && D <= FKNN_MAX_D, "f32_norms: D must be in [1, %d], got %d", FKNN_MAX_D, D);
  hipLaunchKernelGGL(k_f32_norms, dim3((unsigned)((n_rows + FKNN_TILE - 1) / FKNN_TILE)), dim3(256), 0, st,
                     (const float*)x, f32_rows_vec(x, D) ? 1 : 0, (int)n_rows, D, norms);
  EDM_CHECK_LAUNCH("f32_norms");
  return EDM_OK;
}

// Partial search: queries float32 [Q][D] against references float32 [R][D] (row-contiguous, 4-byte aligned).  Writes
// keys_d2 uint64 [splits][Q][k] (the bit pattern of the fp64 d2) and keys_idx int32 [splits][Q][k] (ref_base + reference
// row), each list ascending by (d2, idx), unused slots (all-ones, -1).  The arguments as in edm_u8_knn_partial.
extern "C" int edm_f32_knn_partial(const void* queries, const void* refs, long Q, long R, int D, int k, int exclude_self,
                                   long ref_base, int partial, int splits, const double* qnorms, const double* rnorms,
                                   unsigned long long* keys_d2, int* keys_idx, hipStream_t st) {
  EDM_REQUIRE(queries && refs && qnorms && rnorms && keys_d2 && keys_idx, "f32_knn_partial: null pointer");
  EDM_REQUIRE(Q >= 1 && Q <= FKNN_MAX_Q, "f32_knn_partial: Q must be in [1, %ld], got %ld", FKNN_MAX_Q, Q);
  EDM_REQUIRE(D >= 1 && D <= FKNN_MAX_D, "f32_knn_partial: D must be in [1, %d], got %d", FKNN_MAX_D, D);
  EDM_REQUIRE(k >= 1 && k <= FKNN_MAX_K, "f32_knn_partial: k must be in [1, %d], got %d", FKNN_MAX_K, k);
  EDM_REQUIRE(R >= 1 && ref_base >= 0 && ref_base + R <= FKNN_MAX_INDEX,
              "f32_knn_partial: need R >= 1 and ref_base + R <= 2^31 - 64, got R = %ld, ref_base = %ld", R, ref_base);
  EDM_REQUIRE(partial || k <= R - (exclude_self ? 1 : 0),
              "f32_knn_partial: k = %d needs at least that many references%s, got R = %ld", k,
              exclude_self ? " besides the query itself" : "", R);
  EDM_REQUIRE(splits >= 1 && splits <= FKNN_MAX_SPLITS, "f32_knn_partial: splits must be in [1, %d], got %d",
              FKNN_MAX_SPLITS, splits);
  const dim3 grid((unsigned)splits, (unsigned)((Q + FKNN_TILE - 1) / FKNN_TILE));
  EDM_MAX_LDS(k_f32_knn, fknn_lds_bytes(FKNN_MAX_K));
  hipLaunchKernelGGL(k_f32_knn, grid, dim3(256), fknn_lds_bytes(k), st, (const float*)queries, (const float*)refs,
                     f32_rows_vec(queries, D) ? 1 : 0, f32_rows_vec(refs, D) ? 1 : 0, qnorms, rnorms, (int)Q, (int)R, D, k,
                     exclude_self, (int)ref_base, keys_d2, keys_idx);
  EDM_CHECK_LAUNCH("f32_knn_partial");
  return EDM_OK;
}

// Merge n_lists key lists per query (as edm_f32_knn_partial writes them: the splits of one call, or of every chunk of a
// chunked search laid end to end) into dist fp64 [Q][k] and idx int32 [Q][k], ascending by (d2, idx).
extern "C" int edm_fknn_merge(const unsigned long long* keys_d2, const int* keys_idx, int n_lists, long Q, int k,
                              double* dist, int* idx, hipStream_t st) {
  EDM_REQUIRE(keys_d2 && keys_idx && dist && idx, "fknn_merge: null pointer");
  EDM_REQUIRE(n_lists >= 1 && Q >= 1 && Q <= FKNN_MAX_Q && k >= 1 && k <= FKNN_MAX_K,
              "fknn_merge: bad args n_lists=%d Q=%ld k=%d", n_lists, Q, k);
  EDM_REQUIRE((long)n_lists * k < (1L << 31), "fknn_merge: too many lists (%d)", n_lists);
  hipLaunchKernelGGL(k_fknn_merge, dim3((unsigned)Q), dim3(64), 0, st, keys_d2, keys_idx, n_lists, (int)Q, k, dist, idx);
  EDM_CHECK_LAUNCH("fknn_merge");
  return EDM_OK;
}

// Ball membership counts on the same distance tile: counts int32 [splits][Q], counts[s][q] = the number of references r in
// share s with d2(q, r) <= radii[r] (closed, fp64; radii fp64 [R], finite and >= 0 by the caller's check).  The arguments as
// in edm_u8_ball_count_partial.
extern "C" int edm_f32_ball_count_partial(const void* queries, const void* refs, long Q, long R, int D, const double* radii,
                                          int exclude_self, long ref_base, int splits, const double* qnorms,
                                          const double* rnorms, int* counts, hipStream_t st) {
  EDM_REQUIRE(queries && refs && radii && qnorms && rnorms && counts, "f32_ball_count_partial: null pointer");
  EDM_REQUIRE(Q >= 1 && Q <= FKNN_MAX_Q, "f32_ball_count_partial: Q must be in [1, %ld], got %ld", FKNN_MAX_Q, Q);
  EDM_REQUIRE(D >= 1 && D <= FKNN_MAX_D, "f32_ball_count_partial: D must be in [1, %d], got %d", FKNN_MAX_D, D);
  EDM_REQUIRE(R >= 1 && ref_base >= 0 && ref_base + R <= FKNN_MAX_INDEX,
              "f32_ball_count_partial: need R >= 1 and ref_base + R <= 2^31 - 64, got R = %ld, ref_base = %ld", R, ref_base);
  EDM_REQUIRE(splits >= 1 && splits <= FKNN_MAX_SPLITS, "f32_ball_count_partial: splits must be in [1, %d], got %d",
              FKNN_MAX_SPLITS, splits);
  const dim3 grid((unsigned)splits, (unsigned)((Q + FKNN_TILE - 1) / FKNN_TILE));
  hipLaunchKernelGGL(k_f32_ball_count, grid, dim3(256), 0, st, (const float*)queries, (const float*)refs,
                     f32_rows_vec(queries, D) ? 1 : 0, f32_rows_vec(refs, D) ? 1 : 0, qnorms, rnorms, radii, (int)Q, (int)R, D,
                     exclude_self, (int)ref_base, counts);
  EDM_CHECK_LAUNCH("f32_ball_count_partial");
  return EDM_OK;
}
