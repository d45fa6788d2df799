// Exact pixel-space nearest neighbours of uint8 images: for every query row the k reference rows with the smallest key
// (d2, reference index), d2 = sum_j (q_j - r_j)^2 as an exact integer.  Ties in distance go to the lower index, so the
// answer is unique and does not depend on tiling, split count or arrival order.
//
// Arithmetic.  x ^ 0x80 turns a uint8 into the int8 x - 128 (one XOR with 0x80808080 per dword does four); the shift cancels
// in q - r, so d2 = |q'|^2 + |r'|^2 - 2 q'.r' on the shifted rows.  q'.r' runs on v_mfma_i32_16x16x64_i8 with int32
// accumulation; D <= 32768 keeps every term below 2^31 (|x'|^2 <= 2^29, |q'.r'| <= 2^29, d2 <= 65025 * 32768 < 2^31).
// Row numbers are ints: ref_base + R <= 2^31 - 128, so that the last tile's base + 127 does not overflow.
// A K tail is padded with ZERO IN THE SHIFTED DOMAIN; the norms (k_u8_norms) run over the real elements only.
//
// Tiling (k_u8_knn).  A workgroup of 256 threads (4 waves as 2 x 2) owns 128 queries and walks a contiguous share of the
// 128-reference tiles (the R axis is split over blockIdx.x so that a small Q still fills the chip).  Per 128-byte K step both
// operand tiles (128 rows x 128 B each, already shifted) go global -> registers -> LDS as 16-byte chunks, chunk c of row r at
// slot c ^ ((r >> 1) & 7) of the row, so that the 16 rows one ds_read_b128 lane group touches fall on 16 different 16-byte
// slots of the 256-byte bank row.  The loads of step t + 1 are issued before the MFMAs of step t, without a branch
// around any of them (load_chunk_raw), and shifted / zeroed only when they are written to LDS.  A wave holds a 64 x 64
// block of dot products as 4 x 4 accumulators (64 VGPRs); per 64-byte K half it reads 4 + 4 fragments and issues 16 MFMAs.
// Fragments: lane l holds the 16-byte segment (l >> 4) of the 64-byte K chunk of row (l & 15), the same assignment for A and
// B (a dot product does not care which k a lane holds as long as both operands agree); C is the dtype-independent 16x16 map
// col = l & 15 (reference), row = 4 (l >> 4) + reg (query).
//
// Top-k.  Each workgroup keeps, per query, a sorted list of its k best 64-bit keys d2 << 32 | index in LDS.  After a tile
// every lane checks its 64 candidates against the k-th key of their query (one 64-bit compare); survivors go through a
// 1024-entry LDS queue (slots by one LDS atomic add per wave and candidate position: the order of arrival is irrelevant
// because the key is total) and the thread
// that owns a query inserts them into its list.  When the queue overflows (the first tiles of a split) the round repeats
// with the candidates that are still below the updated k-th key.  The lists leave as [split][Q][k] keys with ordinary stores
// and k_knn_merge folds the splits (or the chunks of a chunked search) in key order; empty slots are all-ones keys.
#include "common.h"

namespace {

typedef __attribute__((ext_vector_type(4))) int i32x4;
typedef unsigned long long u64;

constexpr int KNN_TILE = 128;        // queries and references per workgroup tile
constexpr int KNN_BK = 128;          // bytes of K per staged step (two MFMA K = 64 halves)
constexpr int KNN_QCAP = 1024;       // candidate queue entries
constexpr int KNN_MAX_K = 32;
constexpr int KNN_MAX_D = 32768;
constexpr int KNN_MAX_SPLITS = 1024;
constexpr u64 KNN_EMPTY = ~0ull;
constexpr int KNN_STAGE_BYTES = 2 * KNN_TILE * KNN_BK;   // A and B tiles

__host__ __device__ inline int knn_list_stride(int k) { return k | 1; }   // odd 8-byte stride: owners hit different banks
inline int knn_lds_bytes(int k) {
  return KNN_STAGE_BYTES + KNN_TILE * knn_list_stride(k) * 8 + KNN_QCAP * 8 + KNN_QCAP * 4 + 16;
}

// 16 bytes of a row starting at byte k0, shifted to int8 (x ^ 0x80); bytes at or past D, and rows that do not exist
// (!row_ok), read as 0 (shifted domain).  `row` must point at a readable row even when !row_ok (the callers pass the
// tile's first row).  VEC: rows are 16-byte aligned and D % 16 == 0, so a chunk is wholly inside or wholly outside the row;
// the load itself is unconditional (from byte 0 when the chunk is outside) and the result is selected afterwards -- a
// branch around each load makes the compiler wait for every load before it issues the next.
// (the shift and the zeroing are a separate step, chunk_finish, so that the K loop can apply them when it writes the
// chunk to LDS -- a whole step of MFMAs after the load was issued -- and not right behind the load)
template <bool VEC>
__device__ __forceinline__ u32x4 load_chunk_raw(const unsigned char* __restrict__ row, int k0, int D, bool row_ok) {
  u32x4 v = {0u, 0u, 0u, 0u};
  if (VEC) {
    v = *reinterpret_cast<const u32x4*>(row + (row_ok && k0 < D ? k0 : 0));
  } else {
    if (!row_ok) return v;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      uint32_t x = 0;
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const int k = k0 + 4 * w + b;
        if (k < D) x |= (uint32_t)(row[k] ^ 0x80u) << (8 * b);
      }
      v[w] = x;
    }
  }
  return v;
}
template <bool VEC>
__device__ __forceinline__ u32x4 chunk_finish(u32x4 x, int k0, int D, bool row_ok) {
  if (!VEC) return x;   // the element path shifts and zeroes as it loads
  return (x ^ 0x80808080u) & (row_ok && k0 < D ? 0xFFFFFFFFu : 0u);
}
template <bool VEC>
__device__ __forceinline__ u32x4 load_chunk(const unsigned char* __restrict__ row, int k0, int D, bool row_ok) {
  return chunk_finish<VEC>(load_chunk_raw<VEC>(row, k0, D, row_ok), k0, D, row_ok);
}

__device__ __forceinline__ int sq_sum4(uint32_t w) {   // sum of squares of the four int8 of a shifted dword
  int s = 0;
#pragma unroll
  for (int b = 0; b < 4; ++b) {
    const int x = (int)(signed char)(w >> (8 * b));
    s += x * x;
  }
  return s;
}

// norms[row] = sum_j (x_j - 128)^2 over the D real elements: one wave per row, four rows per workgroup pass
template <bool VEC>
__global__ __launch_bounds__(256) void k_u8_norms(const unsigned char* __restrict__ X, long n_rows, int D,
                                                   int* __restrict__ norms) {
  const int lane = threadIdx.x & 63;
  for (long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6); row < n_rows; row += (long)gridDim.x * 4) {
    const unsigned char* p = X + row * (long)D;
    int s = 0;
    for (int k0 = lane * 16; k0 < D; k0 += 64 * 16) {
      const u32x4 v = load_chunk<VEC>(p, k0, D, true);
      s += sq_sum4(v[0]) + sq_sum4(v[1]) + sq_sum4(v[2]) + sq_sum4(v[3]);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (lane == 0) norms[row] = s;
  }
}

// byte offset of 16-byte chunk c (0..7) of row r inside a staged [128][128 B] tile
__device__ __forceinline__ int stage_off(int r, int c) { return r * KNN_BK + ((c ^ ((r >> 1) & 7)) << 4); }

template <bool VEC>
__global__ __launch_bounds__(256, 2) void k_u8_knn(const unsigned char* __restrict__ Qm, const unsigned char* __restrict__ Rm,
                                                 const int* __restrict__ qn, const int* __restrict__ rn, int Q, int R, int D,
                                                 int k, int exclude_self, int ref_base, u64* __restrict__ keys) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* sA = smem;
  char* sB = smem + KNN_TILE * KNN_BK;
  const int lstride = knn_list_stride(k);
  u64* lists = reinterpret_cast<u64*>(smem + KNN_STAGE_BYTES);
  u64* qkey = lists + KNN_TILE * lstride;
  int* qrow = reinterpret_cast<int*>(qkey + KNN_QCAP);
  int* qcount = qrow + KNN_QCAP;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wq = (wave >> 1) * 64, wr = (wave & 1) * 64;   // the wave's 64 x 64 block inside the tile
  const int l15 = lane & 15, lq = lane >> 4;
  const int S = gridDim.x, s = blockIdx.x;   // this workgroup's share of the reference tiles
  const int q0 = blockIdx.y * KNN_TILE;
  const int n_rt = (R + KNN_TILE - 1) / KNN_TILE;
  const int rt_lo = (int)((long)n_rt * s / S), rt_hi = (int)((long)n_rt * (s + 1) / S);

  for (int i = tid; i < KNN_TILE * lstride; i += 256) lists[i] = KNN_EMPTY;
  if (tid == 0) *qcount = 0;
  __syncthreads();

  const int n_kt = (D + KNN_BK - 1) / KNN_BK;
  // staging: chunk id = tid + 256 n (n = 0..3) -> row id >> 3, chunk id & 7: a row's 128 bytes are 8 consecutive threads
  for (int rt = rt_lo; rt < rt_hi; ++rt) {
    const int r0 = rt * KNN_TILE;
    i32x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = i32x4{0, 0, 0, 0};

    // (tile bases are wave-uniform; a lane's own offset fits 32 bits: 128 rows x D <= 32768)
    const unsigned char* qbase = Qm + (long)q0 * D;
    const unsigned char* rbase = Rm + (long)r0 * D;
    // the chunks of step t + 1 are loaded (32 VGPRs) before the MFMAs of step t and written to LDS behind them
    u32x4 ra[4], rb[4];
    auto fetch = [&](int kt) {
#pragma unroll
      for (int n = 0; n < 4; ++n) {
        const int row = (tid >> 3) + 32 * n, c = tid & 7;
        const int kb = kt * KNN_BK + c * 16;
        const bool q_ok = q0 + row < Q, r_ok = r0 + row < R;   // (a missing row reads the tile's first row and is zeroed)
        ra[n] = load_chunk_raw<VEC>(qbase + (unsigned)((q_ok ? row : 0) * D), kb, D, q_ok);
        rb[n] = load_chunk_raw<VEC>(rbase + (unsigned)((r_ok ? row : 0) * D), kb, D, r_ok);
      }
    };
    fetch(0);
    for (int kt = 0; kt < n_kt; ++kt) {
#pragma unroll
      for (int n = 0; n < 4; ++n) {
        const int id = tid + 256 * n, row = id >> 3, c = id & 7;
        const int kb = kt * KNN_BK + c * 16;
        *reinterpret_cast<u32x4*>(sA + stage_off(row, c)) = chunk_finish<VEC>(ra[n], kb, D, q0 + row < Q);
        *reinterpret_cast<u32x4*>(sB + stage_off(row, c)) = chunk_finish<VEC>(rb[n], kb, D, r0 + row < R);
      }
      __syncthreads();
      if (kt + 1 < n_kt) fetch(kt + 1);
      // all 16 fragments of the step first, then its 32 MFMAs: the LDS latency is paid once per step, not once per
      // fragment (a K half that is all padding holds zeros and adds nothing)
      i32x4 fa[2][4], fb[2][4];
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          fa[h][i] = *reinterpret_cast<const i32x4*>(sA + stage_off(wq + 16 * i + l15, 4 * h + lq));
          fb[h][i] = *reinterpret_cast<const i32x4*>(sB + stage_off(wr + 16 * i + l15, 4 * h + lq));
        }
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(fa[h][i], fb[h][j], acc[i][j], 0, 0, 0);
      __syncthreads();
    }

    // ---- candidates: acc[i][j][r] is query wq + 16 i + 4 lq + r against reference wr + 16 j + l15
    // The candidate phase works from copies of the lane coordinates that the compiler cannot see through: its 16 list
    // addresses, row numbers and norms are then formed here, once per tile, instead of being hoisted out of the tile loop
    // and held in registers through the K loop (which made the K loop serialise its fragment reads for lack of registers).
    int lq_c = lq, l15_c = l15, wq_c = wq, wr_c = wr;
    asm volatile("" : "+v"(lq_c), "+v"(l15_c), "+v"(wq_c), "+v"(wr_c));
    // norms of the lane's 16 queries (rows wq_c + 16 i + 4 lq + r) and 4 references: read per tile (cache hits) so that they
    // do not hold registers through the K loop
    int qnorm[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int q = q0 + wq_c + 16 * i + 4 * lq_c + r;
        qnorm[i][r] = q < Q ? qn[q] : 0;
      }
    int rnorm[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int rr = r0 + wr_c + 16 * j + l15_c;
      rnorm[j] = rr < R ? rn[rr] : 0;
    }
    // the accumulators become the distances in place (one register per candidate; the 64-bit keys are never all live)
    u64 pending = 0;   // bit (i * 16 + j * 4 + r): candidate still below its query's k-th key
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int q = q0 + wq_c + 16 * i + 4 * lq_c + r;
          const int rr = r0 + wr_c + 16 * j + l15_c;
          const bool ok = q < Q && rr < R && !(exclude_self && ref_base + rr == q);
          if (ok) pending |= 1ull << (i * 16 + j * 4 + r);
          acc[i][j][r] = qnorm[i][r] + rnorm[j] - 2 * acc[i][j][r];
        }
    for (;;) {
      // per block of four queries (i): their k-th keys as two words (they move only between rounds), then the 16 candidates;
      // the scheduling fence keeps the four blocks apart so that their operands are not all live at once
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        uint32_t thr_d[4], thr_i[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const u64 t = lists[(wq_c + 16 * i + 4 * lq_c + r) * lstride + k - 1];
          thr_d[r] = (uint32_t)(t >> 32);
          thr_i[r] = (uint32_t)t;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const u64 bit = 1ull << (i * 16 + j * 4 + r);
            const uint32_t d2 = (uint32_t)acc[i][j][r];
            const uint32_t gi = (uint32_t)(ref_base + r0 + wr_c + 16 * j + l15_c);
            const bool want = (pending & bit) && (d2 < thr_d[r] || (d2 == thr_d[r] && gi < thr_i[r]));
            if (!want) pending &= ~bit;
            // one LDS atomic per wave and candidate slot: the lanes that want a queue entry take consecutive ones
            const u64 m = __ballot(want);
            if (m) {   // wave-uniform
              const int first = __ffsll((long long)m) - 1;
              int base = 0;
              if (lane == first) base = atomicAdd(qcount, __popcll(m));
              base = __shfl(base, first, 64);
              const int pos = base + __popcll(m & ((1ull << lane) - 1ull));
              if (want && pos < KNN_QCAP) {
                qkey[pos] = ((u64)d2 << 32) | gi;
                qrow[pos] = wq_c + 16 * i + 4 * lq_c + r;
                pending &= ~bit;
              }
            }
          }
        __builtin_amdgcn_sched_barrier(0);
      }
      __syncthreads();
      const int total = *qcount;
      const int n = total < KNN_QCAP ? total : KNN_QCAP;
      if (tid < KNN_TILE) {
        u64* L = lists + tid * lstride;
        for (int e = 0; e < n; ++e) {
          if (qrow[e] != tid) continue;
          const u64 key = qkey[e];
          if (key < L[k - 1]) {
            int p = k - 1;
            while (p > 0 && L[p - 1] > key) {
              L[p] = L[p - 1];
              --p;
            }
            L[p] = key;
          }
        }
      }
      __syncthreads();
      if (tid == 0) *qcount = 0;
      __syncthreads();
      if (total <= KNN_QCAP) break;   // uniform: every thread read the same count
    }
  }

  // lists -> keys[s][q][0..k)
  for (int i = tid; i < KNN_TILE * k; i += 256) {
    const int ql = i / k, e = i - ql * k;
    if (q0 + ql < Q) keys[((long)s * Q + q0 + ql) * k + e] = lists[ql * lstride + e];
  }
}

// keys [S][Q][k] (each list ascending, empty slots all-ones) -> the k smallest keys of each query, ascending, split into
// dist (high word) and idx (low word).  One wave per query: the running best k (lanes 64..95 of a 96-entry LDS window) and 64
// new candidates are ranked against each other by counting smaller keys; keys are unique, so ranks below k are too.
__global__ __launch_bounds__(64) void k_knn_merge(const u64* __restrict__ keys, int S, int Q, int k,
                                                   unsigned* __restrict__ dist, int* __restrict__ idx) {
  __shared__ u64 win[96];
  __shared__ u64 best[KNN_MAX_K];
  const int q = blockIdx.x, lane = threadIdx.x;
  if (lane < KNN_MAX_K) best[lane] = KNN_EMPTY;
  __syncthreads();
  const int per = S * k;   // candidate c of this query: split c / k, slot c % k
  for (int c0 = 0; c0 < per; c0 += 64) {
    const int c = c0 + lane;
    u64 mine = KNN_EMPTY;
    if (c < per) {
      const int sp = c / k, e = c - sp * k;
      mine = keys[((long)sp * Q + q) * k + e];
    }
    win[lane] = mine;
    const u64 old = lane < KNN_MAX_K ? best[lane] : KNN_EMPTY;
    if (lane < KNN_MAX_K) win[64 + lane] = old;
    __syncthreads();
    int rank_new = 0, rank_old = 0;
#pragma unroll 8
    for (int e = 0; e < 96; ++e) {
      const u64 o = win[e];
      rank_new += o < mine ? 1 : 0;
      rank_old += o < old ? 1 : 0;
    }
    __syncthreads();
    if (lane < KNN_MAX_K) best[lane] = KNN_EMPTY;
    __syncthreads();
    if (mine != KNN_EMPTY && rank_new < k) best[rank_new] = mine;
    if (old != KNN_EMPTY && rank_old < k) best[rank_old] = old;
    __syncthreads();
  }
  if (lane < k) {
    const u64 b = best[lane];
    dist[(long)q * k + lane] = (unsigned)(b >> 32);
    idx[(long)q * k + lane] = (int)(unsigned)b;
  }
}

// Ball membership counts: counts[s][q] = the number of references r in share s of the 128-reference tiles with
// d2(q, r) <= radii[r], a radius per REFERENCE (the k-NN radius of r inside its own set), which no top-k list can answer.
// The distance tile is k_u8_knn's, step for step (same staging, swizzle, prefetch, fragments and MFMAs, through the same
// helpers; its own copy of the K loop so that k_u8_knn's register allocation is not touched).  The epilogue is smaller: a lane
// holds 16 query rows x 4 reference columns of a tile; each d2 is compared with its column's radius and the 0/1 results add
// up in 16 per-lane registers (one per query row) that live across the share's tiles.  d2 < 2^31 but a radius may be anything
// up to 2^32 - 1: the compare is UNSIGNED.  After the last tile the 16 lanes that hold a query row and the two waves that
// share the query half meet in LDS (the staging area, free by then): red[128][32 (+1 pad)] ints, one thread per query sums
// its 32 partial counts and stores one int.  Every counts[s][q], q < Q, is written by an ordinary store; an empty share writes
// 0.  No atomics of any kind.
constexpr int BALL_RED_STRIDE = 33;   // ints per query row of the final reduction: odd, so the 128 owners hit different banks
static_assert(KNN_TILE * BALL_RED_STRIDE * 4 <= KNN_STAGE_BYTES, "the final reduction reuses the staging area");

template <bool VEC>
__global__ __launch_bounds__(256, 2) void k_u8_ball_count(const unsigned char* __restrict__ Qm,
                                                        const unsigned char* __restrict__ Rm, const int* __restrict__ qn,
                                                        const int* __restrict__ rn, const uint32_t* __restrict__ radii, int Q,
                                                        int R, int D, int exclude_self, int ref_base, int* __restrict__ counts) {
  __shared__ __attribute__((aligned(16))) char smem[KNN_STAGE_BYTES];
  char* sA = smem;
  char* sB = smem + KNN_TILE * KNN_BK;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wq = (wave >> 1) * 64, wr = (wave & 1) * 64;   // the wave's 64 x 64 block inside the tile
  const int l15 = lane & 15, lq = lane >> 4;
  const int S = gridDim.x, s = blockIdx.x;   // this workgroup's share of the reference tiles
  const int q0 = blockIdx.y * KNN_TILE;
  const int n_rt = (R + KNN_TILE - 1) / KNN_TILE;
  const int rt_lo = (int)((long)n_rt * s / S), rt_hi = (int)((long)n_rt * (s + 1) / S);

  int cnt[4][4];   // [i][r]: query wq + 16 i + 4 lq + r, summed over this lane's reference columns of every tile so far
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int r = 0; r < 4; ++r) cnt[i][r] = 0;

  const int n_kt = (D + KNN_BK - 1) / KNN_BK;
  for (int rt = rt_lo; rt < rt_hi; ++rt) {
    const int r0 = rt * KNN_TILE;
    i32x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = i32x4{0, 0, 0, 0};

    // ---- the distance tile of k_u8_knn (see there for the staging, the prefetch and the fragment map)
    const unsigned char* qbase = Qm + (long)q0 * D;
    const unsigned char* rbase = Rm + (long)r0 * D;
    u32x4 ra[4], rb[4];
    auto fetch = [&](int kt) {
#pragma unroll
      for (int n = 0; n < 4; ++n) {
        const int row = (tid >> 3) + 32 * n, c = tid & 7;
        const int kb = kt * KNN_BK + c * 16;
        const bool q_ok = q0 + row < Q, r_ok = r0 + row < R;   // (a missing row reads the tile's first row and is zeroed)
        ra[n] = load_chunk_raw<VEC>(qbase + (unsigned)((q_ok ? row : 0) * D), kb, D, q_ok);
        rb[n] = load_chunk_raw<VEC>(rbase + (unsigned)((r_ok ? row : 0) * D), kb, D, r_ok);
      }
    };
    fetch(0);
    for (int kt = 0; kt < n_kt; ++kt) {
#pragma unroll
      for (int n = 0; n < 4; ++n) {
        const int id = tid + 256 * n, row = id >> 3, c = id & 7;
        const int kb = kt * KNN_BK + c * 16;
        *reinterpret_cast<u32x4*>(sA + stage_off(row, c)) = chunk_finish<VEC>(ra[n], kb, D, q0 + row < Q);
        *reinterpret_cast<u32x4*>(sB + stage_off(row, c)) = chunk_finish<VEC>(rb[n], kb, D, r0 + row < R);
      }
      __syncthreads();
      if (kt + 1 < n_kt) fetch(kt + 1);
      i32x4 fa[2][4], fb[2][4];
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          fa[h][i] = *reinterpret_cast<const i32x4*>(sA + stage_off(wq + 16 * i + l15, 4 * h + lq));
          fb[h][i] = *reinterpret_cast<const i32x4*>(sB + stage_off(wr + 16 * i + l15, 4 * h + lq));
        }
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(fa[h][i], fb[h][j], acc[i][j], 0, 0, 0);
      __syncthreads();
    }

    // ---- membership: acc[i][j][r] is query wq + 16 i + 4 lq + r against reference wr + 16 j + l15
    // (opaque copies of the lane coordinates, as in k_u8_knn: the norms, radii and row numbers are formed here, once per
    // tile, and do not hold registers through the K loop)
    int lq_c = lq, l15_c = l15, wq_c = wq, wr_c = wr;
    asm volatile("" : "+v"(lq_c), "+v"(l15_c), "+v"(wq_c), "+v"(wr_c));
    int rnorm[4], self_q[4];   // self_q: the query row that reference column j must skip (-1: none)
    uint32_t rad[4];
    bool col_ok[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int rr = r0 + wr_c + 16 * j + l15_c;
      col_ok[j] = rr < R;
      rnorm[j] = col_ok[j] ? rn[rr] : 0;
      rad[j] = col_ok[j] ? radii[rr] : 0u;
      self_q[j] = exclude_self ? ref_base + rr : -1;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int q = q0 + wq_c + 16 * i + 4 * lq_c + r;
        const bool row_ok = q < Q;
        const int qnorm = row_ok ? qn[q] : 0;
        int c = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const uint32_t d2 = (uint32_t)(qnorm + rnorm[j] - 2 * acc[i][j][r]);   // exact and < 2^31 for a real pair
          c += (col_ok[j] && q != self_q[j] && d2 <= rad[j]) ? 1 : 0;           // unsigned: a radius may be >= 2^31
        }
        cnt[i][r] += row_ok ? c : 0;
      }
  }

  // ---- the 16 lanes of a query row, and the two waves of a query half, meet in LDS.  The K loop ended with a barrier (and
  // an empty share never touched the staging area), so the area is free.
  int* red = reinterpret_cast<int*>(smem);
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int r = 0; r < 4; ++r) red[(wq + 16 * i + 4 * lq + r) * BALL_RED_STRIDE + (wave & 1) * 16 + l15] = cnt[i][r];
  __syncthreads();
  if (tid < KNN_TILE && q0 + tid < Q) {
    int total = 0;
#pragma unroll
    for (int e = 0; e < 32; ++e) total += red[tid * BALL_RED_STRIDE + e];
    counts[(long)s * Q + q0 + tid] = total;
  }
}

constexpr long KNN_MAX_Q = 65535L * KNN_TILE;          // grid.y
constexpr long KNN_MAX_INDEX = (1L << 31) - KNN_TILE;   // the last tile's row numbers (tile base + 127) stay in an int

}  // namespace

// Split count the library picks for a Q x R search (host logic only).  Two workgroups fit a CU (512 at a time on the chip) and
// a workgroup's time is proportional to its share of the reference tiles, so a grid of one or two waves of workgroups can
// leave half the chip idle behind the last one: aim at about 8 waves (4096 workgroups), but give every share at least 4
// reference tiles (the first tile of a share pays for filling the lists).  ops.u8_knn asks before it allocates the keys.
extern "C" int edm_u8_knn_splits(long Q, long R) {
  if (Q < 1 || R < 1) return 1;
  const long qt = (Q + KNN_TILE - 1) / KNN_TILE, rt = (R + KNN_TILE - 1) / KNN_TILE;
  long s = (4096 + qt - 1) / qt;
  if (s > rt / 4) s = rt / 4;
  if (s > KNN_MAX_SPLITS) s = KNN_MAX_SPLITS;
  return (int)(s < 1 ? 1 : s);
}

// norms[row] = sum_j (x_j - 128)^2 of the rows of x u8 [n_rows][D]: the |q'|^2 and |r'|^2 of edm_u8_knn_partial, computed
// once per set (a chunked search reuses the query norms for every chunk).  16-byte loads when x is 16-byte aligned and
// D % 16 == 0, element loads otherwise.
extern "C" int edm_u8_norms(const void* x, long n_rows, int D, int* norms, hipStream_t st) {
  EDM_REQUIRE(x && norms, "u8_norms: null pointer");
  EDM_REQUIRE(n_rows >= 1 && n_rows <= KNN_MAX_INDEX && D >= 1 && D <= KNN_MAX_D, "u8_norms: bad args n_rows=%ld D=%d",
              n_rows, D);
  const long want = (n_rows + 3) / 4;
  const unsigned grid = (unsigned)(want < 65536 ? want : 65536);   // the kernel strides over the rows
  if (D % 16 == 0 && ((uintptr_t)x & 15) == 0)
    hipLaunchKernelGGL(k_u8_norms<true>, dim3(grid), dim3(256), 0, st, (const unsigned char*)x, n_rows, D, norms);
  else
    hipLaunchKernelGGL(k_u8_norms<false>, dim3(grid), dim3(256), 0, st, (const unsigned char*)x, n_rows, D, norms);
  EDM_CHECK_LAUNCH("u8_norms");
  return EDM_OK;
}

// Partial search: queries u8 [Q][D] against references u8 [R][D] (row-contiguous, any byte alignment; the 16-byte path runs
// when both bases are 16-byte aligned and D % 16 == 0, the element path otherwise, same results).  Writes
// keys [splits][Q][k] (uint64 d2 << 32 | ref_base + reference row, each list ascending, unused slots all-ones).  ref_base is
// added to the reported indices (a chunk of a larger reference set); exclude_self skips reference ref_base + r == query row.
// qnorms [Q], rnorms [R]: edm_u8_norms of the two sets.  Limits (status -1 otherwise): 1 <= Q <= 65535 * 128,
// 1 <= D <= 32768, 1 <= k <= 32, k <= R (k <= R - 1 with exclude_self) unless partial != 0 (a chunk of a larger set may hold
// fewer than k rows; the caller has checked the whole set), ref_base + R <= 2^31 - 128, 1 <= splits <= 1024 (the caller's
// choice; edm_u8_knn_splits gives the library's).
extern "C" int edm_u8_knn_partial(const void* queries, const void* refs, long Q, long R, int D, int k, int exclude_self,
                                  long ref_base, int partial, int splits, const int* qnorms, const int* rnorms,
                                  unsigned long long* keys, hipStream_t st) {
  EDM_REQUIRE(queries && refs && qnorms && rnorms && keys, "u8_knn_partial: null pointer");
  EDM_REQUIRE(Q >= 1 && Q <= KNN_MAX_Q, "u8_knn_partial: Q must be in [1, %ld], got %ld", KNN_MAX_Q, Q);
  EDM_REQUIRE(D >= 1 && D <= KNN_MAX_D, "u8_knn_partial: D must be in [1, %d], got %d", KNN_MAX_D, D);
  EDM_REQUIRE(k >= 1 && k <= KNN_MAX_K, "u8_knn_partial: k must be in [1, %d], got %d", KNN_MAX_K, k);
  EDM_REQUIRE(R >= 1 && ref_base >= 0 && ref_base + R <= KNN_MAX_INDEX,
              "u8_knn_partial: need R >= 1 and ref_base + R <= 2^31 - 128, got R = %ld, ref_base = %ld", R, ref_base);
  EDM_REQUIRE(partial || k <= R - (exclude_self ? 1 : 0),
              "u8_knn_partial: k = %d needs at least that many references%s, got R = %ld", k,
              exclude_self ? " besides the query itself" : "", R);
  EDM_REQUIRE(splits >= 1 && splits <= KNN_MAX_SPLITS, "u8_knn_partial: splits must be in [1, %d], got %d", KNN_MAX_SPLITS,
              splits);
  const bool vec = D % 16 == 0 && ((uintptr_t)queries & 15) == 0 && ((uintptr_t)refs & 15) == 0;
  const unsigned char* q = (const unsigned char*)queries;
  const unsigned char* r = (const unsigned char*)refs;
  const int lds = knn_lds_bytes(k);
  const dim3 grid((unsigned)splits, (unsigned)((Q + KNN_TILE - 1) / KNN_TILE));
  if (vec) {
    EDM_MAX_LDS(k_u8_knn<true>, knn_lds_bytes(KNN_MAX_K));
    hipLaunchKernelGGL(k_u8_knn<true>, grid, dim3(256), lds, st, q, r, qnorms, rnorms, (int)Q, (int)R, D, k, exclude_self,
                       (int)ref_base, keys);
  } else {
    EDM_MAX_LDS(k_u8_knn<false>, knn_lds_bytes(KNN_MAX_K));
    hipLaunchKernelGGL(k_u8_knn<false>, grid, dim3(256), lds, st, q, r, qnorms, rnorms, (int)Q, (int)R, D, k, exclude_self,
                       (int)ref_base, keys);
  }
  EDM_CHECK_LAUNCH("u8_knn_partial");
  return EDM_OK;
}

// Ball membership counts (improved precision and recall, Kynkaanniemi et al. 2019; density and coverage, Naeem et al. 2020):
// counts [splits][Q] int32, counts[s][q] = the number of references r in share s of the 128-reference tiles with
// d2(q, r) <= radii[r] (closed balls, a radius per reference, uint32 [R], any value up to 2^32 - 1; the compare is unsigned).
// queries, refs, qnorms, rnorms, exclude_self, ref_base and splits as in edm_u8_knn_partial, with the same two load paths.
// Every element of counts is written by an ordinary store (an empty share writes 0); the caller adds the shares, an integer
// sum, so that neither splits nor chunking can change the total.  Limits (status -1 otherwise): 1 <= Q <= 65535 * 128,
// 1 <= D <= 32768, R >= 1, ref_base >= 0, ref_base + R <= 2^31 - 128, 1 <= splits <= 1024.
extern "C" int edm_u8_ball_count_partial(const void* queries, const void* refs, long Q, long R, int D, const unsigned* radii,
                                         int exclude_self, long ref_base, int splits, const int* qnorms, const int* rnorms,
                                         int* counts, hipStream_t st) {
  EDM_REQUIRE(queries && refs && radii && qnorms && rnorms && counts, "u8_ball_count_partial: null pointer");
  EDM_REQUIRE(Q >= 1 && Q <= KNN_MAX_Q, "u8_ball_count_partial: Q must be in [1, %ld], got %ld", KNN_MAX_Q, Q);
  EDM_REQUIRE(D >= 1 && D <= KNN_MAX_D, "u8_ball_count_partial: D must be in [1, %d], got %d", KNN_MAX_D, D);
  EDM_REQUIRE(R >= 1 && ref_base >= 0 && ref_base + R <= KNN_MAX_INDEX,
              "u8_ball_count_partial: need R >= 1 and ref_base + R <= 2^31 - 128, got R = %ld, ref_base = %ld", R, ref_base);
  EDM_REQUIRE(splits >= 1 && splits <= KNN_MAX_SPLITS, "u8_ball_count_partial: splits must be in [1, %d], got %d",
              KNN_MAX_SPLITS, splits);
  const bool vec = D % 16 == 0 && ((uintptr_t)queries & 15) == 0 && ((uintptr_t)refs & 15) == 0;
  const unsigned char* q = (const unsigned char*)queries;
  const unsigned char* r = (const unsigned char*)refs;
  const dim3 grid((unsigned)splits, (unsigned)((Q + KNN_TILE - 1) / KNN_TILE));
  if (vec)
    hipLaunchKernelGGL(k_u8_ball_count<true>, grid, dim3(256), 0, st, q, r, qnorms, rnorms, radii, (int)Q, (int)R, D,
                       exclude_self, (int)ref_base, counts);
  else
    hipLaunchKernelGGL(k_u8_ball_count<false>, grid, dim3(256), 0, st, q, r, qnorms, rnorms, radii, (int)Q, (int)R, D,
                       exclude_self, (int)ref_base, counts);
  EDM_CHECK_LAUNCH("u8_ball_count_partial");
  return EDM_OK;
}

// Merge n_lists key lists per query (keys [n_lists][Q][k], as edm_u8_knn_partial writes them: the splits of one call, or
// the splits of every chunk of a chunked search laid end to end) into dist uint32 [Q][k] and idx int32 [Q][k], ascending by
// (d2, index).  Every query must own at least k non-empty keys across its lists (guaranteed by k <= R).
extern "C" int edm_knn_merge(const unsigned long long* keys, int n_lists, long Q, int k, unsigned* dist, int* idx,
                             hipStream_t st) {
  EDM_REQUIRE(keys && dist && idx, "knn_merge: null pointer");
  EDM_REQUIRE(n_lists >= 1 && Q >= 1 && Q <= KNN_MAX_Q && k >= 1 && k <= KNN_MAX_K,
              "knn_merge: bad args n_lists=%d Q=%ld k=%d", n_lists, Q, k);
  EDM_REQUIRE((long)n_lists * k < (1L << 31), "knn_merge: too many lists (%d)", n_lists);
  hipLaunchKernelGGL(k_knn_merge, dim3((unsigned)Q), dim3(64), 0, st, keys, n_lists, (int)Q, k, dist, idx);
  EDM_CHECK_LAUNCH("knn_merge");
  return EDM_OK;
}
