// The ideal (empirical) denoiser of a finite training set (Karras et al. 2022, App. B.3, eq. 57):
//   D*(x; sigma) = sum_i w_i y_i,   w = softmax_i(l_i),   l_i = -|x - y_i|^2 / (2 sigma^2)
// over the training images y_i = (u_i / 255 - mean) / std held as uint8 rows, with the per-query statistics
// lse = log sum_i exp(l_i), ent = -sum w_i log w_i and the largest weight with its index (ties to the lower index).
// It is attention with K-wide keys (K = C H W, 3072 for CIFAR) over R tokens; the reference has no call site.
//
// Arithmetic.  Everything runs in UNITS OF ONE GREY LEVEL around 128: b = u - 128 (an integer in [-128, 127], exact in
// fp32) and z = (x - c) / a with a = 1 / (255 std), c = (128 / 255 - mean) / std, so that y = a b + c, x = a z + c and
//   |x - y|^2 = a^2 (|z|^2 - 2 z.b + |b|^2).
// z.b and, later, sum_j p_j b_j run on v_mfma_f32_16x16x4_f32: both operands fp32, the result bit for bit a k-ordered fmaf
// chain (two interleaved chains per element, added at the end), so the uint8 side carries no rounding at all and the fp32
// side none beyond its own.  |b|^2 is the exact integer of edm_u8_norms, |z|^2 an fp64 sum, and the three terms and the
// factor a^2 / (2 sigma^2) are combined in fp64 before the logit is rounded to fp32 once: the only error of a logit beyond
// that rounding is the accumulation error of z.b (DESIGN.md gives the resolution as a function of sigma).
//
// Work split over a chunk of Rc <= ref_chunk reference rows (the caller walks the chunks in order):
//   edm_ideal_begin       per query: |z|^2, a^2 / (2 sigma^2), the bad-value flag, the empty running state
//   edm_ideal_logits      S[q][j] = l of query q against row j of the chunk             (64 x 64 tiles, K steps of 32)
//   edm_ideal_softmax     per query: chunk max / argmax, new running max m', S <- p = exp(l - m') (masked: 0), running
//                         s = sum p, t = sum p (l - m'), the top logit and its index; alpha = exp(m - m') for the next step
//   edm_ideal_accumulate  A[q][k] = alpha_q A[q][k] + sum_j p[q][j] b[j][k]             (64 x 64 tiles, j steps of 32)
//   edm_ideal_finish      D = a A / s + c, lse = m + log s, ent = log s - t / s, top_w = exp(l_top - m) / s
// as attention_long.hip rescales between key tiles.  ent = lse - E_w[l] needs the one running sum t; it is kept relative to
// the running max (t' = alpha (t + (m - m') s)), which is the same identity without the cancellation of two large numbers.
//
// Order.  No floating-point atomics; every output element is written by an ordinary store of the one thread that owns it.
// A row's logits are chains over k in an order fixed by K, its sums over j trees and chains fixed by Rc, and rows of a tile
// never meet: with ref_chunk fixed the bits of row q depend on (x_q, sigma_q, class_q) and the reference set alone.
//
// Class restriction is a label compare: ref_labels[R] against the query's class in edm_ideal_softmax.  A masked logit takes
// no part in max, sum or statistics and its p is 0; it is computed and discarded (DESIGN.md states the cost).  The reference
// set keeps the caller's order, so the label-free call on a labelled set is the unlabelled computation bit for bit.
//
// Bad values.  sigma <= 0 or non-finite, a non-finite x row, or a class outside [0, num_classes) mark the row in
// edm_ideal_begin (health bit 1 << 1, as edm_eval_diffuse for a bad level); a class is only ever compared, never an index.
// Such a row leaves as NaN (top_idx -1) and does not touch the other rows.
#include "common.h"

namespace {

// tiles (compile-time: a tile size that followed Q or R would make a row's summation order follow them too).  64 x 64 for
// both products was the fastest of the five combinations up to 128 x 128 that were timed; -D overrides, for A/B runs
#ifndef IDEAL_LOGITS_TM
#define IDEAL_LOGITS_TM 64
#define IDEAL_LOGITS_TN 64
#define IDEAL_ACC_TM 64
#define IDEAL_ACC_TN 64
#endif
constexpr int ID_LQ = IDEAL_LOGITS_TM, ID_LR = IDEAL_LOGITS_TN;   // logits: queries x reference rows per workgroup
constexpr int ID_AQ = IDEAL_ACC_TM, ID_AN = IDEAL_ACC_TN;         // accumulate: queries x output columns per workgroup
constexpr int ID_BK = 32;            // reduction elements per staged step
constexpr int ID_LDA = ID_BK + 4;    // floats per staged row of a [rows][32] operand tile (144 B: 16-byte aligned rows)
constexpr int ID_STATE = 8;          // floats per query: m, s, t, l_top, alpha, i_top (int), bad (int), spare
constexpr int ID_MAX_K = 32768;
constexpr long ID_MAX_Q = 65535L * 64;
constexpr long ID_MAX_R = (1L << 31) - 128;

__device__ __forceinline__ float to_units(float x, float c, float inv_a) { return (x - c) * inv_a; }
__device__ __forceinline__ float u8_units(uint32_t word, int byte) { return (float)((int)((word >> (8 * byte)) & 0xFFu) - 128); }

struct IdealNorm {   // y = a * (u - 128) + c
  float a, c, inv_a;
  double a2;
};
inline IdealNorm ideal_norm(float mean, float stdv) {
  IdealNorm n;
  const double a = 1.0 / (255.0 * (double)stdv), c = (128.0 / 255.0 - (double)mean) / (double)stdv;
  n.a = (float)a;
  n.c = (float)c;
  n.inv_a = (float)(255.0 * (double)stdv);
  n.a2 = a * a;
  return n;
}

// one workgroup per query: |z|^2 in fp64 (thread-strided chains, a fixed tree), the logit factor, the flag, the empty state
__global__ __launch_bounds__(256) void k_ideal_begin(const float* __restrict__ X, const float* __restrict__ sigma,
                                                      const long long* __restrict__ labels, int num_classes, int K, float c,
                                                      float inv_a, double a2, double* __restrict__ qd,
                                                      float* __restrict__ state, unsigned* __restrict__ health) {
  __shared__ double red[256];
  const int q = blockIdx.x, tid = threadIdx.x;
  const float* p = X + (long)q * K;
  double s = 0.0;
  for (int k = tid; k < K; k += 256) {
    const double z = (double)to_units(p[k], c, inv_a);
    s += z * z;
  }
  red[tid] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) red[tid] += red[tid + o];
    __syncthreads();
  }
  if (tid == 0) {
    const float sg = sigma[q];
    bool bad = !(sg > 0.f) || !(sg <= 3.0e38f) || !(red[0] <= 1.0e300);
    if (labels) {
      const long long cls = labels[q];
      bad |= cls < 0 || cls >= (long long)num_classes;
    }
    qd[2 * (long)q] = bad ? 0.0 : red[0];
    qd[2 * (long)q + 1] = bad ? 0.0 : a2 / (2.0 * (double)sg * (double)sg);
    float* st = state + (long)q * ID_STATE;
    st[0] = -INFINITY;
    st[1] = 0.f;
    st[2] = 0.f;
    st[3] = -INFINITY;
    st[4] = 0.f;
    st[5] = __int_as_float(-1);
    st[6] = __int_as_float(bad ? 1 : 0);
    st[7] = 0.f;
    if (bad && health) atomicOr(health, 2u);
  }
}

// ---- staging of a [64 rows][32 floats] fp32 operand tile (queries of the logits, weights of the accumulate): thread t and
// t + 256 own the 16-byte pieces id = t + 256 n: row id >> 3, piece id & 7.  VEC: rows are 16-byte aligned and whole pieces
// lie inside or outside a row's `len` valid elements rounded up to 4 (the caller masks the elements past `len`); the load
// is unconditional (piece 0 of the tile's first row when outside) and the value is selected when it is written to LDS.
template <bool VEC>
__device__ __forceinline__ f32x4 load_f32_piece(const float* __restrict__ base, long ld, int row0, int row, int n_rows, int k,
                                                int len) {
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  const bool row_ok = row < n_rows;
  if (VEC) {
    v = *reinterpret_cast<const f32x4*>(base + (long)(row_ok ? row : row0) * ld + (row_ok && k < len ? k : 0));
  } else if (row_ok) {
    const float* p = base + (long)row * ld;
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (k + e < len) v[e] = p[k + e];
  }
  return v;
}
// 8 bytes of a uint8 row as two dwords; same rules (VEC: 8-byte aligned pieces wholly inside or outside the row)
template <bool VEC>
__device__ __forceinline__ u32x2 load_u8_piece(const unsigned char* __restrict__ base, long ld, int row, int n_rows, int k,
                                               int len) {
  u32x2 v = {0u, 0u};
  const bool row_ok = row < n_rows;
  if (VEC) {
    v = *reinterpret_cast<const u32x2*>(base + (long)(row_ok ? row : 0) * ld + (row_ok && k < len ? k : 0));
  } else if (row_ok) {
    const unsigned char* p = base + (long)row * ld;
#pragma unroll
    for (int e = 0; e < 8; ++e)
      if (k + e < len) v[e >> 2] |= (uint32_t)p[k + e] << (8 * (e & 3));
  }
  return v;
}

// S[q][j] = -(a^2 / (2 sigma_q^2)) (|z_q|^2 - 2 z_q.b_j + |b_j|^2) for the TM x TN tile (blockIdx.y, blockIdx.x).
// 4 waves as 2 x 2, a wave holds (TM / 2) x (TN / 2) dot products as MI x NJ accumulators of v_mfma_f32_16x16x4_f32, twice
// (the k steps alternate between the two sets: independent chains hide the 40-cycle accumulator latency, and a chain is K / 2
// long).  Fragments: lane l = (g = l >> 4, l15 = l & 15) reads the 16 bytes k = 16 h + 4 g .. + 3 of row l15 of its block for
// the half h of the step and feeds element s to MFMA s: the instruction's k index g stands for k = 16 h + 4 g + s on both
// operands (a dot product does not care which k a lane holds as long as both agree).  C: col = l15 (reference row),
// row = 4 g + reg (query).  The pieces of step t + 1 are loaded before the MFMAs of step t.
template <bool VEC, int TM, int TN>
__global__ __launch_bounds__(256) void k_ideal_logits(const float* __restrict__ X, const unsigned char* __restrict__ Y,
                                                       const int* __restrict__ bb, const double* __restrict__ qd, int Q,
                                                       int Rc, int K, float c, float inv_a, float* __restrict__ S, long ld) {
  static_assert(TM % 32 == 0 && TN % 64 == 0, "tile");
  constexpr int MI = TM / 32, NJ = TN / 32, NA = TM / 32, NB = TN / 64;   // accumulator blocks; staged pieces per thread
  __shared__ __attribute__((aligned(16))) float sA[TM * ID_LDA];
  __shared__ __attribute__((aligned(16))) float sB[TN * ID_LDA];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wq = (wave >> 1) * (TM / 2), wr = (wave & 1) * (TN / 2), l15 = lane & 15, g = lane >> 4;
  const int q0 = blockIdx.y * TM, r0 = blockIdx.x * TN;
  const unsigned char* Yt = Y + (long)r0 * K;   // the tile's first reference row (exists: the grid covers Rc)
  const int nr = Rc - r0;                       // rows of the chunk from there on

  f32x4 acc[2][MI][NJ];
#pragma unroll
  for (int p = 0; p < 2; ++p)
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
      for (int j = 0; j < NJ; ++j) acc[p][i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  // staging: query piece id = tid + 256 n -> row id >> 3, 16-byte piece id & 7; reference piece id -> row id >> 2, 8 bytes id & 3
  f32x4 ra[NA];
  u32x2 rb[NB];
  auto fetch = [&](int kt) {
#pragma unroll
    for (int n = 0; n < NA; ++n) {
      const int id = tid + 256 * n;
      ra[n] = load_f32_piece<VEC>(X, K, q0, q0 + (id >> 3), Q, kt * ID_BK + 4 * (id & 7), K);
    }
#pragma unroll
    for (int n = 0; n < NB; ++n) {
      const int id = tid + 256 * n;
      rb[n] = load_u8_piece<VEC>(Yt, K, id >> 2, nr, kt * ID_BK + 8 * (id & 3), K);
    }
  };
  const int n_kt = (K + ID_BK - 1) / ID_BK;
  fetch(0);
  for (int kt = 0; kt < n_kt; ++kt) {
#pragma unroll
    for (int n = 0; n < NA; ++n) {
      const int id = tid + 256 * n, row = id >> 3, k = kt * ID_BK + 4 * (id & 7);
      const bool row_ok = q0 + row < Q;
      f32x4 z;
#pragma unroll
      for (int e = 0; e < 4; ++e) z[e] = row_ok && k + e < K ? to_units(ra[n][e], c, inv_a) : 0.f;
      *reinterpret_cast<f32x4*>(sA + row * ID_LDA + 4 * (id & 7)) = z;
    }
#pragma unroll
    for (int n = 0; n < NB; ++n) {
      const int id = tid + 256 * n, row = id >> 2, k = kt * ID_BK + 8 * (id & 3);
      const bool row_ok = row < nr;
      f32x4 lo, hi;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        lo[e] = row_ok && k + e < K ? u8_units(rb[n][0], e) : 0.f;
        hi[e] = row_ok && k + 4 + e < K ? u8_units(rb[n][1], e) : 0.f;
      }
      *reinterpret_cast<f32x4*>(sB + row * ID_LDA + 8 * (id & 3)) = lo;
      *reinterpret_cast<f32x4*>(sB + row * ID_LDA + 8 * (id & 3) + 4) = hi;
    }
    __syncthreads();
    if (kt + 1 < n_kt) fetch(kt + 1);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      f32x4 a[MI], b[NJ];
#pragma unroll
      for (int i = 0; i < MI; ++i) a[i] = *reinterpret_cast<const f32x4*>(sA + (wq + 16 * i + l15) * ID_LDA + 16 * h + 4 * g);
#pragma unroll
      for (int j = 0; j < NJ; ++j) b[j] = *reinterpret_cast<const f32x4*>(sB + (wr + 16 * j + l15) * ID_LDA + 16 * h + 4 * g);
#pragma unroll
      for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
          for (int j = 0; j < NJ; ++j)
            acc[s & 1][i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i][s], b[j][s], acc[s & 1][i][j], 0, 0, 0);
    }
    __syncthreads();
  }

  // acc[.][i][j][r]: query q0 + wq + 16 i + 4 g + r against reference row r0 + wr + 16 j + l15
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int q = q0 + wq + 16 * i + 4 * g + r;
      if (q >= Q) continue;
      const double zz = qd[2 * (long)q], coef = qd[2 * (long)q + 1];
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        const int rr = r0 + wr + 16 * j + l15;
        if (rr >= Rc) continue;
        const double dot = (double)acc[0][i][j][r] + (double)acc[1][i][j][r];
        double d2 = zz + (double)bb[rr] - 2.0 * dot;
        d2 = d2 > 0.0 ? d2 : 0.0;   // (a squared distance; also keeps a NaN out)
        S[(long)q * ld + rr] = (float)(-coef * d2);
      }
    }
}

// One workgroup per query over the Rc logits of a chunk, in place: see the file comment.  Reductions: a thread walks
// j = tid, tid + 256, ... in order, the 256 partial results fold by a fixed tree; the argmax prefers the lower index.
__global__ __launch_bounds__(256) void k_ideal_softmax(float* __restrict__ S, long ld, int Rc, long ref_base,
                                                        const int* __restrict__ ref_labels,
                                                        const long long* __restrict__ labels, float* __restrict__ state) {
  __shared__ float rm[256];
  __shared__ int ri[256];
  __shared__ float rs[256], rt[256];
  const int q = blockIdx.x, tid = threadIdx.x;
  float* row = S + (long)q * ld;
  float* st = state + (long)q * ID_STATE;
  const float m_old = st[0];
  if (__float_as_int(st[6]) != 0) {   // a bad row takes no part: zero weights (uniform over the workgroup)
    for (int j = tid; j < Rc; j += 256) row[j] = 0.f;
    return;
  }
  const bool masked = ref_labels != nullptr && labels != nullptr;
  const int cls = masked ? (int)labels[q] : 0;   // in [0, num_classes): checked by k_ideal_begin; compared, never an index
  const int* rl = ref_labels + (masked ? ref_base : 0);

  float lm = -INFINITY;
  int li = 0x7FFFFFFF;
  for (int j = tid; j < Rc; j += 256) {
    const float l = row[j];
    if ((!masked || rl[j] == cls) && l > lm) {
      lm = l;
      li = j;
    }
  }
  rm[tid] = lm;
  ri[tid] = li;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) {
      const float om = rm[tid + o];
      const int oi = ri[tid + o];
      if (om > rm[tid] || (om == rm[tid] && oi < ri[tid])) {
        rm[tid] = om;
        ri[tid] = oi;
      }
    }
    __syncthreads();
  }
  const float cmax = rm[0];
  const int cidx = ri[0];
  const float m_new = fmaxf(m_old, cmax);
  const bool any = m_new > -INFINITY;

  float sp = 0.f, tp = 0.f;
  for (int j = tid; j < Rc; j += 256) {
    const float l = row[j];
    float p = 0.f;
    if (any && (!masked || rl[j] == cls)) p = expf(l - m_new);
    row[j] = p;
    sp += p;
    if (p > 0.f) tp += p * (l - m_new);
  }
  rs[tid] = sp;
  rt[tid] = tp;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) {
      rs[tid] += rs[tid + o];
      rt[tid] += rt[tid + o];
    }
    __syncthreads();
  }
  if (tid == 0) {
    const float s_old = st[1], t_old = st[2];
    float alpha = 0.f, s_prev = 0.f, t_prev = 0.f;
    if (m_old > -INFINITY) {   // (then m_new is finite too)
      alpha = expf(m_old - m_new);
      s_prev = alpha * s_old;
      t_prev = alpha * (t_old + (m_old - m_new) * s_old);
    }
    st[0] = m_new;
    st[1] = s_prev + rs[0];
    st[2] = t_prev + rt[0];
    if (cmax > st[3]) {   // strictly: an equal logit of a later chunk has the higher index
      st[3] = cmax;
      st[5] = __int_as_float((int)(ref_base + cidx));
    }
    st[4] = alpha;
  }
}

// A[q][n] = alpha_q A[q][n] + sum_j p[q][j] b[j][n] for the TM x TN tile (blockIdx.y queries, blockIdx.x columns) over the
// Rc rows of the chunk in steps of 32; `first`: A is written, not read.  Waves and accumulators as k_ideal_logits; the
// weights are the [TM][32] operand (16-byte fragment reads), the reference rows are staged as they lie, [32 j][TN n], and
// read as four dwords per fragment (lanes of a group read consecutive columns).
template <bool VEC, int TM, int TN>
__global__ __launch_bounds__(256) void k_ideal_accumulate(const float* __restrict__ P, long ld,
                                                           const unsigned char* __restrict__ Y,
                                                           const float* __restrict__ state, int Q, int Rc, int K, int first,
                                                           float* __restrict__ A) {
  static_assert(TM % 32 == 0 && TN % 64 == 0, "tile");
  constexpr int MI = TM / 32, NJ = TN / 32, NA = TM / 32, NB = TN / 64, LDN = TN + 4, PPR = TN / 8;   // PPR: 8-byte pieces per row
  __shared__ __attribute__((aligned(16))) float sA[TM * ID_LDA];
  __shared__ __attribute__((aligned(16))) float sB[ID_BK * LDN];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wq = (wave >> 1) * (TM / 2), wn = (wave & 1) * (TN / 2), l15 = lane & 15, g = lane >> 4;
  const int q0 = blockIdx.y * TM, n0 = blockIdx.x * TN;

  f32x4 acc[2][MI][NJ];
#pragma unroll
  for (int p = 0; p < 2; ++p)
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
      for (int j = 0; j < NJ; ++j) acc[p][i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  f32x4 ra[NA];
  u32x2 rb[NB];
  // (P is the library's own workspace: 16-byte aligned rows of ld % 4 == 0 floats, so its pieces are always vector loads;
  // `len` rounded up to 4 stays inside the row and the elements past Rc are masked below)
  auto fetch = [&](int jt) {
#pragma unroll
    for (int n = 0; n < NA; ++n) {
      const int id = tid + 256 * n;
      ra[n] = load_f32_piece<true>(P, ld, q0, q0 + (id >> 3), Q, jt * ID_BK + 4 * (id & 7), Rc);
    }
#pragma unroll
    for (int n = 0; n < NB; ++n) {
      const int id = tid + 256 * n;
      rb[n] = load_u8_piece<VEC>(Y + n0, K, jt * ID_BK + id / PPR, Rc, 8 * (id % PPR), K - n0);
    }
  };
  const int n_jt = (Rc + ID_BK - 1) / ID_BK;
  fetch(0);
  for (int jt = 0; jt < n_jt; ++jt) {
#pragma unroll
    for (int n = 0; n < NA; ++n) {
      const int id = tid + 256 * n, row = id >> 3, j = jt * ID_BK + 4 * (id & 7);
      const bool row_ok = q0 + row < Q;
      f32x4 p;
#pragma unroll
      for (int e = 0; e < 4; ++e) p[e] = row_ok && j + e < Rc ? ra[n][e] : 0.f;
      *reinterpret_cast<f32x4*>(sA + row * ID_LDA + 4 * (id & 7)) = p;
    }
#pragma unroll
    for (int n = 0; n < NB; ++n) {
      const int id = tid + 256 * n, jr = id / PPR, col = 8 * (id % PPR);
      const bool row_ok = jt * ID_BK + jr < Rc;
      f32x4 lo, hi;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        lo[e] = row_ok && n0 + col + e < K ? u8_units(rb[n][0], e) : 0.f;
        hi[e] = row_ok && n0 + col + 4 + e < K ? u8_units(rb[n][1], e) : 0.f;
      }
      *reinterpret_cast<f32x4*>(sB + jr * LDN + col) = lo;
      *reinterpret_cast<f32x4*>(sB + jr * LDN + col + 4) = hi;
    }
    __syncthreads();
    if (jt + 1 < n_jt) fetch(jt + 1);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      f32x4 a[MI];
#pragma unroll
      for (int i = 0; i < MI; ++i) a[i] = *reinterpret_cast<const f32x4*>(sA + (wq + 16 * i + l15) * ID_LDA + 16 * h + 4 * g);
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        float b[NJ];
#pragma unroll
        for (int j = 0; j < NJ; ++j) b[j] = sB[(16 * h + 4 * g + s) * LDN + wn + 16 * j + l15];
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
          for (int j = 0; j < NJ; ++j)
            acc[s & 1][i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i][s], b[j], acc[s & 1][i][j], 0, 0, 0);
      }
    }
    __syncthreads();
  }

  // acc[.][i][j][r]: query q0 + wq + 16 i + 4 g + r, column n0 + wn + 16 j + l15
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int q = q0 + wq + 16 * i + 4 * g + r;
      if (q >= Q) continue;
      const float alpha = state[(long)q * ID_STATE + 4];
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        const int n = n0 + wn + 16 * j + l15;
        if (n >= K) continue;
        float v = acc[0][i][j][r] + acc[1][i][j][r];
        float* dst = A + (long)q * K + n;
        if (!first) v = alpha * *dst + v;
        *dst = v;
      }
    }
}

// one workgroup per query: D = a A / s + c (in place when D == A) and the statistics; a bad row leaves as NaN
__global__ __launch_bounds__(256) void k_ideal_finish(const float* A, const float* __restrict__ state, int K, float a, float c,
                                                       float* D, float* __restrict__ lse, float* __restrict__ ent,
                                                       float* __restrict__ top_w, int* __restrict__ top_idx,
                                                       unsigned* __restrict__ health) {
  const int q = blockIdx.x, tid = threadIdx.x;
  const float* st = state + (long)q * ID_STATE;
  const bool bad = __float_as_int(st[6]) != 0;
  const float m = st[0], s = st[1], t = st[2];
  const float nan = __builtin_nanf("");
  bool flag = false;
  for (int k = tid; k < K; k += 256) {
    const float v = bad ? nan : a * (A[(long)q * K + k] / s) + c;
    flag |= !(fabsf(v) <= 3.0e38f);
    D[(long)q * K + k] = v;
  }
  if (tid == 0) {
    const float ls = logf(s);
    lse[q] = bad ? nan : m + ls;
    ent[q] = bad ? nan : ls - t / s;
    top_w[q] = bad ? nan : expf(st[3] - m) / s;
    top_idx[q] = bad ? -1 : __float_as_int(st[5]);
  }
  if (health && __any(flag) && (threadIdx.x & 63) == 0) atomicOr(health, 2u);
}

inline bool ideal_vec(const void* x, const void* refs, int K) {
  return K % 16 == 0 && ((uintptr_t)x & 15) == 0 && ((uintptr_t)refs & 15) == 0;
}

}  // namespace

#define IDEAL_NORM_ARGS(name)                                                                                      \
  EDM_REQUIRE(mean == mean && fabsf(mean) <= 3.0e38f && stdv > 0.f && stdv <= 3.0e38f,                           \
              name ": mean must be finite and std finite and > 0, got %g, %g", (double)mean, (double)stdv)

// Per query: |z|^2 -> qd[q][0], a^2 / (2 sigma_q^2) -> qd[q][1] (fp64 [Q][2]), and the empty running state
// (fp32 [Q][8]: m = -inf, s = t = 0, no top).  x fp32 [Q][K] row-contiguous, sigma fp32 [Q], labels int64 [Q] or null
// (null: no class restriction; num_classes is then ignored).  Marks bad rows and sets the health bit (see the file comment).
extern "C" int edm_ideal_begin(const float* x, const float* sigma, const long long* labels, int num_classes, long Q, int K,
                               float mean, float stdv, double* qd, float* state, unsigned* health, hipStream_t st) {
  EDM_REQUIRE(x && sigma && qd && state, "ideal_begin: null pointer");
  EDM_REQUIRE(Q >= 1 && Q <= ID_MAX_Q, "ideal_begin: Q must be in [1, %ld], got %ld", ID_MAX_Q, Q);
  EDM_REQUIRE(K >= 1 && K <= ID_MAX_K, "ideal_begin: K must be in [1, %d], got %d", ID_MAX_K, K);
  EDM_REQUIRE(!labels || num_classes >= 1, "ideal_begin: labels need num_classes >= 1, got %d", num_classes);
  IDEAL_NORM_ARGS("ideal_begin");
  const IdealNorm n = ideal_norm(mean, stdv);
  hipLaunchKernelGGL(k_ideal_begin, dim3((unsigned)Q), dim3(256), 0, st, x, sigma, labels, num_classes, K, n.c, n.inv_a, n.a2,
                     qd, state, health);
  EDM_CHECK_LAUNCH("ideal_begin");
  return EDM_OK;
}

// S[q][j] (fp32, row stride ld floats) = the logit of query q against row j of the chunk refs u8 [Rc][K] (row-contiguous, any
// byte alignment; the vector path runs when x and refs are 16-byte aligned and K % 16 == 0, the element path otherwise, same
// results).  rnorms [Rc]: edm_u8_norms of the chunk; qd: edm_ideal_begin's.
extern "C" int edm_ideal_logits(const float* x, const void* refs, const int* rnorms, const double* qd, long Q, long Rc, int K,
                                float mean, float stdv, float* S, long ld, hipStream_t st) {
  EDM_REQUIRE(x && refs && rnorms && qd && S, "ideal_logits: null pointer");
  EDM_REQUIRE(Q >= 1 && Q <= ID_MAX_Q, "ideal_logits: Q must be in [1, %ld], got %ld", ID_MAX_Q, Q);
  EDM_REQUIRE(K >= 1 && K <= ID_MAX_K, "ideal_logits: K must be in [1, %d], got %d", ID_MAX_K, K);
  EDM_REQUIRE(Rc >= 1 && Rc <= ID_MAX_R, "ideal_logits: the chunk must hold 1 to 2^31 - 128 rows, got %ld", Rc);
  EDM_REQUIRE(ld >= Rc, "ideal_logits: ld = %ld is below the chunk's %ld rows", ld, Rc);
  IDEAL_NORM_ARGS("ideal_logits");
  const IdealNorm n = ideal_norm(mean, stdv);
  const dim3 grid((unsigned)((Rc + ID_LR - 1) / ID_LR), (unsigned)((Q + ID_LQ - 1) / ID_LQ));
  if (ideal_vec(x, refs, K))
    hipLaunchKernelGGL((k_ideal_logits<true, ID_LQ, ID_LR>), grid, dim3(256), 0, st, x, (const unsigned char*)refs, rnorms, qd, (int)Q,
                       (int)Rc, K, n.c, n.inv_a, S, ld);
  else
    hipLaunchKernelGGL((k_ideal_logits<false, ID_LQ, ID_LR>), grid, dim3(256), 0, st, x, (const unsigned char*)refs, rnorms, qd, (int)Q,
                       (int)Rc, K, n.c, n.inv_a, S, ld);
  EDM_CHECK_LAUNCH("ideal_logits");
  return EDM_OK;
}

// The chunk's logits S -> its weights p = exp(l - m') in place, and the running state of every query moved on by the chunk.
// ref_base: the set index of the chunk's row 0 (reported top indices; ref_base + Rc <= 2^31 - 128).  ref_labels int32 [R of the
// whole set] and labels int64 [Q]: both given = the softmax of query q runs over the rows with ref_labels == labels[q].
extern "C" int edm_ideal_softmax(float* S, long ld, long Q, long Rc, long ref_base, const int* ref_labels,
                                 const long long* labels, float* state, hipStream_t st) {
  EDM_REQUIRE(S && state, "ideal_softmax: null pointer");
  EDM_REQUIRE(Q >= 1 && Q <= ID_MAX_Q, "ideal_softmax: Q must be in [1, %ld], got %ld", ID_MAX_Q, Q);
  EDM_REQUIRE(Rc >= 1 && ref_base >= 0 && ref_base + Rc <= ID_MAX_R,
              "ideal_softmax: need Rc >= 1 and ref_base + Rc <= 2^31 - 128, got Rc = %ld, ref_base = %ld", Rc, ref_base);
  EDM_REQUIRE(ld >= Rc, "ideal_softmax: ld = %ld is below the chunk's %ld rows", ld, Rc);
  hipLaunchKernelGGL(k_ideal_softmax, dim3((unsigned)Q), dim3(256), 0, st, S, ld, (int)Rc, ref_base, ref_labels, labels, state);
  EDM_CHECK_LAUNCH("ideal_softmax");
  return EDM_OK;
}

// acc[q][k] = alpha_q acc[q][k] + sum_j p[q][j] (refs[j][k] - 128): the chunk's share of the output, in grey levels, with
// the rescaling edm_ideal_softmax left in the state.  first != 0: acc is written, not read (the first chunk of a call).
// P: the weights (16-byte aligned, ld % 4 == 0); refs as edm_ideal_logits (vector path: refs 16-byte aligned, K % 16 == 0).
extern "C" int edm_ideal_accumulate(const float* P, long ld, const void* refs, const float* state, long Q, long Rc, int K,
                                    int first, float* acc, hipStream_t st) {
  EDM_REQUIRE(P && refs && state && acc, "ideal_accumulate: null pointer");
  EDM_REQUIRE(Q >= 1 && Q <= ID_MAX_Q, "ideal_accumulate: Q must be in [1, %ld], got %ld", ID_MAX_Q, Q);
  EDM_REQUIRE(K >= 1 && K <= ID_MAX_K, "ideal_accumulate: K must be in [1, %d], got %d", ID_MAX_K, K);
  EDM_REQUIRE(Rc >= 1 && Rc <= ID_MAX_R, "ideal_accumulate: the chunk must hold 1 to 2^31 - 128 rows, got %ld", Rc);
  EDM_REQUIRE(ld >= Rc && ld % 4 == 0 && ((uintptr_t)P & 15) == 0,
              "ideal_accumulate: the weights need 16-byte aligned rows of ld %% 4 == 0 >= Rc floats, got ld = %ld", ld);
  const dim3 grid((unsigned)((K + ID_AN - 1) / ID_AN), (unsigned)((Q + ID_AQ - 1) / ID_AQ));
  if (ideal_vec(P, refs, K))
    hipLaunchKernelGGL((k_ideal_accumulate<true, ID_AQ, ID_AN>), grid, dim3(256), 0, st, P, ld, (const unsigned char*)refs, state, (int)Q,
                       (int)Rc, K, first, acc);
  else
    hipLaunchKernelGGL((k_ideal_accumulate<false, ID_AQ, ID_AN>), grid, dim3(256), 0, st, P, ld, (const unsigned char*)refs, state, (int)Q,
                       (int)Rc, K, first, acc);
  EDM_CHECK_LAUNCH("ideal_accumulate");
  return EDM_OK;
}

// D[q][k] = acc[q][k] / (255 std s_q) + (128 / 255 - mean) / std (D may be acc itself) and lse, ent, top_w fp32 [Q],
// top_idx int32 [Q] from the final state.  Bad rows: NaN and -1.  Sets the health bit on a non-finite output.
extern "C" int edm_ideal_finish(const float* acc, const float* state, long Q, int K, float mean, float stdv, float* D,
                                float* lse, float* ent, float* top_w, int* top_idx, unsigned* health, hipStream_t st) {
  EDM_REQUIRE(acc && state && D && lse && ent && top_w && top_idx, "ideal_finish: null pointer");
  EDM_REQUIRE(Q >= 1 && Q <= ID_MAX_Q, "ideal_finish: Q must be in [1, %ld], got %ld", ID_MAX_Q, Q);
  EDM_REQUIRE(K >= 1 && K <= ID_MAX_K, "ideal_finish: K must be in [1, %d], got %d", ID_MAX_K, K);
  IDEAL_NORM_ARGS("ideal_finish");
  const IdealNorm n = ideal_norm(mean, stdv);
  hipLaunchKernelGGL(k_ideal_finish, dim3((unsigned)Q), dim3(256), 0, st, acc, state, K, n.a, n.c, D, lse, ent, top_w, top_idx,
                     health);
  EDM_CHECK_LAUNCH("ideal_finish");
  return EDM_OK;
}
