// Per-sample evaluation kernels on the quads of quads.h: the likelihood along the probability-flow ODE (Hutchinson probes,
// the Heun updates with the divergence term, the Gaussian prior) and the loss by noise level (the diffusion that belongs
// to an image, the order-fixed squared error and their class-sweep forms).
#include "common.h"
#include "quads.h"

#include <math.h>
#include <cmath>

namespace {

// Likelihood evaluation along the probability-flow ODE: the Heun updates (solver_steps.hip) plus the divergence of the drift,
// estimated without a backward pass (Hutchinson, Rademacher probes, central difference through the network):
//   q_b = 1/K sum_p sum_j eps_pj (D(x + h eps_p)_bj - D(x - h eps_p)_bj) / (2h)  ~  tr dD/dx,   L_b += c (CHW - q_b) / t.
// The evaluation batch E is [(1 + 2K) B, CHW]: rows [0, B) hold x, rows [(1 + 2p) B, (2 + 2p) B) x + h eps_p and rows
// [(2 + 2p) B, (3 + 2p) B) x - h eps_p; D is the network's output on it.  eps is never stored: element j = 4q + k of
// sample b takes bit p of word k of
//   philox4x32_10(ctr = (q, b, (0x4E4C0000 + (ev << 16)) ^ step, solve_index), key = (seed_lo, seed_hi)),
// bit clear = +1, set = -1; ev = 0 for the Euler evaluation of a step, 1 for its correction, p < 32 the probe.  The tags
// 0x4E4C / 0x4E4D differ from the churn's 0x4348 and the blend's 0x4950 in the high half for every step < 2^16.  x +- h
// is one fp32 add (no product to contract).  VEC: CHW % 4 == 0 and every operand 16-byte aligned -> dwordx4 per quad,
// otherwise the same quads element by element (the last quad of a sample may be partial); both draw the same bits.
// The per-sample sums are order-fixed: workgroup (chunk, b) sums its quads of sample b in fp64 (thread-serial, then the
// xor butterfly of whole waves, then four wave totals in index order) into part[b][chunk]; k_nll_finish adds a sample's
// chunks in index order and updates L_b, fp64.  No atomics on floating point, no dependence on arrival order.
constexpr uint32_t NLL_TAG = 0x4E4C0000u;

__device__ __forceinline__ void nll_words(uint32_t (&w)[4], long q, long b, uint32_t ev, uint32_t step,
                                          const uint32_t* __restrict__ rec) {
  const Philox4 r = philox4x32_10((uint32_t)q, (uint32_t)b, (NLL_TAG + (ev << 16)) ^ step, rec[2], rec[0], rec[1]);
  w[0] = r.x; w[1] = r.y; w[2] = r.z; w[3] = r.w;
}
// the probes of one quad: E[(1 + 2p) rows + e] = o + s, E[(2 + 2p) rows + e] = o - s, s = +-h by bit p of w[k]
template <bool VEC>
__device__ __forceinline__ void nll_write_probes(float* __restrict__ E, long rows, long e, int m, const float (&o)[4],
                                                 const uint32_t (&w)[4], float h, int K, bool& bad) {
  for (int p = 0; p < K; ++p) {
    float pl[4], mi[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float s = ((w[k] >> p) & 1u) ? -h : h;
      pl[k] = o[k] + s;
      mi[k] = o[k] - s;
      bad |= nonfinite(pl[k]) || nonfinite(mi[k]);
    }
    store4<VEC>(E + (1 + 2 * p) * rows + e, m, pl);
    store4<VEC>(E + (2 + 2 * p) * rows + e, m, mi);
  }
}
// sum_p sum_k eps_pk (D+ - D-) of one quad; the difference is taken in fp64 (exact), the sign is a select
template <bool VEC>
__device__ __forceinline__ double nll_quad_dot(const float* __restrict__ Dn, long rows, long e, int m,
                                               const uint32_t (&w)[4], int K) {
  double acc = 0.0;
  for (int p = 0; p < K; ++p) {
    float dp[4], dm[4];
    load4<VEC>(Dn + (1 + 2 * p) * rows + e, m, dp);
    load4<VEC>(Dn + (2 + 2 * p) * rows + e, m, dm);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const double dd = (double)dp[k] - (double)dm[k];
      acc += ((w[k] >> p) & 1u) ? -dd : dd;
    }
  }
  return acc;
}
// grid (B * nq quads, grid-stride); writes the evaluation batch of x
template <bool VEC>
__global__ __launch_bounds__(256) void k_nll_probe(const float* __restrict__ x, float h, const uint32_t* __restrict__ rec,
                                                   uint32_t step, uint32_t ev, int K, int B, long CHW,
                                                   float* __restrict__ E, unsigned* __restrict__ health) {
  const long nq = (CHW + 3) / 4, total = (long)B * nq, rows = (long)B * CHW;
  bool bad = false;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const long b = i / nq, q = i - b * nq, e = b * CHW + 4 * q;
    const int m = quad_len<VEC>(CHW, q);
    uint32_t w[4];
    nll_words(w, q, b, ev, step, rec);
    float xv[4];
    load4<VEC>(x + e, m, xv);
#pragma unroll
    for (int k = 0; k < 4; ++k) bad |= nonfinite(xv[k]);
    store4<VEC>(E + e, m, xv);
    nll_write_probes<VEC>(E, rows, e, m, xv, w, h, K, bad);
  }
  EDM_RAISE_HEALTH(health, bad, 2u);
}
// grid (chunks, B), 256 threads.  k_heun_euler's update on rows [0, B) of (E, D): dx, and x1 with its probes (+-h1,
// evaluation 1 of the step) into E1; part[b][chunk] = this chunk's share of sum eps (D+ - D-) under evaluation 0
template <bool VEC>
__global__ __launch_bounds__(256) void k_heun_euler_div(const float* __restrict__ E, const float* __restrict__ Dn, float t0,
                                                        float t1, float h1, const uint32_t* __restrict__ rec,
                                                        uint32_t step, int K, int B, long CHW, float* __restrict__ dx,
                                                        float* __restrict__ E1, double* __restrict__ part,
                                                        unsigned* __restrict__ health) {
  const long nq = (CHW + 3) / 4, rows = (long)B * CHW, b = blockIdx.y;
  bool bad = false;
  double acc = 0.0;
  for (long q = (long)blockIdx.x * 256 + threadIdx.x; q < nq; q += (long)gridDim.x * 256) {
    const long e = b * CHW + 4 * q;
    const int m = quad_len<VEC>(CHW, q);
    uint32_t w0[4], w1[4];
    nll_words(w0, q, b, 0u, step, rec);
    nll_words(w1, q, b, 1u, step, rec);
    float xv[4], dv[4], d[4], o[4];
    load4<VEC>(E + e, m, xv);
    load4<VEC>(Dn + e, m, dv);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      o[k] = heun_euler_stage(xv[k], dv[k], t0, t1, d[k]);
      bad |= nonfinite(o[k]);
    }
    store4<VEC>(dx + e, m, d);
    store4<VEC>(E1 + e, m, o);
    nll_write_probes<VEC>(E1, rows, e, m, o, w1, h1, K, bad);
    acc += nll_quad_dot<VEC>(Dn, rows, e, m, w0, K);
  }
  block_partial(acc, part + b * EDM_NLL_MAX_CHUNKS + blockIdx.x);
  EDM_RAISE_HEALTH(health, bad, 2u);
}
// k_heun_correct's update on rows [0, B) of (E, E1, D1) into rows [0, B) of out, with the probes of the NEXT step's
// Euler evaluation (+-hn, step - 1, evaluation 0) when Kout == K (Kout == 0: out is [B, CHW], the solve's last state);
// part[b][chunk] = this chunk's share of sum eps (D1+ - D1-) under evaluation 1 of this step
template <bool VEC>
__global__ __launch_bounds__(256) void k_heun_correct_div(const float* __restrict__ E, const float* __restrict__ dx,
                                                          const float* __restrict__ E1, const float* __restrict__ D1,
                                                          float t0, float t1, float hn,
                                                          const uint32_t* __restrict__ rec, uint32_t step, int K,
                                                          int Kout, int B, long CHW, float* __restrict__ out,
                                                          double* __restrict__ part, unsigned* __restrict__ health) {
  const long nq = (CHW + 3) / 4, rows = (long)B * CHW, b = blockIdx.y;
  bool bad = false;
  double acc = 0.0;
  for (long q = (long)blockIdx.x * 256 + threadIdx.x; q < nq; q += (long)gridDim.x * 256) {
    const long e = b * CHW + 4 * q;
    const int m = quad_len<VEC>(CHW, q);
    uint32_t w1[4];
    nll_words(w1, q, b, 1u, step, rec);
    float xv[4], dxv[4], x1v[4], d1[4], o[4];
    load4<VEC>(E + e, m, xv);
    load4<VEC>(dx + e, m, dxv);
    load4<VEC>(E1 + e, m, x1v);
    load4<VEC>(D1 + e, m, d1);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      o[k] = heun_update(xv[k], heun_slope(dxv[k], x1v[k], d1[k], t1), t0, t1);
      bad |= nonfinite(o[k]);
    }
    store4<VEC>(out + e, m, o);
    if (Kout) {
      uint32_t wn[4];
      nll_words(wn, q, b, 0u, step - 1u, rec);
      nll_write_probes<VEC>(out, rows, e, m, o, wn, hn, Kout, bad);
    }
    acc += nll_quad_dot<VEC>(D1, rows, e, m, w1, K);
  }
  block_partial(acc, part + b * EDM_NLL_MAX_CHUNKS + blockIdx.x);
  EDM_RAISE_HEALTH(health, bad, 2u);
}
// part[b][chunk] = this chunk's share of sum_j (x_bj * inv_t)^2: the Gaussian prior's quadratic form
template <bool VEC>
__global__ __launch_bounds__(256) void k_nll_prior(const float* __restrict__ x, double inv_t, long CHW,
                                                   double* __restrict__ part) {
  const long nq = (CHW + 3) / 4, b = blockIdx.y;
  double acc = 0.0;
  for (long q = (long)blockIdx.x * 256 + threadIdx.x; q < nq; q += (long)gridDim.x * 256) {
    const int m = quad_len<VEC>(CHW, q);
    float xv[4];
    load4<VEC>(x + b * CHW + 4 * q, m, xv);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const double v = (double)xv[k] * inv_t;
      acc = fma(v, v, acc);
    }
  }
  block_partial(acc, part + b * EDM_NLL_MAX_CHUNKS + blockIdx.x);
}
// L_b += c0 + c1 * (part[b][0] + part[b][1] + ... in index order), one thread per sample; health bit 1 on a non-finite L
__global__ __launch_bounds__(64) void k_nll_finish(const double* __restrict__ part, int chunks, int B, double c0,
                                                   double c1, double* __restrict__ L, unsigned* __restrict__ health) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  bool bad = false;
  if (b < B) {
    const double s = chunk_sum(part + (long)b * EDM_NLL_MAX_CHUNKS, chunks);
    const double v = L[b] + fma(c1, s, c0);
    L[b] = v;
    bad = !(fabs(v) <= 1.0e300);
  }
  EDM_RAISE_HEALTH(health, bad, 2u);
}
// Loss by noise level (evaluate.py): noisy_b = clean_b + sigma_b * n with sigma_b = sigmas[level[b]] and n ~ N(0, 1) that
// belongs to the IMAGE ids[b], not to the row b: element j = 4q + k of sample b takes normal k of
//   philox4x32_10(ctr = (q, ids[b], 0x45560000 ^ level[b], draw), key = (seed_lo, seed_hi)),
// Box-Muller of words (0, 1) and (2, 3) as k_heun_churn; rec = {seed_lo, seed_hi, draw, 0} is the churn's device record.
// level < 65536 keeps the tag's high half 0x4556 apart from 0x4348 (churn), 0x4950 (blend), 0x4E4C / 0x4E4D (likelihood
// probes) and from the 16-bit tags 0xD1FF / 0x5167 (high half 0).  The noise of (id, level, draw) depends neither on B,
// on the row, on the row's neighbours nor on the memory path.  A level outside [0, L) is never used as an index: the
// sample's sigma and outputs become NaN and the health bit is set (ops refuses such a level before the launch).
// C (the row divisor of the class sweep, classify.py): pair b is drawn once per element and stored to the C rows b * C + c
// of noisy / sigma_out, each with the bits of the C = 1 form; edm_eval_diffuse is C = 1.
template <bool VEC>
__global__ __launch_bounds__(256) void k_eval_diffuse(const float* __restrict__ clean, const uint32_t* __restrict__ ids,
                                                      const int* __restrict__ level, const float* __restrict__ sigmas,
                                                      int L, const uint32_t* __restrict__ rec, int B, int C, long CHW,
                                                      float* __restrict__ noisy, float* __restrict__ sigma_out,
                                                      unsigned* __restrict__ health) {
  const uint32_t seed_lo = rec[0], seed_hi = rec[1], draw = rec[2];
  const long nq = (CHW + 3) / 4, total = (long)B * nq;
  bool bad = false;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const long b = i / nq, q = i - b * nq;
    const int lv = level[b];
    const bool lv_ok = lv >= 0 && lv < L;
    const float s = lv_ok ? sigmas[lv] : __builtin_nanf("");
    if (q == 0)
      for (int c = 0; c < C; ++c) sigma_out[b * C + c] = s;
    bad |= !lv_ok;
    const Philox4 r = philox4x32_10((uint32_t)q, ids[b], 0x45560000u ^ (uint32_t)lv, draw, seed_lo, seed_hi);
    float nn[4], xv[4], ov[4];
    box_muller(r.x, r.y, nn[0], nn[1]);
    box_muller(r.z, r.w, nn[2], nn[3]);
    const int m = quad_len<VEC>(CHW, q);
    load4<VEC>(clean + b * CHW + 4 * q, m, xv);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      ov[k] = fmaf(s, nn[k], xv[k]);
      bad |= k < m && nonfinite(ov[k]);
    }
    for (int c = 0; c < C; ++c) store4<VEC>(noisy + (b * C + c) * CHW + 4 * q, m, ov);
  }
  EDM_RAISE_HEALTH(health, bad, 2u);
}
// part[b][chunk] = this chunk's share of sum_j ((double)D_bj - (double)clean_bj)^2.  The difference of two fp32 values
// is exact in fp64.  grid (sample_chunks(CHW), B): a sample's chunking, and with it the order of every add, depends on CHW
// alone, so se[b] has the same bits whatever B, the row or the memory path (the padding of a partial quad adds +0.0).
// C (the row divisor of the class sweep): row b of D is compared with row b / C of clean, which is never replicated;
// edm_eval_sqerr is C = 1.
template <bool VEC>
__global__ __launch_bounds__(256) void k_eval_sqerr(const float* __restrict__ D, const float* __restrict__ clean, int C,
                                                    long CHW, double* __restrict__ part) {
  const long nq = (CHW + 3) / 4, b = blockIdx.y, p = b / C;
  double acc = 0.0;
  for (long q = (long)blockIdx.x * 256 + threadIdx.x; q < nq; q += (long)gridDim.x * 256) {
    const int m = quad_len<VEC>(CHW, q);
    float dv[4], cv[4];
    load4<VEC>(D + b * CHW + 4 * q, m, dv);
    load4<VEC>(clean + p * CHW + 4 * q, m, cv);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const double d = (double)dv[k] - (double)cv[k];
      acc = fma(d, d, acc);
    }
  }
  block_partial(acc, part + b * EDM_NLL_MAX_CHUNKS + blockIdx.x);
}
// se[b] = part[b][0] + part[b][1] + ... in index order (written, not accumulated); health bit 1 on a non-finite se
__global__ __launch_bounds__(64) void k_eval_sqerr_finish(const double* __restrict__ part, int chunks, int B,
                                                          double* __restrict__ se, unsigned* __restrict__ health) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  bool bad = false;
  if (b < B) {
    const double s = chunk_sum(part + (long)b * EDM_NLL_MAX_CHUNKS, chunks);
    se[b] = s;
    bad = !(fabs(s) <= 1.0e300);
  }
  EDM_RAISE_HEALTH(health, bad, 2u);
}

}  // namespace

inline void launch_eval_diffuse(const float* clean, const unsigned* ids, const int* level, const float* sigmas, int L,
                                const void* rec, int P, int C, long CHW, float* noisy, float* sigma_out,
                                unsigned* health, hipStream_t st) {
  const dim3 grid(grid_for((long)P * ((CHW + 3) / 4), 256)), block(256);
  if (CHW % 4 == 0 && aligned16({clean, noisy}))
    hipLaunchKernelGGL(k_eval_diffuse<true>, grid, block, 0, st, clean, (const uint32_t*)ids, level, sigmas, L,
                       (const uint32_t*)rec, P, C, CHW, noisy, sigma_out, health);
  else
    hipLaunchKernelGGL(k_eval_diffuse<false>, grid, block, 0, st, clean, (const uint32_t*)ids, level, sigmas, L,
                       (const uint32_t*)rec, P, C, CHW, noisy, sigma_out, health);
}
// rows = the rows of D and se; row b is compared with row b / C of clean
inline void launch_eval_sqerr(const float* D, const float* clean, int rows, int C, long CHW, double* part, double* se,
                              unsigned* health, hipStream_t st) {
  const int chunks = sample_chunks(CHW);
  const dim3 grid(chunks, rows), block(256);
  if (CHW % 4 == 0 && aligned16({D, clean}))
    hipLaunchKernelGGL(k_eval_sqerr<true>, grid, block, 0, st, D, clean, C, CHW, part);
  else
    hipLaunchKernelGGL(k_eval_sqerr<false>, grid, block, 0, st, D, clean, C, CHW, part);
  hipLaunchKernelGGL(k_eval_sqerr_finish, dim3((rows + 63) / 64), dim3(64), 0, st, (const double*)part, chunks, rows, se,
                     health);
}
// ids [B] uint32, level [B] int32, sigmas [L] float: DEVICE arrays; rec: the churn's device record with the draw in word 2
extern "C" int edm_eval_diffuse(const float* clean, const unsigned* ids, const int* level, const float* sigmas, int L,
                                const void* rec, int B, long CHW, float* noisy, float* sigma_out, unsigned* health,
                                hipStream_t st) {
  EDM_REQUIRE(clean && ids && level && sigmas && rec && noisy && sigma_out && B > 0 && CHW > 0 && L >= 1 && L <= 65535,
              "eval_diffuse: bad args (1 <= L <= 65535)");
  EDM_REQUIRE((CHW + 3) / 4 <= 0xFFFFFFFFL, "eval_diffuse: CHW / 4 must fit the 32-bit Philox counter word");
  launch_eval_diffuse(clean, ids, level, sigmas, L, rec, B, 1, CHW, noisy, sigma_out, health, st);
  EDM_CHECK_LAUNCH("eval_diffuse");
  return EDM_OK;
}
// part: device workspace of B * EDM_NLL_MAX_CHUNKS doubles; se: device fp64 [B], written
extern "C" int edm_eval_sqerr(const float* D, const float* clean, int B, long CHW, double* part, double* se,
                              unsigned* health, hipStream_t st) {
  EDM_REQUIRE(D && clean && part && se && B > 0 && B <= 65535 && CHW > 0, "eval_sqerr: bad args (B <= 65535)");
  launch_eval_sqerr(D, clean, B, 1, CHW, part, se, health, st);
  EDM_CHECK_LAUNCH("eval_sqerr");
  return EDM_OK;
}
// the class sweep (classify.py): P pairs x C classes, row p * C + c; ids / level [P]; noisy [P * C, CHW], sigma_out [P * C]
extern "C" int edm_eval_diffuse_classes(const float* clean, const unsigned* ids, const int* level, const float* sigmas,
                                        int L, const void* rec, int P, int C, long CHW, float* noisy, float* sigma_out,
                                        unsigned* health, hipStream_t st) {
  EDM_REQUIRE(clean && ids && level && sigmas && rec && noisy && sigma_out && P > 0 && C > 0 && CHW > 0 && L >= 1 &&
                  L <= 65535 && (long)P * C <= 0x7FFFFFFFL,
              "eval_diffuse_classes: bad args (1 <= L <= 65535, P * C < 2^31)");
  EDM_REQUIRE((CHW + 3) / 4 <= 0xFFFFFFFFL, "eval_diffuse_classes: CHW / 4 must fit the 32-bit Philox counter word");
  launch_eval_diffuse(clean, ids, level, sigmas, L, rec, P, C, CHW, noisy, sigma_out, health, st);
  EDM_CHECK_LAUNCH("eval_diffuse_classes");
  return EDM_OK;
}
// part: device workspace of P * C * EDM_NLL_MAX_CHUNKS doubles; se: device fp64 [P * C], written; clean [P, CHW]
extern "C" int edm_eval_sqerr_classes(const float* D, const float* clean, int P, int C, long CHW, double* part,
                                      double* se, unsigned* health, hipStream_t st) {
  EDM_REQUIRE(D && clean && part && se && P > 0 && C > 0 && (long)P * C <= 65535 && CHW > 0,
              "eval_sqerr_classes: bad args (P * C <= 65535)");
  launch_eval_sqerr(D, clean, P * C, C, CHW, part, se, health, st);
  EDM_CHECK_LAUNCH("eval_sqerr_classes");
  return EDM_OK;
}
// Likelihood evaluation (see the kernels).  E / D / E1 / D1: [(1 + 2K) B, CHW] fp32, rows [0, B) the state; rec: the
// churn's device record; part: device workspace of B * EDM_NLL_MAX_CHUNKS doubles; L: device fp64 [B], += in place.
static bool nll_common_ok(const void* rec, int step, int K, int B, long CHW) {
  return rec && step >= 0 && step < 65536 && K >= 1 && K <= 32 && B > 0 && B <= 65535 && CHW > 0 &&
         (CHW + 3) / 4 <= 0xFFFFFFFFL;
}
extern "C" int edm_nll_probe(const float* x, float h, const void* rec, int step, int ev, int K, int B, long CHW, float* E,
                             unsigned* health, hipStream_t st) {
  EDM_REQUIRE(x && E && nll_common_ok(rec, step, K, B, CHW) && (ev == 0 || ev == 1) && std::isfinite(h) && h > 0.f,
              "nll_probe: bad args (step < 65536, 1 <= K <= 32, ev in {0, 1}, h > 0)");
  const bool vec = CHW % 4 == 0 && aligned16({x, E});
  const dim3 grid(grid_for((long)B * ((CHW + 3) / 4), 256)), block(256);
  if (vec)
    hipLaunchKernelGGL(k_nll_probe<true>, grid, block, 0, st, x, h, (const uint32_t*)rec, (uint32_t)step, (uint32_t)ev, K,
                       B, CHW, E, health);
  else
    hipLaunchKernelGGL(k_nll_probe<false>, grid, block, 0, st, x, h, (const uint32_t*)rec, (uint32_t)step, (uint32_t)ev,
                       K, B, CHW, E, health);
  EDM_CHECK_LAUNCH("nll_probe");
  return EDM_OK;
}
static int nll_finish(const double* part, int chunks, int B, double c0, double c1, double* L, unsigned* health,
                      hipStream_t st, const char* name) {
  hipLaunchKernelGGL(k_nll_finish, dim3((B + 63) / 64), dim3(64), 0, st, part, chunks, B, c0, c1, L, health);
  EDM_CHECK_LAUNCH(name);
  return EDM_OK;
}
extern "C" int edm_heun_euler_div(const float* E, const float* D, float t0, float t1, float h0, float h1, const void* rec,
                                  int step, int K, int B, long CHW, float* dx, float* E1, double* part, double* L,
                                  unsigned* health, hipStream_t st) {
  EDM_REQUIRE(E && D && dx && E1 && part && L && nll_common_ok(rec, step, K, B, CHW) && t0 > 0.f && std::isfinite(t0) &&
              std::isfinite(t1) && std::isfinite(h0) && h0 > 0.f && std::isfinite(h1) && h1 > 0.f,
              "heun_euler_div: bad args (step < 65536, 1 <= K <= 32, t0 > 0, h0 > 0, h1 > 0)");
  const bool vec = CHW % 4 == 0 && aligned16({E, D, dx, E1});
  const int chunks = sample_chunks(CHW);
  const dim3 grid(chunks, B), block(256);
  if (vec)
    hipLaunchKernelGGL(k_heun_euler_div<true>, grid, block, 0, st, E, D, t0, t1, h1, (const uint32_t*)rec, (uint32_t)step,
                       K, B, CHW, dx, E1, part, health);
  else
    hipLaunchKernelGGL(k_heun_euler_div<false>, grid, block, 0, st, E, D, t0, t1, h1, (const uint32_t*)rec,
                       (uint32_t)step, K, B, CHW, dx, E1, part, health);
  EDM_CHECK_LAUNCH("heun_euler_div");
  // L += (t1 - t0) / 2 * (CHW - q) / t0,  q = sum / (2 h0 K)
  const double c = ((double)t1 - (double)t0) * 0.5 / (double)t0;
  return nll_finish(part, chunks, B, c * (double)CHW, -c / (2.0 * (double)h0 * (double)K), L, health, st,
                    "heun_euler_div (finish)");
}
extern "C" int edm_heun_correct_div(const float* E, const float* dx, const float* E1, const float* D1, float t0, float t1,
                                    float h1, float hn, const void* rec, int step, int K, int probes_out, int B,
                                    long CHW, float* out, double* part, double* L, unsigned* health, hipStream_t st) {
  EDM_REQUIRE(E && dx && E1 && D1 && out && part && L && nll_common_ok(rec, step, K, B, CHW) && t1 > 0.f &&
              std::isfinite(t0) && std::isfinite(t1) && std::isfinite(h1) && h1 > 0.f &&
              (!probes_out || (step >= 1 && std::isfinite(hn) && hn > 0.f)),
              "heun_correct_div: bad args (step < 65536, 1 <= K <= 32, t1 > 0, h1 > 0; probes_out needs step >= 1, hn > 0)");
  const bool vec = CHW % 4 == 0 && aligned16({E, dx, E1, D1, out});
  const int chunks = sample_chunks(CHW);
  const dim3 grid(chunks, B), block(256);
  const int Kout = probes_out ? K : 0;
  if (vec)
    hipLaunchKernelGGL(k_heun_correct_div<true>, grid, block, 0, st, E, dx, E1, D1, t0, t1, hn, (const uint32_t*)rec,
                       (uint32_t)step, K, Kout, B, CHW, out, part, health);
  else
    hipLaunchKernelGGL(k_heun_correct_div<false>, grid, block, 0, st, E, dx, E1, D1, t0, t1, hn, (const uint32_t*)rec,
                       (uint32_t)step, K, Kout, B, CHW, out, part, health);
  EDM_CHECK_LAUNCH("heun_correct_div");
  const double c = ((double)t1 - (double)t0) * 0.5 / (double)t1;
  return nll_finish(part, chunks, B, c * (double)CHW, -c / (2.0 * (double)h1 * (double)K), L, health, st,
                    "heun_correct_div (finish)");
}
extern "C" int edm_nll_prior(const float* x, float t, int B, long CHW, double* part, double* L, unsigned* health,
                             hipStream_t st) {
  EDM_REQUIRE(x && part && L && B > 0 && B <= 65535 && CHW > 0 && std::isfinite(t) && t > 0.f, "nll_prior: bad args");
  const bool vec = CHW % 4 == 0 && aligned16({x});
  const int chunks = sample_chunks(CHW);
  const dim3 grid(chunks, B), block(256);
  const double inv_t = 1.0 / (double)t;
  if (vec)
    hipLaunchKernelGGL(k_nll_prior<true>, grid, block, 0, st, x, inv_t, CHW, part);
  else
    hipLaunchKernelGGL(k_nll_prior<false>, grid, block, 0, st, x, inv_t, CHW, part);
  EDM_CHECK_LAUNCH("nll_prior");
  // log N(x; 0, t^2 I) = -CHW/2 log(2 pi t^2) - sum (x / t)^2 / 2
  const double c0 = -0.5 * (double)CHW * log(2.0 * 3.14159265358979323846 * (double)t * (double)t);
  return nll_finish(part, chunks, B, c0, -0.5, L, health, st, "nll_prior (finish)");
}
// host logic only: the chunk rule of quads.h for the Python side, which sizes `part` workspaces with it
extern "C" int edm_sample_chunks(long CHW) { return CHW > 0 ? sample_chunks(CHW) : 0; }
