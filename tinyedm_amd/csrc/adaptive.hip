// Adaptive integration of the probability-flow ODE: the embedded Heun(2) / Euler(1) pair with local extrapolation and a
// step controller that lives on the device.  Every sample carries its own time and step size, so the Heun updates of
// solver_steps.hip (t0, t1 by value for the whole batch) appear here with the times read per sample; both evaluate the
// step functions of quads.h (as k_heun_euler_div / k_heun_correct_div do), so a batch whose samples all sit at one pair
// (t0, t1) gets the bits of edm_heun_euler / edm_heun_correct.
//
// Per-sample state: EDM_ADAPT_ROWS rows of B 32-bit words, row r at state + r * B (include/tinyedm_hip.h):
//   T, T1, H, ERR fp32; STATUS (0 active, 1 done, 2 failed), ACCEPTED, REJECTED, AFTER_REJECT uint32.
// A sample that is not active has t1 == t: the update kernels then copy x through (dx = 0, y = x) whatever D holds, and
// its error partials are +0.
//
// The error norm is order-fixed, as edm_eval_sqerr's (block_partial and chunk_sum of quads.h): the controller adds a
// sample's chunks in index order.  The chunking depends on CHW alone.  No atomics on floating point.
#include "common.h"
#include "quads.h"

#include <cmath>

namespace {

enum { ROW_T = 0, ROW_T1, ROW_H, ROW_ERR, ROW_STATUS, ROW_ACCEPTED, ROW_REJECTED, ROW_AFTER_REJECT, ADAPT_ROWS };
enum : uint32_t { ST_ACTIVE = 0, ST_DONE = 1, ST_FAILED = 2 };

// the snap rule: the trial time of a step of h from t towards t_end.  When t + h passes t_end, or comes within 1 % of
// |h| of it, the step ends on t_end exactly (a sliver of a last step is never taken)
__device__ __forceinline__ float snap_t1(float t, float h, float t_end) {
  const double tn = (double)t + (double)h, te = (double)t_end;
  const bool passes = h > 0.f ? tn >= te : tn <= te;
  const bool close_by = fabs(te - tn) <= 0.01 * fabs((double)h);
  return (passes || close_by) ? t_end : (float)tn;
}

__global__ __launch_bounds__(64) void k_adapt_begin(float t_start, float t_end, float h0, int B,
                                                    uint32_t* __restrict__ state) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= B) return;
  float* sf = reinterpret_cast<float*>(state);
  sf[ROW_T * B + b] = t_start;
  sf[ROW_T1 * B + b] = snap_t1(t_start, h0, t_end);
  sf[ROW_H * B + b] = h0;
  sf[ROW_ERR * B + b] = 0.f;
  state[ROW_STATUS * B + b] = ST_ACTIVE;
  state[ROW_ACCEPTED * B + b] = 0u;
  state[ROW_REJECTED * B + b] = 0u;
  state[ROW_AFTER_REJECT * B + b] = 0u;
}

// k_heun_euler with t0 = t[b], t1 = t1[b]: dx = (x - D) / t0, x1 = x + (t1 - t0) * dx.  grid-stride over B * nq quads
template <bool VEC>
__global__ __launch_bounds__(256) void k_adapt_euler(const float* __restrict__ x, const float* __restrict__ Dn,
                                                     const float* __restrict__ t, const float* __restrict__ t1, int B,
                                                     long CHW, float* __restrict__ dx, float* __restrict__ x1,
                                                     unsigned* __restrict__ health) {
  const long nq = (CHW + 3) / 4, total = (long)B * nq;
  bool bad = false;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const long b = i / nq, q = i - b * nq, e = b * CHW + 4 * q;
    const int m = quad_len<VEC>(CHW, q);
    const float t0 = t[b], tn = t1[b];
    float xv[4], d[4], o[4];
    load4<VEC>(x + e, m, xv);
    if (tn == t0) {             // not active: the state rides along untouched
#pragma unroll
      for (int k = 0; k < 4; ++k) { d[k] = 0.f; o[k] = xv[k]; }
    } else {
      float dv[4];
      load4<VEC>(Dn + e, m, dv);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        o[k] = heun_euler_stage(xv[k], dv[k], t0, tn, d[k]);
        bad |= nonfinite(o[k]);
      }
    }
    store4<VEC>(dx + e, m, d);
    store4<VEC>(x1 + e, m, o);
  }
  EDM_RAISE_HEALTH(health, bad, 2u);
}

// grid (chunks, B).  k_heun_correct with the times of sample b: y = x + (t1 - t0) * (0.5 dx + 0.5 (x1 - D1) / t1), and
// part[b][chunk] = this chunk's share of sum_j ((y_j - x1_j) / (atol + rtol max(|x_j|, |y_j|)))^2, every term in fp64 from
// the fp32 values (the difference of two fp32 values is exact in fp64; the padding of a partial quad adds +0.0)
template <bool VEC>
__global__ __launch_bounds__(256) void k_adapt_correct(const float* __restrict__ x, const float* __restrict__ dx,
                                                       const float* __restrict__ x1, const float* __restrict__ D1,
                                                       const float* __restrict__ t, const float* __restrict__ t1, long CHW,
                                                       double atol, double rtol, float* __restrict__ y,
                                                       double* __restrict__ part, unsigned* __restrict__ health) {
  const long nq = (CHW + 3) / 4, b = blockIdx.y;
  const float t0 = t[b], tn = t1[b];
  const bool active = tn != t0;
  bool bad = false;
  double acc = 0.0;
  for (long q = (long)blockIdx.x * 256 + threadIdx.x; q < nq; q += (long)gridDim.x * 256) {
    const long e = b * CHW + 4 * q;
    const int m = quad_len<VEC>(CHW, q);
    float xv[4], o[4];
    load4<VEC>(x + e, m, xv);
    if (active) {
      float dxv[4], x1v[4], d1[4];
      load4<VEC>(dx + e, m, dxv);
      load4<VEC>(x1 + e, m, x1v);
      load4<VEC>(D1 + e, m, d1);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        o[k] = heun_update(xv[k], heun_slope(dxv[k], x1v[k], d1[k], tn), t0, tn);
        bad |= nonfinite(o[k]);
        const double sc = fma(rtol, fmax(fabs((double)xv[k]), fabs((double)o[k])), atol);
        const double r = ((double)o[k] - (double)x1v[k]) / sc;
        if (k < m) acc = fma(r, r, acc);
      }
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) o[k] = xv[k];
    }
    store4<VEC>(y + e, m, o);
  }
  block_partial(acc, part + b * EDM_NLL_MAX_CHUNKS + blockIdx.x);
  EDM_RAISE_HEALTH(health, bad, 2u);
}

// One thread per sample, fp64.  E = sqrt(sum of the sample's partials in index order / CHW); accept iff E <= 1 (a NaN E
// rejects); factor = clamp(safety / sqrt(E), fac_min, fac_max), fac_max replaced by 1 on a rejection and on the step after
// one; h <- (t1 - t) * factor; on accept t <- t1, done when t == t_end.  |h| < h_floor |t| fails the sample (health bit 1).
// Then the next t1 by the snap rule (t1 = t for a sample that is not active), the accept byte, and the number of samples
// still active added to *active (one integer atomic per wave).
__global__ __launch_bounds__(64) void k_adapt_control(const double* __restrict__ part, int chunks, int B, long CHW,
                                                      float t_end, double safety, double fac_min, double fac_max,
                                                      double h_floor, uint32_t* __restrict__ state,
                                                      unsigned char* __restrict__ accept, int* __restrict__ active,
                                                      unsigned* __restrict__ health) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  float* sf = reinterpret_cast<float*>(state);
  bool failed = false, still = false;
  if (b < B) {
    uint32_t status = state[ROW_STATUS * B + b];
    unsigned char acc = 0;
    if (status == ST_ACTIVE) {
      const double s = chunk_sum(part + (long)b * EDM_NLL_MAX_CHUNKS, chunks);
      const double E = sqrt(s / (double)CHW);
      float t = sf[ROW_T * B + b];
      const float t1 = sf[ROW_T1 * B + b];
      const bool ok = E <= 1.0;
      const bool capped = !ok || state[ROW_AFTER_REJECT * B + b] != 0u;
      const double top = capped ? 1.0 : fac_max;
      double f = safety / sqrt(E);
      if (!(f >= fac_min)) f = fac_min;         // (a NaN lands here)
      if (f > top) f = top;
      const float h = (float)(((double)t1 - (double)t) * f);
      sf[ROW_ERR * B + b] = (float)E;
      sf[ROW_H * B + b] = h;
      state[ROW_AFTER_REJECT * B + b] = ok ? 0u : 1u;
      if (ok) {
        t = t1;
        sf[ROW_T * B + b] = t;
        state[ROW_ACCEPTED * B + b] += 1u;
        acc = 1;
        if (t == t_end) status = ST_DONE;
      } else {
        state[ROW_REJECTED * B + b] += 1u;
      }
      if (status == ST_ACTIVE && !(fabs((double)h) >= h_floor * fabs((double)t))) {
        status = ST_FAILED;
        failed = true;
      }
      state[ROW_STATUS * B + b] = status;
      sf[ROW_T1 * B + b] = status == ST_ACTIVE ? snap_t1(t, h, t_end) : t;
      still = status == ST_ACTIVE;
    }
    accept[b] = acc;
  }
  const unsigned long long live = __ballot(still);      // (both votes outside any divergent branch)
  const bool any_failed = __any(failed);
  if ((threadIdx.x & 63) == 0) {
    if (live) atomicAdd(active, (int)__popcll(live));
    if (health && any_failed) atomicOr(health, 2u);
  }
}

// x <- accept[b] ? y : x, in place: a sample that was not accepted is never written
template <bool VEC>
__global__ __launch_bounds__(256) void k_adapt_commit(float* __restrict__ x, const float* __restrict__ y,
                                                      const unsigned char* __restrict__ accept, int B, long CHW) {
  const long nq = (CHW + 3) / 4, total = (long)B * nq;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const long b = i / nq, q = i - b * nq, e = b * CHW + 4 * q;
    if (!accept[b]) continue;
    const int m = quad_len<VEC>(CHW, q);
    float v[4];
    load4<VEC>(y + e, m, v);
    store4<VEC>(x + e, m, v);
  }
}

}  // namespace

// state: device, EDM_ADAPT_ROWS * B 32-bit words, written
extern "C" int edm_adapt_begin(float t_start, float t_end, float h0, int B, void* state, hipStream_t st) {
  EDM_REQUIRE(state && B > 0 && std::isfinite(t_start) && std::isfinite(t_end) && std::isfinite(h0) && t_start > 0.f &&
                  t_end > 0.f && t_start != t_end && (h0 > 0.f) == (t_end > t_start) && h0 != 0.f,
              "adapt_begin: bad args (positive times, h0 pointing from t_start to t_end)");
  hipLaunchKernelGGL(k_adapt_begin, dim3((B + 63) / 64), dim3(64), 0, st, t_start, t_end, h0, B, (uint32_t*)state);
  EDM_CHECK_LAUNCH("adapt_begin");
  return EDM_OK;
}
// t, t1: device fp32 [B] (rows of the state, or any per-sample times with t != 0)
extern "C" int edm_adapt_euler(const float* x, const float* D, const float* t, const float* t1, int B, long CHW, float* dx,
                               float* x1, unsigned* health, hipStream_t st) {
  EDM_REQUIRE(x && D && t && t1 && dx && x1 && B > 0 && CHW > 0, "adapt_euler: bad args");
  const dim3 grid(grid_for((long)B * ((CHW + 3) / 4), 256)), block(256);
  if (CHW % 4 == 0 && aligned16({x, D, dx, x1}))
    hipLaunchKernelGGL(k_adapt_euler<true>, grid, block, 0, st, x, D, t, t1, B, CHW, dx, x1, health);
  else
    hipLaunchKernelGGL(k_adapt_euler<false>, grid, block, 0, st, x, D, t, t1, B, CHW, dx, x1, health);
  EDM_CHECK_LAUNCH("adapt_euler");
  return EDM_OK;
}
// part: device workspace of B * EDM_NLL_MAX_CHUNKS doubles; the first sample_chunks(CHW) of every row are written
extern "C" int edm_adapt_correct(const float* x, const float* dx, const float* x1, const float* D1, const float* t,
                                 const float* t1, int B, long CHW, double atol, double rtol, float* y, double* part,
                                 unsigned* health, hipStream_t st) {
  EDM_REQUIRE(x && dx && x1 && D1 && t && t1 && y && part && B > 0 && B <= 65535 && CHW > 0,
              "adapt_correct: bad args (B <= 65535)");
  EDM_REQUIRE(std::isfinite(atol) && std::isfinite(rtol) && atol >= 0.0 && rtol >= 0.0 && atol + rtol > 0.0,
              "adapt_correct: atol and rtol must be finite, >= 0 and not both 0");
  const dim3 grid(sample_chunks(CHW), B), block(256);
  if (CHW % 4 == 0 && aligned16({x, dx, x1, D1, y}))
    hipLaunchKernelGGL(k_adapt_correct<true>, grid, block, 0, st, x, dx, x1, D1, t, t1, CHW, atol, rtol, y, part, health);
  else
    hipLaunchKernelGGL(k_adapt_correct<false>, grid, block, 0, st, x, dx, x1, D1, t, t1, CHW, atol, rtol, y, part, health);
  EDM_CHECK_LAUNCH("adapt_correct");
  return EDM_OK;
}
// accept: device uint8 [B], written; active: device int32, += the samples still active
extern "C" int edm_adapt_control(const double* part, int B, long CHW, float t_end, double safety, double fac_min,
                                 double fac_max, double h_floor, void* state, unsigned char* accept, int* active,
                                 unsigned* health, hipStream_t st) {
  EDM_REQUIRE(part && state && accept && active && B > 0 && CHW > 0 && t_end > 0.f, "adapt_control: bad args");
  EDM_REQUIRE(safety > 0.0 && safety <= 1.0 && fac_min > 0.0 && fac_min < 1.0 && fac_max >= 1.0 && std::isfinite(fac_max) &&
                  h_floor >= 0.0 && h_floor < 1.0,
              "adapt_control: needs 0 < safety <= 1, 0 < fac_min < 1 <= fac_max < inf, 0 <= h_floor < 1");
  hipLaunchKernelGGL(k_adapt_control, dim3((B + 63) / 64), dim3(64), 0, st, part, sample_chunks(CHW), B, CHW, t_end, safety,
                     fac_min, fac_max, h_floor, (uint32_t*)state, accept, active, health);
  EDM_CHECK_LAUNCH("adapt_control");
  return EDM_OK;
}
extern "C" int edm_adapt_commit(float* x, const float* y, const unsigned char* accept, int B, long CHW, hipStream_t st) {
  EDM_REQUIRE(x && y && accept && x != y && B > 0 && CHW > 0, "adapt_commit: bad args");
  const dim3 grid(grid_for((long)B * ((CHW + 3) / 4), 256)), block(256);
  if (CHW % 4 == 0 && aligned16({x, y}))
    hipLaunchKernelGGL(k_adapt_commit<true>, grid, block, 0, st, x, y, accept, B, CHW);
  else
    hipLaunchKernelGGL(k_adapt_commit<false>, grid, block, 0, st, x, y, accept, B, CHW);
  EDM_CHECK_LAUNCH("adapt_commit");
  return EDM_OK;
}
