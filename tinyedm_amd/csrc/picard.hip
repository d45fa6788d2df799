// Parallel-in-time sampling (ParaDiGMS, Shih et al. 2023): Picard iteration of the Heun / Euler step over a window of
// P consecutive steps of the sigma table, every sample with its own window start.  The network evaluations and the
// Euler stage (edm_adapt_euler on the P * B rows of the window) happen outside; here are the three small kernels of an
// iteration: the scan that rebuilds the window from the step increments, the controller that decides how far each
// sample's window slides, and the slide itself.
//
// Window of sample b: position j = 0 .. P stands at table index s_b + j; position 0 is converged, the next
// L_b = min(P, N - 1 - s_b) positions are live, the rest are inactive and ride along (T[j][b] = t[min(s_b + j, N - 1)],
// so an inactive row has t1 == t).  Buffers are position-major: X[P + 1][B][CHW], T[P + 1][B].
// Per-sample state: EDM_PICARD_ROWS rows of B 32-bit words (include/tinyedm_hip.h): START, STATUS (0 active, 1 done),
// ITERATIONS.
//
// Bit rules, as adaptive.hip's: the step expressions are the functions of quads.h that k_adapt_euler / k_adapt_correct call,
// so at the fixed point a step has the bits of edm_heun_euler / edm_heun_correct; the error norm is order-fixed (thread-serial
// per position, the xor butterfly of whole waves, four wave totals in index order, chunks in index order) with a chunking
// that depends on CHW alone; no atomics on floating point; nothing is read on the host.
#include "common.h"
#include "quads.h"

#include <cmath>

namespace {

constexpr int PICARD_MAX_WINDOW = 64;       // = EDM_PICARD_MAX_WINDOW: sizes the LDS of the scan
enum { ROW_START = 0, ROW_STATUS, ROW_ITERATIONS, PICARD_ROWS };
enum : uint32_t { ST_ACTIVE = 0, ST_DONE = 1 };

// the window start as the kernels use it: inside the table whatever the word holds
__device__ __forceinline__ int table_start(uint32_t word, int N) {
  const int s = (int)word;
  return s < 0 ? 0 : (s > N - 1 ? N - 1 : s);
}
__device__ __forceinline__ int live_length(int s, int N, int P) {
  const int L = N - 1 - s;
  return L < P ? L : P;         // (>= 0: s <= N - 1)
}

// grid (chunks, B), 256 threads.  A thread owns a quad of sample b and walks the live positions with the running state
// in registers: new_0 = X[0], new_{j+1} = fma(t1 - t0, slope_j, new_j) with slope_j from the OLD iterate (HEUN: k_adapt_correct's
// 0.5 dx + 0.5 (X1 - D1) / t1; otherwise dx), positions past L copy new_L.  Per live position j + 1 the quad's share of
// sum ((new - old) / (atol + rtol max(|old|, |new|)))^2 goes through the wave butterfly into red[wave][j]; after the one
// barrier thread j adds the four wave totals in index order into part[b][j][chunk].
template <bool VEC, bool HEUN>
__global__ __launch_bounds__(256) void k_picard_scan(const float* __restrict__ X, const float* __restrict__ dx,
                                                     const float* __restrict__ X1, const float* __restrict__ D1,
                                                     const float* __restrict__ T, const uint32_t* __restrict__ state,
                                                     const double* __restrict__ tol, int B, int N, int P, long CHW,
                                                     float* __restrict__ Xnew, double* __restrict__ part,
                                                     unsigned* __restrict__ health) {
  __shared__ double red[4][PICARD_MAX_WINDOW];
  const long nq = (CHW + 3) / 4, row = (long)B * CHW;
  const int b = blockIdx.y, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int L = live_length(table_start(state[ROW_START * B + b], N), N, P);
  const double atol = tol[0], rtol = tol[1];
  bool bad = false, first = true;
  for (long base = (long)blockIdx.x * 256; base < nq; base += (long)gridDim.x * 256) {      // (block-uniform trip count)
    const long q = base + threadIdx.x, e = (long)b * CHW + 4 * q;
    const bool valid = q < nq;
    const int m = quad_len<VEC>(CHW, q);
    float cur[4] = {0.f, 0.f, 0.f, 0.f};
    if (valid) {
      load4<VEC>(X + e, m, cur);
      store4<VEC>(Xnew + e, m, cur);
    }
    for (int j = 0; j < L; ++j) {
      double acc = 0.0;
      if (valid) {
        const float t0 = T[j * B + b], t1 = T[(j + 1) * B + b];
        const long o = (long)j * row + e;
        float dxv[4], old[4], nw[4], x1v[4], d1[4];
        load4<VEC>(dx + o, m, dxv);
        load4<VEC>(X + o + row, m, old);
        if (HEUN) {
          load4<VEC>(X1 + o, m, x1v);
          load4<VEC>(D1 + o, m, d1);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const float slope = HEUN ? heun_slope(dxv[k], x1v[k], d1[k], t1) : dxv[k];
          nw[k] = heun_update(cur[k], slope, t0, t1);
          const double od = (double)old[k], nd = (double)nw[k];
          const double sc = fma(rtol, fmax(fabs(od), fabs(nd)), atol);
          const double d = nd - od;                     // (exact: the difference of two fp32 values)
          double r = d / sc;
          if (sc == 0.0) r = d == 0.0 ? 0.0 : (double)INFINITY;
          if (k < m) {
            bad |= nonfinite(nw[k]);
            acc = fma(r, r, acc);
          }
          cur[k] = nw[k];
        }
        store4<VEC>(Xnew + o + row, m, nw);
      }
      acc = wave_sum_f64(acc);          // (every lane of every wave: outside the divergent branch)
      if (lane == 0) red[wave][j] = first ? acc : red[wave][j] + acc;
    }
    if (valid)
      for (int j = L + 1; j <= P; ++j) store4<VEC>(Xnew + (long)j * row + e, m, cur);     // inactive: copies of new_L
    first = false;
  }
  __syncthreads();
  if ((int)threadIdx.x < P) {
    const int j = threadIdx.x;
    part[((long)b * P + j) * gridDim.x + blockIdx.x] = j < L ? ((red[0][j] + red[1][j]) + red[2][j]) + red[3][j] : 0.0;
  }
  EDM_RAISE_HEALTH(health, bad, 2u);
}

// One thread per sample, fp64.  E_j = sqrt(sum of part[b][j - 1][.] in index order / CHW) for the live positions
// j = 1 .. L; m = the number of leading positions with E_j <= 1 (a NaN is not converged); stride = min(m + 1, L): the
// position after the converged ones is one sequential step from a converged state, hence exact.  s += stride, the
// iteration count + 1, done when s == N - 1.  The samples still active are added to *active, one integer atomic per wave.
__global__ __launch_bounds__(64) void k_picard_control(const double* __restrict__ part, int chunks, int B, long CHW, int N,
                                                       int P, uint32_t* __restrict__ state, int* __restrict__ stride,
                                                       double* __restrict__ err, int* __restrict__ active) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  bool still = false;
  if (b < B) {
    int r = 0;
    if (state[ROW_STATUS * B + b] == ST_ACTIVE) {
      int s = table_start(state[ROW_START * B + b], N);
      const int L = live_length(s, N, P);
      int m = 0;
      bool leading = true;
      for (int j = 0; j < L; ++j) {
        const double sum = chunk_sum(part + ((long)b * P + j) * chunks, chunks);
        const double E = sqrt(sum / (double)CHW);
        if (err) err[(long)b * P + j] = E;
        if (leading && E <= 1.0) ++m; else leading = false;
      }
      r = m + 1 < L ? m + 1 : L;
      s += r;
      still = s < N - 1;
      state[ROW_START * B + b] = (uint32_t)s;
      state[ROW_ITERATIONS * B + b] += 1u;
      state[ROW_STATUS * B + b] = still ? ST_ACTIVE : ST_DONE;
    }
    stride[b] = r;
  }
  const unsigned long long live = __ballot(still);      // (outside any divergent branch)
  if ((threadIdx.x & 63) == 0 && live) atomicAdd(active, (int)__popcll(live));
}

// grid (x, B), 256 threads, grid-stride over the quads of sample b.  With stride r and live length L before the slide:
// X[j] = Xnew[j + r] while j + r <= L; a position entering at table index i <= N - 1 is the frozen-denoiser solution
// fma(Xnew[L] - Dh, t_i / t_{s + L}, Dh) with Dh = D[L - 1]; indices past N - 1 copy Xnew[L].  T is rewritten from the new
// start.  begin: the empty window at s = 0 (L = 0, Dh = 0) of the unit noise Xnew = x0 [B][CHW]: X[j] = t_j x0 in one
// rounding, and the state is written.
template <bool VEC>
__global__ __launch_bounds__(256) void k_picard_slide(const float* __restrict__ Xnew, const float* __restrict__ D,
                                                      const int* __restrict__ stride, uint32_t* __restrict__ state,
                                                      const float* __restrict__ tt, int begin, int B, int N, int P,
                                                      long CHW, float* __restrict__ X, float* __restrict__ T) {
  const long nq = (CHW + 3) / 4, row = (long)B * CHW;
  const int b = blockIdx.y;
  const int s_new = begin ? 0 : table_start(state[ROW_START * B + b], N);
  int r = begin ? 0 : stride[b];
  r = r < 0 ? 0 : (r > P ? P : r);
  if (r > s_new) r = s_new;
  const int s_old = s_new - r;
  const int L = begin ? 0 : live_length(s_old, N, P);
  if (blockIdx.x == 0 && (int)threadIdx.x <= P) {
    const int i = s_new + threadIdx.x;
    T[threadIdx.x * B + b] = tt[i < N - 1 ? i : N - 1];
  }
  if (begin && blockIdx.x == 0 && threadIdx.x == 0) {
    state[ROW_START * B + b] = 0u;
    state[ROW_STATUS * B + b] = N > 1 ? ST_ACTIVE : ST_DONE;
    state[ROW_ITERATIONS * B + b] = 0u;
  }
  const bool enters = s_old + L < N - 1;        // some position of the new window is extrapolated
  const float t_base = tt[s_old + L];
  for (long q = (long)blockIdx.x * 256 + threadIdx.x; q < nq; q += (long)gridDim.x * 256) {
    const long e = (long)b * CHW + 4 * q;
    const int m = quad_len<VEC>(CHW, q);
    float xl[4], dh[4] = {0.f, 0.f, 0.f, 0.f}, v[4];
    load4<VEC>(Xnew + (long)L * row + e, m, xl);
    if (!begin && enters && L > 0) load4<VEC>(D + (long)(L - 1) * row + e, m, dh);
    for (int j = 0; j <= P; ++j) {
      const int src = j + r, i = s_new + j;
      if (begin) {
        const float t = tt[i <= N - 1 ? i : 0];
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = t * xl[k];
      } else if (src <= L) {
        load4<VEC>(Xnew + (long)src * row + e, m, v);
      } else if (i <= N - 1) {
        const float ratio = tt[i] / t_base;
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = fmaf(xl[k] - dh[k], ratio, dh[k]);
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = xl[k];
      }
      store4<VEC>(X + (long)j * row + e, m, v);
    }
  }
}

}  // namespace

// X: [P + 1][B][CHW]; dx, X1, D1: [P][B][CHW] (D1 NULL: the Euler iteration); T: [P + 1][B]; tol: DEVICE {atol, rtol};
// Xnew: [P + 1][B][CHW], written; part: [B][P][chunks(CHW)] doubles, written
extern "C" int edm_picard_scan(const float* X, const float* dx, const float* X1, const float* D1, const float* T,
                               const void* state, const double* tol, int B, int N, int P, long CHW, float* Xnew,
                               double* part, unsigned* health, hipStream_t st) {
  EDM_REQUIRE(X && dx && T && state && tol && Xnew && part && X != Xnew && (D1 == nullptr || X1 != nullptr),
              "picard_scan: bad args (X1 goes with D1; Xnew must not alias X)");
  EDM_REQUIRE(B > 0 && B <= 65535 && N >= 2 && P >= 1 && P <= PICARD_MAX_WINDOW && CHW > 0,
              "picard_scan: needs 0 < B <= 65535, N >= 2, 1 <= P <= 64");
  const dim3 grid(sample_chunks(CHW), B), block(256);
  const uint32_t* s = (const uint32_t*)state;
  const bool vec = CHW % 4 == 0 && aligned16({X, dx, X1, D1, Xnew});
  if (D1) {
    if (vec)
      hipLaunchKernelGGL((k_picard_scan<true, true>), grid, block, 0, st, X, dx, X1, D1, T, s, tol, B, N, P, CHW, Xnew, part, health);
    else
      hipLaunchKernelGGL((k_picard_scan<false, true>), grid, block, 0, st, X, dx, X1, D1, T, s, tol, B, N, P, CHW, Xnew, part, health);
  } else {
    if (vec)
      hipLaunchKernelGGL((k_picard_scan<true, false>), grid, block, 0, st, X, dx, X1, D1, T, s, tol, B, N, P, CHW, Xnew, part, health);
    else
      hipLaunchKernelGGL((k_picard_scan<false, false>), grid, block, 0, st, X, dx, X1, D1, T, s, tol, B, N, P, CHW, Xnew, part, health);
  }
  EDM_CHECK_LAUNCH("picard_scan");
  return EDM_OK;
}
// stride: DEVICE int32 [B], written (0 for a sample that was not active); err: DEVICE [B][P] doubles or NULL, E of the
// live positions written; active: DEVICE int32, += the samples still active
extern "C" int edm_picard_control(const double* part, int B, long CHW, int N, int P, void* state, int* stride, double* err,
                                  int* active, hipStream_t st) {
  EDM_REQUIRE(part && state && stride && active && B > 0 && CHW > 0 && N >= 2 && P >= 1 && P <= PICARD_MAX_WINDOW,
              "picard_control: bad args (N >= 2, 1 <= P <= 64)");
  hipLaunchKernelGGL(k_picard_control, dim3((B + 63) / 64), dim3(64), 0, st, part, sample_chunks(CHW), B, CHW, N, P,
                     (uint32_t*)state, stride, err, active);
  EDM_CHECK_LAUNCH("picard_control");
  return EDM_OK;
}
// t_table: DEVICE fp32, at least N entries; X: [P + 1][B][CHW] and T: [P + 1][B], written.  begin != 0: Xnew is the unit
// noise [B][CHW], D and stride are not read, the state is written
extern "C" int edm_picard_slide(const float* Xnew, const float* D, const int* stride, void* state, const float* t_table,
                                int begin, int B, int N, int P, long CHW, float* X, float* T, hipStream_t st) {
  EDM_REQUIRE(Xnew && state && t_table && X && T && X != Xnew && (begin || (D && stride)),
              "picard_slide: bad args (X must not alias Xnew)");
  EDM_REQUIRE(B > 0 && B <= 65535 && N >= 2 && P >= 1 && P <= PICARD_MAX_WINDOW && CHW > 0,
              "picard_slide: needs 0 < B <= 65535, N >= 2, 1 <= P <= 64");
  const dim3 grid(sample_chunks(CHW), B), block(256);
  if (CHW % 4 == 0 && aligned16({Xnew, D, X}))
    hipLaunchKernelGGL(k_picard_slide<true>, grid, block, 0, st, Xnew, D, stride, (uint32_t*)state, t_table, begin, B, N, P, CHW, X, T);
  else
    hipLaunchKernelGGL(k_picard_slide<false>, grid, block, 0, st, Xnew, D, stride, (uint32_t*)state, t_table, begin, B, N, P, CHW, X, T);
  EDM_CHECK_LAUNCH("picard_slide");
  return EDM_OK;
}
