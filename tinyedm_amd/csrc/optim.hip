// Step-level fp32 kernels around the network: Diffuser (edm.py:84-93), sigma-weighted MSE
// (edm.py:212, metric.py:8-18), fused Adam + power-function EMA over the flat parameter arena
// (edm.py:251-253, ema.py:137-140, 273), and the Heun updates of the sampler (solvers.py:49-57).
#include "common.h"
#include <math.h>
#include <cmath>

namespace {

__device__ __forceinline__ void box_muller(uint32_t a, uint32_t b, float& n0, float& n1) {
  const float u1 = ((float)(a >> 8) + 0.5f) * (1.0f / 16777216.0f);  // (0,1)
  const float u2 = ((float)(b >> 8) + 0.5f) * (1.0f / 16777216.0f);
  const float r = sqrtf(-2.0f * __logf(u1));
  float s, c;
  __sincosf(6.28318530717958648f * u2, &s, &c);
  n0 = r * c;
  n1 = r * s;
}

// sigma_b = exp(P_mean + P_std*eps_b);  noisy = clean + sigma_b * n      (4 elements per thread)
__global__ void k_diffuse(const float* __restrict__ clean, float* __restrict__ noisy, float* __restrict__ sigma,
                          float P_mean, float P_std, int B, long CHW, uint32_t seed_lo, uint32_t seed_hi,
                          uint32_t step, const StepParams* __restrict__ dyn) {
  if (dyn) { step = dyn->step; seed_lo = dyn->seed_lo ^ 0xD1FF05E5u; seed_hi = dyn->seed_hi; }
  const long n4 = ((long)B * CHW + 3) / 4;
  const long total = (long)B * CHW;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
    Philox4 r = philox4x32_10((uint32_t)i, (uint32_t)(i >> 32), 0xD1FFu, step, seed_lo, seed_hi);
    float nn[4];
    box_muller(r.x, r.y, nn[0], nn[1]);
    box_muller(r.z, r.w, nn[2], nn[3]);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const long e = i * 4 + j;
      if (e < total) {
        const int b = (int)(e / CHW);
        Philox4 rb = philox4x32_10((uint32_t)b, 0u, 0x5167u, step, seed_lo, seed_hi);
        float e0, e1;
        box_muller(rb.x, rb.y, e0, e1);
        const float s = __expf(P_mean + P_std * e0);
        noisy[e] = clean[e] + s * nn[j];
        if (e % CHW == 0) sigma[b] = s;
      }
    }
  }
}

// same with the two normal draws supplied (deterministic tests / external RNG)
__global__ void k_diffuse_given(const float* __restrict__ clean, const float* __restrict__ eps,
                                const float* __restrict__ noise, float* __restrict__ noisy, float* __restrict__ sigma,
                                float P_mean, float P_std, int B, long CHW) {
  const long total = (long)B * CHW;
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
    const int b = (int)(e / CHW);
    const float s = expf(P_mean + P_std * eps[b]);
    noisy[e] = clean[e] + s * noise[e];
    if (e % CHW == 0) sigma[b] = s;
  }
}

// loss += sum_b mean_j w_b (D-x)^2 / B ;  dD = 2 w_b (D-x) / (CHW*B)   [w_b optional override]
__global__ void k_loss(const float* __restrict__ Dn, const float* __restrict__ clean, const float* __restrict__ sigma,
                       const float* __restrict__ wext, float sd, float* __restrict__ loss, float* __restrict__ dD, int B,
                       long CHW, float* __restrict__ acc_sum, long long* __restrict__ acc_total) {
  const long total = (long)B * CHW;
  const float inv = 1.0f / ((float)CHW * (float)B);
  float part = 0.f;
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
    const int b = (int)(e / CHW);
    float w;
    if (wext) {
      w = wext[b];
    } else {
      const float s = sigma[b];
      w = (s * s + sd * sd) / ((s * sd) * (s * sd));
    }
    const float d = Dn[e] - clean[e];
    part += w * d * d;
    if (dD) dD[e] = 2.0f * w * d * inv;
  }
  // one atomic per workgroup (one per wave serialised ~6000 adds on a single address: 81 us for 0.4 M elements)
  __shared__ float red[4];
  part = wave_sum(part);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = part;
  __syncthreads();
  if (threadIdx.x == 0) {
    const float p = red[0] + red[1] + red[2] + red[3];
    atomicAdd(loss, p * inv);
    // epoch state of the metric (metric.py:38-49): sum_i mean_j w_i d_ij^2 and the sample count
    if (acc_sum) atomicAdd(acc_sum, p / (float)CHW);
    if (acc_total && blockIdx.x == 0) *acc_total += B;
  }
}

// (struct AdamArgs and the per-element update adam_ema_update: common.h, shared with conv_wgrad3.hip)
// k_adam_ema keeps its own text of the update below (the same expressions as adam_ema_update): written over the shared
// function the compiler packs one more multiply-add pair of the quad into v_pk_fma_f32, which moves last bits against
// k_adam_ema_phema (the bitwise comparison of tests/test_posthoc_ema_gpu.py) and against every earlier result of this kernel.
// fused multi-tensor Adam + EMA over the flat arenas: 5 streams read, 4 written, one pass
// zero_grad: the gradient arena is cleared in the same pass (saves the separate fill of optimizer.zero_grad()).
__global__ void k_adam_ema(float* __restrict__ theta, float* __restrict__ grad, float* __restrict__ m,
                           float* __restrict__ v, float* __restrict__ ema, long n4, long n, AdamArgs a,
                           const StepParams* __restrict__ dyn, int zero_grad, unsigned* __restrict__ health) {
  if (dyn) { a.lr = dyn->lr; a.ema_beta = dyn->ema_beta; a.grad_scale = dyn->grad_scale; a.bc1 = dyn->bc1; a.bc2sqrt = dyn->bc2sqrt; }
  const float step_size = a.lr / a.bc1;
  bool bad = false;     // health word (nullable): bit 0 = a non-finite gradient or weight passed through this step
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
    if (i * 4 + 3 < n) {
      f32x4 t = *reinterpret_cast<f32x4*>(theta + i * 4);
      f32x4 g = *reinterpret_cast<const f32x4*>(grad + i * 4);
      if (zero_grad) *reinterpret_cast<f32x4*>(grad + i * 4) = f32x4{0.f, 0.f, 0.f, 0.f};
      f32x4 mm = *reinterpret_cast<f32x4*>(m + i * 4);
      f32x4 vv = *reinterpret_cast<f32x4*>(v + i * 4);
      f32x4 ee;
      if (ema) ee = *reinterpret_cast<f32x4*>(ema + i * 4);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float gj = g[j] * a.grad_scale;
        mm[j] = a.b1 * mm[j] + (1.f - a.b1) * gj;
        vv[j] = a.b2 * vv[j] + (1.f - a.b2) * gj * gj;
        t[j] -= step_size * mm[j] / (sqrtf(vv[j]) / a.bc2sqrt + a.eps);
        if (ema) ee[j] = a.ema_beta * ee[j] + (1.f - a.ema_beta) * t[j];
        bad |= !(fabsf(gj) <= 3.0e38f) || !(fabsf(t[j]) <= 3.0e38f);
      }
      *reinterpret_cast<f32x4*>(theta + i * 4) = t;
      *reinterpret_cast<f32x4*>(m + i * 4) = mm;
      *reinterpret_cast<f32x4*>(v + i * 4) = vv;
      if (ema) *reinterpret_cast<f32x4*>(ema + i * 4) = ee;
    } else {
      for (long e = i * 4; e < n; ++e) {
        const float gj = grad[e] * a.grad_scale;
        const float mj = a.b1 * m[e] + (1.f - a.b1) * gj;
        const float vj = a.b2 * v[e] + (1.f - a.b2) * gj * gj;
        const float tj = theta[e] - step_size * mj / (sqrtf(vj) / a.bc2sqrt + a.eps);
        m[e] = mj;
        v[e] = vj;
        theta[e] = tj;
        if (zero_grad) grad[e] = 0.f;
        if (ema) ema[e] = a.ema_beta * ema[e] + (1.f - a.ema_beta) * tj;
        bad |= !(fabsf(gj) <= 3.0e38f) || !(fabsf(tj) <= 3.0e38f);
      }
    }
  }
  if (health && __any(bad) && (threadIdx.x & 63) == 0) atomicOr(health, 1u);
}

// The same pass over a SET OF RANGES of the arenas (the rest of the arena when the 3x3 weight-gradient finish has updated its
// rows itself: conv_wgrad3.hip k_wgrad3_finish<true>).  Driven by a device table, as k_weight_prep_multi is by `groups`:
// ranges[r] = (first element, length), chunks[c] = (range id, offset inside the range); workgroup c takes up to ADAM_CHUNK
// elements from there: the elements up to the first 16-byte boundary and behind the last one singly, the quads between as
// dwordx4.  Elements outside the ranges are neither read nor written; a chunk that would leave [0, n) is skipped whole.
constexpr int ADAM_CHUNK = 1024;        // = ops.ADAM_RANGE_CHUNK: 256 threads x one quad
struct AdamRange {
  long start, len;
};
__global__ __launch_bounds__(256) void k_adam_ema_ranges(float* __restrict__ theta, float* __restrict__ grad,
                                                         float* __restrict__ m, float* __restrict__ v,
                                                         float* __restrict__ ema, long n,
                                                         const AdamRange* __restrict__ ranges, int n_ranges,
                                                         const int2* __restrict__ chunks, AdamArgs a,
                                                         const StepParams* __restrict__ dyn, int zero_grad,
                                                         unsigned* __restrict__ health) {
  if (dyn) adam_args_from(a, dyn);
  const float step_size = a.lr / a.bc1;
  const int2 c = chunks[blockIdx.x];
  if (c.x < 0 || c.x >= n_ranges || c.y < 0) return;
  const AdamRange r = ranges[c.x];
  const long first = r.start + c.y;
  const long left = r.len - c.y;
  const int cnt = (int)(left < ADAM_CHUNK ? left : ADAM_CHUNK);
  if (r.start < 0 || cnt <= 0 || first + cnt > n) return;
  const int head = (int)((4 - (first & 3)) & 3) < cnt ? (int)((4 - (first & 3)) & 3) : cnt;   // singles before the first quad
  const int nq = (cnt - head) >> 2;
  bool bad = false;
  auto single = [&](long e) {
    float tj = theta[e], mj = m[e], vj = v[e], ej = ema ? ema[e] : 0.f;
    bad |= adam_ema_update(tj, grad[e], mj, vj, ej, ema != nullptr, a, step_size);
    m[e] = mj;
    v[e] = vj;
    theta[e] = tj;
    if (zero_grad) grad[e] = 0.f;
    if (ema) ema[e] = ej;
  };
  if ((int)threadIdx.x < nq) {
    const long i = first + head + 4 * (long)threadIdx.x;
    f32x4 t = *reinterpret_cast<f32x4*>(theta + i);
    f32x4 g = *reinterpret_cast<const f32x4*>(grad + i);
    if (zero_grad) *reinterpret_cast<f32x4*>(grad + i) = f32x4{0.f, 0.f, 0.f, 0.f};
    f32x4 mm = *reinterpret_cast<f32x4*>(m + i);
    f32x4 vv = *reinterpret_cast<f32x4*>(v + i);
    f32x4 ee = {0.f, 0.f, 0.f, 0.f};
    if (ema) ee = *reinterpret_cast<f32x4*>(ema + i);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float tj = t[j], mj = mm[j], vj = vv[j], ej = ee[j];
      bad |= adam_ema_update(tj, g[j], mj, vj, ej, ema != nullptr, a, step_size);
      t[j] = tj; mm[j] = mj; vv[j] = vj; ee[j] = ej;
    }
    *reinterpret_cast<f32x4*>(theta + i) = t;
    *reinterpret_cast<f32x4*>(m + i) = mm;
    *reinterpret_cast<f32x4*>(v + i) = vv;
    if (ema) *reinterpret_cast<f32x4*>(ema + i) = ee;
  }
  // at most 3 singles in front and 3 behind: one thread each, counted from the far end of the workgroup
  const int tail0 = head + 4 * nq, k = 255 - (int)threadIdx.x;
  if (k < head) single(first + k);
  else if (k - head < cnt - tail0) single(first + tail0 + (k - head));
  if (health && __any(bad) && (threadIdx.x & 63) == 0) atomicOr(health, 1u);
}

// Post-hoc EMA tracking (Karras et al. 2024, Sec. 3): k_adam_ema plus K power-function profile arenas updated from the
// new weights in the same pass, p_k = beta_k * p_k + (1 - beta_k) * theta_new.  The theta / m / v / ema expressions are
// k_adam_ema's verbatim: theta, m and v come out bitwise equal; the main EMA may differ in the last bit, because the
// compiler fuses b*e + (1-b)*t into an FMA for some lanes and not others, differently in the two kernels.  The K betas are read from device memory so that the eager and the
// captured step share one launch form and a replay picks up the betas the host wrote before it.
struct PhemaArenas {
  float* p[4];
};
template <int K>
__global__ void k_adam_ema_phema(float* __restrict__ theta, float* __restrict__ grad, float* __restrict__ m,
                                 float* __restrict__ v, float* __restrict__ ema, PhemaArenas prof,
                                 const float* __restrict__ betas, long n4, long n, AdamArgs a,
                                 const StepParams* __restrict__ dyn, int zero_grad, unsigned* __restrict__ health) {
  if (dyn) { a.lr = dyn->lr; a.ema_beta = dyn->ema_beta; a.grad_scale = dyn->grad_scale; a.bc1 = dyn->bc1; a.bc2sqrt = dyn->bc2sqrt; }
  float pb[K];
#pragma unroll
  for (int k = 0; k < K; ++k) pb[k] = betas[k];
  const float step_size = a.lr / a.bc1;
  bool bad = false;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
    if (i * 4 + 3 < n) {
      f32x4 t = *reinterpret_cast<f32x4*>(theta + i * 4);
      f32x4 g = *reinterpret_cast<const f32x4*>(grad + i * 4);
      if (zero_grad) *reinterpret_cast<f32x4*>(grad + i * 4) = f32x4{0.f, 0.f, 0.f, 0.f};
      f32x4 mm = *reinterpret_cast<f32x4*>(m + i * 4);
      f32x4 vv = *reinterpret_cast<f32x4*>(v + i * 4);
      f32x4 ee;
      if (ema) ee = *reinterpret_cast<f32x4*>(ema + i * 4);
      f32x4 pp[K];
#pragma unroll
      for (int k = 0; k < K; ++k) pp[k] = *reinterpret_cast<f32x4*>(prof.p[k] + i * 4);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float gj = g[j] * a.grad_scale;
        mm[j] = a.b1 * mm[j] + (1.f - a.b1) * gj;
        vv[j] = a.b2 * vv[j] + (1.f - a.b2) * gj * gj;
        t[j] -= step_size * mm[j] / (sqrtf(vv[j]) / a.bc2sqrt + a.eps);
        if (ema) ee[j] = a.ema_beta * ee[j] + (1.f - a.ema_beta) * t[j];
#pragma unroll
        for (int k = 0; k < K; ++k) pp[k][j] = pb[k] * pp[k][j] + (1.f - pb[k]) * t[j];
        bad |= !(fabsf(gj) <= 3.0e38f) || !(fabsf(t[j]) <= 3.0e38f);
      }
      *reinterpret_cast<f32x4*>(theta + i * 4) = t;
      *reinterpret_cast<f32x4*>(m + i * 4) = mm;
      *reinterpret_cast<f32x4*>(v + i * 4) = vv;
      if (ema) *reinterpret_cast<f32x4*>(ema + i * 4) = ee;
#pragma unroll
      for (int k = 0; k < K; ++k) *reinterpret_cast<f32x4*>(prof.p[k] + i * 4) = pp[k];
    } else {
      for (long e = i * 4; e < n; ++e) {
        const float gj = grad[e] * a.grad_scale;
        const float mj = a.b1 * m[e] + (1.f - a.b1) * gj;
        const float vj = a.b2 * v[e] + (1.f - a.b2) * gj * gj;
        const float tj = theta[e] - step_size * mj / (sqrtf(vj) / a.bc2sqrt + a.eps);
        m[e] = mj;
        v[e] = vj;
        theta[e] = tj;
        if (zero_grad) grad[e] = 0.f;
        if (ema) ema[e] = a.ema_beta * ema[e] + (1.f - a.ema_beta) * tj;
#pragma unroll
        for (int k = 0; k < K; ++k) prof.p[k][e] = pb[k] * prof.p[k][e] + (1.f - pb[k]) * tj;
        bad |= !(fabsf(gj) <= 3.0e38f) || !(fabsf(tj) <= 3.0e38f);
      }
    }
  }
  if (health && __any(bad) && (threadIdx.x & 63) == 0) atomicOr(health, 1u);
}

// Post-hoc EMA reconstruction: acc[l][i] += w[l] * snap[i] for L <= 8 target lengths in one pass over a snapshot.  The
// accumulator is fp64, so hundreds of terms with |w| ~ 3 sum to the same result in any order.  vec: n % 4 == 0 and
// snap / acc 16-byte aligned -> dwordx4 loads of snap, the rest element by element.
struct PhemaWeights {
  double w[8];
};
template <int L>
__global__ void k_phema_accumulate(double* __restrict__ acc, const float* __restrict__ snap, PhemaWeights w, long n,
                                   bool vec) {
  const long tid = (long)blockIdx.x * blockDim.x + threadIdx.x, stride = (long)gridDim.x * blockDim.x;
  long head = 0;
  if (vec) {
    head = n;
    for (long i = tid * 4; i < n; i += stride * 4) {
      const f32x4 s = *reinterpret_cast<const f32x4*>(snap + i);
#pragma unroll
      for (int l = 0; l < L; ++l) {
        double2* d = reinterpret_cast<double2*>(acc + l * n + i);
        double2 lo = d[0], hi = d[1];
        lo.x = fma(w.w[l], (double)s[0], lo.x);
        lo.y = fma(w.w[l], (double)s[1], lo.y);
        hi.x = fma(w.w[l], (double)s[2], hi.x);
        hi.y = fma(w.w[l], (double)s[3], hi.y);
        d[0] = lo;
        d[1] = hi;
      }
    }
  }
  for (long i = head + tid; i < n; i += stride) {
    const double s = (double)snap[i];
#pragma unroll
    for (int l = 0; l < L; ++l) acc[l * n + i] = fma(w.w[l], s, acc[l * n + i]);
  }
}
__global__ void k_f64_to_f32(const double* __restrict__ a, float* __restrict__ out, long n) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x)
    out[i] = (float)a[i];
}

// dx = (x-D)/t0 ; x1 = x + (t1-t0)*dx
__global__ void k_heun_euler(const float* __restrict__ x, const float* __restrict__ Dn, float t0, float t1,
                             float* __restrict__ dx, float* __restrict__ x1, long n, unsigned* __restrict__ health) {
  bool bad = false;     // health word (nullable): bit 1 = a non-finite sampler state
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const float d = (x[i] - Dn[i]) / t0;
    dx[i] = d;
    const float o = x[i] + (t1 - t0) * d;
    x1[i] = o;
    bad |= !(fabsf(o) <= 3.0e38f);
  }
  if (health && __any(bad) && (threadIdx.x & 63) == 0) atomicOr(health, 2u);
}
// dxp = (x1-D1)/t1 ; out = x + (t1-t0)*(0.5*dx + 0.5*dxp)
__global__ void k_heun_correct(const float* __restrict__ x, const float* __restrict__ dx, const float* __restrict__ x1,
                               const float* __restrict__ D1, float t0, float t1, float* __restrict__ out, long n,
                               unsigned* __restrict__ health) {
  bool bad = false;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const float dp = (x1[i] - D1[i]) / t1;
    const float o = x[i] + (t1 - t0) * (0.5f * dx[i] + 0.5f * dp);
    out[i] = o;
    bad |= !(fabsf(o) <= 3.0e38f);
  }
  if (health && __any(bad) && (threadIdx.x & 63) == 0) atomicOr(health, 2u);
}
// Guided updates: D = Dg + w*(Dm - Dg) in registers, then the unguided kernels' expressions verbatim (w == 0 gives
// exactly the unguided result on Dg: fmaf(0, d, Dg) == Dg).  w is read from device memory so that a captured solve
// replays with whatever guidance the host wrote there.  vec: every pointer 16-byte aligned -> dwordx4 over the first
// n/4*4 elements, the tail (and the whole range when !vec) element by element.
__device__ __forceinline__ float heun_euler_guided_1(float x, float Dm, float Dg, float w, float t0, float t1,
                                                     float& dx, bool& bad) {
  const float D = fmaf(w, Dm - Dg, Dg);
  const float d = (x - D) / t0;
  dx = d;
  const float o = x + (t1 - t0) * d;
  bad |= !(fabsf(o) <= 3.0e38f);
  return o;
}
__device__ __forceinline__ float heun_correct_guided_1(float x, float dx, float x1, float Dm1, float Dg1, float w,
                                                       float t0, float t1, bool& bad) {
  const float D1 = fmaf(w, Dm1 - Dg1, Dg1);
  const float dp = (x1 - D1) / t1;
  const float o = x + (t1 - t0) * (0.5f * dx + 0.5f * dp);
  bad |= !(fabsf(o) <= 3.0e38f);
  return o;
}
__global__ void k_heun_euler_guided(const float* __restrict__ x, const float* __restrict__ Dm,
                                    const float* __restrict__ Dg, const float* __restrict__ w, float t0, float t1,
                                    float* __restrict__ dx, float* __restrict__ x1, long n, bool vec,
                                    unsigned* __restrict__ health) {
  const float wv = *w;
  const long tid = (long)blockIdx.x * blockDim.x + threadIdx.x, stride = (long)gridDim.x * blockDim.x;
  bool bad = false;
  long head = 0;
  if (vec) {
    head = n / 4 * 4;
    for (long i = tid * 4; i < head; i += stride * 4) {
      const f32x4 xv = *reinterpret_cast<const f32x4*>(x + i);
      const f32x4 mv = *reinterpret_cast<const f32x4*>(Dm + i);
      const f32x4 gv = *reinterpret_cast<const f32x4*>(Dg + i);
      f32x4 dv, ov;
      for (int j = 0; j < 4; ++j) {
        float d;
        ov[j] = heun_euler_guided_1(xv[j], mv[j], gv[j], wv, t0, t1, d, bad);
        dv[j] = d;
      }
      *reinterpret_cast<f32x4*>(dx + i) = dv;
      *reinterpret_cast<f32x4*>(x1 + i) = ov;
    }
  }
  for (long i = head + tid; i < n; i += stride) {
    float d;
    x1[i] = heun_euler_guided_1(x[i], Dm[i], Dg[i], wv, t0, t1, d, bad);
    dx[i] = d;
  }
  if (health && __any(bad) && (threadIdx.x & 63) == 0) atomicOr(health, 2u);
}
__global__ void k_heun_correct_guided(const float* __restrict__ x, const float* __restrict__ dx,
                                      const float* __restrict__ x1, const float* __restrict__ Dm1,
                                      const float* __restrict__ Dg1, const float* __restrict__ w, float t0, float t1,
                                      float* __restrict__ out, long n, bool vec, unsigned* __restrict__ health) {
  const float wv = *w;
  const long tid = (long)blockIdx.x * blockDim.x + threadIdx.x, stride = (long)gridDim.x * blockDim.x;
  bool bad = false;
  long head = 0;
  if (vec) {
    head = n / 4 * 4;
    for (long i = tid * 4; i < head; i += stride * 4) {
      const f32x4 xv = *reinterpret_cast<const f32x4*>(x + i);
      const f32x4 dv = *reinterpret_cast<const f32x4*>(dx + i);
      const f32x4 x1v = *reinterpret_cast<const f32x4*>(x1 + i);
      const f32x4 mv = *reinterpret_cast<const f32x4*>(Dm1 + i);
      const f32x4 gv = *reinterpret_cast<const f32x4*>(Dg1 + i);
      f32x4 ov;
      for (int j = 0; j < 4; ++j) ov[j] = heun_correct_guided_1(xv[j], dv[j], x1v[j], mv[j], gv[j], wv, t0, t1, bad);
      *reinterpret_cast<f32x4*>(out + i) = ov;
    }
  }
  for (long i = head + tid; i < n; i += stride)
    out[i] = heun_correct_guided_1(x[i], dx[i], x1[i], Dm1[i], Dg1[i], wv, t0, t1, bad);
  if (health && __any(bad) && (threadIdx.x & 63) == 0) atomicOr(health, 2u);
}
// Churn of the stochastic sampler (Karras et al. 2022, Algorithm 2): x_hat = x + c*n, n ~ N(0, 1) drawn here.  One
// thread per quad q of a sample b: element j = 4q + k of sample b takes normal k of
//   philox4x32_10(ctr = (q, b, 0x43480000 ^ step, solve_index), key = (seed_lo, seed_hi))
// (the four normals: box_muller(r.x, r.y), box_muller(r.z, r.w), as k_diffuse), so a sample's noise depends only on
// (seed, solve_index, step, b, j): not on the batch size, the grid or the memory path.  seed and solve_index come from
// the device record rec = {seed_lo, seed_hi, solve_index, 0}, so a captured solve draws new noise whenever the host
// rewrites it.  vec: x and x_hat 16-byte aligned and CHW % 4 == 0 -> one dwordx4 load and store per quad; otherwise
// the same quads element by element (the last quad of a sample may be partial).
__global__ void k_heun_churn(const float* __restrict__ x, float c, const uint32_t* __restrict__ rec, uint32_t step,
                             int B, long CHW, float* __restrict__ x_hat, bool vec, unsigned* __restrict__ health) {
  const uint32_t seed_lo = rec[0], seed_hi = rec[1], solve_index = rec[2];
  const long nq = (CHW + 3) / 4, total = (long)B * nq;
  bool bad = false;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const long b = i / nq, q = i - b * nq;
    const Philox4 r = philox4x32_10((uint32_t)q, (uint32_t)b, 0x43480000u ^ step, solve_index, seed_lo, seed_hi);
    float nn[4];
    box_muller(r.x, r.y, nn[0], nn[1]);
    box_muller(r.z, r.w, nn[2], nn[3]);
    const long e = b * CHW + 4 * q;
    if (vec) {
      const f32x4 xv = *reinterpret_cast<const f32x4*>(x + e);
      f32x4 ov;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        ov[k] = fmaf(c, nn[k], xv[k]);
        bad |= !(fabsf(ov[k]) <= 3.0e38f);
      }
      *reinterpret_cast<f32x4*>(x_hat + e) = ov;
    } else {
      const int m = (int)(CHW - 4 * q < 4 ? CHW - 4 * q : 4);
      for (int k = 0; k < m; ++k) {
        const float o = fmaf(c, nn[k], x[e + k]);
        bad |= !(fabsf(o) <= 3.0e38f);
        x_hat[e + k] = o;
      }
    }
  }
  if (health && __any(bad) && (threadIdx.x & 63) == 0) atomicOr(health, 2u);
}
// State of an image-conditioned solve at noise level t: out = image + t*x0 as one fma (x0 the caller's unit noise).
// image == nullptr: out = x0*t, the product k_scale_f32 computes, bit for bit.  vec: every operand 16-byte aligned ->
// dwordx4 over the first n/4*4 elements, the tail (and the whole range when !vec) element by element.
__global__ void k_state_init(const float* __restrict__ image, const float* __restrict__ x0, float t,
                             float* __restrict__ out, long n, bool vec, unsigned* __restrict__ health) {
  const long tid = (long)blockIdx.x * blockDim.x + threadIdx.x, stride = (long)gridDim.x * blockDim.x;
  bool bad = false;
  long head = 0;
  if (vec) {
    head = n / 4 * 4;
    for (long i = tid * 4; i < head; i += stride * 4) {
      const f32x4 nv = *reinterpret_cast<const f32x4*>(x0 + i);
      f32x4 iv{}, ov;
      if (image) iv = *reinterpret_cast<const f32x4*>(image + i);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        ov[j] = image ? fmaf(t, nv[j], iv[j]) : nv[j] * t;
        bad |= !(fabsf(ov[j]) <= 3.0e38f);
      }
      *reinterpret_cast<f32x4*>(out + i) = ov;
    }
  }
  for (long i = head + tid; i < n; i += stride) {
    const float o = image ? fmaf(t, x0[i], image[i]) : x0[i] * t;
    bad |= !(fabsf(o) <= 3.0e38f);
    out[i] = o;
  }
  if (health && __any(bad) && (threadIdx.x & 63) == 0) atomicOr(health, 2u);
}
// Replacement step of inpainting (Song et al. 2021): out = mask ? image + t*n : x, n ~ N(0, 1) drawn here: the known
// pixels are re-noised to the level t of the state they are pasted into.  mask: uint8 [mask_B, HW], mask_B in {1, B},
// broadcast over the C channels (and over the batch when mask_B == 1); non-zero = known pixel.  The noise is k_heun_churn's
// construction under its own tag: one thread per quad q of a sample b, element j = 4q + k of sample b takes normal k of
//   philox4x32_10(ctr = (q, b, 0x49500000 ^ step, solve_index), key = (seed_lo, seed_hi))
// so it depends only on (seed, solve_index, step, b, j): not on the batch size, the grid, the mask or the memory path,
// and it is independent of the churn noise of the same (seed, solve_index, step).  A quad whose mask is clear, and every
// quad when t == 0, draws nothing; t == 0 returns image itself on the mask.  vec: CHW % 4 == 0, HW % 4 == 0 (a quad
// then lies in one channel and its four mask bytes are one aligned 32-bit word), x / image / out 16-byte aligned and
// mask 4-byte aligned -> one dwordx4 per operand and one dword of mask per quad; otherwise the same quads element by
// element (the last quad of a sample may be partial).
__global__ void k_inpaint_blend(const float* __restrict__ x, const float* __restrict__ image,
                                const uint8_t* __restrict__ mask, float t, const uint32_t* __restrict__ rec,
                                uint32_t step, int B, long CHW, long HW, int mask_B, float* __restrict__ out, bool vec,
                                unsigned* __restrict__ health) {
  const uint32_t seed_lo = rec[0], seed_hi = rec[1], solve_index = rec[2];
  const long nq = (CHW + 3) / 4, total = (long)B * nq;
  bool bad = false;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const long b = i / nq, q = i - b * nq;
    const long e = b * CHW + 4 * q;
    const uint8_t* mrow = mask + (mask_B == 1 ? 0 : b * HW);
    const int m = vec ? 4 : (int)(CHW - 4 * q < 4 ? CHW - 4 * q : 4);
    bool keep[4] = {false, false, false, false};
    if (vec) {
      const uint32_t mw = *reinterpret_cast<const uint32_t*>(mrow + (4 * q) % HW);
#pragma unroll
      for (int k = 0; k < 4; ++k) keep[k] = ((mw >> (8 * k)) & 0xFFu) != 0;
    } else {
      for (int k = 0; k < m; ++k) keep[k] = mrow[(4 * q + k) % HW] != 0;
    }
    float nn[4] = {0.f, 0.f, 0.f, 0.f};
    if (t != 0.f && (keep[0] || keep[1] || keep[2] || keep[3])) {
      const Philox4 r = philox4x32_10((uint32_t)q, (uint32_t)b, 0x49500000u ^ step, solve_index, seed_lo, seed_hi);
      box_muller(r.x, r.y, nn[0], nn[1]);
      box_muller(r.z, r.w, nn[2], nn[3]);
    }
    if (vec) {
      const f32x4 xv = *reinterpret_cast<const f32x4*>(x + e);
      const f32x4 iv = *reinterpret_cast<const f32x4*>(image + e);
      f32x4 ov;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        ov[k] = keep[k] ? (t != 0.f ? fmaf(t, nn[k], iv[k]) : iv[k]) : xv[k];
        bad |= !(fabsf(ov[k]) <= 3.0e38f);
      }
      *reinterpret_cast<f32x4*>(out + e) = ov;
    } else {
      for (int k = 0; k < m; ++k) {
        const float o = keep[k] ? (t != 0.f ? fmaf(t, nn[k], image[e + k]) : image[e + k]) : x[e + k];
        bad |= !(fabsf(o) <= 3.0e38f);
        out[e + k] = o;
      }
    }
  }
  if (health && __any(bad) && (threadIdx.x & 63) == 0) atomicOr(health, 2u);
}
// DPM-Solver++ multistep update in data-prediction form (sigma(t) = t, s(t) = 1):
//   m = Dg + w*(Dm - Dg)  (G; else m = Dm),   x_out = a*x + c0*m + c1*m1 + c2*m2   (H = number of history terms)
// evaluated as fmaf(a, x, fmaf(c2, m2, fmaf(c1, m1, c0*m))), so the row (0, 1, 0, 0) of the final step returns m
// itself.  m is also written to m_out (nullable): the solver's history buffer, read back as m1 / m2 by the next steps.
// w is read from device memory (a captured solve follows later writes to it); w == 0 mixes to exactly Dg.  vec: every
// operand 16-byte aligned -> dwordx4 over the first n/4*4 elements, the tail (and the whole range when !vec) scalar.
template <bool G, int H>
__device__ __forceinline__ float dpm_multistep_1(float x, float Dm, float Dg, float w, float m1, float m2, float a,
                                                 float c0, float c1, float c2, float& m, bool& bad) {
  m = G ? fmaf(w, Dm - Dg, Dg) : Dm;
  float o = c0 * m;
  if (H >= 1) o = fmaf(c1, m1, o);
  if (H >= 2) o = fmaf(c2, m2, o);
  o = fmaf(a, x, o);
  bad |= !(fabsf(o) <= 3.0e38f);
  return o;
}
template <bool G, int H>
__global__ void k_dpm_multistep(const float* __restrict__ x, const float* __restrict__ Dm,
                                const float* __restrict__ Dg, const float* __restrict__ w,
                                const float* __restrict__ m1, const float* __restrict__ m2, float a, float c0, float c1,
                                float c2, float* __restrict__ x_out, float* __restrict__ m_out, long n, bool vec,
                                unsigned* __restrict__ health) {
  const float wv = G ? *w : 0.f;
  const long tid = (long)blockIdx.x * blockDim.x + threadIdx.x, stride = (long)gridDim.x * blockDim.x;
  bool bad = false;
  long head = 0;
  if (vec) {
    head = n / 4 * 4;
    for (long i = tid * 4; i < head; i += stride * 4) {
      const f32x4 xv = *reinterpret_cast<const f32x4*>(x + i);
      const f32x4 dv = *reinterpret_cast<const f32x4*>(Dm + i);
      f32x4 gv{}, h1{}, h2{}, ov, mv;
      if (G) gv = *reinterpret_cast<const f32x4*>(Dg + i);
      if (H >= 1) h1 = *reinterpret_cast<const f32x4*>(m1 + i);
      if (H >= 2) h2 = *reinterpret_cast<const f32x4*>(m2 + i);
      for (int j = 0; j < 4; ++j) {
        float m;
        ov[j] = dpm_multistep_1<G, H>(xv[j], dv[j], gv[j], wv, h1[j], h2[j], a, c0, c1, c2, m, bad);
        mv[j] = m;
      }
      *reinterpret_cast<f32x4*>(x_out + i) = ov;
      if (m_out) *reinterpret_cast<f32x4*>(m_out + i) = mv;
    }
  }
  for (long i = head + tid; i < n; i += stride) {
    float m;
    x_out[i] = dpm_multistep_1<G, H>(x[i], Dm[i], G ? Dg[i] : 0.f, wv, H >= 1 ? m1[i] : 0.f, H >= 2 ? m2[i] : 0.f,
                                     a, c0, c1, c2, m, bad);
    if (m_out) m_out[i] = m;
  }
  if (health && __any(bad) && (threadIdx.x & 63) == 0) atomicOr(health, 2u);
}
// Likelihood evaluation along the probability-flow ODE: the Heun updates above plus the divergence of the drift,
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
constexpr int NLL_MAX_CHUNKS = 64;      // = EDM_NLL_MAX_CHUNKS (include/tinyedm_hip.h)
constexpr uint32_t NLL_TAG = 0x4E4C0000u;

__device__ __forceinline__ void nll_words(uint32_t (&w)[4], long q, long b, uint32_t ev, uint32_t step,
                                          const uint32_t* __restrict__ rec) {
  const Philox4 r = philox4x32_10((uint32_t)q, (uint32_t)b, (NLL_TAG + (ev << 16)) ^ step, rec[2], rec[0], rec[1]);
  w[0] = r.x; w[1] = r.y; w[2] = r.z; w[3] = r.w;
}
template <bool VEC>
__device__ __forceinline__ void nll_load4(const float* __restrict__ p, int m, float (&v)[4]) {
  if (VEC) {
    const f32x4 t = *reinterpret_cast<const f32x4*>(p);
    v[0] = t[0]; v[1] = t[1]; v[2] = t[2]; v[3] = t[3];
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = k < m ? p[k] : 0.f;
  }
}
template <bool VEC>
__device__ __forceinline__ void nll_store4(float* __restrict__ p, int m, const float (&v)[4]) {
  if (VEC) {
    *reinterpret_cast<f32x4*>(p) = f32x4{v[0], v[1], v[2], v[3]};
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (k < m) p[k] = v[k];
  }
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
      bad |= !(fabsf(pl[k]) <= 3.0e38f) || !(fabsf(mi[k]) <= 3.0e38f);
    }
    nll_store4<VEC>(E + (1 + 2 * p) * rows + e, m, pl);
    nll_store4<VEC>(E + (2 + 2 * p) * rows + e, m, mi);
  }
}
// sum_p sum_k eps_pk (D+ - D-) of one quad; the difference is taken in fp64 (exact), the sign is a select
template <bool VEC>
__device__ __forceinline__ double nll_quad_dot(const float* __restrict__ Dn, long rows, long e, int m,
                                               const uint32_t (&w)[4], int K) {
  double acc = 0.0;
  for (int p = 0; p < K; ++p) {
    float dp[4], dm[4];
    nll_load4<VEC>(Dn + (1 + 2 * p) * rows + e, m, dp);
    nll_load4<VEC>(Dn + (2 + 2 * p) * rows + e, m, dm);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const double dd = (double)dp[k] - (double)dm[k];
      acc += ((w[k] >> p) & 1u) ? -dd : dd;
    }
  }
  return acc;
}
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
// EVERY thread of the 256-thread workgroup calls this, after its loop and outside any divergent branch (threads without
// a quad pass 0): the butterfly then never reads an inactive lane
__device__ __forceinline__ void nll_block_partial(double v, double* __restrict__ slot) {
  __shared__ double red[4];
  v = wave_sum_f64(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) *slot = ((red[0] + red[1]) + red[2]) + red[3];
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
    const int m = VEC ? 4 : (int)(CHW - 4 * q < 4 ? CHW - 4 * q : 4);
    uint32_t w[4];
    nll_words(w, q, b, ev, step, rec);
    float xv[4];
    nll_load4<VEC>(x + e, m, xv);
#pragma unroll
    for (int k = 0; k < 4; ++k) bad |= !(fabsf(xv[k]) <= 3.0e38f);
    nll_store4<VEC>(E + e, m, xv);
    nll_write_probes<VEC>(E, rows, e, m, xv, w, h, K, bad);
  }
  if (health && __any(bad) && (threadIdx.x & 63) == 0) atomicOr(health, 2u);
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
    const int m = VEC ? 4 : (int)(CHW - 4 * q < 4 ? CHW - 4 * q : 4);
    uint32_t w0[4], w1[4];
    nll_words(w0, q, b, 0u, step, rec);
    nll_words(w1, q, b, 1u, step, rec);
    float xv[4], dv[4], d[4], o[4];
    nll_load4<VEC>(E + e, m, xv);
    nll_load4<VEC>(Dn + e, m, dv);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      d[k] = (xv[k] - dv[k]) / t0;
      o[k] = fmaf(t1 - t0, d[k], xv[k]);      // (k_heun_euler's x + (t1 - t0) * d as the compiler contracts it)
      bad |= !(fabsf(o[k]) <= 3.0e38f);
    }
    nll_store4<VEC>(dx + e, m, d);
    nll_store4<VEC>(E1 + e, m, o);
    nll_write_probes<VEC>(E1, rows, e, m, o, w1, h1, K, bad);
    acc += nll_quad_dot<VEC>(Dn, rows, e, m, w0, K);
  }
  nll_block_partial(acc, part + b * NLL_MAX_CHUNKS + blockIdx.x);
  if (health && __any(bad) && (threadIdx.x & 63) == 0) atomicOr(health, 2u);
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
    const int m = VEC ? 4 : (int)(CHW - 4 * q < 4 ? CHW - 4 * q : 4);
    uint32_t w1[4];
    nll_words(w1, q, b, 1u, step, rec);
    float xv[4], dxv[4], x1v[4], d1[4], o[4];
    nll_load4<VEC>(E + e, m, xv);
    nll_load4<VEC>(dx + e, m, dxv);
    nll_load4<VEC>(E1 + e, m, x1v);
    nll_load4<VEC>(D1 + e, m, d1);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float dp = (x1v[k] - d1[k]) / t1;
      o[k] = fmaf(t1 - t0, 0.5f * dxv[k] + 0.5f * dp, xv[k]);      // (k_heun_correct's sum, contracted as there)
      bad |= !(fabsf(o[k]) <= 3.0e38f);
    }
    nll_store4<VEC>(out + e, m, o);
    if (Kout) {
      uint32_t wn[4];
      nll_words(wn, q, b, 0u, step - 1u, rec);
      nll_write_probes<VEC>(out, rows, e, m, o, wn, hn, Kout, bad);
    }
    acc += nll_quad_dot<VEC>(D1, rows, e, m, w1, K);
  }
  nll_block_partial(acc, part + b * NLL_MAX_CHUNKS + blockIdx.x);
  if (health && __any(bad) && (threadIdx.x & 63) == 0) atomicOr(health, 2u);
}
// part[b][chunk] = this chunk's share of sum_j (x_bj * inv_t)^2: the Gaussian prior's quadratic form
template <bool VEC>
__global__ __launch_bounds__(256) void k_nll_prior(const float* __restrict__ x, double inv_t, long CHW,
                                                   double* __restrict__ part) {
  const long nq = (CHW + 3) / 4, b = blockIdx.y;
  double acc = 0.0;
  for (long q = (long)blockIdx.x * 256 + threadIdx.x; q < nq; q += (long)gridDim.x * 256) {
    const int m = VEC ? 4 : (int)(CHW - 4 * q < 4 ? CHW - 4 * q : 4);
    float xv[4];
    nll_load4<VEC>(x + b * CHW + 4 * q, m, xv);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const double v = (double)xv[k] * inv_t;
      acc = fma(v, v, acc);
    }
  }
  nll_block_partial(acc, part + b * NLL_MAX_CHUNKS + blockIdx.x);
}
// L_b += c0 + c1 * (part[b][0] + part[b][1] + ... in index order), one thread per sample; health bit 1 on a non-finite L
__global__ __launch_bounds__(64) void k_nll_finish(const double* __restrict__ part, int chunks, int B, double c0,
                                                   double c1, double* __restrict__ L, unsigned* __restrict__ health) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  bool bad = false;
  if (b < B) {
    double s = 0.0;
    for (int c = 0; c < chunks; ++c) s += part[(long)b * NLL_MAX_CHUNKS + c];
    const double v = L[b] + fma(c1, s, c0);
    L[b] = v;
    bad = !(fabs(v) <= 1.0e300);
  }
  if (health && __any(bad) && (threadIdx.x & 63) == 0) atomicOr(health, 2u);
}
inline int nll_chunks(long CHW) {
  const long c = ((CHW + 3) / 4 + 255) / 256;
  return (int)(c < NLL_MAX_CHUNKS ? c : NLL_MAX_CHUNKS);
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
    const int m = VEC ? 4 : (int)(CHW - 4 * q < 4 ? CHW - 4 * q : 4);
    nll_load4<VEC>(clean + b * CHW + 4 * q, m, xv);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      ov[k] = fmaf(s, nn[k], xv[k]);
      bad |= k < m && !(fabsf(ov[k]) <= 3.0e38f);
    }
    for (int c = 0; c < C; ++c) nll_store4<VEC>(noisy + (b * C + c) * CHW + 4 * q, m, ov);
  }
  if (health && __any(bad) && (threadIdx.x & 63) == 0) atomicOr(health, 2u);
}
// part[b][chunk] = this chunk's share of sum_j ((double)D_bj - (double)clean_bj)^2.  The difference of two fp32 values
// is exact in fp64.  grid (nll_chunks(CHW), B): a sample's chunking, and with it the order of every add, depends on CHW
// alone, so se[b] has the same bits whatever B, the row or the memory path (the padding of a partial quad adds +0.0).
// C (the row divisor of the class sweep): row b of D is compared with row b / C of clean, which is never replicated;
// edm_eval_sqerr is C = 1.
template <bool VEC>
__global__ __launch_bounds__(256) void k_eval_sqerr(const float* __restrict__ D, const float* __restrict__ clean, int C,
                                                    long CHW, double* __restrict__ part) {
  const long nq = (CHW + 3) / 4, b = blockIdx.y, p = b / C;
  double acc = 0.0;
  for (long q = (long)blockIdx.x * 256 + threadIdx.x; q < nq; q += (long)gridDim.x * 256) {
    const int m = VEC ? 4 : (int)(CHW - 4 * q < 4 ? CHW - 4 * q : 4);
    float dv[4], cv[4];
    nll_load4<VEC>(D + b * CHW + 4 * q, m, dv);
    nll_load4<VEC>(clean + p * CHW + 4 * q, m, cv);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const double d = (double)dv[k] - (double)cv[k];
      acc = fma(d, d, acc);
    }
  }
  nll_block_partial(acc, part + b * NLL_MAX_CHUNKS + blockIdx.x);
}
// se[b] = part[b][0] + part[b][1] + ... in index order (written, not accumulated); health bit 1 on a non-finite se
__global__ __launch_bounds__(64) void k_eval_sqerr_finish(const double* __restrict__ part, int chunks, int B,
                                                          double* __restrict__ se, unsigned* __restrict__ health) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  bool bad = false;
  if (b < B) {
    double s = 0.0;
    for (int c = 0; c < chunks; ++c) s += part[(long)b * NLL_MAX_CHUNKS + c];
    se[b] = s;
    bad = !(fabs(s) <= 1.0e300);
  }
  if (health && __any(bad) && (threadIdx.x & 63) == 0) atomicOr(health, 2u);
}
__global__ void k_scale_f32(const float* __restrict__ x, float s, float* __restrict__ y, long n) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) y[i] = x[i] * s;
}

inline int grid_for(long work, int block) {
  long g = (work + block - 1) / block;
  if (g > 256 * 16) g = 256 * 16;
  return g < 1 ? 1 : (int)g;
}

}  // namespace

// dyn (nullable, device edm_step_params): step and seed come from it; the Diffuser's stream is the network seed with
// its low word XORed by 0xD1FF05E5 (what tinyedm_amd.Diffuser passes by value otherwise).
extern "C" int edm_diffuse(const float* clean, float* noisy, float* sigma, float P_mean, float P_std, int B, long CHW,
                           unsigned long long seed, unsigned step, const void* dyn, hipStream_t st) {
  EDM_REQUIRE(clean && noisy && sigma && B > 0 && CHW > 0, "diffuse: bad args");
  hipLaunchKernelGGL(k_diffuse, dim3(grid_for((long)B * CHW / 4 + 1, 256)), dim3(256), 0, st, clean, noisy, sigma,
                     P_mean, P_std, B, CHW, (uint32_t)seed, (uint32_t)(seed >> 32), step, (const StepParams*)dyn);
  EDM_CHECK_LAUNCH("diffuse");
  return EDM_OK;
}
extern "C" int edm_diffuse_given(const float* clean, const float* eps, const float* noise, float* noisy, float* sigma,
                                 float P_mean, float P_std, int B, long CHW, hipStream_t st) {
  EDM_REQUIRE(clean && eps && noise && noisy && sigma && B > 0 && CHW > 0, "diffuse_given: bad args");
  hipLaunchKernelGGL(k_diffuse_given, dim3(grid_for((long)B * CHW, 256)), dim3(256), 0, st, clean, eps, noise, noisy,
                     sigma, P_mean, P_std, B, CHW);
  EDM_CHECK_LAUNCH("diffuse_given");
  return EDM_OK;
}
// loss (device scalar) is accumulated (+=): caller zero-fills.  dD may be null (validation).  acc_sum / acc_total
// (nullable device scalars): the metric's epoch state, sum_i mean_j w_i d_ij^2 and the number of samples, += in place.
extern "C" int edm_weighted_mse(const float* D, const float* clean, const float* sigma, const float* weight_override,
                                float sigma_data, float* loss, float* dD, int B, long CHW, float* acc_sum,
                                long long* acc_total, hipStream_t st) {
  EDM_REQUIRE(D && clean && (sigma || weight_override) && loss && B > 0 && CHW > 0, "weighted_mse: bad args");
  const long blocks = ((long)B * CHW + 1023) / 1024;  // ~4 elements per thread, at most 256 workgroups
  hipLaunchKernelGGL(k_loss, dim3((unsigned)(blocks < 256 ? blocks : 256)), dim3(256), 0, st, D, clean, sigma,
                     weight_override, sigma_data, loss, dD, B, CHW, acc_sum, acc_total);
  EDM_CHECK_LAUNCH("weighted_mse");
  return EDM_OK;
}
// step is 1-based (bias corrections use it); ema may be null.  dyn (nullable, device edm_step_params) overrides lr,
// ema_beta, grad_scale and the two bias corrections; zero_grad != 0 clears `grad` in the same pass.  health (nullable
// device word): bit 0 is OR-ed in when a non-finite gradient or updated weight was seen -- the in-graph sentinel a
// replayed step leaves behind for the host to read at its log interval.
extern "C" int edm_adam_ema(float* theta, float* grad, float* m, float* v, float* ema, long n, float lr, float b1,
                            float b2, float eps, int step, float ema_beta, float grad_scale, const void* dyn,
                            int zero_grad, unsigned* health, hipStream_t st) {
  EDM_REQUIRE(theta && grad && m && v && n > 0 && step >= 1, "adam_ema: bad args");
  EDM_REQUIRE(((uintptr_t)theta % 16 == 0) && ((uintptr_t)grad % 16 == 0) && ((uintptr_t)m % 16 == 0) &&
                  ((uintptr_t)v % 16 == 0) && (!ema || (uintptr_t)ema % 16 == 0),
              "adam_ema: arenas must be 16-byte aligned");
  AdamArgs a;
  a.lr = lr; a.b1 = b1; a.b2 = b2; a.eps = eps;
  a.bc1 = (float)(1.0 - pow((double)b1, (double)step));
  a.bc2sqrt = (float)sqrt(1.0 - pow((double)b2, (double)step));
  a.ema_beta = ema_beta;
  a.grad_scale = grad_scale;
  const long n4 = (n + 3) / 4;
  hipLaunchKernelGGL(k_adam_ema, dim3(grid_for(n4, 256)), dim3(256), 0, st, theta, grad, m, v, ema, n4, n, a,
                     (const StepParams*)dyn, zero_grad, health);
  EDM_CHECK_LAUNCH("adam_ema");
  return EDM_OK;
}
// edm_adam_ema over element ranges only (k_adam_ema_ranges): ranges = DEVICE array of n_ranges (first element, length)
// pairs of longs, chunks = DEVICE array of n_chunks (range id, offset inside the range) pairs of ints, one per 1024
// elements.  Both must stay valid and unchanged until the launch has executed (for a captured stream: for the life of the
// graph).  n_chunks == 0 launches nothing.  Everything else as edm_adam_ema.
extern "C" int edm_adam_ema_ranges(float* theta, float* grad, float* m, float* v, float* ema, long n, const long* ranges,
                                   int n_ranges, const int* chunks, int n_chunks, float lr, float b1, float b2,
                                   float eps, int step, float ema_beta, float grad_scale, const void* dyn,
                                   int zero_grad, unsigned* health, hipStream_t st) {
  EDM_REQUIRE(theta && grad && m && v && n > 0 && step >= 1, "adam_ema_ranges: bad args");
  EDM_REQUIRE(n_ranges >= 0 && n_chunks >= 0 && (n_chunks == 0 || (ranges && chunks && n_ranges > 0)),
              "adam_ema_ranges: %d chunks over %d ranges need both tables", n_chunks, n_ranges);
  EDM_REQUIRE(((uintptr_t)theta % 16 == 0) && ((uintptr_t)grad % 16 == 0) && ((uintptr_t)m % 16 == 0) &&
                  ((uintptr_t)v % 16 == 0) && (!ema || (uintptr_t)ema % 16 == 0),
              "adam_ema_ranges: arenas must be 16-byte aligned");
  if (n_chunks == 0) return EDM_OK;
  AdamArgs a;
  a.lr = lr; a.b1 = b1; a.b2 = b2; a.eps = eps;
  a.bc1 = (float)(1.0 - pow((double)b1, (double)step));
  a.bc2sqrt = (float)sqrt(1.0 - pow((double)b2, (double)step));
  a.ema_beta = ema_beta;
  a.grad_scale = grad_scale;
  static_assert(sizeof(AdamRange) == 2 * sizeof(long), "ranges are pairs of longs");
  hipLaunchKernelGGL(k_adam_ema_ranges, dim3((unsigned)n_chunks), dim3(256), 0, st, theta, grad, m, v, ema, n,
                     (const AdamRange*)ranges, n_ranges, (const int2*)chunks, a, (const StepParams*)dyn, zero_grad, health);
  EDM_CHECK_LAUNCH("adam_ema_ranges");
  return EDM_OK;
}
// edm_adam_ema plus K (1..4) post-hoc EMA profile arenas of n floats each: profiles is a HOST array of K device pointers
// (taken by value, so the arenas are fixed for a captured launch), betas a DEVICE array of K floats read at run time.
extern "C" int edm_adam_ema_phema(float* theta, float* grad, float* m, float* v, float* ema, float* const* profiles,
                                  int K, const float* betas, long n, float lr, float b1, float b2, float eps, int step,
                                  float ema_beta, float grad_scale, const void* dyn, int zero_grad, unsigned* health,
                                  hipStream_t st) {
  EDM_REQUIRE(theta && grad && m && v && n > 0 && step >= 1, "adam_ema_phema: bad args");
  EDM_REQUIRE(profiles && betas && K >= 1 && K <= 4, "adam_ema_phema: 1 <= K <= 4 profiles and a beta array required");
  PhemaArenas prof = {{nullptr, nullptr, nullptr, nullptr}};
  for (int k = 0; k < K; ++k) {
    EDM_REQUIRE(profiles[k] && (uintptr_t)profiles[k] % 16 == 0, "adam_ema_phema: profile arenas must be 16-byte aligned");
    prof.p[k] = profiles[k];
  }
  EDM_REQUIRE(((uintptr_t)theta % 16 == 0) && ((uintptr_t)grad % 16 == 0) && ((uintptr_t)m % 16 == 0) &&
                  ((uintptr_t)v % 16 == 0) && (!ema || (uintptr_t)ema % 16 == 0),
              "adam_ema_phema: arenas must be 16-byte aligned");
  AdamArgs a;
  a.lr = lr; a.b1 = b1; a.b2 = b2; a.eps = eps;
  a.bc1 = (float)(1.0 - pow((double)b1, (double)step));
  a.bc2sqrt = (float)sqrt(1.0 - pow((double)b2, (double)step));
  a.ema_beta = ema_beta;
  a.grad_scale = grad_scale;
  const long n4 = (n + 3) / 4;
  const dim3 grid(grid_for(n4, 256)), block(256);
  const StepParams* d = (const StepParams*)dyn;
  switch (K) {
    case 1: hipLaunchKernelGGL(k_adam_ema_phema<1>, grid, block, 0, st, theta, grad, m, v, ema, prof, betas, n4, n, a, d, zero_grad, health); break;
    case 2: hipLaunchKernelGGL(k_adam_ema_phema<2>, grid, block, 0, st, theta, grad, m, v, ema, prof, betas, n4, n, a, d, zero_grad, health); break;
    case 3: hipLaunchKernelGGL(k_adam_ema_phema<3>, grid, block, 0, st, theta, grad, m, v, ema, prof, betas, n4, n, a, d, zero_grad, health); break;
    default: hipLaunchKernelGGL(k_adam_ema_phema<4>, grid, block, 0, st, theta, grad, m, v, ema, prof, betas, n4, n, a, d, zero_grad, health); break;
  }
  EDM_CHECK_LAUNCH("adam_ema_phema");
  return EDM_OK;
}
// acc: DEVICE fp64 [L][n] (row l at acc + l*n), snap: DEVICE fp32 [n], w: HOST array of L doubles; acc_l += w_l * snap
extern "C" int edm_phema_accumulate(double* acc, const float* snap, const double* w, int L, long n, hipStream_t st) {
  EDM_REQUIRE(acc && snap && w && L >= 1 && L <= 8 && n > 0, "phema_accumulate: bad args (1 <= L <= 8)");
  PhemaWeights pw = {};
  for (int l = 0; l < L; ++l) pw.w[l] = w[l];
  const bool vec = n % 4 == 0 && (uintptr_t)acc % 16 == 0 && (uintptr_t)snap % 16 == 0;
  const dim3 grid(grid_for(vec ? n / 4 : n, 256)), block(256);
  switch (L) {
#define EDM_PHEMA_ACC(LL) case LL: hipLaunchKernelGGL(k_phema_accumulate<LL>, grid, block, 0, st, acc, snap, pw, n, vec); break;
    EDM_PHEMA_ACC(1) EDM_PHEMA_ACC(2) EDM_PHEMA_ACC(3) EDM_PHEMA_ACC(4)
    EDM_PHEMA_ACC(5) EDM_PHEMA_ACC(6) EDM_PHEMA_ACC(7) EDM_PHEMA_ACC(8)
#undef EDM_PHEMA_ACC
  }
  EDM_CHECK_LAUNCH("phema_accumulate");
  return EDM_OK;
}
// out = (float)acc, n elements (round to nearest): the last step of a reconstruction
extern "C" int edm_phema_finish(const double* acc, float* out, long n, hipStream_t st) {
  EDM_REQUIRE(acc && out && n > 0, "phema_finish: bad args");
  hipLaunchKernelGGL(k_f64_to_f32, dim3(grid_for(n, 256)), dim3(256), 0, st, acc, out, n);
  EDM_CHECK_LAUNCH("phema_finish");
  return EDM_OK;
}
// health (nullable device word): bit 1 is OR-ed in when the new state holds a non-finite value
extern "C" int edm_heun_euler(const float* x, const float* D, float t0, float t1, float* dx, float* x1, long n,
                              unsigned* health, hipStream_t st) {
  EDM_REQUIRE(x && D && dx && x1 && n > 0 && t0 != 0.f, "heun_euler: bad args");
  hipLaunchKernelGGL(k_heun_euler, dim3(grid_for(n, 256)), dim3(256), 0, st, x, D, t0, t1, dx, x1, n, health);
  EDM_CHECK_LAUNCH("heun_euler");
  return EDM_OK;
}
extern "C" int edm_heun_correct(const float* x, const float* dx, const float* x1, const float* D1, float t0, float t1,
                                float* out, long n, unsigned* health, hipStream_t st) {
  EDM_REQUIRE(x && dx && x1 && D1 && out && n > 0 && t1 != 0.f, "heun_correct: bad args");
  hipLaunchKernelGGL(k_heun_correct, dim3(grid_for(n, 256)), dim3(256), 0, st, x, dx, x1, D1, t0, t1, out, n, health);
  EDM_CHECK_LAUNCH("heun_correct");
  return EDM_OK;
}
static bool aligned16(std::initializer_list<const void*> ps) {
  for (const void* p : ps)
    if (reinterpret_cast<uintptr_t>(p) & 15) return false;
  return true;
}
// w: device pointer to the guidance weight (read by the kernel, so a captured graph follows later writes to it)
extern "C" int edm_heun_euler_guided(const float* x, const float* Dm, const float* Dg, const float* w, float t0,
                                     float t1, float* dx, float* x1, long n, unsigned* health, hipStream_t st) {
  EDM_REQUIRE(x && Dm && Dg && w && dx && x1 && n > 0 && t0 != 0.f, "heun_euler_guided: bad args");
  const bool vec = aligned16({x, Dm, Dg, dx, x1});
  hipLaunchKernelGGL(k_heun_euler_guided, dim3(grid_for(vec ? (n + 3) / 4 : n, 256)), dim3(256), 0, st, x, Dm, Dg, w,
                     t0, t1, dx, x1, n, vec, health);
  EDM_CHECK_LAUNCH("heun_euler_guided");
  return EDM_OK;
}
extern "C" int edm_heun_correct_guided(const float* x, const float* dx, const float* x1, const float* Dm1,
                                       const float* Dg1, const float* w, float t0, float t1, float* out, long n,
                                       unsigned* health, hipStream_t st) {
  EDM_REQUIRE(x && dx && x1 && Dm1 && Dg1 && w && out && n > 0 && t1 != 0.f, "heun_correct_guided: bad args");
  const bool vec = aligned16({x, dx, x1, Dm1, Dg1, out});
  hipLaunchKernelGGL(k_heun_correct_guided, dim3(grid_for(vec ? (n + 3) / 4 : n, 256)), dim3(256), 0, st, x, dx, x1,
                     Dm1, Dg1, w, t0, t1, out, n, vec, health);
  EDM_CHECK_LAUNCH("heun_correct_guided");
  return EDM_OK;
}
// rec: device pointer to {seed_lo, seed_hi, solve_index, 0} (uint32), read by the kernel; step and c by value
extern "C" int edm_heun_churn(const float* x, float c, const void* rec, int step, int B, long CHW, float* x_hat,
                              unsigned* health, hipStream_t st) {
  EDM_REQUIRE(x && rec && x_hat && B > 0 && CHW > 0 && step >= 0 && std::isfinite(c), "heun_churn: bad args");
  EDM_REQUIRE((CHW + 3) / 4 <= 0xFFFFFFFFL, "heun_churn: CHW / 4 must fit the 32-bit Philox counter word");
  const bool vec = CHW % 4 == 0 && aligned16({x, x_hat});
  hipLaunchKernelGGL(k_heun_churn, dim3(grid_for((long)B * ((CHW + 3) / 4), 256)), dim3(256), 0, st, x, c,
                     (const uint32_t*)rec, (uint32_t)step, B, CHW, x_hat, vec, health);
  EDM_CHECK_LAUNCH("heun_churn");
  return EDM_OK;
}
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
  const int chunks = nll_chunks(CHW);
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
// Dg and w both given (guided) or both null; m2 needs m1; m_out nullable.  x_out and m_out alias no operand.
extern "C" int edm_dpm_multistep(const float* x, const float* Dm, const float* Dg, const float* w, const float* m1,
                                 const float* m2, float a, float c0, float c1, float c2, float* x_out, float* m_out,
                                 long n, unsigned* health, hipStream_t st) {
  EDM_REQUIRE(x && Dm && x_out && n > 0 && (Dg == nullptr) == (w == nullptr) && (m1 != nullptr || m2 == nullptr) &&
              std::isfinite(a) && std::isfinite(c0) && std::isfinite(c1) && std::isfinite(c2),
              "dpm_multistep: bad args");
  const bool vec = aligned16({x, Dm, Dg, m1, m2, x_out, m_out});       // (a null pointer counts as aligned)
  const dim3 grid(grid_for(vec ? (n + 3) / 4 : n, 256)), block(256);
  const int H = m2 ? 2 : m1 ? 1 : 0;
#define EDM_DPM_LAUNCH(G_, H_)                                                                                     \
  hipLaunchKernelGGL((k_dpm_multistep<G_, H_>), grid, block, 0, st, x, Dm, Dg, w, m1, m2, a, c0, c1, c2, x_out, \
                     m_out, n, vec, health)
  if (Dg) {
    if (H == 0) EDM_DPM_LAUNCH(true, 0); else if (H == 1) EDM_DPM_LAUNCH(true, 1); else EDM_DPM_LAUNCH(true, 2);
  } else {
    if (H == 0) EDM_DPM_LAUNCH(false, 0); else if (H == 1) EDM_DPM_LAUNCH(false, 1); else EDM_DPM_LAUNCH(false, 2);
  }
#undef EDM_DPM_LAUNCH
  EDM_CHECK_LAUNCH("dpm_multistep");
  return EDM_OK;
}
// image nullable: out = x0*t (edm_scale_f32's result); else out = image + t*x0.  out aliases no operand.
extern "C" int edm_state_init(const float* image, const float* x0, float t, float* out, long n, unsigned* health,
                              hipStream_t st) {
  EDM_REQUIRE(x0 && out && n > 0 && std::isfinite(t) && t >= 0.f, "state_init: bad args");
  const bool vec = aligned16({image, x0, out});        // (a null pointer counts as aligned)
  hipLaunchKernelGGL(k_state_init, dim3(grid_for(vec ? (n + 3) / 4 : n, 256)), dim3(256), 0, st, image, x0, t, out, n,
                     vec, health);
  EDM_CHECK_LAUNCH("state_init");
  return EDM_OK;
}
// rec: device pointer to {seed_lo, seed_hi, solve_index, 0} (uint32), read by the kernel; step and t by value.  step is
// below 2^16: the tag then differs from the churn's in its high half whatever the two steps are.
extern "C" int edm_inpaint_blend(const float* x, const float* image, const unsigned char* mask, float t,
                                 const void* rec, int step, int B, int C, long HW, int mask_B, float* out,
                                 unsigned* health, hipStream_t st) {
  EDM_REQUIRE(x && image && mask && rec && out && B > 0 && C > 0 && HW > 0 && step >= 0 && step < 65536 &&
              (mask_B == 1 || mask_B == B) && std::isfinite(t) && t >= 0.f, "inpaint_blend: bad args");
  const long CHW = (long)C * HW;
  EDM_REQUIRE((CHW + 3) / 4 <= 0xFFFFFFFFL, "inpaint_blend: CHW / 4 must fit the 32-bit Philox counter word");
  const bool vec = CHW % 4 == 0 && HW % 4 == 0 && aligned16({x, image, out}) &&
                   (reinterpret_cast<uintptr_t>(mask) & 3) == 0;
  hipLaunchKernelGGL(k_inpaint_blend, dim3(grid_for((long)B * ((CHW + 3) / 4), 256)), dim3(256), 0, st, x, image, mask,
                     t, (const uint32_t*)rec, (uint32_t)step, B, CHW, HW, mask_B, out, vec, health);
  EDM_CHECK_LAUNCH("inpaint_blend");
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
  const int chunks = nll_chunks(CHW);
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
  const int chunks = nll_chunks(CHW);
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
  const int chunks = nll_chunks(CHW);
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
extern "C" int edm_scale_f32(const float* x, float s, float* y, long n, hipStream_t st) {
  EDM_REQUIRE(x && y && n > 0, "scale_f32: bad args");
  hipLaunchKernelGGL(k_scale_f32, dim3(grid_for(n, 256)), dim3(256), 0, st, x, s, y, n);
  EDM_CHECK_LAUNCH("scale_f32");
  return EDM_OK;
}
