// The fp32 kernels of the training step around the network: Diffuser (edm.py:84-93), sigma-weighted MSE
// (edm.py:212, metric.py:8-18), fused Adam + power-function EMA over the flat parameter arena
// (edm.py:251-253, ema.py:137-140, 273) and the post-hoc EMA reconstruction.  The sampler's updates live in
// solver_steps.hip, the likelihood and noise-level evaluation kernels in sample_eval.hip.
#include "common.h"
#include "quads.h"
#include <math.h>
#include <cmath>

namespace {

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

// same with the two normal draws supplied (deterministic tests / external RNG).  Not on the training path, and what other
// code is compared against: sigma is exp(P_mean + P_std*eps) evaluated in double and rounded once (half an ulp).  In
// fp32 the rounding of the argument alone is up to 2 u of sigma at |argument| in [2, 4) and the device expf adds 2-3 u more.
__global__ void k_diffuse_given(const float* __restrict__ clean, const float* __restrict__ eps,
                                const float* __restrict__ noise, float* __restrict__ noisy, float* __restrict__ sigma,
                                float P_mean, float P_std, int B, long CHW) {
  const long total = (long)B * CHW;
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
    const int b = (int)(e / CHW);
    const float s = (float)exp((double)P_mean + (double)P_std * (double)eps[b]);
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
        bad |= nonfinite(gj) || nonfinite(t[j]);
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
        bad |= nonfinite(gj) || nonfinite(tj);
      }
    }
  }
  EDM_RAISE_HEALTH(health, bad, 1u);
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
  EDM_RAISE_HEALTH(health, bad, 1u);
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
        bad |= nonfinite(gj) || nonfinite(t[j]);
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
        bad |= nonfinite(gj) || nonfinite(tj);
      }
    }
  }
  EDM_RAISE_HEALTH(health, bad, 1u);
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
