// The updates of the samplers around the network evaluations (solvers.py): the Heun stages and their guided forms, the
// churn of the stochastic sampler, the state of an image-conditioned solve, the replacement step of inpainting and the
// DPM-Solver++ multistep update.  One pass over the state each, fp32; the step expressions are those of quads.h.
#include "common.h"
#include "quads.h"

#include <cmath>

namespace {

// dx = (x-D)/t0 ; x1 = x + (t1-t0)*dx
__global__ void k_heun_euler(const float* __restrict__ x, const float* __restrict__ Dn, float t0, float t1,
                             float* __restrict__ dx, float* __restrict__ x1, long n, unsigned* __restrict__ health) {
  bool bad = false;     // health word (nullable): bit 1 = a non-finite sampler state
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    float d;
    const float o = heun_euler_stage(x[i], Dn[i], t0, t1, d);
    dx[i] = d;
    x1[i] = o;
    bad |= nonfinite(o);
  }
  EDM_RAISE_HEALTH(health, bad, 2u);
}
// dxp = (x1-D1)/t1 ; out = x + (t1-t0)*(0.5*dx + 0.5*dxp)
__global__ void k_heun_correct(const float* __restrict__ x, const float* __restrict__ dx, const float* __restrict__ x1,
                               const float* __restrict__ D1, float t0, float t1, float* __restrict__ out, long n,
                               unsigned* __restrict__ health) {
  bool bad = false;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const float o = heun_update(x[i], heun_slope(dx[i], x1[i], D1[i], t1), t0, t1);
    out[i] = o;
    bad |= nonfinite(o);
  }
  EDM_RAISE_HEALTH(health, bad, 2u);
}
// Guided updates: D = Dg + w*(Dm - Dg) in registers, then the unguided kernels' functions (w == 0 gives
// exactly the unguided result on Dg: fmaf(0, d, Dg) == Dg).  w is read from device memory so that a captured solve
// replays with whatever guidance the host wrote there.  vec: every pointer 16-byte aligned -> dwordx4 over the first
// n/4*4 elements, the tail (and the whole range when !vec) element by element.
__device__ __forceinline__ float heun_euler_guided_1(float x, float Dm, float Dg, float w, float t0, float t1,
                                                     float& dx, bool& bad) {
  const float o = heun_euler_stage(x, guidance_mix(w, Dm, Dg), t0, t1, dx);
  bad |= nonfinite(o);
  return o;
}
__device__ __forceinline__ float heun_correct_guided_1(float x, float dx, float x1, float Dm1, float Dg1, float w,
                                                       float t0, float t1, bool& bad) {
  const float o = heun_update(x, heun_slope(dx, x1, guidance_mix(w, Dm1, Dg1), t1), t0, t1);
  bad |= nonfinite(o);
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
  EDM_RAISE_HEALTH(health, bad, 2u);
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
  EDM_RAISE_HEALTH(health, bad, 2u);
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
        bad |= nonfinite(ov[k]);
      }
      *reinterpret_cast<f32x4*>(x_hat + e) = ov;
    } else {
      const int m = quad_len<false>(CHW, q);
      for (int k = 0; k < m; ++k) {
        const float o = fmaf(c, nn[k], x[e + k]);
        bad |= nonfinite(o);
        x_hat[e + k] = o;
      }
    }
  }
  EDM_RAISE_HEALTH(health, bad, 2u);
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
        bad |= nonfinite(ov[j]);
      }
      *reinterpret_cast<f32x4*>(out + i) = ov;
    }
  }
  for (long i = head + tid; i < n; i += stride) {
    const float o = image ? fmaf(t, x0[i], image[i]) : x0[i] * t;
    bad |= nonfinite(o);
    out[i] = o;
  }
  EDM_RAISE_HEALTH(health, bad, 2u);
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
    const int m = vec ? 4 : quad_len<false>(CHW, q);
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
        bad |= nonfinite(ov[k]);
      }
      *reinterpret_cast<f32x4*>(out + e) = ov;
    } else {
      for (int k = 0; k < m; ++k) {
        const float o = keep[k] ? (t != 0.f ? fmaf(t, nn[k], image[e + k]) : image[e + k]) : x[e + k];
        bad |= nonfinite(o);
        out[e + k] = o;
      }
    }
  }
  EDM_RAISE_HEALTH(health, bad, 2u);
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
  m = G ? guidance_mix(w, Dm, Dg) : Dm;
  float o = c0 * m;
  if (H >= 1) o = fmaf(c1, m1, o);
  if (H >= 2) o = fmaf(c2, m2, o);
  o = fmaf(a, x, o);
  bad |= nonfinite(o);
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
  EDM_RAISE_HEALTH(health, bad, 2u);
}
__global__ void k_scale_f32(const float* __restrict__ x, float s, float* __restrict__ y, long n) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) y[i] = x[i] * s;
}

}  // namespace

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
extern "C" int edm_scale_f32(const float* x, float s, float* y, long n, hipStream_t st) {
  EDM_REQUIRE(x && y && n > 0, "scale_f32: bad args");
  hipLaunchKernelGGL(k_scale_f32, dim3(grid_for(n, 256)), dim3(256), 0, st, x, s, y, n);
  EDM_CHECK_LAUNCH("scale_f32");
  return EDM_OK;
}
