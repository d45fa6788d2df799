// Zero-shot restoration (DDNM, Wang et al. 2023): the measurement operator A of the box down-sampling / grey-value
// family and the range / null-space projection of a denoiser output onto {x : A x = y},
//   D^ = D + A+ (y - A D).
// A averages every S x S pixel block (S in {1, 2, 4, 8}) and, with `gray`, also the C <= 8 channels; A+ replicates a
// value to its block.  Tensors are the solver state's: contiguous fp32 NCHW.
#include "common.h"
#include "quads.h"

namespace {

// SW consecutive values of a row of D = Dg + w*(Dm - Dg) (Dg non-null; guidance_mix of quads.h) or of D = Dm
template <int SW, bool VEC>
__device__ __forceinline__ void load_row(const float* __restrict__ Dm, const float* __restrict__ Dg, float w, long e,
                                         float (&v)[SW]) {
  if constexpr (VEC) {
#pragma unroll
    for (int q = 0; q < SW / 4; ++q) {
      const f32x4 m = *reinterpret_cast<const f32x4*>(Dm + e + 4 * q);
      f32x4 g{};
      if (Dg) g = *reinterpret_cast<const f32x4*>(Dg + e + 4 * q);
#pragma unroll
      for (int j = 0; j < 4; ++j) v[4 * q + j] = Dg ? guidance_mix(w, m[j], g[j]) : m[j];
    }
  } else {
#pragma unroll
    for (int j = 0; j < SW; ++j) v[j] = Dg ? guidance_mix(w, Dm[e + j], Dg[e + j]) : Dm[e + j];
  }
}

// One thread owns whole blocks: a strip of SW columns (NB = SW / S blocks side by side) over the S rows of a block row,
// and over all C channels when gray.  VEC (W % 4 == 0, every operand 16-byte aligned): SW = max(4, S), every row of the
// strip is one dwordx4 (two for S = 8); otherwise SW = S, one block per thread, element by element.  Neighbouring
// threads take neighbouring strips of the same rows.  The sum of a block is ONE sequential fp32 chain whatever the path:
//   acc = 0;  for c ascending (gray only): for row ascending: for column ascending: acc += D[c][row][column]
//   mean = acc * inv_n      (inv_n = 1.0f / n on the host, n = S*S*(gray ? C : 1))
// PROJECT: out = D + (y_block - mean), the correction formed once per block (product, subtraction and addition each
// rounded on its own), D read a second time (it has just been read: the cache serves it) instead of being kept in up
// to S*S*C registers.  !PROJECT: out = y = mean, [B, gray ? 1 : C, H/S, W/S].
template <int S, bool VEC, bool PROJECT>
__global__ void __launch_bounds__(256)
k_restore(const float* __restrict__ Dm, const float* __restrict__ Dg, const float* __restrict__ w,
          const float* __restrict__ y, float* __restrict__ out, int B, int C, int H, int W, int gray, float inv_n,
          unsigned* __restrict__ health) {
  constexpr int NB = VEC && S < 4 ? 4 / S : 1, SW = NB * S;
  constexpr int UNR = S > 4 ? 4 : S;        // rows in flight per thread: at most 4 (x 2 dwordx4 for S = 8)
  const float wv = Dg ? *w : 0.f;
  const int Cp = gray ? 1 : C, CC = gray ? C : 1;
  const int Hs = H / S, Ws = W / S, nstrip = W / SW;
  const long HW = (long)H * W, total = (long)B * Cp * Hs * nstrip;
  bool bad = false;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int strip = (int)(i % nstrip);
    long r = i / nstrip;
    const int by = (int)(r % Hs);
    r /= Hs;
    const int cp = (int)(r % Cp);
    const long b = r / Cp;
    const long e0 = ((b * C + cp) * H + (long)by * S) * W + (long)strip * SW;
    float acc[NB];
#pragma unroll
    for (int k = 0; k < NB; ++k) acc[k] = 0.f;
    for (int c = 0; c < CC; ++c) {
#pragma unroll UNR
      for (int row = 0; row < S; ++row) {
        float v[SW];
        load_row<SW, VEC>(Dm, Dg, wv, e0 + c * HW + (long)row * W, v);
#pragma unroll
        for (int j = 0; j < SW; ++j) acc[j / S] += v[j];
      }
    }
    const long ye = ((b * Cp + cp) * Hs + by) * Ws + (long)strip * NB;
    if constexpr (!PROJECT) {
#pragma unroll
      for (int k = 0; k < NB; ++k) out[ye + k] = acc[k] * inv_n;
    } else {
      float corr[NB];
#pragma unroll
      for (int k = 0; k < NB; ++k) {
        // the product is rounded on its own, as edm_degrade stores it: the library is built with -ffp-contract=fast,
        // whose fusion of mean into the subtraction (one rounding less) would make project(D, degrade(D)) differ from
        // D; the empty asm pins the rounded product in a register
        float mean = acc[k] * inv_n;
        asm volatile("" : "+v"(mean));
        corr[k] = y[ye + k] - mean;
      }
      for (int c = 0; c < CC; ++c) {
#pragma unroll UNR
        for (int row = 0; row < S; ++row) {
          const long e = e0 + c * HW + (long)row * W;
          float v[SW];
          load_row<SW, VEC>(Dm, Dg, wv, e, v);
#pragma unroll
          for (int j = 0; j < SW; ++j) {
            v[j] = v[j] + corr[j / S];
            bad |= nonfinite(v[j]);
          }
          if constexpr (VEC) {
#pragma unroll
            for (int q = 0; q < SW / 4; ++q)
              *reinterpret_cast<f32x4*>(out + e + 4 * q) = f32x4{v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]};
          } else {
#pragma unroll
            for (int j = 0; j < SW; ++j) out[e + j] = v[j];
          }
        }
      }
    }
  }
  if (PROJECT) EDM_RAISE_HEALTH(health, bad, 2u);
}

bool shape_ok(int B, int C, int H, int W, int scale, int gray) {
  return B > 0 && C > 0 && H > 0 && W > 0 && (scale == 1 || scale == 2 || scale == 4 || scale == 8) &&
         !(scale == 1 && !gray) && H % scale == 0 && W % scale == 0 && (!gray || C <= 8);
}

template <bool PROJECT>
void launch(const float* Dm, const float* Dg, const float* w, const float* y, float* out, int B, int C, int H, int W,
            int scale, int gray, bool vec, unsigned* health, hipStream_t st) {
  const int sw = vec && scale < 4 ? 4 : scale;
  const long total = (long)B * (gray ? 1 : C) * (H / scale) * (W / sw);
  const float inv_n = 1.0f / (float)(scale * scale * (gray ? C : 1));
  const dim3 grid(grid_for(total, 256)), block(256);
#define EDM_RESTORE_LAUNCH(S_)                                                                                       \
  if (vec)                                                                                                           \
    hipLaunchKernelGGL((k_restore<S_, true, PROJECT>), grid, block, 0, st, Dm, Dg, w, y, out, B, C, H, W, gray,      \
                       inv_n, health);                                                                               \
  else                                                                                                               \
    hipLaunchKernelGGL((k_restore<S_, false, PROJECT>), grid, block, 0, st, Dm, Dg, w, y, out, B, C, H, W, gray,     \
                       inv_n, health)
  switch (scale) {
    case 1: EDM_RESTORE_LAUNCH(1); break;
    case 2: EDM_RESTORE_LAUNCH(2); break;
    case 4: EDM_RESTORE_LAUNCH(4); break;
    default: EDM_RESTORE_LAUNCH(8); break;
  }
#undef EDM_RESTORE_LAUNCH
}

}  // namespace

// y = A x.  x: [B, C, H, W], y: [B, gray ? 1 : C, H/scale, W/scale], both contiguous fp32; y does not alias x.
extern "C" int edm_degrade(const float* x, float* y, int B, int C, int H, int W, int scale, int gray, hipStream_t st) {
  EDM_REQUIRE(x && y && shape_ok(B, C, H, W, scale, gray),
              "degrade: bad args (scale in {1, 2, 4, 8}, not the identity, H and W multiples of scale, gray needs C <= 8)");
  launch<false>(x, nullptr, nullptr, nullptr, y, B, C, H, W, scale, gray, W % 4 == 0 && aligned16({x, y}), nullptr, st);
  EDM_CHECK_LAUNCH("degrade");
  return EDM_OK;
}
// out = D + A+ (y - A D), D = Dg + w*(Dm - Dg) when Dg and w are both given (w: device pointer to the guidance weight,
// read by the kernel), else D = Dm.  out aliases no operand.
extern "C" int edm_project_denoised(const float* Dm, const float* Dg, const float* w, const float* y, float* out, int B,
                                    int C, int H, int W, int scale, int gray, unsigned* health, hipStream_t st) {
  EDM_REQUIRE(Dm && y && out && (Dg == nullptr) == (w == nullptr) && shape_ok(B, C, H, W, scale, gray),
              "project_denoised: bad args (scale in {1, 2, 4, 8}, not the identity, H and W multiples of scale, gray "
              "needs C <= 8, Dg and w together)");
  EDM_REQUIRE(out != Dm && out != Dg && out != y, "project_denoised: out must not alias an operand");
  const bool vec = W % 4 == 0 && aligned16({Dm, Dg, y, out});       // (a null pointer counts as aligned)
  launch<true>(Dm, Dg, w, y, out, B, C, H, W, scale, gray, vec, health, st);
  EDM_CHECK_LAUNCH("project_denoised");
  return EDM_OK;
}

// ------------------------------------------------------------------ diffusion posterior sampling (Chung et al. 2023)
// The measurement side of a DPS step: the adjoint of the averaging operator, a small zero-padded Gaussian blur (its own
// adjoint), the residual r = y - A D with its per-sample 2-norm, and the guided update x' + (zeta / ||r||) g.
namespace {

struct BlurTaps {
  float k[9];     // 2 * radius + 1 normalised taps
};

// out[b,c,h,w] = r[b, gray ? 0 : c, h / S, w / S] * inv_n: A^T of the block (and channel) mean
__global__ void __launch_bounds__(256)
k_degrade_adjoint(const float* __restrict__ r, float* __restrict__ out, int C, int H, int W, int S, int gray,
                  float inv_n, long total) {
  const int Hs = H / S, Ws = W / S, Cp = gray ? 1 : C;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int w = (int)(i % W);
    long q = i / W;
    const int h = (int)(q % H);
    q /= H;
    const int c = (int)(q % C);
    const long b = q / C;
    out[i] = r[((b * Cp + (gray ? 0 : c)) * Hs + h / S) * Ws + w / S] * inv_n;
  }
}

// y[p,h,w] = sum_dy k[dy] * (sum_dx k[dx] * x[p, h+dy-R, w+dx-R]), zero outside the map; both sums are fma chains in
// ascending order over ALL 2R+1 taps (a tap off the map adds 0), so a plane's bits depend on nothing but the plane
__global__ void __launch_bounds__(256)
k_blur2d(const float* __restrict__ x, float* __restrict__ y, BlurTaps taps, int R, int H, int W, long total) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int w = (int)(i % W);
    const long q = i / W;
    const int h = (int)(q % H);
    const float* xp = x + (q / H) * (long)H * W;
    float acc = 0.f;
    for (int dy = 0; dy <= 2 * R; ++dy) {
      const int hh = h + dy - R;
      float row = 0.f;
      if (hh >= 0 && hh < H) {
        for (int dx = 0; dx <= 2 * R; ++dx) {
          const int ww = w + dx - R;
          const float v = (ww >= 0 && ww < W) ? xp[(long)hh * W + ww] : 0.f;
          row = fmaf(taps.k[dx], v, row);
        }
      }
      acc = fmaf(taps.k[dy], row, acc);
    }
    y[i] = acc;
  }
}

// r = y - AD and nrm[b] = sqrt(sum r^2) of sample b: one workgroup per sample; thread t adds the squares of elements
// t, t + 256, ... in that order, then the 256 partial sums meet in a fixed binary tree -- no atomics, nothing that depends
// on B or on the grid: the same bits on every run
__global__ void __launch_bounds__(256)
k_dps_residual(const float* __restrict__ y, const float* __restrict__ AD, float* __restrict__ r, float* __restrict__ nrm,
               long n) {
  __shared__ float part[256];
  const long base = (long)blockIdx.x * n;
  float acc = 0.f;
  for (long i = threadIdx.x; i < n; i += 256) {
    const float d = y[base + i] - AD[base + i];
    r[base + i] = d;
    acc = fmaf(d, d, acc);
  }
  part[threadIdx.x] = acc;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) part[threadIdx.x] += part[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) nrm[blockIdx.x] = sqrtf(part[0]);
}

// out = x + (scale / nrm[b]) * g, out = x where nrm[b] == 0 (bit for bit x); the factor is one division per sample
__global__ void __launch_bounds__(256)
k_dps_update(const float* __restrict__ x, const float* __restrict__ g, const float* __restrict__ nrm, float scale,
             float* __restrict__ out, long n, long total, unsigned* __restrict__ health) {
  bool bad = false;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const float nb = nrm[i / n];
    float v = x[i];
    if (nb != 0.f && scale != 0.f) v = fmaf(scale / nb, g[i], v);
    bad |= nonfinite(v);
    out[i] = v;
  }
  EDM_RAISE_HEALTH(health, bad, 2u);
}

}  // namespace

// out = A^T r for the averaging A of edm_degrade: r [B, gray ? 1 : C, H/scale, W/scale] -> out [B, C, H, W], every value
// replicated to its block (and channels) and multiplied by 1 / n, n = scale*scale*(gray ? C : 1).  out does not alias r.
extern "C" int edm_degrade_adjoint(const float* r, float* out, int B, int C, int H, int W, int scale, int gray,
                                   hipStream_t st) {
  EDM_REQUIRE(r && out && r != out && shape_ok(B, C, H, W, scale, gray),
              "degrade_adjoint: bad args (scale in {1, 2, 4, 8}, not the identity, H and W multiples of scale, gray needs "
              "C <= 8)");
  const long total = (long)B * C * H * W;
  const float inv_n = 1.0f / (float)(scale * scale * (gray ? C : 1));
  hipLaunchKernelGGL(k_degrade_adjoint, dim3(grid_for(total, 256)), dim3(256), 0, st, r, out, C, H, W, scale, gray, inv_n,
                     total);
  EDM_CHECK_LAUNCH("degrade_adjoint");
  return EDM_OK;
}
// y = K x: the separable blur with the 2*radius+1 taps `taps` (HOST pointer, copied into the launch), zero padding,
// on each of the `planes` H x W planes of x (contiguous fp32; y does not alias x).  radius 1..4.
extern "C" int edm_blur2d(const float* x, float* y, const float* taps, int radius, long planes, int H, int W,
                          hipStream_t st) {
  EDM_REQUIRE(x && y && x != y && taps && radius >= 1 && radius <= 4 && planes > 0 && H > 0 && W > 0,
              "blur2d: bad args (radius 1..4, y must not alias x)");
  BlurTaps t{};
  for (int k = 0; k <= 2 * radius; ++k) t.k[k] = taps[k];
  const long total = planes * H * W;
  hipLaunchKernelGGL(k_blur2d, dim3(grid_for(total, 256)), dim3(256), 0, st, x, y, t, radius, H, W, total);
  EDM_CHECK_LAUNCH("blur2d");
  return EDM_OK;
}
// r = y - AD (n elements per sample, all contiguous fp32 [B, n]; r may alias neither) and nrm[b] = ||r_b||_2, an
// order-fixed reduction: bit-identical from run to run and independent of B.
extern "C" int edm_dps_residual(const float* y, const float* AD, float* r, float* nrm, int B, long n, hipStream_t st) {
  EDM_REQUIRE(y && AD && r && nrm && B > 0 && n > 0 && r != y && r != AD, "dps_residual: bad args");
  hipLaunchKernelGGL(k_dps_residual, dim3(B), dim3(256), 0, st, y, AD, r, nrm, n);
  EDM_CHECK_LAUNCH("dps_residual");
  return EDM_OK;
}
// out = x + (scale / nrm[b]) * g for sample b, out = x bit for bit where nrm[b] == 0 or scale == 0; [B, n] fp32, out aliases
// no operand.  Same health bit as the Heun updates.
extern "C" int edm_dps_update(const float* x, const float* g, const float* nrm, float scale, float* out, int B, long n,
                              unsigned* health, hipStream_t st) {
  EDM_REQUIRE(x && g && nrm && out && B > 0 && n > 0 && out != g && out != x, "dps_update: bad args (out aliases no operand)");
  const long total = (long)B * n;
  hipLaunchKernelGGL(k_dps_update, dim3(grid_for(total, 256)), dim3(256), 0, st, x, g, nrm, scale, out, n, total, health);
  EDM_CHECK_LAUNCH("dps_update");
  return EDM_OK;
}
