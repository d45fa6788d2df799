// Zero-shot restoration (DDNM, Wang et al. 2023): the measurement operator A of the box down-sampling / grey-value
// family and the range / null-space projection of a denoiser output onto {x : A x = y},
//   D^ = D + A+ (y - A D).
// A averages every S x S pixel block (S in {1, 2, 4, 8}) and, with `gray`, also the C <= 8 channels; A+ replicates a
// value to its block.  Tensors are the solver state's: contiguous fp32 NCHW.
#include "common.h"
#include <initializer_list>

namespace {

inline int grid_for(long work, int block) {
  long g = (work + block - 1) / block;
  if (g > 256 * 16) g = 256 * 16;
  return g < 1 ? 1 : (int)g;
}
bool aligned16(std::initializer_list<const void*> ps) {
  for (const void* p : ps)
    if (reinterpret_cast<uintptr_t>(p) & 15) return false;
  return true;
}

// SW consecutive values of a row of D = Dg + w*(Dm - Dg) (Dg non-null; heun_euler_guided's expression) or of D = Dm
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
      for (int j = 0; j < 4; ++j) v[4 * q + j] = Dg ? fmaf(w, m[j] - g[j], g[j]) : m[j];
    }
  } else {
#pragma unroll
    for (int j = 0; j < SW; ++j) v[j] = Dg ? fmaf(w, Dm[e + j] - Dg[e + j], Dg[e + j]) : Dm[e + j];
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
            bad |= !(fabsf(v[j]) <= 3.0e38f);
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
  if (PROJECT && health && __any(bad) && (threadIdx.x & 63) == 0) atomicOr(health, 2u);
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
