// The input gradient of the denoiser: conv_in's 3x3 dgrad into the IMAGE with the preconditioning folded in
// (networks.py:584-587, 602-603),
//   gx[b,c,h,w] = c_in(sigma_b) * sum_{ky,kx,co} gy[b, h+1-ky, w+1-kx, co] * w^[co,c,ky,kx]      (zero outside the map)
//               + c_skip(sigma_b) * gD[b,c,h,w]                                                   (gD nullable)
// gy: bf16 NHWC [B,H,W,C0]; gx, gD: fp32 NCHW [B,Cimg,H,W], Cimg <= 8.  The constant ones channel gets no gradient.
//
// The kernel is bound by ONE read of gy; the output side is a skinny N (9 * Cimg <= 72 columns per gy pixel), far below an
// MFMA tile, so the products run on the vector ALU in fp32:
//   phase 1  a thread owns a gy pixel and forms its 9 * Cimg dot products over C0,
//              t[p][tap * Cimg + c] = sum_co gy[p, co] * w^[co, c, tap]                 (co ascending, one fma chain each)
//            the pixel's channels are read as 16-byte pieces, eight in flight (one 128-byte line per thread and round);
//            the weights sit in LDS as fp32 [C0][NT] and are read as broadcasts (every lane the same address);
//   phase 2  a thread owns an output element and gathers its nine taps out of the LDS table t,
//              sum = t[(h+1-ky, w+1-kx)][(ky,kx), c]      ky ascending, then kx ascending, taps off the map skipped
//            then gx = fma(c_in, sum, c_skip * gD), written along w (NCHW rows, coalesced).
// A workgroup takes a band of R output rows of one sample (plus one gy row above and below).  The order of every sum is
// fixed and belongs to the sample alone: the result of a sample depends neither on B nor on the band height.
#include "common.h"

namespace {

constexpr int CIN_THREADS = 256;
constexpr int CIN_LDS_BUDGET = 128 * 1024;    // the most a band may take (wide maps, Cimg = 8); the usual shapes use 30-45 KB

__host__ __device__ inline int nt_of(int cimg) { return (9 * cimg + 3) & ~3; }   // weight row pitch: 16-byte rows
__host__ __device__ inline int tp_of(int cimg) { return (9 * cimg) | 1; }        // table row pitch: odd (LDS banks)

// VW: channels per load (8: 16-byte pieces, C0 % 8 == 0 and gy 16-byte aligned; 2: bf16 pairs, C0 even and gy 4-byte
// aligned; 1: element by element).  The three forms run the same fma chains: same bits.
template <int CIMG, int VW>
__global__ void __launch_bounds__(CIN_THREADS)
k_conv_in_dgrad(const bf16* __restrict__ gy, const float* __restrict__ wpk, const float* __restrict__ gD,
                const float* __restrict__ sigma, int sstride, float sd, float* __restrict__ gx, int H, int W, int C0,
                int R) {
  constexpr int NK = 9 * CIMG, NT = (NK + 3) & ~3, TP = NK | 1;
  extern __shared__ __align__(16) float lds[];
  float* wl = lds;                       // [C0][NT]
  float* tl = lds + (long)C0 * NT;       // [(R + 2) * W][TP]
  const int b = blockIdx.y, r0 = blockIdx.x * R;
  const int tid = threadIdx.x;
  for (int i = tid; i < C0 * NT / 4; i += CIN_THREADS)
    reinterpret_cast<f32x4*>(wl)[i] = reinterpret_cast<const f32x4*>(wpk)[i];
  __syncthreads();

  const int NP = (R + 2) * W;
  for (int p = tid; p < NP; p += CIN_THREADS) {
    const int row = r0 - 1 + p / W, col = p % W;
    float acc[NK];
#pragma unroll
    for (int k = 0; k < NK; ++k) acc[k] = 0.f;
    if (row >= 0 && row < H) {
      const bf16* gp = gy + (((long)b * H + row) * W + col) * C0;
      if constexpr (VW == 8) {
        int co = 0;
        for (; co + 64 <= C0; co += 64) {      // one 128-byte line per round: eight loads in flight
          bf16x8 v[8];
#pragma unroll
          for (int q = 0; q < 8; ++q) v[q] = *reinterpret_cast<const bf16x8*>(gp + co + 8 * q);
#pragma unroll
          for (int q = 0; q < 8; ++q)
#pragma unroll
            for (int j = 0; j < 8; ++j) {
              const float g = (float)v[q][j];
              const float* wr = wl + (co + 8 * q + j) * NT;
#pragma unroll
              for (int k = 0; k < NK; ++k) acc[k] = fmaf(g, wr[k], acc[k]);
            }
        }
        for (; co < C0; co += 8) {
          const bf16x8 v = *reinterpret_cast<const bf16x8*>(gp + co);
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            const float g = (float)v[j];
            const float* wr = wl + (co + j) * NT;
#pragma unroll
            for (int k = 0; k < NK; ++k) acc[k] = fmaf(g, wr[k], acc[k]);
          }
        }
      } else {
        for (int co = 0; co < C0; co += VW) {
          float g[VW];
          if constexpr (VW == 2) {
            const bf16x2 v = *reinterpret_cast<const bf16x2*>(gp + co);
            g[0] = (float)v[0];
            g[1] = (float)v[1];
          } else {
            g[0] = (float)gp[co];
          }
#pragma unroll
          for (int j = 0; j < VW; ++j) {
            const float* wr = wl + (co + j) * NT;
#pragma unroll
            for (int k = 0; k < NK; ++k) acc[k] = fmaf(g[j], wr[k], acc[k]);
          }
        }
      }
    }
    float* tp = tl + (long)p * TP;
#pragma unroll
    for (int k = 0; k < NK; ++k) tp[k] = acc[k];
  }
  __syncthreads();

  const float s = sigma[(long)b * sstride];
  const float den = s * s + sd * sd;
  const float cin = rsqrtf(sd * sd + s * s);      // (k_precond_in's expression)
  const float cskip = sd * sd / den;              // (k_conv_out_fwd's expression)
  const int RW = R * W;
  for (int o = tid; o < RW * CIMG; o += CIN_THREADS) {
    const int c = o / RW, rem = o - c * RW;
    const int rr = rem / W, col = rem - rr * W;
    const int h = r0 + rr;
    if (h >= H) continue;
    float sum = 0.f;
#pragma unroll
    for (int ky = 0; ky < 3; ++ky)
#pragma unroll
      for (int kx = 0; kx < 3; ++kx) {
        const int sc = col + 1 - kx;        // rows off the map hold zeros; columns off the map are not in the table
        if (sc >= 0 && sc < W) sum += tl[(long)((rr + 2 - ky) * W + sc) * TP + (ky * 3 + kx) * CIMG + c];
      }
    const long e = (((long)b * CIMG + c) * H + h) * W + col;
    float add = 0.f;
    if (gD) {
      add = cskip * gD[e];
      asm volatile("" : "+v"(add));         // the product is rounded on its own: gy = 0 gives c_skip * gD bit for bit
    }
    gx[e] = fmaf(cin, sum, add);
  }
}

template <int CIMG>
void launch_c(int vw, dim3 grid, size_t lds, hipStream_t st, const bf16* gy, const float* wpk, const float* gD,
              const float* sigma, int sstride, float sd, float* gx, int H, int W, int C0, int R) {
#define EDM_CIN_LAUNCH(VW_)                                                                                          \
  do {                                                                                                               \
    EDM_MAX_LDS((k_conv_in_dgrad<CIMG, VW_>), CIN_LDS_BUDGET);                                                       \
    hipLaunchKernelGGL((k_conv_in_dgrad<CIMG, VW_>), grid, dim3(CIN_THREADS), lds, st, gy, wpk, gD, sigma, sstride,  \
                       sd, gx, H, W, C0, R);                                                                         \
  } while (0)
  if (vw == 8) EDM_CIN_LAUNCH(8);
  else if (vw == 2) EDM_CIN_LAUNCH(2);
  else EDM_CIN_LAUNCH(1);
#undef EDM_CIN_LAUNCH
}

// rows of a band: about one gy pixel per thread and round (8 table rows at least), within the LDS budget; 0 = does not fit
int band_rows(int H, int W, int C0, int Cimg) {
  int rows = (CIN_THREADS + W - 1) / W;
  if (rows < 8) rows = 8;
  int R = rows - 2 < H ? rows - 2 : H;
  const long wbytes = (long)C0 * nt_of(Cimg) * 4;
  while (R >= 1 && wbytes + (long)(R + 2) * W * tp_of(Cimg) * 4 > CIN_LDS_BUDGET) --R;
  return R;
}

}  // namespace

// elements of the weight pack of edm_conv_in_dgrad: fp32 [C0][NT], NT = 9 * Cimg rounded up to 4,
// pack[co][(ky * 3 + kx) * Cimg + c] = w^[co, c, ky, kx] (the bf16-rounded forward operand), the padding columns zero
extern "C" int edm_conv_in_dgrad_pack_cols(int Cimg) { return nt_of(Cimg); }

extern "C" int edm_conv_in_dgrad(const void* gy, const float* wpack, const float* gD, const float* sigma,
                                 int sigma_stride, float sigma_data, float* gx, int B, int Cimg, int H, int W, int C0,
                                 hipStream_t st) {
  EDM_REQUIRE(gy && wpack && sigma && gx && B > 0 && B <= 65535 && Cimg >= 1 && Cimg <= 8 && H > 0 && W > 0 && C0 > 0 &&
                  (sigma_stride == 0 || sigma_stride == 1),
              "conv_in_dgrad: bad args (1 <= Cimg <= 8, B <= 65535, sigma_stride 0 or 1)");
  EDM_REQUIRE((long)B * H * W * C0 < (1L << 40) && (reinterpret_cast<uintptr_t>(wpack) & 15) == 0 &&
                  (reinterpret_cast<uintptr_t>(gy) & 1) == 0 && (reinterpret_cast<uintptr_t>(gx) & 3) == 0 &&
                  (reinterpret_cast<uintptr_t>(gD) & 3) == 0,
              "conv_in_dgrad: operands too large or misaligned (pack: 16 bytes; gy: 2; gx, gD: 4)");
  const int R = band_rows(H, W, C0, Cimg);
  if (R < 1) {
    edm_set_error("conv_in_dgrad: a band of W = %d, C0 = %d, Cimg = %d does not fit the LDS", W, C0, Cimg);
    return EDM_ERR_UNSUPPORTED;
  }
  const uintptr_t ga = reinterpret_cast<uintptr_t>(gy);
  const int vw = (C0 % 8 == 0 && (ga & 15) == 0) ? 8 : ((C0 % 2 == 0 && (ga & 3) == 0) ? 2 : 1);
  const size_t lds = ((size_t)C0 * nt_of(Cimg) + (size_t)(R + 2) * W * tp_of(Cimg)) * 4;
  const dim3 grid((H + R - 1) / R, B);
  const bf16* g = (const bf16*)gy;
  switch (Cimg) {
    case 1: launch_c<1>(vw, grid, lds, st, g, wpack, gD, sigma, sigma_stride, sigma_data, gx, H, W, C0, R); break;
    case 2: launch_c<2>(vw, grid, lds, st, g, wpack, gD, sigma, sigma_stride, sigma_data, gx, H, W, C0, R); break;
    case 3: launch_c<3>(vw, grid, lds, st, g, wpack, gD, sigma, sigma_stride, sigma_data, gx, H, W, C0, R); break;
    case 4: launch_c<4>(vw, grid, lds, st, g, wpack, gD, sigma, sigma_stride, sigma_data, gx, H, W, C0, R); break;
    case 5: launch_c<5>(vw, grid, lds, st, g, wpack, gD, sigma, sigma_stride, sigma_data, gx, H, W, C0, R); break;
    case 6: launch_c<6>(vw, grid, lds, st, g, wpack, gD, sigma, sigma_stride, sigma_data, gx, H, W, C0, R); break;
    case 7: launch_c<7>(vw, grid, lds, st, g, wpack, gD, sigma, sigma_stride, sigma_data, gx, H, W, C0, R); break;
    default: launch_c<8>(vw, grid, lds, st, g, wpack, gD, sigma, sigma_stride, sigma_data, gx, H, W, C0, R); break;
  }
  EDM_CHECK_LAUNCH("conv_in_dgrad");
  return EDM_OK;
}
