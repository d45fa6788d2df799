// Paired image quality: SSIM and the squared error of image i against image i, and the LPIPS-form distance between two
// sets of denoiser activations (include/tinyedm_hip.h states the contracts).
//
// edm_pair_ssim (Wang, Bovik, Sheikh, Simoncelli 2004).  Everything is fp64: E[a^2] - mu_a^2 in fp32 at L = 255 loses the
// variance of flat regions.  The valid region (window centres at least (win - 1) / 2 from every edge) is cut into tiles of
// SSIM_TH x SSIM_TW centres anchored at its corner, so the tiling is a function of (H, W, win) alone.  One workgroup owns
// one (image, channel, tile): it stages the two input tiles with their halo in LDS as doubles (element strides: uint8
// NHWC and float32 NCHW go through the same code, no copy), filters rows, then columns, out of LDS, forms the SSIM map and
// adds it up in a fixed order: thread t of 256 adds its centres t, t + 256 in ascending order, then a halving tree over
// the 256 threads.  A second kernel adds the tile partials in tile order and divides once.  The squared error rides
// along: a tile owns the pixels of its SSIM_TH x SSIM_TW block (the last tile row / column also the halo behind it), so
// every pixel is counted once.  No atomics; every output element is one ordinary store.
// LDS: consecutive lanes read consecutive doubles of one row in both passes (no bank conflicts for 8-byte reads); 62 KiB
// per workgroup, two workgroups per CU.
//
// edm_f32_pair_feature_distance (the distance of Zhang et al. 2018 without its learned layers).  One workgroup per
// sample, FD_WAVES waves; a wave owns pixel rows wave, wave + FD_WAVES, ... and keeps one row of each map (at most
// FD_MAX_C channels: 12 floats per lane and map) in registers between the two passes: the norms first, then the squared
// differences of the scaled values.  Lane l holds the quads l, l + 64, l + 128 of the row; a quad past C reads as zeros,
// which change no bit of a sum of squares.  Both load paths (16-byte loads, element loads) fill the same registers, so
// they give the same bits.
//
// The two scaled values are rounded BEFORE they are subtracted (the library is built with -ffp-contract=fast, which
// would turn a * ra - b * rb into fma(a, ra, -(b * rb)): not zero for identical inputs); see scaled_difference.
#include "common.h"

namespace {

constexpr int SSIM_TH = 16, SSIM_TW = 32;         // window centres per tile
constexpr int SSIM_MAX_WIN = 15;
constexpr int SSIM_THREADS = 256;
constexpr long SSIM_MAX_GRID = 1L << 23;          // workgroups per launch: 2^31 threads, below the 2^32 some runtimes cap at
constexpr int SSIM_IH = SSIM_TH + SSIM_MAX_WIN - 1, SSIM_IW = SSIM_TW + SSIM_MAX_WIN - 1;   // a tile with its halo

struct SsimArgs {
  const void* a;
  const void* b;
  long san, sac, sah, saw;      // element strides of a: image, channel, row, column
  long sbn, sbc, sbh, sbw;
  const double* window;         // [win]
  const unsigned char* region;  // [n or 1][H][W] or null
  long region_stride;           // H * W, or 0 for a region shared by every image
  double* partial;              // [n * C * tiles][4]: ssim sum, squared error, counted pixels, counted centres
  double c1, c2;
  long block0;                  // the first (image, channel, tile) of this launch: a launch holds at most SSIM_MAX_GRID
  int C, H, W, win, tiles_x, tiles_y;
};

template <typename T>
__global__ __launch_bounds__(SSIM_THREADS) void k_pair_ssim(SsimArgs p) {
  __shared__ double sa[SSIM_IH][SSIM_IW + 1];
  __shared__ double sb[SSIM_IH][SSIM_IW + 1];
  __shared__ double rowf[5][SSIM_IH][SSIM_TW];     // the row-filtered a, b, a^2, b^2, ab; afterwards the reduction
  __shared__ double wt[SSIM_MAX_WIN];
  __shared__ unsigned char sr[SSIM_IH][SSIM_IW + 2];
  const int t = threadIdx.x;
  const int tiles = p.tiles_x * p.tiles_y;
  const long blk = p.block0 + blockIdx.x;
  const int tile = (int)(blk % tiles);
  const long ic = blk / tiles;
  const int c = (int)(ic % p.C);
  const long i = ic / p.C;
  const int ty = tile / p.tiles_x, tx = tile - ty * p.tiles_x;
  const int win = p.win, half = win >> 1;
  const int Hv = p.H - win + 1, Wv = p.W - win + 1;
  const int y0 = ty * SSIM_TH, x0 = tx * SSIM_TW;
  const int oh = min(SSIM_TH, Hv - y0), ow = min(SSIM_TW, Wv - x0);
  const int ih = oh + win - 1, iw = ow + win - 1;     // y0 + ih <= H, x0 + iw <= W
  if (t < win) wt[t] = p.window[t];
  const T* ap = static_cast<const T*>(p.a) + i * p.san + c * p.sac;
  const T* bp = static_cast<const T*>(p.b) + i * p.sbn + c * p.sbc;
  const unsigned char* rp = p.region ? p.region + i * p.region_stride : nullptr;
  for (int idx = t; idx < ih * iw; idx += SSIM_THREADS) {
    const int y = idx / iw, x = idx - y * iw;
    const long gy = y0 + y, gx = x0 + x;
    sa[y][x] = (double)ap[gy * p.sah + gx * p.saw];
    sb[y][x] = (double)bp[gy * p.sbh + gx * p.sbw];
    sr[y][x] = rp ? (rp[gy * p.W + gx] != 0 ? 1 : 0) : 1;
  }
  __syncthreads();
  // the squared error over the pixels this tile owns
  double sse = 0.0, npix = 0.0;
  {
    const int own_h = ty == p.tiles_y - 1 ? ih : SSIM_TH, own_w = tx == p.tiles_x - 1 ? iw : SSIM_TW;
    for (int idx = t; idx < own_h * own_w; idx += SSIM_THREADS) {
      const int y = idx / own_w, x = idx - y * own_w;
      if (sr[y][x]) {
        const double d = sa[y][x] - sb[y][x];
        sse += d * d;
        npix += 1.0;
      }
    }
  }
  // rows
  for (int idx = t; idx < ih * SSIM_TW; idx += SSIM_THREADS) {
    const int r = idx / SSIM_TW, x = idx % SSIM_TW;
    if (x < ow) {
      double ma = 0.0, mb = 0.0, eaa = 0.0, ebb = 0.0, eab = 0.0;
      for (int k = 0; k < win; ++k) {
        const double w = wt[k], av = sa[r][x + k], bv = sb[r][x + k];
        ma += w * av;
        mb += w * bv;
        eaa += w * (av * av);
        ebb += w * (bv * bv);
        eab += w * (av * bv);
      }
      rowf[0][r][x] = ma;
      rowf[1][r][x] = mb;
      rowf[2][r][x] = eaa;
      rowf[3][r][x] = ebb;
      rowf[4][r][x] = eab;
    }
  }
  __syncthreads();
  // columns, and the map
  double ssum = 0.0, ncen = 0.0;
  for (int idx = t; idx < SSIM_TH * SSIM_TW; idx += SSIM_THREADS) {
    const int y = idx / SSIM_TW, x = idx % SSIM_TW;
    if (y < oh && x < ow && sr[y + half][x + half]) {
      double m[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
      for (int k = 0; k < win; ++k) {
        const double w = wt[k];
#pragma unroll
        for (int q = 0; q < 5; ++q) m[q] += w * rowf[q][y + k][x];
      }
      const double va = m[2] - m[0] * m[0], vb = m[3] - m[1] * m[1], cov = m[4] - m[0] * m[1];
      const double num = (2.0 * m[0] * m[1] + p.c1) * (2.0 * cov + p.c2);
      const double den = (m[0] * m[0] + m[1] * m[1] + p.c1) * (va + vb + p.c2);
      ssum += num / den;
      ncen += 1.0;
    }
  }
  __syncthreads();
  double(*red)[SSIM_THREADS] = reinterpret_cast<double(*)[SSIM_THREADS]>(&rowf[0][0][0]);
  red[0][t] = ssum;
  red[1][t] = sse;
  red[2][t] = npix;
  red[3][t] = ncen;
  __syncthreads();
  for (int s = SSIM_THREADS / 2; s > 0; s >>= 1) {
    if (t < s) {
#pragma unroll
      for (int q = 0; q < 4; ++q) red[q][t] += red[q][t + s];
    }
    __syncthreads();
  }
  if (t < 4) p.partial[blk * 4 + t] = red[t][0];
}

// one thread per (image, channel): the tile partials in tile order
__global__ __launch_bounds__(256) void k_pair_ssim_finish(const double* __restrict__ partial, int tiles, int C, long rows,
                                                          double* __restrict__ ssim, double* __restrict__ sse,
                                                          int* __restrict__ counts) {
  const long g = (long)blockIdx.x * 256 + threadIdx.x;
  if (g >= rows) return;
  const double* pp = partial + g * tiles * 4;
  double s = 0.0, e = 0.0, np = 0.0, nc = 0.0;
  for (int k = 0; k < tiles; ++k) {
    s += pp[4 * k];
    e += pp[4 * k + 1];
    np += pp[4 * k + 2];
    nc += pp[4 * k + 3];
  }
  ssim[g] = s / nc;       // no counted centre: 0 / 0 = NaN
  sse[g] = e;
  if (g % C == 0) {
    counts[(g / C) * 2] = (int)np;
    counts[(g / C) * 2 + 1] = (int)nc;
  }
}

// ---------------------------------------------------------------------------------------------- the feature distance
constexpr int FD_WAVES = 8;
constexpr int FD_MAX_C = 768;

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// round(a * ra) - round(b * rb): the empty asm makes the products opaque, so that neither is folded into an FMA with the
// subtraction; identical operands give exactly +0.0
__device__ __forceinline__ double scaled_difference(double a, double ra, double b, double rb) {
  double sa = a * ra, sb = b * rb;
  asm volatile("" : "+v"(sa), "+v"(sb));
  return sa - sb;
}

// NQ quads per lane (C <= 256 NQ); VEC: 16-byte loads (C % 4 == 0, a and b 16-byte aligned), else element loads
template <int NQ, bool VEC>
__global__ __launch_bounds__(FD_WAVES * 64) void k_pair_feature_distance(const float* __restrict__ a,
                                                                         const float* __restrict__ b,
                                                                         double* __restrict__ out, int HW, int C,
                                                                         long out_stride, int column) {
  __shared__ double tot[FD_WAVES];
  const long s = blockIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float* as = a + s * HW * C;
  const float* bs = b + s * HW * C;
  double acc = 0.0;
  for (int p = wave; p < HW; p += FD_WAVES) {
    const float* ar = as + (long)p * C;
    const float* br = bs + (long)p * C;
    float va[NQ][4], vb[NQ][4];
#pragma unroll
    for (int j = 0; j < NQ; ++j) {
      const int c0 = 4 * (lane + 64 * j);
      if constexpr (VEC) {
        f32x4 qa = {0.f, 0.f, 0.f, 0.f}, qb = {0.f, 0.f, 0.f, 0.f};
        if (c0 < C) {
          qa = *reinterpret_cast<const f32x4*>(ar + c0);
          qb = *reinterpret_cast<const f32x4*>(br + c0);
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          va[j][e] = qa[e];
          vb[j][e] = qb[e];
        }
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          va[j][e] = c0 + e < C ? ar[c0 + e] : 0.f;
          vb[j][e] = c0 + e < C ? br[c0 + e] : 0.f;
        }
      }
    }
    double na = 0.0, nb = 0.0;
#pragma unroll
    for (int j = 0; j < NQ; ++j)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const double x = (double)va[j][e], y = (double)vb[j][e];
        na += x * x;
        nb += y * y;
      }
    na = wave_sum_f64(na);
    nb = wave_sum_f64(nb);
    const double ra = 1.0 / (sqrt(na) + 1e-10), rb = 1.0 / (sqrt(nb) + 1e-10);
    double d = 0.0;
#pragma unroll
    for (int j = 0; j < NQ; ++j)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const double u = scaled_difference((double)va[j][e], ra, (double)vb[j][e], rb);
        d += u * u;
      }
    acc += wave_sum_f64(d);
  }
  if (lane == 0) tot[wave] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    double v = tot[0];
#pragma unroll
    for (int w = 1; w < FD_WAVES; ++w) v += tot[w];
    out[s * out_stride + column] = v / (double)HW;
  }
}

template <int NQ>
void launch_feature_distance(bool vec, const float* a, const float* b, double* out, int B, int HW, int C, long out_stride,
                             int column, hipStream_t st) {
  if (vec)
    hipLaunchKernelGGL((k_pair_feature_distance<NQ, true>), dim3((unsigned)B), dim3(FD_WAVES * 64), 0, st, a, b, out, HW, C,
                       out_stride, column);
  else
    hipLaunchKernelGGL((k_pair_feature_distance<NQ, false>), dim3((unsigned)B), dim3(FD_WAVES * 64), 0, st, a, b, out, HW, C,
                       out_stride, column);
}

}  // namespace

extern "C" long edm_pair_ssim_tiles(int H, int W, int win) {
  if (win < 3 || win > SSIM_MAX_WIN || !(win & 1) || win > H || win > W) return 0;
  const long ty = (H - win + 1 + SSIM_TH - 1) / SSIM_TH, tx = (W - win + 1 + SSIM_TW - 1) / SSIM_TW;
  return ty * tx;
}

extern "C" int edm_pair_ssim(const void* a, const void* b, int is_u8, long n, int C, int H, int W, const long* strides_a,
                             const long* strides_b, const double* window, int win, double data_range,
                             const unsigned char* region, int region_shared, double* partial, double* ssim, double* sse,
                             int* counts, hipStream_t st) {
  EDM_REQUIRE(a && b && strides_a && strides_b && window && partial && ssim && sse && counts, "pair_ssim: null argument");
  EDM_REQUIRE(n > 0 && C > 0 && H > 0 && W > 0 && (long)H * W < (1L << 31), "pair_ssim: bad shape");
  EDM_REQUIRE(win >= 3 && win <= SSIM_MAX_WIN && (win & 1) && win <= H && win <= W,
              "pair_ssim: the window must be odd, 3 <= win <= %d and win <= min(H, W) = %d, got %d", SSIM_MAX_WIN,
              H < W ? H : W, win);
  EDM_REQUIRE(data_range > 0.0 && data_range < 1e300, "pair_ssim: data_range must be finite and > 0");
  const long tiles = edm_pair_ssim_tiles(H, W, win);
  EDM_REQUIRE(n * C < (1L << 31) / tiles, "pair_ssim: n * C * tiles = %ld * %d * %ld exceeds 2^31", n, C, tiles);
  for (int k = 0; k < 4; ++k)
    EDM_REQUIRE(strides_a[k] >= 0 && strides_b[k] >= 0, "pair_ssim: negative stride");
  SsimArgs p;
  p.a = a;
  p.b = b;
  p.san = strides_a[0]; p.sac = strides_a[1]; p.sah = strides_a[2]; p.saw = strides_a[3];
  p.sbn = strides_b[0]; p.sbc = strides_b[1]; p.sbh = strides_b[2]; p.sbw = strides_b[3];
  p.window = window;
  p.region = region;
  p.region_stride = region_shared ? 0 : (long)H * W;
  p.partial = partial;
  p.c1 = (0.01 * data_range) * (0.01 * data_range);
  p.c2 = (0.03 * data_range) * (0.03 * data_range);
  p.C = C; p.H = H; p.W = W; p.win = win;
  p.tiles_x = (W - win + 1 + SSIM_TW - 1) / SSIM_TW;
  p.tiles_y = (H - win + 1 + SSIM_TH - 1) / SSIM_TH;
  const long blocks = n * C * tiles;
  for (p.block0 = 0; p.block0 < blocks; p.block0 += SSIM_MAX_GRID) {      // (the chunking changes no bit: a workgroup is
    const long left = blocks - p.block0;                                   //  a function of its global number alone)
    const dim3 grid((unsigned)(left < SSIM_MAX_GRID ? left : SSIM_MAX_GRID));
    if (is_u8)
      hipLaunchKernelGGL(k_pair_ssim<unsigned char>, grid, dim3(SSIM_THREADS), 0, st, p);
    else
      hipLaunchKernelGGL(k_pair_ssim<float>, grid, dim3(SSIM_THREADS), 0, st, p);
    EDM_CHECK_LAUNCH("pair_ssim");
  }
  const long rows = n * C;      // (one thread per row: at most 2^31 threads)
  hipLaunchKernelGGL(k_pair_ssim_finish, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, st, partial, (int)tiles, C, rows,
                     ssim, sse, counts);
  EDM_CHECK_LAUNCH("pair_ssim_finish");
  return EDM_OK;
}

extern "C" int edm_f32_pair_feature_distance(const float* a, const float* b, double* out, int B, int HW, int C,
                                             long out_stride, int column, hipStream_t st) {
  EDM_REQUIRE(a && b && out && B > 0 && HW > 0 && C > 0, "f32_pair_feature_distance: bad args");
  EDM_REQUIRE(C <= FD_MAX_C, "f32_pair_feature_distance: C = %d exceeds the %d channels a wave keeps in registers", C,
              FD_MAX_C);
  EDM_REQUIRE(column >= 0 && out_stride > column, "f32_pair_feature_distance: column %d does not fit a row of %ld", column,
              out_stride);
  const bool vec = C % 4 == 0 && ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) & 15) == 0;
  const int nq = (C + 255) / 256;
  if (nq == 1)
    launch_feature_distance<1>(vec, a, b, out, B, HW, C, out_stride, column, st);
  else if (nq == 2)
    launch_feature_distance<2>(vec, a, b, out, B, HW, C, out_stride, column, st);
  else
    launch_feature_distance<3>(vec, a, b, out, B, HW, C, out_stride, column, st);
  EDM_CHECK_LAUNCH("f32_pair_feature_distance");
  return EDM_OK;
}
