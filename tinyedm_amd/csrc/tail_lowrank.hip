// The output end of the network in factored form.
//
// conv_out maps C channels to Co <= 8, so its input gradient g_h[p, c] = sum_o dF[p, o] * Wout[o, c] has rank Co per
// pixel.  The last decoder block's second 3x3 conv consumed it as a full C-channel operand twice (dgrad, weight
// gradient), 2 * 9 * C * C FLOP per pixel each, inside the MFMA kernels.  Here both are computed from dF itself:
//
//   ga2[p, ci]   = b * sum_t sum_o dF[p - d(t), o] * Wc[o, t, ci]          Wc[o, t, ci] = sum_c Wout[o, c] * W2[c, ci, t]
//   dW2[c, ci, t] = b * sum_o Wout[o, c] * G[o, t, ci]                     G[o, t, ci]  = sum_p dF[p, o] * a2[p + d(t), ci]
//
// (t = 3 ky + kx, d(t) = (ky - 1, kx - 1): the forward conv reads in[p + d(t)]; zero padding, never across samples),
// 2 * 9 * Co * C FLOP per pixel each: plain SIMT kernels bound by the bytes they must touch.  conv_out's own weight
// gradient is the same G reduction with one tap.  dF is fp32 NCHW [B, Co, H, W] (k_lowrank_df).
#include "common.h"

typedef __attribute__((ext_vector_type(2))) float f32x2;

// Dynamic LDS of the two main kernels for R rows per workgroup (the launchers shrink R until it fits, down to one row), and
// the host query the Python side asks BEFORE it takes this path: a shape whose tables do not fit keeps the dense path.
constexpr size_t LOWRANK_LDS_MAX = 60 * 1024;
static size_t dgrad_lds(int Co, int C, int W, int R, bool fused) {
  const int CL = C / 8, PS = ((256 / CL) * CL) / CL, TP = (W + 3) / 4 * 4 + 4;
  return ((size_t)Co * 9 * C + (size_t)Co * (R + 2) * TP + (fused ? (size_t)PS * C : 0)) * sizeof(float);
}
static size_t wgrad_lds(int Co, int taps, int C, int W, int R) {
  const int halo = taps == 9 ? 1 : 0;
  return ((size_t)Co * taps * C + (size_t)Co * (R + 2 * halo) * (W + 2 * halo)) * sizeof(float);
}
// 1 when edm_lowrank_wgrad(taps) -- and, taps == 9, the fused edm_lowrank_dgrad3x3 -- run maps of width W with C channels
extern "C" int edm_lowrank_supported(int C, int Co, int W, int taps) {
  if (C <= 0 || C % 8 || C > 1024 || Co < 1 || Co > 8 || W <= 0 || (taps != 1 && taps != 9)) return 0;
  if (wgrad_lds(Co, taps, C, W, 1) > LOWRANK_LDS_MAX) return 0;
  return taps == 1 || dgrad_lds(Co, C, W, 1, true) <= LOWRANK_LDS_MAX;
}

// ------------------------------------------------------------------ dF = dD * c_out(b) * gain_out
// aux (optional) = dD * c_out(b) * Fraw: its sum is d loss / d gain_out (edm_lowrank_wgrad adds it up in a fixed order)
__global__ void k_lowrank_df(const float* __restrict__ dD, const float* __restrict__ Fraw,
                             const float* __restrict__ gain_out, const float* __restrict__ sigma, int sstride, float sd,
                             float* __restrict__ dF, float* __restrict__ aux, int CoHW, long n) {
  const float go = *gain_out;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const int b = (int)(i / CoHW);
    const float s = sigma[b * sstride];
    const float c = s * sd * rsqrtf(s * s + sd * sd);
    const float d = dD[i];
    dF[i] = d * (c * go);           // (the rounding of k_conv_out_bwd_x's factor)
    if (aux) aux[i] = (d * c) * Fraw[i];
  }
}

extern "C" int edm_lowrank_df(const float* dD, const float* Fraw, const float* gain_out, const float* sigma,
                              int sigma_stride, float sigma_data, float* dF, float* aux, int B, int Co, int HW,
                              hipStream_t st) {
  EDM_REQUIRE(dD && gain_out && sigma && dF && (!aux || Fraw), "lowrank_df: null pointer");
  EDM_REQUIRE(B > 0 && HW > 0 && Co >= 1 && Co <= 8 && (sigma_stride == 0 || sigma_stride == 1), "lowrank_df: bad args");
  EDM_REQUIRE((long)Co * HW < (1L << 31), "lowrank_df: sample too large");
  const long n = (long)B * Co * HW;
  const long blocks = (n + 255) / 256;
  hipLaunchKernelGGL(k_lowrank_df, dim3((unsigned)(blocks < 2048 ? blocks : 2048)), dim3(256), 0, st, dD, Fraw, gain_out,
                     sigma, sigma_stride, sigma_data, dF, aux, Co * HW, n);
  EDM_CHECK_LAUNCH("lowrank_df");
  return EDM_OK;
}

// ------------------------------------------------------------------ the transposed 3x3 conv from Co channels
// grid = (ceil(H / R), B): a workgroup owns R whole rows of one sample.  LDS: the Wc table [CO * 9][C], the dF rows with
// their halo [CO][R + 2][TP] (zeros outside the image: no bounds test in the loop), and -- fused form -- the [PS][C] table
// that folds the modulation sums.  A thread owns 8 channels (chunk c8) and walks strips of 4 pixels along a row: a weight
// vector read from LDS serves 4 pixels, the dF scalars of a strip are the same address for every lane of a pixel phase.
// FUSED: ga2 is rounded to bf16 exactly as the MFMA dgrad's result and handed in registers to mod_silu_drop_bwd8
// (common.h: the epilogue of edm_conv3x3_modbwd) -- gr = ga2 * keep * mp_silu'(u m) * m, gm[b, c] += sum ga2 * keep * mp_silu'(u m) * u.
template <int CO, bool FUSED>
__global__ __launch_bounds__(256, 4) void k_lowrank_dgrad3x3(const float* __restrict__ dF, const float* __restrict__ Wc,
                                                          float scale, bf16* __restrict__ ga, const bf16* __restrict__ U,
                                                          const float* __restrict__ lin, long lin_stride,
                                                          const float* __restrict__ gain, bf16* __restrict__ gr,
                                                          float* __restrict__ gm, long gm_stride, float pdrop,
                                                          uint32_t seed_lo, uint32_t seed_hi, uint32_t sub, uint32_t step,
                                                          int u_marks, const StepParams* __restrict__ dyn, int H, int W,
                                                          int C, int R, int TP) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  float* wl = sm;                               // [CO * 9][C]
  float* tl = wl + CO * 9 * C;                  // [CO][R + 2][TP]
  float* red = tl + CO * (R + 2) * TP;          // [PS][C]   (FUSED)
  const int CL = C >> 3;
  const int PS = blockDim.x / CL;
  const int c8 = threadIdx.x % CL, ps = threadIdx.x / CL;
  const int b = blockIdx.y, y0 = blockIdx.x * R;
  const int rows = min(R, H - y0);
  for (int i = threadIdx.x; i < CO * 9 * C / 4; i += blockDim.x)
    reinterpret_cast<f32x4*>(wl)[i] = reinterpret_cast<const f32x4*>(Wc)[i];
  for (int i = threadIdx.x; i < CO * (R + 2) * TP; i += blockDim.x) {
    const int o = i / ((R + 2) * TP), rem = i - o * (R + 2) * TP;
    const int ry = rem / TP, cx = rem - ry * TP;
    const int y = y0 + ry - 1, x = cx - 1;
    float v = 0.f;
    if (y >= 0 && y < H && x >= 0 && x < W) v = dF[(((long)b * CO + o) * H + y) * W + x];
    tl[i] = v;
  }
  __syncthreads();
  ModEpilogue m{};
  float mv[8], part[8];
  if constexpr (FUSED) {
    m.pdrop = pdrop; m.seed_lo = seed_lo; m.seed_hi = seed_hi; m.sub = sub; m.step = step; m.u_marks = u_marks; m.dyn = dyn;
    apply_dyn(m);
    const float g = *gain;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      mv[j] = lin[(long)b * lin_stride + c8 * 8 + j] * g + 1.0f;
      part[j] = 0.f;
    }
  }
  const int NSX = (W + 3) >> 2;
  const int nstrips = rows * NSX;
  for (int s = ps; s < nstrips; s += PS) {
    const int ry = s / NSX, x0 = (s - ry * NSX) * 4;
    const long p = ((long)b * H + y0 + ry) * W + x0;        // first pixel of the strip
    u32x4 ub[4];
    if constexpr (FUSED) {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        ub[k] = u32x4{0u, 0u, 0u, 0u};
        if (x0 + k < W) ub[k] = *reinterpret_cast<const u32x4*>(U + (p + k) * C + c8 * 8);
      }
    }
    f32x2 acc[4][4];
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[k][j] = f32x2{0.f, 0.f};
    // (a real loop over the 3 CO (ky, o) groups: fully unrolled, the scheduler issues all 27 CO weight reads first and
    // spills them -- 300 to 900 registers)
#pragma unroll 1
    for (int g = 0; g < 3 * CO; ++g) {
      const int ky = g / CO, o = g - ky * CO;
      {
        // pixel (y, x) reads dF at (y - (ky - 1), x - (kx - 1)): tile row ry + 2 - ky, tile column x + 2 - kx
        const float* tp = tl + (o * (R + 2) + ry + 2 - ky) * TP + x0;
        float dd[6];
#pragma unroll
        for (int j = 0; j < 6; ++j) dd[j] = tp[j];
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
          const float* wp = wl + (o * 9 + ky * 3 + kx) * C + c8 * 8;
          const f32x4 w0 = *reinterpret_cast<const f32x4*>(wp), w1 = *reinterpret_cast<const f32x4*>(wp + 4);
          const f32x2 w[4] = {f32x2{w0[0], w0[1]}, f32x2{w0[2], w0[3]}, f32x2{w1[0], w1[1]}, f32x2{w1[2], w1[3]}};
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            const float d = dd[k + 2 - kx];
            const f32x2 d2 = {d, d};
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[k][j] += d2 * w[j];
          }
        }
      }
    }
    // (rounded for all four pixels before the first bounds test: with the only use of the sums inside `if (x0 + k < W)`
    // the compiler sinks the whole FMA chain into that branch, behind all 27 CO weight reads -- 890 spilled registers)
    u32x4 o8[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      bf16x8 v;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        v[2 * j] = (bf16)(scale * acc[k][j][0]);
        v[2 * j + 1] = (bf16)(scale * acc[k][j][1]);
      }
      o8[k] = __builtin_bit_cast(u32x4, v);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (x0 + k < W) {
        const long e = (p + k) * C + c8 * 8;
        if (ga) *reinterpret_cast<u32x4*>(ga + e) = o8[k];
        if constexpr (FUSED) *reinterpret_cast<u32x4*>(gr + e) = mod_silu_drop_bwd8(o8[k], ub[k], e >> 3, mv, m, part);
      }
    }
  }
  if constexpr (FUSED) {
    // the PS partial sums per channel meet in LDS, one atomic per (b, c) and workgroup (as k_mod_silu_drop_bwd)
#pragma unroll
    for (int j = 0; j < 8; ++j) red[ps * C + c8 * 8 + j] = part[j];
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += blockDim.x) {
      float s = 0.f;
      for (int q = 0; q < PS; ++q) s += red[q * C + c];
      atomicAdd(gm + (long)b * gm_stride + c, s);
    }
  }
}

template <int CO>
static int launch_dgrad(const float* dF, const float* Wc, float scale, void* ga, const void* U, const float* lin,
                        long lin_stride, const float* gain, void* gr, float* gm, long gm_stride, float pdrop,
                        unsigned long long seed, unsigned sub, unsigned step, int u_marked, int B, int H, int W, int C,
                        const void* dyn, hipStream_t st) {
  const int CL = C / 8, block = (256 / CL) * CL, PS = block / CL;
  const int NSX = (W + 3) / 4, TP = NSX * 4 + 4;
  // rows per workgroup: ~128 pixels (16 per thread at C = 256), shrunk until the tables fit
  int R = 128 / W;
  R = R < 1 ? 1 : (R > H ? H : R);
  auto lds = [&](int r) { return dgrad_lds(CO, C, W, r, U != nullptr); };
  while (R > 1 && lds(R) > LOWRANK_LDS_MAX) --R;
  EDM_REQUIRE(lds(R) <= LOWRANK_LDS_MAX, "lowrank_dgrad3x3: Co=%d, C=%d, W=%d need %zu bytes of LDS (60 KB at most)", CO, C, W,
              lds(R));
  const dim3 grid((H + R - 1) / R, B);
  if (U)
    hipLaunchKernelGGL((k_lowrank_dgrad3x3<CO, true>), grid, dim3(block), lds(R), st, dF, Wc, scale, (bf16*)ga,
                       (const bf16*)U, lin, lin_stride, gain, (bf16*)gr, gm, gm_stride, pdrop, (uint32_t)seed,
                       (uint32_t)(seed >> 32), sub, step, u_marked, (const StepParams*)dyn, H, W, C, R, TP);
  else
    hipLaunchKernelGGL((k_lowrank_dgrad3x3<CO, false>), grid, dim3(block), lds(R), st, dF, Wc, scale, (bf16*)ga,
                       (const bf16*)nullptr, (const float*)nullptr, 0L, (const float*)nullptr, (bf16*)nullptr,
                       (float*)nullptr, 0L, 0.f, 0u, 0u, 0u, 0u, 0, (const StepParams*)nullptr, H, W, C, R, TP);
  EDM_CHECK_LAUNCH("lowrank_dgrad3x3");
  return EDM_OK;
}

#define EDM_CO_SWITCH(Co, CALL)      \
  switch (Co) {                      \
    case 1: return CALL(1);          \
    case 2: return CALL(2);          \
    case 3: return CALL(3);          \
    case 4: return CALL(4);          \
    case 5: return CALL(5);          \
    case 6: return CALL(6);          \
    case 7: return CALL(7);          \
    default: return CALL(8);         \
  }

// ga2 (bf16 NHWC [B, H, W, C], nullable in the fused form) = scale * transposed 3x3 conv of dF (fp32 NCHW [B, Co, H, W]) with
// Wc (fp32 [Co][9][C]).  r1 != NULL: the modulation / mp_silu / dropout backward of edm_conv3x3_modbwd on ga2 in registers:
// gr (bf16, like r1) and the raw modulation sums accumulated (atomics) into gm (zero-filled rows of gm_stride floats).
extern "C" int edm_lowrank_dgrad3x3(const float* dF, const float* Wc, float scale, void* ga, const void* r1,
                                    const float* lin, long lin_stride, const float* gain, void* gr, float* gm,
                                    long gm_stride, float pdrop, unsigned long long seed, unsigned sub, unsigned step,
                                    int u_marked, int B, int H, int W, int C, int Co, const void* dyn, hipStream_t st) {
  EDM_REQUIRE(dF && Wc && (ga || r1), "lowrank_dgrad3x3: null pointer");
  EDM_REQUIRE(B > 0 && B <= 65535 && H > 0 && W > 0 && C > 0 && C % 8 == 0 && C <= 2048 && Co >= 1 && Co <= 8,
              "lowrank_dgrad3x3: bad args (C %% 8 == 0, Co <= 8 required)");
  EDM_REQUIRE(((uintptr_t)Wc & 15) == 0, "lowrank_dgrad3x3: Wc must be 16-byte aligned");
  if (r1)
    EDM_REQUIRE(lin && gain && gr && gm && lin_stride >= C && gm_stride >= C && pdrop >= 0.f && pdrop < 1.f,
                "lowrank_dgrad3x3: bad modulation-backward args");
#define CALL(CO_) launch_dgrad<CO_>(dF, Wc, scale, ga, r1, lin, lin_stride, gain, gr, gm, gm_stride, pdrop, seed, sub, step, \
                                    u_marked, B, H, W, C, dyn, st)
  EDM_CO_SWITCH(Co, CALL)
#undef CALL
}

// ------------------------------------------------------------------ G[o, t, c] = sum_p dF[p, o] * X[p + d(t), c]
// X-stationary: every X element is read once and feeds TAPS * CO accumulators of its thread (a thread owns 4 channels:
// 108 accumulators at Co = 3, 9 taps; 2 channels from Co = 5 on).  A workgroup owns whole units (R rows of one sample) whose dF rows + halo sit in
// LDS; X is loaded NB pixels ahead.  Deterministic: the PS pixel phases of a workgroup are added in phase order into one
// LDS table, the table goes to the workgroup's row of `ws`, and k_lowrank_reduce adds the rows in a fixed order.
// ws row = [CO * TAPS * C sums | sum of aux over the workgroup's pixels | 3 pad].
template <int CO, int TAPS, int VEC>
__global__ __launch_bounds__(512) void k_lowrank_wgrad(const float* __restrict__ dF, const bf16* __restrict__ X,
                                                       const float* __restrict__ aux, float* __restrict__ ws, int H,
                                                       int W, int C, int R, int upb, int nunits) {
  constexpr int HALO = TAPS == 9 ? 1 : 0, K = TAPS == 9 ? 3 : 1, NB = 8;
  extern __shared__ __attribute__((aligned(16))) float sm[];
  __shared__ float asums[512];
  const int N = CO * TAPS * C, TPW = W + 2 * HALO, TR = R + 2 * HALO;
  float* accl = sm;             // [CO * TAPS][C]
  float* tl = sm + N;           // [CO][TR][TPW]
  typedef __attribute__((ext_vector_type(VEC / 2))) unsigned int uraw;      // VEC bf16 channels of a pixel
  const int CLV = C / VEC;
  const int PS = blockDim.x / CLV;
  const int cv = threadIdx.x % CLV, ps = threadIdx.x / CLV;
  f32x2 acc[CO * TAPS][VEC / 2];
#pragma unroll
  for (int e = 0; e < CO * TAPS; ++e)
#pragma unroll
    for (int h = 0; h < VEC / 2; ++h) acc[e][h] = f32x2{0.f, 0.f};
  float asum = 0.f;
  for (int u = blockIdx.x; u < nunits; u += gridDim.x) {
    const int b = u / upb, y0 = (u - b * upb) * R;
    const int rows = min(R, H - y0);
    __syncthreads();            // (the previous unit's readers of tl)
    for (int i = threadIdx.x; i < CO * TR * TPW; i += blockDim.x) {
      const int o = i / (TR * TPW), rem = i - o * TR * TPW;
      const int ry = rem / TPW, cx = rem - ry * TPW;
      const int y = y0 + ry - HALO, x = cx - HALO;
      float v = 0.f;
      if (y >= 0 && y < H && x >= 0 && x < W)      // (halo rows inside the sample hold the neighbouring unit's dF)
        v = dF[(((long)b * CO + o) * H + y) * W + x];
      tl[i] = v;
    }
    if (aux) {
      for (int o = 0; o < CO; ++o) {
        const float* ap = aux + (((long)b * CO + o) * H + y0) * W;
        for (int i = threadIdx.x; i < rows * W; i += blockDim.x) asum += ap[i];
      }
    }
    __syncthreads();
    const int np = rows * W;
    const bf16* xp = X + (((long)b * H + y0) * W) * C + cv * VEC;     // the unit's pixels are contiguous rows of X
    int ry = ps / W, x = ps - (ps / W) * W;                         // position of pixel q = ps + i * PS, kept incrementally
    uraw nx[NB];
    auto fetch = [&](int q0) {
#pragma unroll
      for (int i = 0; i < NB; ++i) {
        const int q = q0 + i * PS;
        nx[i] = uraw{};
        if (q < np) nx[i] = *reinterpret_cast<const uraw*>(xp + (long)q * C);
      }
    };
    fetch(ps);
    for (int q0 = ps; q0 < np; q0 += NB * PS) {
      uraw cur[NB];
#pragma unroll
      for (int i = 0; i < NB; ++i) cur[i] = nx[i];
      if (q0 + NB * PS < np) fetch(q0 + NB * PS);
#pragma unroll
      for (int i = 0; i < NB; ++i) {
        if (q0 + i * PS < np) {
          typedef __attribute__((ext_vector_type(VEC))) __bf16 bfv;
          const bfv xv = __builtin_bit_cast(bfv, cur[i]);
          f32x2 xf[VEC / 2];
#pragma unroll
          for (int h = 0; h < VEC / 2; ++h) xf[h] = f32x2{(float)xv[2 * h], (float)xv[2 * h + 1]};
#pragma unroll
          for (int o = 0; o < CO; ++o)
#pragma unroll
            for (int ky = 0; ky < K; ++ky)
#pragma unroll
              for (int kx = 0; kx < K; ++kx) {
                // X[q] is the operand of output pixel p = q - d(t): tile row ry + 2 HALO - ky, column x + 2 HALO - kx
                const float d = tl[(o * TR + ry + 2 * HALO - ky) * TPW + x + 2 * HALO - kx];
                const f32x2 d2 = {d, d};
#pragma unroll
                for (int h = 0; h < VEC / 2; ++h) acc[o * TAPS + ky * K + kx][h] += d2 * xf[h];
              }
        }
        x += PS;
        while (x >= W) {
          x -= W;
          ++ry;
        }
      }
    }
  }
  // the phases in order 0, 1, ... PS - 1 (fixed: bit-equal from run to run)
  for (int r = 0; r < PS; ++r) {
    __syncthreads();
    if (ps == r) {
#pragma unroll
      for (int e = 0; e < CO * TAPS; ++e) {
#pragma unroll
        for (int h = 0; h < VEC / 2; ++h) {
          f32x2* ap = reinterpret_cast<f32x2*>(accl + e * C + cv * VEC + 2 * h);
          f32x2 v = acc[e][h];
          if (r) v += *ap;
          *ap = v;
        }
      }
    }
  }
  asums[threadIdx.x] = asum;
  __syncthreads();
  float* row = ws + (long)blockIdx.x * (N + 4);
  for (int i = threadIdx.x; i < N; i += blockDim.x) row[i] = accl[i];
  if (threadIdx.x == 0) {
    float s = 0.f;
    for (int i = 0; i < (int)blockDim.x; ++i) s += asums[i];
    row[N] = s;
  }
}

// G[e] = sum over the nwg <= 256 workspace rows, e < N; element N: *aux_out += the sum (one thread: no atomics).
// block = 64 elements x 16 segments of <= 16 rows: a segment's loads are issued together and added in row order, the
// segments in segment order (fixed: bit-equal from run to run).
__global__ __launch_bounds__(1024) void k_lowrank_reduce(const float* __restrict__ ws, int nwg, int N, float* __restrict__ G,
                                                         float* __restrict__ aux_out) {
  __shared__ float part[16][64];
  const int l = threadIdx.x & 63, seg = threadIdx.x >> 6;
  const int e = blockIdx.x * 64 + l;
  const int per = (nwg + 15) / 16;          // <= 16
  const int r0 = seg * per;
  float v[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    const int r = r0 + k;
    v[k] = (e <= N && k < per && r < nwg) ? ws[(long)r * (N + 4) + e] : 0.f;
  }
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < 16; ++k) s += v[k];
  part[seg][l] = s;
  __syncthreads();
  if (seg == 0 && e <= N) {
    float t = 0.f;
#pragma unroll
    for (int k = 0; k < 16; ++k) t += part[k][l];
    if (e < N) G[e] = t;
    else if (aux_out) *aux_out += t;
  }
}

template <int CO>
static int launch_wgrad(const float* dF, const void* X, int taps, const float* aux, float* G, float* aux_out, float* ws,
                        long ws_floats, int B, int H, int W, int C, int nwg, hipStream_t st) {
  // channels per thread: 4 up to Co = 4 (108 / 144 accumulators at 9 taps), 2 above (<= 144)
  constexpr int VEC = CO <= 4 ? 4 : 2;
  const int CLV = C / VEC;
  int PS = 512 / CLV;
  PS = PS > 16 ? 16 : PS;
  const int block = PS * CLV, halo = taps == 9 ? 1 : 0;
  const int N = CO * taps * C;
  // rows per unit: ~512 pixels, shrunk until the dF tile fits beside the accumulator table
  int R = 512 / W;
  R = R < 1 ? 1 : (R > H ? H : R);
  auto lds = [&](int r) { return wgrad_lds(CO, taps, C, W, r); };
  while (R > 1 && lds(R) > LOWRANK_LDS_MAX) --R;
  EDM_REQUIRE(lds(R) <= LOWRANK_LDS_MAX, "lowrank_wgrad: Co=%d, taps=%d, C=%d, W=%d need %zu bytes of LDS (60 KB at most)", CO,
              taps, C, W, lds(R));
  const int upb = (H + R - 1) / R;
  EDM_REQUIRE((long)B * upb < (1L << 31), "lowrank_wgrad: too many units");
  const int nunits = B * upb;
  const int grid = nunits < nwg ? nunits : nwg;
  EDM_REQUIRE(ws_floats >= (long)grid * (N + 4), "lowrank_wgrad: workspace of %ld floats, %ld needed", ws_floats,
              (long)grid * (N + 4));
  if (taps == 9)
    hipLaunchKernelGGL((k_lowrank_wgrad<CO, 9, VEC>), dim3(grid), dim3(block), lds(R), st, dF, (const bf16*)X, aux, ws, H, W, C,
                       R, upb, nunits);
  else
    hipLaunchKernelGGL((k_lowrank_wgrad<CO, 1, VEC>), dim3(grid), dim3(block), lds(R), st, dF, (const bf16*)X, aux, ws, H, W, C,
                       R, upb, nunits);
  EDM_CHECK_LAUNCH("lowrank_wgrad");
  hipLaunchKernelGGL(k_lowrank_reduce, dim3((N + 1 + 63) / 64), dim3(1024), 0, st, ws, grid, N, G, aux_out);
  EDM_CHECK_LAUNCH("lowrank_reduce");
  return EDM_OK;
}

// workgroups of the first stage = rows of the workspace (a constant: the summation order does not depend on the device)
constexpr int LOWRANK_WGRAD_NWG = 256;     // (k_lowrank_reduce: 16 segments of at most 16 rows)
extern "C" long edm_lowrank_wgrad_workspace(int C, int Co, int taps) {
  return (long)LOWRANK_WGRAD_NWG * ((long)Co * taps * C + 4);
}

// G (fp32 [Co][taps][C], overwritten) = sum_p dF[p, o] * X[p + d(t), c]; X bf16 NHWC [B, H, W, C], taps 1 or 9.
// aux (nullable, fp32 like dF): *aux_out += sum of aux, added up in the same fixed order.  ws: edm_lowrank_wgrad_workspace floats.
extern "C" int edm_lowrank_wgrad(const float* dF, const void* X, int taps, const float* aux, float* G, float* aux_out,
                                 float* ws, long ws_floats, int B, int H, int W, int C, int Co, hipStream_t st) {
  EDM_REQUIRE(dF && X && G && ws && (!aux || aux_out), "lowrank_wgrad: null pointer");
  EDM_REQUIRE(B > 0 && H > 0 && W > 0 && C > 0 && C % 8 == 0 && C <= 1024 && Co >= 1 && Co <= 8 && (taps == 1 || taps == 9),
              "lowrank_wgrad: bad args (C %% 8 == 0, Co <= 8, taps 1 or 9 required)");
#define CALL(CO_) launch_wgrad<CO_>(dF, X, taps, aux, G, aux_out, ws, ws_floats, B, H, W, C, LOWRANK_WGRAD_NWG, st)
  EDM_CO_SWITCH(Co, CALL)
#undef CALL
}

// ------------------------------------------------------------------ the two tiny expansions through Wout
// (a) Wc[o][t][ci] = sum_c Wout[o, c] * float(wd[taps - 1 - t][ci][c]): from the dgrad pack of the conv ([tap][I][O] bf16,
// taps flipped, plain layout) -- the very bf16 values the MFMA dgrad multiplies.  One wave per pack row.
__global__ void k_lowrank_expand_wc(const float* __restrict__ wout, const bf16* __restrict__ wd, float* __restrict__ Wc,
                                    int Co, int O, int I, int taps) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);      // (tap of the pack, ci)
  if (row >= taps * I) return;
  const int tt = row / I, ci = row - tt * I;
  float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int c = lane * 8; c < O; c += 64 * 8) {
    float v[8];
    load8(wd + (long)row * O + c, v);
#pragma unroll
    for (int o = 0; o < 8; ++o)
      if (o < Co) {
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[o] += wout[(long)o * O + c + j] * v[j];
      }
  }
#pragma unroll
  for (int o = 0; o < 8; ++o)
    if (o < Co) {
      const float s = wave_sum(acc[o]);
      if (lane == 0) Wc[((long)o * taps + (taps - 1 - tt)) * I + ci] = s;
    }
}
extern "C" int edm_lowrank_expand_wc(const float* wout_hat, const void* wd, float* Wc, int Co, int O, int I, int taps,
                                     hipStream_t st) {
  EDM_REQUIRE(wout_hat && wd && Wc, "lowrank_expand_wc: null pointer");
  EDM_REQUIRE(Co >= 1 && Co <= 8 && O > 0 && O % 8 == 0 && I > 0 && taps >= 1, "lowrank_expand_wc: bad args");
  hipLaunchKernelGGL(k_lowrank_expand_wc, dim3((taps * I + 3) / 4), dim3(256), 0, st, wout_hat, (const bf16*)wd, Wc, Co, O,
                     I, taps);
  EDM_CHECK_LAUNCH("lowrank_expand_wc");
  return EDM_OK;
}

// (b) slab[t][c][i] = scale * sum_o Wout[o, c] * G[o][t][i] (i < I; zero up to Ipad): ONE weight-gradient slab
// [1][taps][O][Ipad] in packed order, which edm_wgrad_finish / edm_wgrad_finish_multi project like any other
__global__ void k_lowrank_expand_slab(const float* __restrict__ wout, const float* __restrict__ G, float* __restrict__ slab,
                                      float scale, int Co, int O, int I, int Ipad, int taps, long n) {
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (long)gridDim.x * blockDim.x) {
    const int i = (int)(e % Ipad);
    const long tc = e / Ipad;
    const int c = (int)(tc % O), t = (int)(tc / O);
    float s = 0.f;
    if (i < I)
      for (int o = 0; o < Co; ++o) s += wout[(long)o * O + c] * G[((long)o * taps + t) * I + i];
    slab[e] = scale * s;
  }
}
extern "C" int edm_lowrank_expand_slab(const float* wout_hat, const float* G, float* slab, float scale, int Co, int O, int I,
                                       int Ipad, int taps, hipStream_t st) {
  EDM_REQUIRE(wout_hat && G && slab, "lowrank_expand_slab: null pointer");
  EDM_REQUIRE(Co >= 1 && Co <= 8 && O > 0 && I > 0 && Ipad >= I && taps >= 1, "lowrank_expand_slab: bad args");
  const long n = (long)taps * O * Ipad;
  const long blocks = (n + 255) / 256;
  hipLaunchKernelGGL(k_lowrank_expand_slab, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, st, wout_hat, G,
                     slab, scale, Co, O, I, Ipad, taps, n);
  EDM_CHECK_LAUNCH("lowrank_expand_slab");
  return EDM_OK;
}

// ================================================================== the forward side of the same algebra
// The last decoder block ends in h = b * conv3x3(a2, W2) + a * conv1x1(cat, W1) and conv_out reduces h to Co channels at
// once (F = Wout . h, nothing in between), so
//   F[p, o] = b * sum_t sum_ci a2[p + d(t), ci] * Wc[o, t, ci]  +  a * sum_cj cat[p, cj] * Wp[o, cj]        Wp = Wout . W1
// (Wp = Wout itself when the block has no 1x1 conv: cat is then the block input, Cc == C): 2 * (9 C + Cc) * Co FLOP per
// pixel from tables of Co * (9 C + Cc) floats, and h never exists.
//
// grid = (ceil(H / R), B): a workgroup owns R whole rows of one sample.  LDS: Wc [CO * 9][C], Wp [CO][Cc] and the tile of
// partial sums pt [3 ky][R * W][3 kx * CO] + [R * W][CO].  Input-stationary: 8 lanes share a pixel (lane `lig` takes the
// 8-channel chunks lig, lig + 8, ...), a lane works on PX pixels at once so that a weight vector read from LDS serves PX
// of them; the 8 partial dot products meet by a butterfly (fixed order) and land in pt at the slot of the OUTPUT row they
// belong to (input row y feeds output row y - (ky - 1): for each ky only the rows that have an output row in the tile are
// read, so the halo rows cost one ky pass, not three).  The second phase adds, per output value, its taps in the order
// t = 0 .. 8 (skipping those outside the image: zero padding), then the 1x1 term: bit-equal from run to run.
constexpr int TAIL_LPP = 8;     // lanes per pixel
static size_t tail_fwd_lds(int Co, int C, int Cc, int W, int R) {
  return ((size_t)Co * 9 * C + (size_t)Co * Cc + (size_t)R * W * 10 * Co) * sizeof(float);
}
// 1 when edm_lowrank_tail_fwd runs maps of width W: a2 with C channels, cat with Cc, Co outputs
extern "C" int edm_lowrank_tail_supported(int C, int Cc, int Co, int W) {
  if (C <= 0 || C % 8 || C > 1024 || Cc <= 0 || Cc % 8 || Cc > 2048 || Co < 1 || Co > 8 || W <= 0) return 0;
  return tail_fwd_lds(Co, C, Cc, W, 1) <= LOWRANK_LDS_MAX;
}

// NV = NK * CO dot products over Cx channels of PX pixels (xp[k]: the lane's view of pixel k, NULL = no pixel) against
// the LDS rows w[(o * wso + k) * Cx ...]; every lane of the pixel's group returns the full sums in s
template <int CO, int NK, int PX>
__device__ __forceinline__ void tail_dots(const bf16* const (&xp)[PX], int Cx, const float* __restrict__ w, int wso, int lig,
                                          float (&s)[PX][NK * CO]) {
  f32x2 acc[PX][NK * CO];
#pragma unroll
  for (int k = 0; k < PX; ++k)
#pragma unroll
    for (int v = 0; v < NK * CO; ++v) acc[k][v] = f32x2{0.f, 0.f};
  const int CL = Cx >> 3;
  for (int c8 = lig; c8 < CL; c8 += TAIL_LPP) {
    f32x2 xf[PX][4];
#pragma unroll
    for (int k = 0; k < PX; ++k) {
      u32x4 raw = u32x4{0u, 0u, 0u, 0u};
      if (xp[k]) raw = *reinterpret_cast<const u32x4*>(xp[k] + c8 * 8);
      const bf16x8 xv = __builtin_bit_cast(bf16x8, raw);
#pragma unroll
      for (int h = 0; h < 4; ++h) xf[k][h] = f32x2{(float)xv[2 * h], (float)xv[2 * h + 1]};
    }
#pragma unroll
    for (int o = 0; o < CO; ++o)
#pragma unroll
      for (int kk = 0; kk < NK; ++kk) {
        const float* wp = w + (long)(o * wso + kk) * Cx + c8 * 8;
        const f32x4 w0 = *reinterpret_cast<const f32x4*>(wp), w1 = *reinterpret_cast<const f32x4*>(wp + 4);
        const f32x2 wv[4] = {f32x2{w0[0], w0[1]}, f32x2{w0[2], w0[3]}, f32x2{w1[0], w1[1]}, f32x2{w1[2], w1[3]}};
#pragma unroll
        for (int k = 0; k < PX; ++k)
#pragma unroll
          for (int h = 0; h < 4; ++h) acc[k][kk * CO + o] += xf[k][h] * wv[h];
      }
  }
#pragma unroll
  for (int k = 0; k < PX; ++k)
#pragma unroll
    for (int v = 0; v < NK * CO; ++v) s[k][v] = group_sum<TAIL_LPP>(acc[k][v][0] + acc[k][v][1]);
}

template <int CO, int PX>
__global__ __launch_bounds__(512) void k_lowrank_tail_fwd(const bf16* __restrict__ a2, const bf16* __restrict__ cat,
                                                          const float* __restrict__ Wc, const float* __restrict__ Wp,
                                                          float sb, float sa, const float* __restrict__ gain_out,
                                                          const float* __restrict__ noisy, const float* __restrict__ sigma,
                                                          int sstride, float sd, float* __restrict__ D,
                                                          float* __restrict__ Fraw, int H, int W, int C, int Cc, int R) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  float* wl = sm;                               // [CO * 9][C]
  float* wpl = wl + CO * 9 * C;                 // [CO][Cc]
  float* pt = wpl + CO * Cc;                    // [3][R * W][3 * CO], then [R * W][CO]
  const int RW = R * W;
  float* qt = pt + 3 * RW * 3 * CO;
  const int b = blockIdx.y, y0 = blockIdx.x * R;
  const int rows = min(R, H - y0);
  for (int i = threadIdx.x; i < CO * 9 * C / 4; i += blockDim.x)
    reinterpret_cast<f32x4*>(wl)[i] = reinterpret_cast<const f32x4*>(Wc)[i];
  for (int i = threadIdx.x; i < CO * Cc / 4; i += blockDim.x)
    reinterpret_cast<f32x4*>(wpl)[i] = reinterpret_cast<const f32x4*>(Wp)[i];
  __syncthreads();
  const int lig = threadIdx.x % TAIL_LPP, grp = threadIdx.x / TAIL_LPP, NG = blockDim.x / TAIL_LPP;
  // ---- the nine taps: per ky, the input rows y0 + ky - 1 ... that lie in the image (contiguous pixels of the sample)
#pragma unroll 1
  for (int ky = 0; ky < 3; ++ky) {
    const int r_lo = max(y0 + ky - 1, 0), r_hi = min(y0 + rows - 1 + ky - 1, H - 1);
    const int np = (r_hi - r_lo + 1) * W;                    // (<= 0: a one-row image has no row above / below)
    const int slot0 = (r_lo - (y0 + ky - 1)) * W;            // slot of the first pixel: its OUTPUT row's place in the tile
    const bf16* base = a2 + (((long)b * H + r_lo) * W) * C;
    float* po = pt + (long)ky * RW * 3 * CO;
    for (int n0 = grp * PX; n0 < np; n0 += NG * PX) {
      const bf16* xp[PX];
#pragma unroll
      for (int k = 0; k < PX; ++k) xp[k] = n0 + k < np ? base + (long)(n0 + k) * C : nullptr;
      float s[PX][3 * CO];
      tail_dots<CO, 3, PX>(xp, C, wl + ky * 3 * C, 9, lig, s);
#pragma unroll
      for (int k = 0; k < PX; ++k)
        if (n0 + k < np) {
#pragma unroll
          for (int v = 0; v < 3 * CO; ++v)
            if ((v % TAIL_LPP) == lig) po[(long)(slot0 + n0 + k) * 3 * CO + v] = s[k][v];
        }
    }
  }
  // ---- the 1x1 term over cat: the tile's own rows
  {
    const int np = rows * W;
    const bf16* base = cat + (((long)b * H + y0) * W) * Cc;
    for (int n0 = grp * PX; n0 < np; n0 += NG * PX) {
      const bf16* xp[PX];
#pragma unroll
      for (int k = 0; k < PX; ++k) xp[k] = n0 + k < np ? base + (long)(n0 + k) * Cc : nullptr;
      float s[PX][CO];
      tail_dots<CO, 1, PX>(xp, Cc, wpl, 1, lig, s);
#pragma unroll
      for (int k = 0; k < PX; ++k)
        if (n0 + k < np) {
#pragma unroll
          for (int v = 0; v < CO; ++v)
            if ((v % TAIL_LPP) == lig) qt[(long)(n0 + k) * CO + v] = s[k][v];
        }
    }
  }
  __syncthreads();
  // ---- every output value: its taps in the order t = 0 .. 8, then the 1x1 term; D as k_conv_out_fwd forms it
  const float go = *gain_out;
  const float sg = sigma[b * sstride];
  const float den = sg * sg + sd * sd;
  const float cskip = sd * sd / den, cout = sg * sd * rsqrtf(den);
  for (int i = threadIdx.x; i < CO * rows * W; i += blockDim.x) {
    const int o = i / (rows * W), n = i - o * rows * W;
    const int ry = n / W, x = n - ry * W;
    float s = 0.f;
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) {
      const int iy = y0 + ry + ky - 1;
      if (iy < 0 || iy >= H) continue;
#pragma unroll
      for (int kx = 0; kx < 3; ++kx) {
        const int ix = x + kx - 1;
        if (ix < 0 || ix >= W) continue;
        s += pt[((long)ky * RW + ry * W + ix) * 3 * CO + kx * CO + o];
      }
    }
    const float f = sb * s + sa * qt[(long)n * CO + o];
    const long idx = (((long)b * CO + o) * H + y0 + ry) * W + x;
    if (Fraw) Fraw[idx] = f;
    D[idx] = f * go * cout + noisy[idx] * cskip;
  }
}

template <int CO>
static int launch_tail_fwd(const void* a2, const void* cat, const float* Wc, const float* Wp, float sb, float sa,
                           const float* gain_out, const float* noisy, const float* sigma, int sstride, float sd, float* D,
                           float* Fraw, int B, int H, int W, int C, int Cc, hipStream_t st) {
  // two pixels per lane up to Co = 4 (2 * 9 * Co packed accumulators), one above
  constexpr int PX = CO <= 4 ? 2 : 1;
  // rows per workgroup: ~128 pixels (the tile of partial sums: 10 Co floats per pixel), shrunk until the tables fit
  int R = 128 / W;
  R = R < 1 ? 1 : (R > H ? H : R);
  auto lds = [&](int r) { return tail_fwd_lds(CO, C, Cc, W, r); };
  while (R > 1 && lds(R) > LOWRANK_LDS_MAX) --R;
  EDM_REQUIRE(lds(R) <= LOWRANK_LDS_MAX, "lowrank_tail_fwd: Co=%d, C=%d, Cc=%d, W=%d need %zu bytes of LDS (60 KB at most)", CO,
              C, Cc, W, lds(R));
  // a workgroup has 8 lanes per pixel: no more threads than the tile's largest pass can use
  const long want = ((long)(R + 1) * W + PX - 1) / PX * TAIL_LPP;
  int block = want >= 512 ? 512 : (int)((want + 63) / 64 * 64);
  const dim3 grid((H + R - 1) / R, B);
  hipLaunchKernelGGL((k_lowrank_tail_fwd<CO, PX>), grid, dim3(block), lds(R), st, (const bf16*)a2, (const bf16*)cat, Wc, Wp, sb,
                     sa, gain_out, noisy, sigma, sstride, sd, D, Fraw, H, W, C, Cc, R);
  EDM_CHECK_LAUNCH("lowrank_tail_fwd");
  return EDM_OK;
}

// Fraw (fp32 NCHW [B, Co, H, W], nullable) = sb * conv3x3(a2, Wc) + sa * cat . Wp and D = Fraw * gain_out * c_out(sigma) +
// noisy * c_skip(sigma): what edm_conv_out_fwd writes for the block's output.  a2 bf16 NHWC [B, H, W, C], cat bf16 NHWC
// [B, H, W, Cc], Wc fp32 [Co][9][C] (edm_lowrank_expand_wc), Wp fp32 [Co][Cc].
extern "C" int edm_lowrank_tail_fwd(const void* a2, const void* cat, const float* Wc, const float* Wp, float sb, float sa,
                                    const float* gain_out, const float* noisy, const float* sigma, int sigma_stride,
                                    float sigma_data, float* D, float* Fraw, int B, int H, int W, int C, int Cc, int Co,
                                    hipStream_t st) {
  EDM_REQUIRE(a2 && cat && Wc && Wp && gain_out && noisy && sigma && D, "lowrank_tail_fwd: null pointer");
  EDM_REQUIRE(B > 0 && B <= 65535 && H > 0 && W > 0 && (sigma_stride == 0 || sigma_stride == 1), "lowrank_tail_fwd: bad args");
  EDM_REQUIRE(edm_lowrank_tail_supported(C, Cc, Co, W), "lowrank_tail_fwd: unsupported shape C=%d Cc=%d Co=%d W=%d", C, Cc, Co, W);
  EDM_REQUIRE((((uintptr_t)Wc | (uintptr_t)Wp | (uintptr_t)a2 | (uintptr_t)cat) & 15) == 0,
              "lowrank_tail_fwd: operands must be 16-byte aligned");
#define CALL(CO_) launch_tail_fwd<CO_>(a2, cat, Wc, Wp, sb, sa, gain_out, noisy, sigma, sigma_stride, sigma_data, D, Fraw, B, \
                                       H, W, C, Cc, st)
  EDM_CO_SWITCH(Co, CALL)
#undef CALL
}

// ------------------------------------------------------------------ conv_out's weight gradient without h
// gwh[o, c] = sb * sum_t sum_ci float(wf2[t][c][ci]) * G[o][t][ci] + sa * sum_cj float(wf1[c][cj]) * G1[o][cj]
// (wf1 == NULL: + sa * G1[o][c]): dWout = dF^T h with h = sb * conv(a2, W2) + sa * W1 cat pushed onto the two reductions
// the backward has anyway.  wf2 / wf1: the plain bf16 forward packs [taps][O][I].  One wave per channel c, lanes over
// 8-channel chunks of the rows, the 64 partial sums meet by a butterfly: bit-equal from run to run.
__global__ __launch_bounds__(256) void k_lowrank_tail_dwout(const float* __restrict__ G, const bf16* __restrict__ wf2,
                                                            const float* __restrict__ G1, const bf16* __restrict__ wf1,
                                                            float sb, float sa, float* __restrict__ gwh, int Co, int C,
                                                            int Cc) {
  const int lane = threadIdx.x & 63;
  const int c = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (c >= C) return;
  float a9[8] = {0, 0, 0, 0, 0, 0, 0, 0}, a1[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int t = 0; t < 9; ++t)
    for (int ci = lane * 8; ci < C; ci += 64 * 8) {
      float v[8];
      load8(wf2 + ((long)t * C + c) * C + ci, v);
#pragma unroll
      for (int o = 0; o < 8; ++o)
        if (o < Co) {
          const float* gp = G + ((long)o * 9 + t) * C + ci;
#pragma unroll
          for (int j = 0; j < 8; ++j) a9[o] += v[j] * gp[j];
        }
    }
  if (wf1)
    for (int cj = lane * 8; cj < Cc; cj += 64 * 8) {
      float v[8];
      load8(wf1 + (long)c * Cc + cj, v);
#pragma unroll
      for (int o = 0; o < 8; ++o)
        if (o < Co) {
          const float* gp = G1 + (long)o * Cc + cj;
#pragma unroll
          for (int j = 0; j < 8; ++j) a1[o] += v[j] * gp[j];
        }
    }
#pragma unroll
  for (int o = 0; o < 8; ++o)
    if (o < Co) {
      const float s9 = wave_sum(a9[o]);
      const float s1 = wf1 ? wave_sum(a1[o]) : G1[(long)o * Cc + c];
      if (lane == 0) gwh[(long)o * C + c] = sb * s9 + sa * s1;
    }
}
extern "C" int edm_lowrank_tail_dwout_supported(int C, int Cc, int Co, int has1) {
  return C > 0 && C % 8 == 0 && Cc > 0 && Cc % 8 == 0 && Co >= 1 && Co <= 8 && (has1 || Cc == C);
}
extern "C" int edm_lowrank_tail_dwout(const float* G, const void* wf2, const float* G1, const void* wf1, float sb, float sa,
                                      float* gwh, int Co, int C, int Cc, hipStream_t st) {
  EDM_REQUIRE(G && wf2 && G1 && gwh, "lowrank_tail_dwout: null pointer");
  EDM_REQUIRE(edm_lowrank_tail_dwout_supported(C, Cc, Co, wf1 != nullptr), "lowrank_tail_dwout: bad args (C=%d Cc=%d Co=%d)", C, Cc,
              Co);
  EDM_REQUIRE((((uintptr_t)wf2 | (uintptr_t)wf1) & 15) == 0, "lowrank_tail_dwout: packs must be 16-byte aligned");
  hipLaunchKernelGGL(k_lowrank_tail_dwout, dim3((C + 3) / 4), dim3(256), 0, st, G, (const bf16*)wf2, G1, (const bf16*)wf1, sb,
                     sa, gwh, Co, C, Cc);
  EDM_CHECK_LAUNCH("lowrank_tail_dwout");
  return EDM_OK;
}

// ------------------------------------------------------------------ d loss / d cat without g_h
// out[p, cj] = bf16(float(t[p, cj]) + sa * sum_o dF[p, o] * Wp[o, cj]): the 1x1 dgrad of g_h = dF . Wout with the dense part
// t (bf16 NHWC [B, H, W, Cc], rounded as the dense kernels round it) as its residual.  The columns below Ci go to gu
// [.., Ci], the others to gcs [.., Cc - Ci] (gcs == NULL: Ci == Cc): the two halves conv_igemm(split =) writes.
__global__ void k_lowrank_gcat_add(const float* __restrict__ dF, const float* __restrict__ Wp, float sa,
                                   const bf16* __restrict__ t, bf16* __restrict__ gu, bf16* __restrict__ gcs, int HW, int Cc,
                                   int Ci, int Co, long n8) {
  const unsigned CL = (unsigned)Cc >> 3, uHW = (unsigned)HW, CiL = (unsigned)Ci >> 3;
  for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < (unsigned)n8; i += gridDim.x * blockDim.x) {
    const unsigned p = i / CL, c8 = i - p * CL;
    const unsigned b = p / uHW, hw = p - b * uHW;
    float v[8] = {0, 0, 0, 0, 0, 0, 0, 0}, tv[8];
    load8(t + (long)i * 8, tv);
    for (int o = 0; o < Co; ++o) {
      const float df = dF[((long)b * Co + o) * HW + hw];
      const float* wp = Wp + (long)o * Cc + c8 * 8;
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] += df * wp[j];
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = tv[j] + sa * v[j];
    if (c8 < CiL) store8(gu + ((long)p * Ci + c8 * 8), v);
    else store8(gcs + ((long)p * (Cc - Ci) + (c8 - CiL) * 8), v);
  }
}
extern "C" int edm_lowrank_gcat_supported(int Cc, int Ci, int Co) {
  return Cc > 0 && Cc % 8 == 0 && Ci > 0 && Ci % 8 == 0 && Ci <= Cc && Co >= 1 && Co <= 8;
}
extern "C" int edm_lowrank_gcat_add(const float* dF, const float* Wp, float sa, const void* t, void* gu, void* gcs, int B,
                                    int HW, int Cc, int Ci, int Co, hipStream_t st) {
  EDM_REQUIRE(dF && Wp && t && gu, "lowrank_gcat_add: null pointer");
  EDM_REQUIRE(B > 0 && HW > 0 && edm_lowrank_gcat_supported(Cc, Ci, Co) && (gcs || Ci == Cc),
              "lowrank_gcat_add: bad args (Cc=%d Ci=%d Co=%d)", Cc, Ci, Co);
  const long n8 = (long)B * HW * (Cc / 8);
  EDM_REQUIRE(n8 < (1L << 31), "lowrank_gcat_add: too many elements");
  const long blocks = (n8 + 255) / 256;
  hipLaunchKernelGGL(k_lowrank_gcat_add, dim3((unsigned)(blocks < 8192 ? blocks : 8192)), dim3(256), 0, st, dF, Wp, sa,
                     (const bf16*)t, (bf16*)gu, (bf16*)gcs, HW, Cc, Ci, Co, n8);
  EDM_CHECK_LAUNCH("lowrank_gcat_add");
  return EDM_OK;
}
