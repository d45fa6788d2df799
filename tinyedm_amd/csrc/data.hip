// Data formats on either side of the hot path: the image datasets stay RESIDENT in HBM
// as uint8 (CIFAR-10 train = 150 MB of 288 GB) and a batch is produced by one gather kernel -- no host dataloader,
// no pinned staging, no H2D copy in the training loop -- and sampled images leave the GPU already as bytes.
//
// Byte/float conversions follow the reference's arithmetic operation by operation (separately rounded fp32
// multiply / add / divide, no FMA contraction) so that the uint8 outputs are bit-exact:
//   * load  : torchvision v2.ToDtype(float32, scale=True) -> x/255, RandomHorizontalFlip, Normalize(0.5, 0.5) ->
//             (x/255 - 0.5)/0.5                      (datamodules/cifar10datamodule.py:18-32, mnistdatamodule.py:18-30)
//   * store : (x*127.5 + 128).clip(0, 255).to(uint8)                    (cifar10datamodule.py:34-35)
//   * PNG   : clamp(pred*std*2 + mean, 0, 1).permute(0,2,3,1)*255 -> uint8          (callbacks.py:126-156)
#include "common.h"

// bit-exact parity with the reference's op-by-op fp32 arithmetic: no mul+add fusion anywhere in this file
#pragma clang fp contract(off)

namespace {

// dataset u8 [N][C][H][W] (planar, the on-disk order of CIFAR-10 / MNIST); out fp32 NCHW [B][C][H][W];
// sample b reads image index[b]; flip decided per sample by Philox(seed, (epoch, b)) bit 0 when flip != 0.
__global__ __launch_bounds__(256) void k_u8_gather_normalize(const unsigned char* __restrict__ data,
                                                               const long* __restrict__ index, float* __restrict__ out,
                                                               int C, int H, int W, long n_images, float mean, float stdv,
                                                               int flip, unsigned long long seed, unsigned epoch) {
  const int b = blockIdx.y;
  const long img = index[b];
  if (img < 0 || img >= n_images) return;  // host validates; never read out of bounds
  bool do_flip = false;
  if (flip) {
    const Philox4 r = philox4x32_10((uint32_t)b, 0u, 0x0da7u, epoch, (uint32_t)seed, (uint32_t)(seed >> 32));
    do_flip = (r.x & 1u) != 0u;
  }
  const int chw = C * H * W;
  const unsigned char* src = data + img * chw;
  float* dst = out + (long)b * chw;
  for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < chw; e += gridDim.x * blockDim.x) {
    const int w = e % W;
    const int se = do_flip ? e - w + (W - 1 - w) : e;
    const float x = (float)src[se] / 255.0f;  // IEEE division (hipcc default: correctly rounded fp32 divide)
    dst[e] = (x - mean) / stdv;
  }
}

// ---- non-leaking augmentation: the exact (pixel-permutation) subset of the EDM pipe (Karras et al. 2022, App. F.2)
// Parameters of sample b, drawn from two Philox streams keyed like the flip above, counter tag AUG_TAG:
//   E = philox4x32_10((b, 0, AUG_TAG, epoch), (seed_lo, seed_hi)):   op i of (xflip, yflip, translate, rot90) is enabled iff
//       bit i of `ops` is set and word i of E (x, y, z, w) < thr   (thr = round(p * 2^32) in [0, 2^32])
//   D_j = philox4x32_10((b, 1 + j, AUG_TAG, epoch), (seed_lo, seed_hi)), j = 0, 1, ...:
//       xflip bit = D_0.x & 1;  yflip bit = (D_0.x >> 1) & 1;  k = (D_0.x >> 2) & 3;
//       sx = u(D_j.y, 2 * (W / 8) + 1) - W / 8;  sy = u(D_j.z, 2 * (H / 8) + 1) - H / 8, where u(word, n) takes the FIRST j
//       whose word < floor(2^32 / n) * n and returns word % n: every value of [0, n) has the same number of accepted words,
//       so the draw is unbiased (a word is rejected with probability < n / 2^32).  sx and sy look for their j
//       independently.  After AUG_TRIES rejected words (probability < 2^-256 for n < 2^16) the last one is used as it is.
// The draws of a disabled op are made and ignored, so enabling one op never moves another's parameters.
constexpr uint32_t AUG_TAG = 0x41554731u;  // "AUG1": differs from 0x0da7 above and from the tags of optim.hip / solver_steps.hip / sample_eval.hip / linear.hip
constexpr int AUG_TRIES = 16;

struct AugDraw {
  int xflip, yflip, sx, sy, k;
};

__device__ __forceinline__ AugDraw aug_draw(uint32_t b, uint32_t epoch, unsigned long long seed, unsigned long long thr,
                                            int ops, int H, int W) {
  AugDraw a = {0, 0, 0, 0, 0};
  if (thr == 0 || ops == 0) return a;
  const uint32_t s0 = (uint32_t)seed, s1 = (uint32_t)(seed >> 32);
  const Philox4 en = philox4x32_10(b, 0u, AUG_TAG, epoch, s0, s1);
  const bool e_x = (ops & 1) && (unsigned long long)en.x < thr, e_y = (ops & 2) && (unsigned long long)en.y < thr;
  const bool e_t = (ops & 4) && (unsigned long long)en.z < thr, e_r = (ops & 8) && (unsigned long long)en.w < thr;
  const uint32_t nw = 2u * (uint32_t)(W / 8) + 1u, nh = 2u * (uint32_t)(H / 8) + 1u;
  const unsigned long long lim_w = (1ull << 32) / nw * nw, lim_h = (1ull << 32) / nh * nh;
  bool have_x = false, have_y = false;
  uint32_t ux = 0, uy = 0;
  for (int j = 0; j < AUG_TRIES && !(have_x && have_y); ++j) {
    const Philox4 d = philox4x32_10(b, 1u + (uint32_t)j, AUG_TAG, epoch, s0, s1);
    if (j == 0) {
      a.xflip = e_x ? (int)(d.x & 1u) : 0;
      a.yflip = e_y ? (int)((d.x >> 1) & 1u) : 0;
      a.k = e_r ? (int)((d.x >> 2) & 3u) : 0;
    }
    if (!have_x && (d.y < lim_w || j == AUG_TRIES - 1)) { ux = d.y % nw; have_x = true; }
    if (!have_y && (d.z < lim_h || j == AUG_TRIES - 1)) { uy = d.z % nh; have_y = true; }
  }
  if (e_t) {
    a.sx = (int)ux - W / 8;
    a.sy = (int)uy - H / 8;
  }
  return a;
}

// k_u8_gather_normalize with the augmentation composed into the gather: forward order flip (the unlabelled CIFAR flip of the
// kernel above, same Philox word), xflip, yflip, translate by (sx, sy) whole pixels with the vacated border reflected
// without edge repeat (numpy pad(mode="reflect")), np.rot90(k) over (H, W).  Each OUTPUT element walks that chain backwards
// to its source byte; the byte -> float arithmetic is the kernel's above.  aug [B][6] fp32 receives the labels
// (xflip, yflip, sx / W, sy / H, cos(k pi/2) - 1, sin(k pi/2)), zeros for a disabled op.  The host guarantees H == W when
// rot90 is in `ops`.  A sample whose index is out of range is skipped whole: neither its image nor its label row is written.
__global__ __launch_bounds__(256) void k_u8_gather_augment_normalize(
    const unsigned char* __restrict__ data, const long* __restrict__ index, float* __restrict__ out, int C, int H, int W,
    long n_images, float mean, float stdv, int flip, unsigned long long seed, unsigned epoch, unsigned long long thr, int ops,
    float* __restrict__ aug) {
  const int b = blockIdx.y;
  const long img = index[b];
  if (img < 0 || img >= n_images) return;  // host validates; never read out of bounds
  bool do_flip = false;
  if (flip) {
    const Philox4 r = philox4x32_10((uint32_t)b, 0u, 0x0da7u, epoch, (uint32_t)seed, (uint32_t)(seed >> 32));
    do_flip = (r.x & 1u) != 0u;
  }
  const AugDraw a = aug_draw((uint32_t)b, epoch, seed, thr, ops, H, W);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    float* l = aug + (long)b * 6;
    l[0] = (float)a.xflip;
    l[1] = (float)a.yflip;
    l[2] = (float)a.sx / (float)W;
    l[3] = (float)a.sy / (float)H;
    l[4] = a.k == 0 ? 0.f : (a.k == 2 ? -2.f : -1.f);  // the exact table (0,0), (-1,1), (-2,0), (-1,-1)
    l[5] = a.k == 1 ? 1.f : (a.k == 3 ? -1.f : 0.f);
  }
  const bool mirror = (a.xflip != 0) != do_flip;  // two left-right flips in a row cancel
  const int chw = C * H * W;
  const unsigned char* src = data + img * chw;
  float* dst = out + (long)b * chw;
  for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < chw; e += gridDim.x * blockDim.x) {
    const int w = e % W, t = e / W, h = t % H, c = t / H;
    int i = h, j = w;
    // rot90 backwards (H == W): out[i][j] = in[j][W-1-i] (k = 1), in[H-1-i][W-1-j] (k = 2), in[W-1-j][i] (k = 3)
    if (a.k == 1) { i = w; j = W - 1 - h; }
    else if (a.k == 2) { i = H - 1 - h; j = W - 1 - w; }
    else if (a.k == 3) { i = W - 1 - w; j = h; }
    // translate backwards; |s| <= size / 8 <= size - 1, so one reflection lands inside
    i -= a.sy;
    i = i < 0 ? -i : (i >= H ? 2 * (H - 1) - i : i);
    j -= a.sx;
    j = j < 0 ? -j : (j >= W ? 2 * (W - 1) - j : j);
    if (a.yflip) i = H - 1 - i;
    if (mirror) j = W - 1 - j;
    const float x = (float)src[(c * H + i) * W + j] / 255.0f;  // the arithmetic of k_u8_gather_normalize
    dst[e] = (x - mean) / stdv;
  }
}

// ---- non-leaking augmentation, the continuous ops of the EDM pipe: zoom, rotate, stretch, shift ("Continuous
// augmentation").  One channel plane S [H][W] of the exactly-augmented image (byte units, the chain above), extended to all
// integers by reflection without edge repeat, goes through
//   up x2 :  U[u][v] = 2 sum_ij S~[i][j] h[u - 2 i + o] h[v - 2 j + o]          (h = sym6 low-pass, 12 taps, o = 5)
//   warp  :  V[u][v] = bilinear interpolation of U at q = Theta (u, v, 1)^T,      u in [-o, 2 H + 4], v in [-o, 2 W + 4]
//   down x2: D[i][j] = 1/2 sum_uv V[u][v] h[u - 2 i + o] h[v - 2 j + o]
// and leaves as ((D / 255) - mean) / std, unclamped.  Theta identity gives D == S up to rounding (h is orthonormal).
// Draws of sample b: same key and AUG_TAG as aug_draw, counter words it never reads:
//   E' = philox4x32_10((b, 32, AUG_TAG, epoch)): op i of (zoom, rotate, stretch, shift) is enabled iff bit i of `wops` is set
//        and word i of E' < thr;   W0 = philox(b, 33, ...), W1 = philox(b, 34, ...)
//   uni(w) = ((w >> 8) + 0.5) 2^-24 (exact in fp32, never 0 or 1);  bm(a, b) = sqrt(-2 ln uni(a)) (cos, sin)(2 pi uni(b))
//   zoom:    n_s = bm(W0.x, W0.y).cos, s = 2^(0.2 n_s)          rotate: theta = pi (2 uni(W0.z) - 1)
//   stretch: n_a = bm(W0.w, W1.x).cos, phi = pi (2 uni(W1.y) - 1), a = 2^(0.2 n_a)
//   shift:   (n_x, n_y) = bm(W1.z, W1.w), t = (0.125 H n_y, 0.125 W n_x) pixels
// Labels 6..12: (n_s, cos(theta) - 1, sin(theta), n_a cos(phi), n_a sin(phi), n_x, n_y), zeros for a disabled op.
// Geometry: 2x-grid index u sits at pixel (u - c) / 2, c = the taps' centroid - o; on (y, x) offsets from the centre ctr the
// content is mapped by F = R(phi) diag(a, 1 / a) R(-phi) R(theta) s and then shifted by t, so an output position reads
// p_src = ctr + F^-1 (p_out - ctr - t) and Theta: u -> k + F^-1 (u - k - 2 t) with k = 2 ctr + c.
constexpr int WARP_O = 5, WARP_MAX = 64;
constexpr float WARP_C = 0.09826089954573103f;
__constant__ float WARP_TAPS[12] = {0.015404109327027373f, 0.0034907120842174702f, -0.11799011114819057f,
                                    -0.048311742585633f,   0.4910559419267466f,    0.787641141030194f,
                                    0.3379294217276218f,   -0.07263752278646252f,  -0.021060292512300564f,
                                    0.04472490177066578f,  0.0017677118642428036f, -0.007800708325034148f};
// floats of LDS: taps[16] | S[H][W] | V[2H+10][2W+10] | T[2H+10][W]
__host__ __device__ constexpr int warp_lds_floats(int H, int W) {
  return 16 + H * W + (2 * H + 10) * (2 * W + 10) + (2 * H + 10) * W;
}

struct WarpDraw {
  bool any;
  float lab[7];
  float th[6];  // Theta row-major [2][3]
};

__device__ __forceinline__ float warp_uni(uint32_t w) { return ((float)(w >> 8) + 0.5f) * (1.0f / 16777216.0f); }

__device__ __forceinline__ WarpDraw warp_draw(uint32_t b, uint32_t epoch, unsigned long long seed, unsigned long long thr,
                                              int wops, int H, int W) {
  WarpDraw d = {false, {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, {1.f, 0.f, 0.f, 0.f, 1.f, 0.f}};
  if (thr == 0 || wops == 0) return d;
  const uint32_t s0 = (uint32_t)seed, s1 = (uint32_t)(seed >> 32);
  const Philox4 en = philox4x32_10(b, 32u, AUG_TAG, epoch, s0, s1);
  const bool e_s = (wops & 1) && (unsigned long long)en.x < thr, e_r = (wops & 2) && (unsigned long long)en.y < thr;
  const bool e_a = (wops & 4) && (unsigned long long)en.z < thr, e_t = (wops & 8) && (unsigned long long)en.w < thr;
  d.any = e_s || e_r || e_a || e_t;
  if (!d.any) return d;
  const Philox4 w0 = philox4x32_10(b, 33u, AUG_TAG, epoch, s0, s1), w1 = philox4x32_10(b, 34u, AUG_TAG, epoch, s0, s1);
  const float two_pi = 6.283185307179586f, pi = 3.141592653589793f;
  float n_s = 0.f, theta = 0.f, n_a = 0.f, phi = 0.f, n_x = 0.f, n_y = 0.f;
  if (e_s) n_s = sqrtf(-2.0f * logf(warp_uni(w0.x))) * cosf(two_pi * warp_uni(w0.y));
  if (e_r) theta = pi * (2.0f * warp_uni(w0.z) - 1.0f);
  if (e_a) {
    n_a = sqrtf(-2.0f * logf(warp_uni(w0.w))) * cosf(two_pi * warp_uni(w1.x));
    phi = pi * (2.0f * warp_uni(w1.y) - 1.0f);
  }
  if (e_t) {
    const float r = sqrtf(-2.0f * logf(warp_uni(w1.z))), ang = two_pi * warp_uni(w1.w);
    n_x = r * cosf(ang);
    n_y = r * sinf(ang);
  }
  const float ct = cosf(theta), st = sinf(theta), cp = cosf(phi), sp = sinf(phi);
  d.lab[0] = n_s;
  d.lab[1] = ct - 1.0f;
  d.lab[2] = st;
  d.lab[3] = n_a * cp;
  d.lab[4] = n_a * sp;
  d.lab[5] = n_x;
  d.lab[6] = n_y;
  // F^-1 = (1 / s) R(-theta) M,  M = R(phi) diag(1 / a, a) R(-phi) (symmetric)
  const float is = exp2f(-0.2f * n_s), a = exp2f(0.2f * n_a), ia = exp2f(-0.2f * n_a);
  const float m00 = ia * cp * cp + a * sp * sp, m01 = (ia - a) * cp * sp, m11 = ia * sp * sp + a * cp * cp;
  const float a00 = is * (ct * m00 + st * m01), a01 = is * (ct * m01 + st * m11);
  const float a10 = is * (ct * m01 - st * m00), a11 = is * (ct * m11 - st * m01);
  const float ky = (float)(H - 1) + WARP_C, kx = (float)(W - 1) + WARP_C;
  const float gy = ky + 2.0f * (0.125f * (float)H * n_y), gx = kx + 2.0f * (0.125f * (float)W * n_x);
  d.th[0] = a00;
  d.th[1] = a01;
  d.th[2] = ky - (a00 * gy + a01 * gx);
  d.th[3] = a10;
  d.th[4] = a11;
  d.th[5] = kx - (a10 * gy + a11 * gx);
  return d;
}

// S~ index: reflection without edge repeat, any int i, n >= 2 -> [0, n)
__device__ __forceinline__ int warp_reflect(int i, int n) {
  const int p = 2 * (n - 1);
  int m = i % p;
  m = m < 0 ? m + p : m;
  return m < n ? m : p - m;
}

// One workgroup per (channel, sample).  A sample with no continuous op enabled takes k_u8_gather_augment_normalize's path,
// bytes to floats (the branch is uniform over the workgroup); otherwise the plane goes to LDS as floats through the same
// inverse index chain, V is formed straight from it -- the bilinear point's four U values share their taps: per axis the
// weights (1 - f) h[u0 + o - 2 i] + f h[u0 + 1 + o - 2 i] over the <= 7 source rows i either U row touches -- and the down
// pass runs separably, rows then columns.  Every LDS index is reduced into range (warp_reflect), whatever q is.  No atomics:
// two launches give the same bits.  aug [B][13]; theta [B][6] (may be null) receives Theta (identity on the exact path).
__global__ __launch_bounds__(256) void k_u8_gather_warp_normalize(
    const unsigned char* __restrict__ data, const long* __restrict__ index, float* __restrict__ out, int C, int H, int W,
    long n_images, float mean, float stdv, int flip, unsigned long long seed, unsigned epoch, unsigned long long thr, int ops,
    int wops, float* __restrict__ aug, float* __restrict__ theta) {
  extern __shared__ __attribute__((aligned(16))) float wsm[];
  const int b = blockIdx.y, c = blockIdx.x;
  const long img = index[b];
  if (img < 0 || img >= n_images) return;  // host validates; never read out of bounds
  bool do_flip = false;
  if (flip) {
    const Philox4 r = philox4x32_10((uint32_t)b, 0u, 0x0da7u, epoch, (uint32_t)seed, (uint32_t)(seed >> 32));
    do_flip = (r.x & 1u) != 0u;
  }
  const AugDraw a = aug_draw((uint32_t)b, epoch, seed, thr, ops, H, W);
  const WarpDraw wd = warp_draw((uint32_t)b, epoch, seed, thr, wops, H, W);
  if (c == 0 && threadIdx.x == 0) {
    float* l = aug + (long)b * 13;
    l[0] = (float)a.xflip;
    l[1] = (float)a.yflip;
    l[2] = (float)a.sx / (float)W;
    l[3] = (float)a.sy / (float)H;
    l[4] = a.k == 0 ? 0.f : (a.k == 2 ? -2.f : -1.f);
    l[5] = a.k == 1 ? 1.f : (a.k == 3 ? -1.f : 0.f);
    for (int i = 0; i < 7; ++i) l[6 + i] = wd.lab[i];
    if (theta)
      for (int i = 0; i < 6; ++i) theta[(long)b * 6 + i] = wd.th[i];
  }
  const bool mirror = (a.xflip != 0) != do_flip;
  const int hw = H * W;
  const unsigned char* src = data + (img * C + c) * hw;
  float* dst = out + ((long)b * C + c) * hw;
  // the inverse index chain of k_u8_gather_augment_normalize: output pixel (h, w) of the exact ops -> its source byte
  auto source = [&](int h, int w) -> float {
    int i = h, j = w;
    if (a.k == 1) { i = w; j = W - 1 - h; }
    else if (a.k == 2) { i = H - 1 - h; j = W - 1 - w; }
    else if (a.k == 3) { i = W - 1 - w; j = h; }
    i -= a.sy;
    i = i < 0 ? -i : (i >= H ? 2 * (H - 1) - i : i);
    j -= a.sx;
    j = j < 0 ? -j : (j >= W ? 2 * (W - 1) - j : j);
    if (a.yflip) i = H - 1 - i;
    if (mirror) j = W - 1 - j;
    return (float)src[i * W + j];
  };
  if (!wd.any) {
    for (int e = threadIdx.x; e < hw; e += blockDim.x) {
      const float x = source(e / W, e % W) / 255.0f;  // the arithmetic of k_u8_gather_normalize
      dst[e] = (x - mean) / stdv;
    }
    return;
  }
  const int VH = 2 * H + 10, VW = 2 * W + 10;
  float* hp = wsm;           // hp[k + 2] = h[k], zero for k = -2, -1, 12, 13
  float* S = wsm + 16;       // [H][W]
  float* V = S + hw;         // [VH][VW], V[u + o][v + o]
  float* T = V + VH * VW;    // [VH][W]
  if (threadIdx.x < 16) hp[threadIdx.x] = threadIdx.x >= 2 && threadIdx.x < 14 ? WARP_TAPS[threadIdx.x - 2] : 0.f;
  for (int e = threadIdx.x; e < hw; e += blockDim.x) S[e] = source(e / W, e % W);
  __syncthreads();
  for (int p = threadIdx.x; p < VH * VW; p += blockDim.x) {
    const float u = (float)(p / VW - WARP_O), v = (float)(p % VW - WARP_O);
    const float qy = fmaf(wd.th[0], u, fmaf(wd.th[1], v, wd.th[2])), qx = fmaf(wd.th[3], u, fmaf(wd.th[4], v, wd.th[5]));
    const float y0 = floorf(qy), x0 = floorf(qx);
    const float fy = qy - y0, fx = qx - x0;
    const int u0 = (int)y0, v0 = (int)x0;
    const int i0 = (u0 - WARP_O) >> 1, j0 = (v0 - WARP_O) >> 1;     // floor: the first source row / column either U value reads
    const int ka = u0 + WARP_O - 2 * i0 + 2, kb = v0 + WARP_O - 2 * j0 + 2;   // 12 or 13: hp index of row i0's tap for u0
    float wy[7], wx[7];
    int ri[7], rj[7];
#pragma unroll
    for (int t = 0; t < 7; ++t) {
      wy[t] = fmaf(fy, hp[ka - 2 * t + 1] - hp[ka - 2 * t], hp[ka - 2 * t]);
      wx[t] = fmaf(fx, hp[kb - 2 * t + 1] - hp[kb - 2 * t], hp[kb - 2 * t]);
      ri[t] = warp_reflect(i0 + t, H) * W;
      rj[t] = warp_reflect(j0 + t, W);
    }
    float acc = 0.f;
#pragma unroll
    for (int t = 0; t < 7; ++t) {
      float row = 0.f;
#pragma unroll
      for (int s = 0; s < 7; ++s) row = fmaf(wx[s], S[ri[t] + rj[s]], row);
      acc = fmaf(wy[t], row, acc);
    }
    V[p] = 2.0f * acc;
  }
  __syncthreads();
  for (int p = threadIdx.x; p < VH * W; p += blockDim.x) {
    const int r = p / W, j = p % W;
    const float* vr = V + r * VW + 2 * j;
    float acc = 0.f;
#pragma unroll
    for (int k = 0; k < 12; ++k) acc = fmaf(vr[k], hp[k + 2], acc);
    T[p] = acc;
  }
  __syncthreads();
  for (int e = threadIdx.x; e < hw; e += blockDim.x) {
    const int i = e / W, j = e % W;
    float acc = 0.f;
#pragma unroll
    for (int k = 0; k < 12; ++k) acc = fmaf(T[(2 * i + k) * W + j], hp[k + 2], acc);
    const float x = (0.5f * acc) / 255.0f;  // the arithmetic of k_u8_gather_normalize, on a float instead of a byte
    dst[e] = (x - mean) / stdv;
  }
}

// x fp32 NCHW -> u8 NCHW: (x*scale + offset).clip(0,255) truncated
__global__ __launch_bounds__(256) void k_denormalize_u8(const float* __restrict__ x, unsigned char* __restrict__ out,
                                                          long n, float scale, float offset) {
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (long)gridDim.x * blockDim.x) {
    const float m = x[e] * scale;  // separately rounded multiply and add (contraction is off in this file)
    float v = m + offset;
    v = fminf(fmaxf(v, 0.0f), 255.0f);
    out[e] = (unsigned char)(int)v;
  }
}

// pred fp32 NCHW -> u8 NHWC: clamp(pred*std[c]*2 + mean[c], 0, 1)*255 truncated
__global__ __launch_bounds__(256) void k_prediction_to_u8_nhwc(const float* __restrict__ pred,
                                                                 unsigned char* __restrict__ out, int C, int HW, long n,
                                                                 const float* __restrict__ mean,
                                                                 const float* __restrict__ stdv) {
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (long)gridDim.x * blockDim.x) {
    const int c = (int)(e % C);
    const long p = e / C;  // b*HW + pixel
    const long b = p / HW, px = p - b * HW;
    const float v0 = pred[(b * C + c) * HW + px];
    const float m = v0 * stdv[c] * 2.0f;
    float v = m + mean[c];
    v = fminf(fmaxf(v, 0.0f), 1.0f);
    out[e] = (unsigned char)(int)(v * 255.0f);
  }
}

}  // namespace

extern "C" int edm_u8_gather_normalize(const void* data, const long* index, float* out, int B, int C, int H, int W,
                                       long n_images, float mean, float stdv, int flip, unsigned long long seed,
                                       unsigned epoch, hipStream_t st) {
  EDM_REQUIRE(data && index && out, "u8_gather_normalize: null pointer");
  EDM_REQUIRE(B > 0 && B <= 65535 && C > 0 && H > 0 && W > 0 && n_images > 0 && stdv != 0.0f,
              "u8_gather_normalize: bad args B=%d C=%d H=%d W=%d", B, C, H, W);
  const int chw = C * H * W;
  const int gx = (chw + 255) / 256 < 64 ? (chw + 255) / 256 : 64;
  hipLaunchKernelGGL(k_u8_gather_normalize, dim3(gx, B), dim3(256), 0, st, (const unsigned char*)data, index, out, C, H,
                     W, n_images, mean, stdv, flip, seed, epoch);
  EDM_CHECK_LAUNCH("u8_gather_normalize");
  return EDM_OK;
}

// The gather above with the non-leaking augmentation of EDM (Karras et al. 2022, App. F.2; exact subset: xflip, yflip,
// integer translation, rot90) composed into it: one launch writes the batch and its augment labels aug [B][6].
// aug_thr = round(p * 2^32) <= 2^32 (0: nothing is ever applied and `out` equals edm_u8_gather_normalize's);
// aug_ops: bit 0 xflip, 1 yflip, 2 translate, 3 rot90 (square images only: EDM_ERR_UNSUPPORTED otherwise).
// Word -> draw mapping: see aug_draw above.
extern "C" int edm_u8_gather_augment_normalize(const void* data, const long* index, float* out, int B, int C, int H, int W,
                                               long n_images, float mean, float stdv, int flip, unsigned long long seed,
                                               unsigned epoch, unsigned long long aug_thr, int aug_ops, float* aug,
                                               hipStream_t st) {
  EDM_REQUIRE(data && index && out && aug, "u8_gather_augment_normalize: null pointer");
  EDM_REQUIRE(B > 0 && B <= 65535 && C > 0 && H > 0 && W > 0 && n_images > 0 && stdv != 0.0f,
              "u8_gather_augment_normalize: bad args B=%d C=%d H=%d W=%d", B, C, H, W);
  EDM_REQUIRE(aug_thr <= (1ull << 32) && aug_ops >= 0 && aug_ops < 16,
              "u8_gather_augment_normalize: bad threshold / op mask %d", aug_ops);
  if ((aug_ops & 8) && H != W) {
    edm_set_error("u8_gather_augment_normalize: rot90 needs square images, got %d x %d", H, W);
    return EDM_ERR_UNSUPPORTED;
  }
  const int chw = C * H * W;
  const int gx = (chw + 255) / 256 < 64 ? (chw + 255) / 256 : 64;
  hipLaunchKernelGGL(k_u8_gather_augment_normalize, dim3(gx, B), dim3(256), 0, st, (const unsigned char*)data, index, out,
                     C, H, W, n_images, mean, stdv, flip, seed, epoch, aug_thr, aug_ops, aug);
  EDM_CHECK_LAUNCH("u8_gather_augment_normalize");
  return EDM_OK;
}

// edm_u8_gather_augment_normalize followed by the continuous ops of the EDM pipe (zoom, rotate, stretch, shift; the
// definition, the draws and the labels are written down at k_u8_gather_warp_normalize above).  warp_ops: bit 0 zoom, 1 rotate,
// 2 stretch, 3 shift, each enabled per sample iff its Philox word < aug_thr.  aug [B][13]: the six labels of the exact ops,
// then seven of the continuous ones.  theta [B][6] (may be null) receives each sample's 2x3 matrix on the 2x grid.  A sample
// with no continuous op enabled is edm_u8_gather_augment_normalize's, bit for bit.  2 <= H, W <= 64, else status -3 before
// any launch.
extern "C" int edm_u8_gather_augment_warp_normalize(const void* data, const long* index, float* out, int B, int C, int H,
                                                    int W, long n_images, float mean, float stdv, int flip,
                                                    unsigned long long seed, unsigned epoch, unsigned long long aug_thr,
                                                    int aug_ops, int warp_ops, float* aug, float* theta, hipStream_t st) {
  EDM_REQUIRE(data && index && out && aug, "u8_gather_augment_warp_normalize: null pointer");
  EDM_REQUIRE(B > 0 && B <= 65535 && C > 0 && C <= 65535 && H > 0 && W > 0 && n_images > 0 && stdv != 0.0f,
              "u8_gather_augment_warp_normalize: bad args B=%d C=%d H=%d W=%d", B, C, H, W);
  EDM_REQUIRE(aug_thr <= (1ull << 32) && aug_ops >= 0 && aug_ops < 16 && warp_ops >= 0 && warp_ops < 16,
              "u8_gather_augment_warp_normalize: bad threshold / op masks %d, %d", aug_ops, warp_ops);
  if (H < 2 || W < 2 || H > WARP_MAX || W > WARP_MAX) {
    edm_set_error("u8_gather_augment_warp_normalize: images of 2 .. %d pixels a side only, got %d x %d", WARP_MAX, H, W);
    return EDM_ERR_UNSUPPORTED;
  }
  if ((aug_ops & 8) && H != W) {
    edm_set_error("u8_gather_augment_warp_normalize: rot90 needs square images, got %d x %d", H, W);
    return EDM_ERR_UNSUPPORTED;
  }
  EDM_MAX_LDS(k_u8_gather_warp_normalize, warp_lds_floats(WARP_MAX, WARP_MAX) * (int)sizeof(float));
  const size_t lds = (size_t)warp_lds_floats(H, W) * sizeof(float);
  hipLaunchKernelGGL(k_u8_gather_warp_normalize, dim3(C, B), dim3(256), lds, st, (const unsigned char*)data, index, out, C,
                     H, W, n_images, mean, stdv, flip, seed, epoch, aug_thr, aug_ops, warp_ops, aug, theta);
  EDM_CHECK_LAUNCH("u8_gather_augment_warp_normalize");
  return EDM_OK;
}

extern "C" int edm_denormalize_u8(const float* x, void* out, long n, float scale, float offset, hipStream_t st) {
  EDM_REQUIRE(x && out && n > 0, "denormalize_u8: bad args");
  const long blocks = (n + 255) / 256;
  hipLaunchKernelGGL(k_denormalize_u8, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, st, x,
                     (unsigned char*)out, n, scale, offset);
  EDM_CHECK_LAUNCH("denormalize_u8");
  return EDM_OK;
}

extern "C" int edm_prediction_to_u8_nhwc(const float* pred, void* out, int B, int C, int H, int W, const float* mean,
                                         const float* stdv, hipStream_t st) {
  EDM_REQUIRE(pred && out && mean && stdv && B > 0 && C > 0 && H > 0 && W > 0, "prediction_to_u8_nhwc: bad args");
  const long n = (long)B * C * H * W;
  const long blocks = (n + 255) / 256;
  hipLaunchKernelGGL(k_prediction_to_u8_nhwc, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, st, pred,
                     (unsigned char*)out, C, H * W, n, mean, stdv);
  EDM_CHECK_LAUNCH("prediction_to_u8_nhwc");
  return EDM_OK;
}
