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
constexpr uint32_t AUG_TAG = 0x41554731u;  // "AUG1": differs from 0x0da7 above and from the tags of optim.hip / linear.hip
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
