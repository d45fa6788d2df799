// fp32 side path: the weight-normalised Linear layers (networks.py:58-60) and the noise / class
// embedding (networks.py:121-178).  The reference keeps these in fp32 under autocast
// (networks.py:164, 255, 319); they are tiny ((B,64..1000)->(B,256..768)): one LDS-tiled fp32 GEMM on the
// f32-input matrix instruction, with arbitrary operand strides, covers forward, dgrad and wgrad.
#include "common.h"

// Launch plan of the GEMM C[M,N] (=|+=) A[M,K] B[K,N] behind the three Linear entry points (edm_linear_fwd (M,N,K) runs
// the GEMM (M,N,K), edm_linear_dgrad (M,N,K) runs (M,K,N), edm_linear_wgrad (M,N,K) runs (N,K,M)): tile_rows = 64 for the
// 64x64 tile (four waves) when that still gives every CU a workgroup, 32 for the 32x64 tile (two waves) of the small
// problems; splits = K shares over gridDim.z, added with atomics (long K, few tiles: split to fill the chip).  accumulate
// does not change the plan; with splits > 1 and accumulate == 0 the launch clears C first.  sgemm() launches what this says.
extern "C" int edm_linear_plan(int M, int N, int K, int accumulate, int* tile_rows, int* splits) {
  EDM_REQUIRE(M > 0 && N > 0 && K > 0 && tile_rows && splits, "linear_plan: bad args");
  (void)accumulate;
  const long t64 = (long)((N + 63) / 64) * ((M + 63) / 64);
  const bool big = t64 >= 256;
  const long tiles = big ? t64 : (long)((N + 63) / 64) * ((M + 31) / 32);
  int sp_out = 1;
  if (K >= 1024 && tiles < 512) {
    long sp = K / 256, cap = (1024 + tiles - 1) / tiles;
    if (sp > cap) sp = cap;
    if (sp > 32) sp = 32;
    sp_out = (int)(sp < 1 ? 1 : sp);
  }
  *tile_rows = big ? 64 : 32;
  *splits = sp_out;
  return EDM_OK;
}

namespace {

// C[m,n] (=|+=) alpha * sum_k A[m*asm + k*ask] * B[k*bsk + n*bsn]
// Round 6: the same GEMM on the f32-input matrix instruction (v_mfma_f32_32x32x2_f32: every product and sum a plain fp32
// operation, as in csrc/eval_f32.hip).  k_sgemm_smallk staged the whole K extent of BOTH operands per 32x32 tile -- the
// batched embed Linear of a sampler evaluation (512 x 256 -> 5 376: networks._EmbedAllFn) re-read 176 MB through L2 and took
// 121 us; this kernel gives a wave a 32x32 output block, a workgroup WM x WN of them, and walks K in chunks of 32 through LDS
// (operands of any stride: forward, dgrad and wgrad of the Linears share it).  Split-K over gridDim.z, partial sums by atomics.
template <int WM, int WN>
__global__ __launch_bounds__(64 * WM * WN) void k_sgemm_mfma(const float* __restrict__ A, long asm_, long ask,
                                                               const float* __restrict__ Bm, long bsk, long bsn,
                                                               float* __restrict__ C, long csm, long csn, int M, int N, int K,
                                                               float alpha, int accumulate) {
  constexpr int TM = 32 * WM, TN = 32 * WN, TK = 32, NT = 64 * WM * WN;
  constexpr int LDA = TM + 1, LDB = TN + 1;        // odd row pitch: the k-contiguous staging writes hit distinct banks
  constexpr int NA_ = TM * TK / NT, NB_ = TN * TK / NT;   // elements of a chunk per thread (compile-time: 8 / 8 or 8 / 16)
  __shared__ float As[TK * LDA];
  __shared__ float Bs[TK * LDB];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave / WN, wn = wave % WN;
  const int l31 = lane & 31, lhi = lane >> 5;
  const int m0 = blockIdx.y * TM, n0 = blockIdx.x * TN;
  const int kper = ((K + gridDim.z - 1) / gridDim.z + TK - 1) / TK * TK;
  const int kbeg = blockIdx.z * kper;
  const int kend = min(K, kbeg + kper);
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  // A chunk's elements go global -> registers -> LDS, ALL loads of a chunk issued before the first is stored (the first form
  // of this kernel stored each element behind its own load: 24 serial round trips per chunk, 51 us per call whatever the
  // problem size), and the NEXT chunk's loads are in flight while this chunk is multiplied.
  float ra[NA_], rb[NB_];
  auto load_chunk = [&](int k0) {
#pragma unroll
    for (int i = 0; i < NA_; ++i) {
      const int e = tid + i * NT;
      const int kk = ask == 1 ? (e & 31) : e / TM, mm = ask == 1 ? (e >> 5) : e % TM;
      const int m = m0 + mm, k = k0 + kk;
      ra[i] = (m < M && k < kend) ? A[m * asm_ + k * ask] : 0.f;
    }
#pragma unroll
    for (int i = 0; i < NB_; ++i) {
      const int e = tid + i * NT;
      const int kk = bsk == 1 ? (e & 31) : e / TN, nn = bsk == 1 ? (e >> 5) : e % TN;
      const int n = n0 + nn, k = k0 + kk;
      rb[i] = (n < N && k < kend) ? Bm[k * bsk + n * bsn] : 0.f;
    }
  };
  auto store_chunk = [&]() {
#pragma unroll
    for (int i = 0; i < NA_; ++i) {
      const int e = tid + i * NT;
      const int kk = ask == 1 ? (e & 31) : e / TM, mm = ask == 1 ? (e >> 5) : e % TM;
      As[kk * LDA + mm] = ra[i];
    }
#pragma unroll
    for (int i = 0; i < NB_; ++i) {
      const int e = tid + i * NT;
      const int kk = bsk == 1 ? (e & 31) : e / TN, nn = bsk == 1 ? (e >> 5) : e % TN;
      Bs[kk * LDB + nn] = rb[i];
    }
  };
  if (kbeg < kend) load_chunk(kbeg);
  for (int k0 = kbeg; k0 < kend; k0 += TK) {
    store_chunk();
    __syncthreads();
    if (k0 + TK < kend) load_chunk(k0 + TK);
#pragma unroll
    for (int kk = 0; kk < TK; kk += 2) {
      const float a = As[(kk + lhi) * LDA + wm * 32 + l31];
      const float b = Bs[(kk + lhi) * LDB + wn * 32 + l31];
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc, 0, 0, 0);
    }
    __syncthreads();
  }
  // accumulator register r of a lane: row (of A) 8 (r / 4) + 4 lhi + (r % 4), column (of B) l31
  const int n = n0 + wn * 32 + l31;
  if (n >= N) return;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int m = m0 + wm * 32 + 8 * (r >> 2) + 4 * lhi + (r & 3);
    if (m < M) {
      float* c = C + m * csm + n * csn;
      if (gridDim.z > 1) atomicAdd(c, alpha * acc[r]);
      else *c = accumulate ? *c + alpha * acc[r] : alpha * acc[r];
    }
  }
}

int sgemm(const float* A, long asm_, long ask, const float* B, long bsk, long bsn, float* C, long csm, long csn, int M,
          int N, int K, float alpha, int accumulate, hipStream_t st) {
  int rows = 32, splits = 1;
  edm_linear_plan(M, N, K, accumulate, &rows, &splits);
  if (csn != 1 || csm != N) splits = 1;     // split-K clears and adds into C as one dense block (every export's C is)
  if (splits > 1 && !accumulate) (void)hipMemsetAsync(C, 0, (size_t)M * N * sizeof(float), st);
  if (rows == 64)
    hipLaunchKernelGGL((k_sgemm_mfma<2, 2>), dim3((N + 63) / 64, (M + 63) / 64, splits), dim3(256), 0, st, A, asm_, ask, B,
                       bsk, bsn, C, csm, csn, M, N, K, alpha, accumulate);
  else
    hipLaunchKernelGGL((k_sgemm_mfma<1, 2>), dim3((N + 63) / 64, (M + 31) / 32, splits), dim3(128), 0, st, A, asm_, ask, B,
                       bsk, bsn, C, csm, csn, M, N, K, alpha, accumulate);
  return 0;
}

// fourier[b,j] = cos(ln(sigma_b)/4 * freqs[j] + phases[j]) * sqrt(2)      (networks.py:138-141,165)
__global__ void k_fourier(const float* __restrict__ sigma, int sstride, const float* __restrict__ freqs,
                          const float* __restrict__ phases, float* __restrict__ out, int B, int Fd) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B * Fd) return;
  const int b = i / Fd, j = i % Fd;
  const float c = logf(sigma[b * sstride]) * 0.25f;
  out[i] = cosf(c * freqs[j] + phases[j]) * 1.41421356237309515f;
}

// pre = labels ? mp_add(emb_sigma, Wcls_hat[:,label]*sqrt(K), t) : emb_sigma ; out = mp_silu(pre)   (networks.py:169-177)
//
// Label dropout (classifier-free guidance training): a dropped sample b takes the labels == nullptr path for its row
// (pre = emb_sigma, no mp_add).  The mask comes from drop_in (given by the caller) or, when drop_in is null and drop_out
// is set, from Philox: r = philox4x32_10((b, 0x4C41424C, 0, step), (seed_lo, seed_hi)), dropped iff r.x < thr
// (thr = round(p * 2^32) in [0, 2^32]; dyn overrides step / seed as in k_mod_silu_drop_fwd).  Every element of row b
// makes the same call: no LDS round trip or barrier, and a row's lanes are one wave whenever E % 64 == 0.  The element
// e == 0 of each row writes the mask it used to drop_out, which the backward reads.  drop_in == drop_out == nullptr is
// the plain path.
__global__ void k_embed_combine_fwd(const float* __restrict__ es, const float* __restrict__ wcls,
                                    const long long* __restrict__ labels, float t, int K, float* __restrict__ pre,
                                    float* __restrict__ out, int B, int E, unsigned long long thr, uint32_t seed_lo,
                                    uint32_t seed_hi, uint32_t step, const StepParams* __restrict__ dyn,
                                    const int* __restrict__ drop_in, int* __restrict__ drop_out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B * E) return;
  const int b = i / E, e = i % E;
  float v = es[i];
  if (labels) {
    bool dropped = false;
    if (drop_in) {
      dropped = drop_in[b] != 0;
    } else if (drop_out) {
      if (dyn) { step = dyn->step; seed_lo = dyn->seed_lo; seed_hi = dyn->seed_hi; }
      const Philox4 r = philox4x32_10((uint32_t)b, 0x4C41424Cu, 0u, step, seed_lo, seed_hi);
      dropped = (unsigned long long)r.x < thr;
    }
    if (drop_out && e == 0) drop_out[b] = dropped ? 1 : 0;
    if (!dropped) {
      const float c = rsqrtf((1.f - t) * (1.f - t) + t * t);
      const long long lab = labels[b];
      const float cls = (lab >= 0 && lab < K) ? wcls[(long)e * K + lab] * sqrtf((float)K) : 0.f;
      v = ((1.f - t) * v + t * cls) * c;
    }
  }
  pre[i] = v;
  out[i] = mp_silu_f(v);
}
// drop (nullable): the forward's mask output; a dropped row passes gout * mp_silu'(pre) to ges and adds nothing to gwcls
__global__ void k_embed_combine_bwd(const float* __restrict__ gout, const float* __restrict__ pre,
                                    const long long* __restrict__ labels, float t, int K, float* __restrict__ ges,
                                    float* __restrict__ gwcls, int B, int E, const int* __restrict__ drop) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B * E) return;
  const int b = i / E, e = i % E;
  float g = gout[i] * mp_silu_grad_f(pre[i]);
  if (labels && !(drop && drop[b])) {
    const float c = rsqrtf((1.f - t) * (1.f - t) + t * t);
    const long long lab = labels[b];
    if (lab >= 0 && lab < K) atomicAdd(gwcls + (long)e * K + lab, g * t * c * sqrtf((float)K));
    g *= (1.f - t) * c;
  }
  ges[i] = g;
}

// Augment-label conditioning (EDM, Karras et al. 2022, App. F.2): es[b][e] += sum_k a[b][k] * w[e][k], in place on the
// output of the sigma Linear, k ascending -- an all-zero label row leaves es as it is.  K is the handful of augment labels
// (6): one thread per output element, no GEMM.
__global__ void k_aug_embed_fwd(float* __restrict__ es, const float* __restrict__ a, const float* __restrict__ w, int B,
                                int E, int K) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B * E) return;
  const int b = i / E, e = i % E;
  float acc = 0.f;
  for (int k = 0; k < K; ++k) acc += a[b * K + k] * w[(long)e * K + k];
  es[i] += acc;
}
// gw[e][k] = sum_b ges[b][e] * a[b][k]: one thread per weight element, b ascending -- a fixed order (no atomics), so an
// eager and a replayed step give the same bits
__global__ void k_aug_embed_wgrad(const float* __restrict__ ges, const float* __restrict__ a, float* __restrict__ gw,
                                  int B, int E, int K) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= E * K) return;
  const int e = i / K, k = i % K;
  float acc = 0.f;
  for (int b = 0; b < B; ++b) acc += ges[(long)b * E + e] * a[b * K + k];
  gw[i] = acc;
}

}  // namespace

// Y[M,N] = X[M,K] W[N,K]^T   (weight-normalised Linear with the effective fp32 weight)
extern "C" int edm_linear_fwd(const float* X, const float* W, float* Y, int M, int N, int K, hipStream_t st) {
  EDM_REQUIRE(X && W && Y && M > 0 && N > 0 && K > 0, "linear_fwd: bad args");
  sgemm(X, K, 1, W, 1, K, Y, N, 1, M, N, K, 1.f, 0, st);
  EDM_CHECK_LAUNCH("linear_fwd");
  return EDM_OK;
}
// dX[M,K] = dY[M,N] W[N,K]
extern "C" int edm_linear_dgrad(const float* dY, const float* W, float* dX, int M, int N, int K, int accumulate,
                                hipStream_t st) {
  EDM_REQUIRE(dY && W && dX && M > 0 && N > 0 && K > 0, "linear_dgrad: bad args");
  sgemm(dY, N, 1, W, K, 1, dX, K, 1, M, K, N, 1.f, accumulate, st);
  EDM_CHECK_LAUNCH("linear_dgrad");
  return EDM_OK;
}
// dW[N,K] = dY[M,N]^T X[M,K]
extern "C" int edm_linear_wgrad(const float* dY, const float* X, float* dW, int M, int N, int K, int accumulate,
                                hipStream_t st) {
  EDM_REQUIRE(dY && X && dW && M > 0 && N > 0 && K > 0, "linear_wgrad: bad args");
  sgemm(dY, 1, N, X, K, 1, dW, K, 1, N, K, M, 1.f, accumulate, st);
  EDM_CHECK_LAUNCH("linear_wgrad");
  return EDM_OK;
}

extern "C" int edm_fourier_fwd(const float* sigma, int sigma_stride, const float* freqs, const float* phases,
                               float* out, int B, int Fd, hipStream_t st) {
  EDM_REQUIRE(sigma && freqs && phases && out && B > 0 && Fd > 0 && (sigma_stride == 0 || sigma_stride == 1),
              "fourier_fwd: bad args");
  hipLaunchKernelGGL(k_fourier, dim3((B * Fd + 255) / 256), dim3(256), 0, st, sigma, sigma_stride, freqs, phases, out,
                     B, Fd);
  EDM_CHECK_LAUNCH("fourier_fwd");
  return EDM_OK;
}
// Label dropout: drop_in (B int32, nullable) gives the mask; otherwise, with drop_out set, the kernel draws it with
// threshold drop_thr (<= 2^32) from (seed, step) or from dyn.  drop_out (B int32, nullable) receives the mask used.
extern "C" int edm_embed_combine_fwd(const float* emb_sigma, const float* wcls_hat, const long long* labels,
                                     float add_factor, int K, float* pre, float* out, int B, int E,
                                     unsigned long long drop_thr, unsigned long long seed, unsigned step, const void* dyn,
                                     const int* drop_in, int* drop_out, hipStream_t st) {
  EDM_REQUIRE(emb_sigma && pre && out && B > 0 && E > 0 && (!labels || (wcls_hat && K > 0)) &&
              drop_thr <= (1ull << 32) && (labels || (!drop_in && !drop_out)), "embed_combine_fwd: bad args");
  hipLaunchKernelGGL(k_embed_combine_fwd, dim3((B * E + 255) / 256), dim3(256), 0, st, emb_sigma, wcls_hat, labels,
                     add_factor, K, pre, out, B, E, drop_thr, (uint32_t)seed, (uint32_t)(seed >> 32), step,
                     (const StepParams*)dyn, drop_in, drop_out);
  EDM_CHECK_LAUNCH("embed_combine_fwd");
  return EDM_OK;
}
// gwcls_hat [E,K] is accumulated (+=): caller zero-fills.  drop (nullable): the mask edm_embed_combine_fwd wrote.
extern "C" int edm_embed_combine_bwd(const float* gout, const float* pre, const long long* labels, float add_factor,
                                     int K, float* gemb_sigma, float* gwcls_hat, int B, int E, const int* drop,
                                     hipStream_t st) {
  EDM_REQUIRE(gout && pre && gemb_sigma && B > 0 && E > 0 && (!labels || (gwcls_hat && K > 0)) && (labels || !drop),
              "embed_combine_bwd: bad args");
  hipLaunchKernelGGL(k_embed_combine_bwd, dim3((B * E + 255) / 256), dim3(256), 0, st, gout, pre, labels, add_factor, K,
                     gemb_sigma, gwcls_hat, B, E, drop);
  EDM_CHECK_LAUNCH("embed_combine_bwd");
  return EDM_OK;
}

// Augment labels a [B][K] through the effective weight w_hat [E][K] of Embedding.aug_embed, added in place to emb_sigma
// [B][E] (the output of edm_linear_fwd) before edm_embed_combine_fwd; and the weight gradient of that product.
extern "C" int edm_aug_embed_fwd(float* emb_sigma, const float* aug, const float* w_hat, int B, int E, int K,
                                 hipStream_t st) {
  EDM_REQUIRE(emb_sigma && aug && w_hat && B > 0 && E > 0 && K > 0 && (long)B * E <= 0x7fffffffL, "aug_embed_fwd: bad args");
  hipLaunchKernelGGL(k_aug_embed_fwd, dim3((B * E + 255) / 256), dim3(256), 0, st, emb_sigma, aug, w_hat, B, E, K);
  EDM_CHECK_LAUNCH("aug_embed_fwd");
  return EDM_OK;
}
// gw_hat [E][K] is overwritten
extern "C" int edm_aug_embed_wgrad(const float* gemb_sigma, const float* aug, float* gw_hat, int B, int E, int K,
                                   hipStream_t st) {
  EDM_REQUIRE(gemb_sigma && aug && gw_hat && B > 0 && E > 0 && K > 0 && (long)E * K <= 0x7fffffffL,
              "aug_embed_wgrad: bad args");
  hipLaunchKernelGGL(k_aug_embed_wgrad, dim3((E * K + 255) / 256), dim3(256), 0, st, gemb_sigma, aug, gw_hat, B, E, K);
  EDM_CHECK_LAUNCH("aug_embed_wgrad");
  return EDM_OK;
}
