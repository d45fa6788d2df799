// Guarded optimizer step: the norm of the whole gradient, the clip coefficient and the decision to skip a step are taken ON
// THE DEVICE, between the last weight-gradient kernel and the optimizer pass, so that a hipGraph-replayed step gets them
// without a host read (torch.nn.utils.clip_grad_norm_ / clip_grad_value_, Lightning's gradient_clip_val).
//   edm_grad_guard              one read of the gradient arena -> per-tensor sums of squares + the 64-byte GuardRecord
//   edm_adam_ema_guarded        k_adam_ema's update with grad_scale * record->coef, or nothing at all when record->skip
//   edm_adam_ema_phema_guarded  the same with the post-hoc EMA profiles
// Every sum is fp64 and runs in a fixed order (quads of a lane, butterfly of a wave = one 1024-element block, blocks of a
// tensor, tensors of the arena): no floating-point atomics, bit-identical from run to run, whatever the grid or chunk length.
#include "common.h"
#include "quads.h"
#include <math.h>
#include <cmath>

namespace {

// chunks[c] = (tensor id, first element, length): no chunk straddles two tensors, none covers the padding between them.
// A chunk is the work of one workgroup and nothing else: the sums are taken over BLOCKS of GUARD_BLOCK elements counted
// from the first element of each tensor, one wave per block, so the result does not depend on the chunk length either.
constexpr int GUARD_BLOCK = 1024;       // = ops.GUARD_BLOCK: 64 lanes x 4 quads
struct GuardChunk {
  long tensor, first, len;
};
// tensors[p] = (first chunk, number of chunks, first block, number of blocks): the chunks of a tensor are consecutive in
// the table and in memory, every chunk but the last a multiple of GUARD_BLOCK long
struct GuardTensor {
  int first_chunk, n_chunks, first_block, n_blocks;
};

__device__ __forceinline__ bool guard_bad(float g, float gs) {     // NaN, or beyond 3e38 before or after the scale
  return nonfinite(g) || nonfinite(g * gs);
}

// launch 1: workgroup c takes chunk c, its four waves the blocks of the chunk in turn.  part[b] = sum (g * grad_scale)^2 of
// block b, bad[b] = a non-finite element was seen.  Within a block: the elements up to the first 16-byte boundary OF THE
// ADDRESS and behind the last one singly, the quads between as dwordx4 (as k_adam_ema_ranges): lane l adds quads l, l + 64,
// ..., then its single, then the butterfly.  A chunk that does not fit its tensor's blocks or [0, n) is skipped whole.
__global__ __launch_bounds__(256) void k_grad_guard_chunks(const float* __restrict__ grad, long n,
                                                           const GuardChunk* __restrict__ chunks, int n_chunks,
                                                           const GuardTensor* __restrict__ tensors, int n_tensors,
                                                           int n_blocks, float grad_scale,
                                                           const StepParams* __restrict__ dyn, double* __restrict__ part,
                                                           unsigned* __restrict__ bad_out) {
  const float gs = dyn ? dyn->grad_scale : grad_scale;
  const double gsd = (double)gs;
  const GuardChunk c = chunks[blockIdx.x];
  if (c.tensor < 0 || c.tensor >= n_tensors || c.first < 0 || c.len <= 0 || c.len > n || c.first > n - c.len) return;
  const GuardTensor T = tensors[c.tensor];
  if (T.first_chunk < 0 || T.first_chunk >= n_chunks || T.first_block < 0 || T.n_blocks <= 0 ||
      T.n_blocks > n_blocks || T.first_block > n_blocks - T.n_blocks)
    return;
  const long rel = c.first - chunks[T.first_chunk].first;     // offset inside the tensor
  const long nb = (c.len + GUARD_BLOCK - 1) / GUARD_BLOCK;
  if (rel < 0 || rel % GUARD_BLOCK != 0 || rel / GUARD_BLOCK + nb > T.n_blocks) return;
  const long b0 = T.first_block + rel / GUARD_BLOCK;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (long b = wave; b < nb; b += 4) {
    const float* __restrict__ p = grad + c.first + b * GUARD_BLOCK;
    const long left = c.len - b * GUARD_BLOCK;
    const int len = (int)(left < GUARD_BLOCK ? left : GUARD_BLOCK);
    const int mis = (int)((16 - ((uintptr_t)p & 15)) & 15) >> 2;
    const int head = mis < len ? mis : len;
    const int nq = (len - head) >> 2;
    const int tail0 = head + 4 * nq;
    double acc = 0.0;
    bool bad = false;
    for (int q = lane; q < nq; q += 64) {
      const f32x4 g = *reinterpret_cast<const f32x4*>(p + head + 4 * q);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const double v = (double)g[j] * gsd;
        acc = fma(v, v, acc);
        bad |= guard_bad(g[j], gs);
      }
    }
    // at most 3 singles in front and 3 behind: one lane each, counted from the far end of the wave
    const int k = 63 - lane;
    int e = -1;
    if (k < head) e = k;
    else if (k - head < len - tail0) e = tail0 + (k - head);
    if (e >= 0) {
      const float g = p[e];
      const double v = (double)g * gsd;
      acc = fma(v, v, acc);
      bad |= guard_bad(g, gs);
    }
    acc = wave_sum_f64(acc);
    const bool wbad = __any(bad);
    if (lane == 0) {
      part[b0 + b] = acc;
      bad_out[b0 + b] = wbad ? 1u : 0u;
    }
  }
}

// launch 2: one wave per tensor.  Lane l adds the block partials l, l + 64, ... in that order, then the butterfly.
__global__ __launch_bounds__(256) void k_grad_guard_tensors(const double* __restrict__ part,
                                                            const unsigned* __restrict__ bad_in,
                                                            const GuardTensor* __restrict__ tensors, int n_tensors,
                                                            int n_blocks, double* __restrict__ sumsq,
                                                            unsigned* __restrict__ tbad) {
  const int t = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  double acc = 0.0;
  bool bad = false;
  if (t < n_tensors) {
    const GuardTensor g = tensors[t];
    if (g.first_block >= 0 && g.n_blocks > 0 && g.n_blocks <= n_blocks && g.first_block <= n_blocks - g.n_blocks) {
      for (int b = lane; b < g.n_blocks; b += 64) {
        acc += part[g.first_block + b];
        bad |= bad_in[g.first_block + b] != 0u;
      }
    }
  }
  acc = wave_sum_f64(acc);
  const bool wbad = __any(bad);
  if (t < n_tensors && lane == 0) {
    sumsq[t] = acc;
    tbad[t] = wbad ? 1u : 0u;
  }
}

// launch 3: one wave adds the tensors (lane l: l, l + 64, ...; then the butterfly) and one thread writes the record.
__global__ __launch_bounds__(64) void k_grad_guard_finish(const double* __restrict__ sumsq, const unsigned* __restrict__ tbad,
                                                          int n_tensors, float max_norm, float clip_value,
                                                          int skip_nonfinite, int count, GuardRecord* __restrict__ rec) {
  double acc = 0.0;
  bool bad = false;
  for (int t = threadIdx.x; t < n_tensors; t += 64) {
    acc += sumsq[t];
    bad |= tbad[t] != 0u;
  }
  acc = wave_sum_f64(acc);
  const bool any_bad = __any(bad);
  if (threadIdx.x == 0) {
    const double norm = sqrt(acc);
    double coef = 1.0;
    if (max_norm <= 3.0e38f) {              // (inf: off, and coef stays exactly 1 whatever the norm)
      const double c = (double)max_norm / (norm + 1e-6);
      coef = c >= 1.0 ? 1.0 : c;            // a NaN norm gives a NaN coef: without skip_nonfinite it goes through as today
    }
    const unsigned skip = (skip_nonfinite && any_bad) ? 1u : 0u;
    rec->coef = (float)coef;
    rec->skip = skip;
    rec->norm = (float)norm;
    rec->clip_value = clip_value;
    rec->sumsq = acc;
    if (count) {
      rec->steps = rec->steps + 1;
      if (skip) {
        rec->skipped = rec->skipped + 1;
        rec->consecutive_skips = rec->consecutive_skips + 1;
      } else {
        rec->consecutive_skips = 0;
        if (coef < 1.0) rec->clipped = rec->clipped + 1;
      }
    }
  }
}

struct GuardProfiles {
  float* p[4];
};
// k_adam_ema / k_adam_ema_phema (K > 0) behind the guard: gradient scale grad_scale * rec->coef, each scaled element limited
// to +-rec->clip_value, and NOTHING but the clearing of the gradient arena when rec->skip is set (the health word included).
// The update is the shared adam_ema_update (common.h), as in k_adam_ema_ranges.
template <int K>
__global__ __launch_bounds__(256) void k_adam_ema_guarded(float* __restrict__ theta, float* __restrict__ grad,
                                                          float* __restrict__ m, float* __restrict__ v,
                                                          float* __restrict__ ema, GuardProfiles prof,
                                                          const float* __restrict__ betas, long n4, long n, AdamArgs a,
                                                          const StepParams* __restrict__ dyn, int zero_grad,
                                                          const GuardRecord* __restrict__ rec,
                                                          unsigned* __restrict__ health) {
  constexpr int KK = K > 0 ? K : 1;
  if (dyn) adam_args_from(a, dyn);
  const bool skip = rec->skip != 0u;
  const float cv = rec->clip_value;
  const bool clip = cv <= 3.0e38f;
  const float raw_scale = a.grad_scale * rec->coef;
  AdamArgs u = a;                 // what adam_ema_update multiplies the gradient by: the scale, or 1 on a clipped value
  u.grad_scale = clip ? 1.0f : raw_scale;
  float pb[KK];
#pragma unroll
  for (int k = 0; k < K; ++k) pb[k] = betas[k];
  const float step_size = a.lr / a.bc1;
  bool bad = false;
  auto scaled = [&](float g) {
    if (!clip) return g;
    const float s = g * raw_scale;
    bad |= nonfinite(s);                              // (a clipped infinity is finite: the health bit still reports it)
    return s > cv ? cv : (s < -cv ? -cv : s);         // NaN passes through
  };
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
    if (i * 4 + 3 < n) {
      if (skip) {
        if (zero_grad) *reinterpret_cast<f32x4*>(grad + i * 4) = f32x4{0.f, 0.f, 0.f, 0.f};
        continue;
      }
      f32x4 t = *reinterpret_cast<f32x4*>(theta + i * 4);
      f32x4 g = *reinterpret_cast<const f32x4*>(grad + i * 4);
      if (zero_grad) *reinterpret_cast<f32x4*>(grad + i * 4) = f32x4{0.f, 0.f, 0.f, 0.f};
      f32x4 mm = *reinterpret_cast<f32x4*>(m + i * 4);
      f32x4 vv = *reinterpret_cast<f32x4*>(v + i * 4);
      f32x4 ee = {0.f, 0.f, 0.f, 0.f};
      if (ema) ee = *reinterpret_cast<f32x4*>(ema + i * 4);
      f32x4 pp[KK];
#pragma unroll
      for (int k = 0; k < K; ++k) pp[k] = *reinterpret_cast<f32x4*>(prof.p[k] + i * 4);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float tj = t[j], mj = mm[j], vj = vv[j], ej = ee[j];
        bad |= adam_ema_update(tj, scaled(g[j]), mj, vj, ej, ema != nullptr, u, step_size);
        t[j] = tj; mm[j] = mj; vv[j] = vj; ee[j] = ej;
#pragma unroll
        for (int k = 0; k < K; ++k) pp[k][j] = pb[k] * pp[k][j] + (1.f - pb[k]) * tj;
      }
      *reinterpret_cast<f32x4*>(theta + i * 4) = t;
      *reinterpret_cast<f32x4*>(m + i * 4) = mm;
      *reinterpret_cast<f32x4*>(v + i * 4) = vv;
      if (ema) *reinterpret_cast<f32x4*>(ema + i * 4) = ee;
#pragma unroll
      for (int k = 0; k < K; ++k) *reinterpret_cast<f32x4*>(prof.p[k] + i * 4) = pp[k];
    } else {
      for (long e = i * 4; e < n; ++e) {
        if (skip) {
          if (zero_grad) grad[e] = 0.f;
          continue;
        }
        float tj = theta[e], mj = m[e], vj = v[e], ej = ema ? ema[e] : 0.f;
        bad |= adam_ema_update(tj, scaled(grad[e]), mj, vj, ej, ema != nullptr, u, step_size);
        m[e] = mj;
        v[e] = vj;
        theta[e] = tj;
        if (zero_grad) grad[e] = 0.f;
        if (ema) ema[e] = ej;
#pragma unroll
        for (int k = 0; k < K; ++k) prof.p[k][e] = pb[k] * prof.p[k][e] + (1.f - pb[k]) * tj;
      }
    }
  }
  EDM_RAISE_HEALTH(health, bad, 1u);
}

int launch_guarded(float* theta, float* grad, float* m, float* v, float* ema, float* const* profiles, int K,
                   const float* betas, long n, float lr, float b1, float b2, float eps, int step, float ema_beta,
                   float grad_scale, const void* dyn, int zero_grad, const void* record, unsigned* health, hipStream_t st,
                   const char* name) {
  EDM_REQUIRE(theta && grad && m && v && n > 0 && step >= 1, "%s: bad args", name);
  EDM_REQUIRE(record && (uintptr_t)record % 8 == 0, "%s: the guard record (device, 64 bytes, 8-byte aligned) is required", name);
  GuardProfiles prof = {{nullptr, nullptr, nullptr, nullptr}};
  for (int k = 0; k < K; ++k) {
    EDM_REQUIRE(profiles[k] && (uintptr_t)profiles[k] % 16 == 0, "%s: profile arenas must be 16-byte aligned", name);
    prof.p[k] = profiles[k];
  }
  EDM_REQUIRE(((uintptr_t)theta % 16 == 0) && ((uintptr_t)grad % 16 == 0) && ((uintptr_t)m % 16 == 0) &&
                  ((uintptr_t)v % 16 == 0) && (!ema || (uintptr_t)ema % 16 == 0),
              "%s: arenas must be 16-byte aligned", name);
  AdamArgs a;
  a.lr = lr; a.b1 = b1; a.b2 = b2; a.eps = eps;
  a.bc1 = (float)(1.0 - pow((double)b1, (double)step));
  a.bc2sqrt = (float)sqrt(1.0 - pow((double)b2, (double)step));
  a.ema_beta = ema_beta;
  a.grad_scale = grad_scale;
  const long n4 = (n + 3) / 4;
  const dim3 grid(grid_for(n4, 256)), block(256);
  const StepParams* d = (const StepParams*)dyn;
  const GuardRecord* r = (const GuardRecord*)record;
#define EDM_GUARDED_LAUNCH(KK_) \
  hipLaunchKernelGGL(k_adam_ema_guarded<KK_>, grid, block, 0, st, theta, grad, m, v, ema, prof, betas, n4, n, a, d, zero_grad, r, health)
  switch (K) {
    case 0: EDM_GUARDED_LAUNCH(0); break;
    case 1: EDM_GUARDED_LAUNCH(1); break;
    case 2: EDM_GUARDED_LAUNCH(2); break;
    case 3: EDM_GUARDED_LAUNCH(3); break;
    default: EDM_GUARDED_LAUNCH(4); break;
  }
#undef EDM_GUARDED_LAUNCH
  EDM_CHECK_LAUNCH(name);
  return EDM_OK;
}

}  // namespace

// grad: n floats at any 4-byte-aligned address.  chunks: DEVICE table of n_chunks (tensor id, first element, length)
// triples of longs; tensors: DEVICE table of n_tensors (first chunk, number of chunks, first block, number of blocks)
// quadruples of ints, a block being 1024 elements counted from the tensor's first; n_blocks: their total.  Both tables must
// stay valid and unchanged until the launches have executed (for a captured stream: for the life of the graph).
// grad_scale, dyn: as edm_adam_ema.  max_norm / clip_value: +inf switches the limit off.  count != 0: the record's counters
// advance (a reduction run for its own sake passes 0).  part (n_blocks doubles), flags (n_blocks + n_tensors words): device
// scratch; sumsq (n_tensors doubles) and record (64 bytes, 8-byte aligned, zeroed once by the caller): the outputs.
// Three launches.
extern "C" int edm_grad_guard(const float* grad, long n, const long* chunks, int n_chunks, const int* tensors,
                              int n_tensors, int n_blocks, float grad_scale, const void* dyn, float max_norm,
                              float clip_value, int skip_nonfinite, int count, double* part, unsigned* flags,
                              double* sumsq, void* record, hipStream_t st) {
  EDM_REQUIRE(grad && n > 0 && (uintptr_t)grad % 4 == 0, "grad_guard: bad gradient arena");
  EDM_REQUIRE(chunks && tensors && n_chunks > 0 && n_tensors > 0 && n_blocks > 0,
              "grad_guard: %d chunks / %d blocks over %d tensors need both tables", n_chunks, n_blocks, n_tensors);
  EDM_REQUIRE(part && flags && sumsq && record && (uintptr_t)record % 8 == 0 && (uintptr_t)part % 8 == 0 &&
                  (uintptr_t)sumsq % 8 == 0,
              "grad_guard: scratch, sums and the 8-byte-aligned record are required");
  EDM_REQUIRE(!(max_norm < 0.f) && !(clip_value < 0.f) && max_norm == max_norm && clip_value == clip_value,
              "grad_guard: max_norm and clip_value are >= 0 (inf: off)");
  static_assert(sizeof(GuardChunk) == 3 * sizeof(long) && sizeof(GuardTensor) == 4 * sizeof(int), "table layouts");
  unsigned* tbad = flags + n_blocks;
  hipLaunchKernelGGL(k_grad_guard_chunks, dim3((unsigned)n_chunks), dim3(256), 0, st, grad, n, (const GuardChunk*)chunks,
                     n_chunks, (const GuardTensor*)tensors, n_tensors, n_blocks, grad_scale, (const StepParams*)dyn, part,
                     flags);
  hipLaunchKernelGGL(k_grad_guard_tensors, dim3((unsigned)((n_tensors + 3) / 4)), dim3(256), 0, st, part, flags,
                     (const GuardTensor*)tensors, n_tensors, n_blocks, sumsq, tbad);
  hipLaunchKernelGGL(k_grad_guard_finish, dim3(1), dim3(64), 0, st, sumsq, tbad, n_tensors, max_norm, clip_value,
                     skip_nonfinite, count, (GuardRecord*)record);
  EDM_CHECK_LAUNCH("grad_guard");
  return EDM_OK;
}

// edm_adam_ema with the decisions of edm_grad_guard (record, DEVICE): see k_adam_ema_guarded.
extern "C" int edm_adam_ema_guarded(float* theta, float* grad, float* m, float* v, float* ema, long n, float lr, float b1,
                                    float b2, float eps, int step, float ema_beta, float grad_scale, const void* dyn,
                                    int zero_grad, const void* record, unsigned* health, hipStream_t st) {
  return launch_guarded(theta, grad, m, v, ema, nullptr, 0, nullptr, n, lr, b1, b2, eps, step, ema_beta, grad_scale, dyn,
                        zero_grad, record, health, st, "adam_ema_guarded");
}
// edm_adam_ema_phema with the decisions of edm_grad_guard; a skipped step leaves the K profiles alone too.
extern "C" int edm_adam_ema_phema_guarded(float* theta, float* grad, float* m, float* v, float* ema,
                                          float* const* profiles, int K, const float* betas, long n, float lr, float b1,
                                          float b2, float eps, int step, float ema_beta, float grad_scale,
                                          const void* dyn, int zero_grad, const void* record, unsigned* health,
                                          hipStream_t st) {
  EDM_REQUIRE(profiles && betas && K >= 1 && K <= 4, "adam_ema_phema_guarded: 1 <= K <= 4 profiles and a beta array required");
  return launch_guarded(theta, grad, m, v, ema, profiles, K, betas, n, lr, b1, b2, eps, step, ema_beta, grad_scale, dyn,
                        zero_grad, record, health, st, "adam_ema_phema_guarded");
}
