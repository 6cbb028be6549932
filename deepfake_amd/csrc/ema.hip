// Exponential moving average of the weights: one more flat fp32 buffer over the parameter store, updated right after
// the optimizer step (inside the same captured graph) and exchanged with the live weights for evaluation.
//   prelude: advances the device update count and writes this step's weight w = 1 - decay_t (fp32), once per step.
//   update:  e <- fma(w, p - e, e) over the WHOLE store [0, n), gaps included (p = 0, e = 0 stays 0).
//   swap:    p <-> e, shadow = bf16(new p); two calls restore all three buffers bit for bit (shadow == bf16(p)).
// Both streams are shaped like optim.hip's *_runs kernels: 256 threads and kEmaBlock = 2048 consecutive elements per
// workgroup, two 16-B quads per thread with both quads' loads issued before the first arithmetic or store, and the
// n % 4 tail one element at a time.  HBM-bound: 12 B per element for the update, 16 B (+ 2 B shadow) for the swap.
#include "common.h"

namespace {

constexpr int kEmaBlock = 2048;

// t = (*num_updates)++ updates were done before this one; d = warmup ? min(decay, (1 + t) / (10 + t)) : decay in
// double (TensorFlow's ExponentialMovingAverage(num_updates=) ramp); *weight = (float)(1 - d).  One thread acts, so
// the count advances once per step however many workgroups the update has, and a replayed graph advances it too.
__global__ void ema_prelude_kernel(int32_t* __restrict__ num_updates, float* __restrict__ weight, double decay,
                                   int warmup) {
  if (threadIdx.x != 0) return;
  const int t = *num_updates;
  *num_updates = t + 1;
  double d = decay;
  if (warmup) {
    const double ramp = (1.0 + (double)t) / (10.0 + (double)t);
    d = ramp < d ? ramp : d;
  }
  *weight = (float)(1.0 - d);
}

// One rounded subtraction and one fma; spelled out, with contraction off, so that quads and tail agree bit for bit.
// w == 1 (decay 0) is the copy e = p: the rounded (p - e) + e need not give p back (p = 1e-8, e = 1 gives 0), and
// torch.lerp, which the host recipes use, also returns its end point exactly at weight 1.  w is uniform: one select.
__device__ __forceinline__ float ema_elem(float p, float e, float w) {
#pragma clang fp contract(off)
  const float d = p - e;
  return w == 1.f ? p : __builtin_fmaf(w, d, e);
}

__global__ __launch_bounds__(256) void ema_update_kernel(const float* __restrict__ P, float* __restrict__ E, long n,
                                                         const float* __restrict__ weight) {
  const float w = *weight;
  const long base = (long)blockIdx.x * kEmaBlock;
  const long idx[2] = {base + threadIdx.x * 4, base + 1024 + threadIdx.x * 4};
  float4 p[2], e[2];
  bool full[2];
#pragma unroll
  for (int u = 0; u < 2; ++u) {     // both quads' loads in flight before the first update
    full[u] = idx[u] + 4 <= n;
    if (full[u]) {
      p[u] = *reinterpret_cast<const float4*>(P + idx[u]);
      e[u] = *reinterpret_cast<const float4*>(E + idx[u]);
    }
  }
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    if (full[u]) {
      const float* pp = reinterpret_cast<const float*>(&p[u]);
      float* ee = reinterpret_cast<float*>(&e[u]);
#pragma unroll
      for (int k = 0; k < 4; ++k) ee[k] = ema_elem(pp[k], ee[k], w);
      *reinterpret_cast<float4*>(E + idx[u]) = e[u];
    } else {
      for (long i = idx[u]; i < n; ++i) E[i] = ema_elem(P[i], E[i], w);   // empty when idx[u] >= n
    }
  }
}

__global__ __launch_bounds__(256) void ema_swap_kernel(float* __restrict__ P, float* __restrict__ E,
                                                       bf16raw* __restrict__ S, long n) {
  const long base = (long)blockIdx.x * kEmaBlock;
  const long idx[2] = {base + threadIdx.x * 4, base + 1024 + threadIdx.x * 4};
  float4 p[2], e[2];
  bool full[2];
#pragma unroll
  for (int u = 0; u < 2; ++u) {     // both quads' loads in flight before the first store
    full[u] = idx[u] + 4 <= n;
    if (full[u]) {
      p[u] = *reinterpret_cast<const float4*>(P + idx[u]);
      e[u] = *reinterpret_cast<const float4*>(E + idx[u]);
    }
  }
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    if (full[u]) {
      *reinterpret_cast<float4*>(P + idx[u]) = e[u];
      *reinterpret_cast<float4*>(E + idx[u]) = p[u];
      if (S) {
        const float* ee = reinterpret_cast<const float*>(&e[u]);
        uint2 w;
        bf16raw* h = reinterpret_cast<bf16raw*>(&w);
#pragma unroll
        for (int k = 0; k < 4; ++k) h[k] = f2bf(ee[k]);
        *reinterpret_cast<uint2*>(S + idx[u]) = w;
      }
    } else {
      for (long i = idx[u]; i < n; ++i) {                                 // empty when idx[u] >= n
        const float pe = P[i], ev = E[i];
        P[i] = ev;
        E[i] = pe;
        if (S) S[i] = f2bf(ev);
      }
    }
  }
}

// 16 B for the fp32 buffers, 8 B for the bf16 shadow (NULL, an absent shadow, passes)
bool ema_misaligned(const void* a, const void* b, const void* shadow) {
  return ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) & 15) ||
         (reinterpret_cast<uintptr_t>(shadow) & 7);
}

// the grid of n > 0 elements, or 0 when it does not fit an int32
unsigned ema_grid(int64_t n) {
  const int64_t blocks = (n + kEmaBlock - 1) / kEmaBlock;
  return blocks > 0x7fffffffL ? 0u : (unsigned)blocks;
}

}  // namespace

extern "C" int dfk_ema_prelude(int32_t* num_updates, float* weight, double decay, int32_t warmup, hipStream_t s) {
  if (!num_updates || !weight) return DFK_EINVAL;
  if (!(decay >= 0.0 && decay < 1.0)) return DFK_EINVAL;   // NaN included
  if ((reinterpret_cast<uintptr_t>(num_updates) & 3) || (reinterpret_cast<uintptr_t>(weight) & 15)) return DFK_EINVAL;
  hipLaunchKernelGGL(ema_prelude_kernel, dim3(1), dim3(64), 0, s, num_updates, weight, decay, (int)(warmup != 0));
  DFK_CHECK_LAUNCH();
  return 0;
}

extern "C" int dfk_ema_update(const float* param, float* ema, int64_t n, const float* weight, hipStream_t s) {
  if (!param || !ema || !weight || param == ema || n < 0) return DFK_EINVAL;
  if (ema_misaligned(param, ema, nullptr) || (reinterpret_cast<uintptr_t>(weight) & 15)) return DFK_EINVAL;
  if (n == 0) return 0;
  const unsigned grid = ema_grid(n);
  if (!grid) return DFK_EINVAL;
  hipLaunchKernelGGL(ema_update_kernel, dim3(grid), dim3(256), 0, s, param, ema, (long)n, weight);
  DFK_CHECK_LAUNCH();
  return 0;
}

extern "C" int dfk_ema_swap(float* param, float* ema, void* bf16_shadow, int64_t n, hipStream_t s) {
  if (!param || !ema || param == ema || n < 0) return DFK_EINVAL;
  if (ema_misaligned(param, ema, bf16_shadow)) return DFK_EINVAL;
  if (n == 0) return 0;
  const unsigned grid = ema_grid(n);
  if (!grid) return DFK_EINVAL;
  hipLaunchKernelGGL(ema_swap_kernel, dim3(grid), dim3(256), 0, s, param, ema, (bf16raw*)bf16_shadow, (long)n);
  DFK_CHECK_LAUNCH();
  return 0;
}
