// wav2vec2 feature-encoder layer 0 (HF modeling_wav2vec2.py:302-323):
//   y[b,t,c] = sum_k w[c,k] x[b,5t+k]          Conv1d(1->512, k10, s5, no bias)
//   z = GroupNorm(512 groups = per channel over time, affine)(y)
//   out = gelu(z)   written channels-last [B, T0, 512] for the implicit-GEMM conv1
// GroupNorm needs whole-time statistics per (clip, channel), so the forward is
// two passes that both recompute the 10-tap conv from the waveform (the
// waveform is 0.26 MB/clip; y is never stored), and the backward likewise.
// The conv itself is VALU work (10 MACs / output) — the pass is HBM-bound on
// the 13 MB/clip output (bf16).
// Padded batches (the RAGGED instantiations, dfk_w2v_conv0_ragged_*): len int64 [B] on the device, clip b holds
// n_b = clamp(len[b], 1, S) samples and T0_b = clamp((n_b - 10) / 5 + 1, 1, T0) frames of its own (both uniform
// over a workgroup: blockIdx.y is the clip).  Samples at or past n_b are staged as zero without being loaded, the
// GroupNorm statistics and the backward's reductions run over t < T0_b with T0_b as the divisor, the rows
// T0_b <= t < T0 of the output are written as zero and those rows of dout are never read: the clip gets the
// arithmetic it would get alone, and with every length full the uniform call's.
#include "common.h"

namespace {

constexpr int TB = 64;    // time steps per workgroup
constexpr int CH = 512;   // channels (conv_dim[0])
constexpr int KW = 10, KS = 5;

// samples and frames of clip b's own; the clamps keep every index these give inside the row
__device__ __forceinline__ long clip_samples(const int64_t* __restrict__ len, int b, long S) {
  return (long)min(max(len[b], (int64_t)1), (int64_t)S);
}
__device__ __forceinline__ int clip_frames(long n, int T0) { return (int)min(max((n - KW) / KS + 1, 1L), (long)T0); }

// stage the waveform segment of this time block (zero from sample n on: n = S, or the clip's own count) and the
// conv weights into LDS
__device__ __forceinline__ void stage(const float* __restrict__ x, const float* __restrict__ w, long S, long n, int b,
                                      int t0, float* xs, float* ws) {
  const long base = (long)b * S + (long)t0 * KS;
  for (int i = threadIdx.x; i < TB * KS + KW; i += 256) {
    const long j = base + i;
    xs[i] = ((long)t0 * KS + i < n) ? x[j] : 0.f;
  }
  for (int i = threadIdx.x; i < CH * KW; i += 256) ws[i] = w[i];
  __syncthreads();
}

__device__ __forceinline__ float conv_at(const float* xs, const float* ws, int tl, int c) {
  float y = 0.f;
#pragma unroll
  for (int k = 0; k < KW; ++k) y += ws[c * KW + k] * xs[tl * KS + k];
  return y;
}

// pass 1: per (b, time block, c) partial sum and sum of squares of y -> the partial slab [b][block][c][2]
// RAGGED: over the clip's own frames; a time block wholly past them writes zero partials (the slab is
// uninitialised and conv0_stats_sum adds every block)
template <bool RAGGED>
__global__ __launch_bounds__(256) void conv0_stats(const float* __restrict__ x, const float* __restrict__ w, long S,
                                                   int T0, float* __restrict__ part, const int64_t* __restrict__ len) {
  __shared__ float xs[TB * KS + KW];
  __shared__ float ws[CH * KW];
  const int b = blockIdx.y, t0 = blockIdx.x * TB;
  const long n = RAGGED ? clip_samples(len, b, S) : S;
  const int Tb = RAGGED ? clip_frames(n, T0) : T0;
  if (RAGGED && t0 >= Tb) {
    float* dst = part + ((long)b * gridDim.x + blockIdx.x) * CH * 2;
    for (int i = threadIdx.x; i < CH * 2; i += 256) dst[i] = 0.f;
    return;
  }
  stage(x, w, S, n, b, t0, xs, ws);
  const int nt = min(TB, Tb - t0);
  for (int c = threadIdx.x; c < CH; c += 256) {
    float s = 0.f, q = 0.f;
    for (int tl = 0; tl < nt; ++tl) {
      const float y = conv_at(xs, ws, tl, c);
      s += y;
      q += y * y;
    }
    float* dst = part + (((long)b * gridDim.x + blockIdx.x) * CH + c) * 2;
    dst[0] = s;
    dst[1] = q;
  }
}

// pass 1b: stats[b][c][2] = sum over the time blocks of the partials, in a fixed order (4 interleaved row phases,
// then (p0 + p1) + (p2 + p3)): the forward's GroupNorm statistics, and so the loss, are bitwise reproducible
__global__ __launch_bounds__(256) void conv0_stats_sum(const float* __restrict__ part, int nblk,
                                                       float* __restrict__ stats) {
  __shared__ float red[4][64];
  const int b = blockIdx.y, lane = threadIdx.x & 63, ph = threadIdx.x >> 6;
  const int j = blockIdx.x * 64 + lane;   // column of the [CH][2] row
  const float* src = part + (long)b * nblk * CH * 2 + j;
  float a[4] = {0.f, 0.f, 0.f, 0.f};
  int r = ph;
  for (; r + 12 < nblk; r += 16) {
#pragma unroll
    for (int u = 0; u < 4; ++u) a[u] += src[(long)(r + 4 * u) * CH * 2];
  }
  for (; r < nblk; r += 4) a[0] += src[(long)r * CH * 2];
  red[ph][lane] = (a[0] + a[1]) + (a[2] + a[3]);
  __syncthreads();
  if (ph == 0) stats[(long)b * CH * 2 + j] = (red[0][lane] + red[1][lane]) + (red[2][lane] + red[3][lane]);
}

// pass 2: out = gelu(gn(y)); one thread per (t, channel pair) -> coalesced channels-last stores
// RAGGED: the rows past the clip's own frames are written as zero
template <typename T, bool RAGGED>
__global__ __launch_bounds__(256) void conv0_apply(const float* __restrict__ x, const float* __restrict__ w, long S,
                                                   int T0, const float* __restrict__ stats, const float* __restrict__ gamma,
                                                   const float* __restrict__ beta, float eps, T* __restrict__ out,
                                                   const int64_t* __restrict__ len) {
  __shared__ float xs[TB * KS + KW];
  __shared__ float ws[CH * KW];
  __shared__ float mu[CH], rs[CH];
  const int b = blockIdx.y, t0 = blockIdx.x * TB;
  const long n = RAGGED ? clip_samples(len, b, S) : S;
  const int Tb = RAGGED ? clip_frames(n, T0) : T0;
  const int nt = max(min(TB, Tb - t0), 0);
  if (nt > 0) {
    stage(x, w, S, n, b, t0, xs, ws);
    for (int c = threadIdx.x; c < CH; c += 256) {
      const float s = stats[((long)b * CH + c) * 2], q = stats[((long)b * CH + c) * 2 + 1];
      const float m = s / Tb;
      mu[c] = m;
      rs[c] = rsqrtf(fmaxf(q / Tb - m * m, 0.f) + eps);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < nt * CH; i += 256) {
      const int tl = i / CH, c = i % CH;
      const float y = conv_at(xs, ws, tl, c);
      const float z = (y - mu[c]) * rs[c] * gamma[c] + beta[c];
      stf<T>(out + ((long)b * T0 + t0 + tl) * CH + c, (sizeof(T) == 2 ? gelu_bf(z) : gelu_f(z)));
    }
  }
  if (RAGGED) {
    const int na = min(TB, T0 - t0);
    for (int i = nt * CH + threadIdx.x; i < na * CH; i += 256) stf<T>(out + ((long)b * T0 + t0) * CH + i, 0.f);
  }
}

// backward pass 1: per (b,c) A = sum_t dz*yhat, Bs = sum_t dz   (dz = dout * gelu'(z))
// RAGGED: over the clip's own frames; a time block wholly past them adds nothing and reads nothing
template <typename T, bool RAGGED>
__global__ __launch_bounds__(256) void conv0_bwd_stats(const float* __restrict__ x, const float* __restrict__ w, long S,
                                                       int T0, const float* __restrict__ stats,
                                                       const float* __restrict__ gamma, const float* __restrict__ beta,
                                                       float eps, const T* __restrict__ dout, float* __restrict__ red,
                                                       const int64_t* __restrict__ len) {
  __shared__ float xs[TB * KS + KW];
  __shared__ float ws[CH * KW];
  const int b = blockIdx.y, t0 = blockIdx.x * TB;
  const long n = RAGGED ? clip_samples(len, b, S) : S;
  const int Tb = RAGGED ? clip_frames(n, T0) : T0;
  if (RAGGED && t0 >= Tb) return;
  stage(x, w, S, n, b, t0, xs, ws);
  const int nt = min(TB, Tb - t0);
  for (int c = threadIdx.x; c < CH; c += 256) {
    const float s = stats[((long)b * CH + c) * 2], q = stats[((long)b * CH + c) * 2 + 1];
    const float m = s / Tb, r = rsqrtf(fmaxf(q / Tb - m * m, 0.f) + eps);
    float A = 0.f, Bs = 0.f;
    for (int tl = 0; tl < nt; ++tl) {
      const float yh = (conv_at(xs, ws, tl, c) - m) * r;
      const float dz = ldf<T>(dout + ((long)b * T0 + t0 + tl) * CH + c) * (sizeof(T) == 2 ? dgelu_bf(yh * gamma[c] + beta[c]) : dgelu_f(yh * gamma[c] + beta[c]));
      A += dz * yh;
      Bs += dz;
    }
    atomicAdd(red + ((long)b * CH + c) * 2, A);
    atomicAdd(red + ((long)b * CH + c) * 2 + 1, Bs);
  }
}

// backward pass 2: dy = rstd*(gamma*dz - gamma*Bs/T0 - yhat*gamma*A/T0);  dw[c,k] += sum_t dy x[5t+k]
// RAGGED: T0_b in T0's place (the sweep ends at the clip's last own time block; a workgroup with no block of the
// clip writes a zero slab row)
template <typename T, bool RAGGED>
__global__ __launch_bounds__(256) void conv0_bwd_dw(const float* __restrict__ x, const float* __restrict__ w, long S,
                                                    int T0, const float* __restrict__ stats,
                                                    const float* __restrict__ gamma, const float* __restrict__ beta,
                                                    float eps, const T* __restrict__ dout, const float* __restrict__ red,
                                                    float* __restrict__ part, const int64_t* __restrict__ len) {
  // each workgroup sweeps a strided set of time blocks and keeps its dw partials in registers, then writes
  // them once to its slab row (four workgroups per CU: the recompute of conv + GroupNorm + GELU' is VALU work
  // that one wave per SIMD left latency-bound)
  __shared__ float xs[TB * KS + KW];
  __shared__ float ws[CH * KW];
  const int b = blockIdx.y;
  const long n = RAGGED ? clip_samples(len, b, S) : S;
  const int Tb = RAGGED ? clip_frames(n, T0) : T0;
  for (int i = threadIdx.x; i < CH * KW; i += 256) ws[i] = w[i];
  constexpr int CPT = CH / 256;   // channels per thread
  float acc[CPT][KW], m[CPT], r[CPT], g[CPT], be[CPT], A[CPT], Bm[CPT];
#pragma unroll
  for (int j = 0; j < CPT; ++j) {
    const int c = threadIdx.x + j * 256;
    const float s = stats[((long)b * CH + c) * 2], q = stats[((long)b * CH + c) * 2 + 1];
    m[j] = s / Tb;
    r[j] = rsqrtf(fmaxf(q / Tb - m[j] * m[j], 0.f) + eps);
    g[j] = gamma[c];
    be[j] = beta[c];
    A[j] = red[((long)b * CH + c) * 2] * g[j] / Tb;
    Bm[j] = red[((long)b * CH + c) * 2 + 1] * g[j] / Tb;
#pragma unroll
    for (int k = 0; k < KW; ++k) acc[j][k] = 0.f;
  }
  const int ntb = (Tb + TB - 1) / TB;
  for (int tb = blockIdx.x; tb < ntb; tb += gridDim.x) {
    const int t0 = tb * TB;
    __syncthreads();
    const long base = (long)b * S + (long)t0 * KS;
    for (int i = threadIdx.x; i < TB * KS + KW; i += 256) xs[i] = ((long)t0 * KS + i < n) ? x[base + i] : 0.f;
    __syncthreads();
    const int nt = min(TB, Tb - t0);
    for (int tl = 0; tl < nt; ++tl) {
#pragma unroll
      for (int j = 0; j < CPT; ++j) {
        const int c = threadIdx.x + j * 256;
        const float yh = (conv_at(xs, ws, tl, c) - m[j]) * r[j];
        const float dz = ldf<T>(dout + ((long)b * T0 + t0 + tl) * CH + c) * (sizeof(T) == 2 ? dgelu_bf(yh * g[j] + be[j]) : dgelu_f(yh * g[j] + be[j]));
        const float dy = r[j] * (g[j] * dz - Bm[j] - yh * A[j]);
#pragma unroll
        for (int k = 0; k < KW; ++k) acc[j][k] += dy * xs[tl * KS + k];
      }
    }
  }
  // this workgroup's partial -> its slab row (summed by dw_slab_sum: no same-address atomics across the
  // workgroups of the grid)
  float* row = part + ((long)blockIdx.y * gridDim.x + blockIdx.x) * (CH * KW);
#pragma unroll
  for (int j = 0; j < CPT; ++j)
#pragma unroll
    for (int k = 0; k < KW; ++k) row[(threadIdx.x + j * 256) * KW + k] = acc[j][k];
}

// dw[i] += sum over the slab rows of part[r][i]  (i < CH*KW): workgroup = 64 columns x one 128-row chunk,
// 4 row phases x 8 loads in flight per lane, one atomic per column and chunk
__global__ __launch_bounds__(256) void dw_slab_sum(const float* __restrict__ part, int rows, float* __restrict__ dw) {
  __shared__ float red[4][64];
  const int lane = threadIdx.x & 63, ph = threadIdx.x >> 6;
  const int i = blockIdx.x * 64 + lane;
  const int r0 = blockIdx.y * 128, r1 = min(rows, r0 + 128);
  float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (i < CH * KW) {
#pragma unroll
    for (int u = 0; u < 32; ++u) {
      const int r = r0 + ph + 4 * u;
      if (r < r1) s[u & 7] += part[(long)r * (CH * KW) + i];
    }
  }
  red[ph][lane] = ((s[0] + s[1]) + (s[2] + s[3])) + ((s[4] + s[5]) + (s[6] + s[7]));
  __syncthreads();
  if (ph == 0 && i < CH * KW) atomicAdd(dw + i, (red[0][lane] + red[1][lane]) + (red[2][lane] + red[3][lane]));
}

// dgamma[c] += sum_b A[b,c] ; dbeta[c] += sum_b Bs[b,c]
__global__ void gn_affine_grad(const float* __restrict__ red, int B, float* dgamma, float* dbeta) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= CH) return;
  float a = 0.f, bs = 0.f;
  for (int b = 0; b < B; ++b) { a += red[((long)b * CH + c) * 2]; bs += red[((long)b * CH + c) * 2 + 1]; }
  if (dgamma) dgamma[c] += a;
  if (dbeta) dbeta[c] += bs;
}

// workgroups per clip of the dw pass: about four per CU over the batch
int conv0_dw_blocks(long B, int T0) { return std::min(dfk_cdiv(T0, TB), std::max(1, (int)(1024 / B))); }

}  // namespace

extern "C" int64_t dfk_w2v_conv0_bwd_workspace(int64_t B, int64_t S) {
  if (B <= 0 || S < KW) return 0;
  const int T0 = (int)((S - KW) / KS + 1);
  return (int64_t)4 * (B * CH * 2 + B * conv0_dw_blocks(B, T0) * (int64_t)(CH * KW));
}

extern "C" int64_t dfk_w2v_conv0_fwd_workspace(int64_t B, int64_t S) {
  if (B <= 0 || S < KW) return 0;
  const int T0 = (int)((S - KW) / KS + 1);
  return (int64_t)4 * B * dfk_cdiv(T0, TB) * CH * 2;
}

namespace {

template <bool RAGGED>
void conv0_fwd_launch(const float* wave, int64_t B, int64_t S, const float* w, const float* gamma, const float* beta,
                      float eps, float* stats, void* out, int dtype, float* ws, const int64_t* len, hipStream_t s) {
  const int T0 = (int)((S - KW) / KS + 1);
  const dim3 grid(dfk_cdiv(T0, TB), (unsigned)B);
  static_assert((CH * 2) % 64 == 0, "stats columns per workgroup");
  hipLaunchKernelGGL(conv0_stats<RAGGED>, grid, dim3(256), 0, s, wave, w, (long)S, T0, ws, len);
  hipLaunchKernelGGL(conv0_stats_sum, dim3(CH * 2 / 64, (unsigned)B), dim3(256), 0, s, ws, (int)grid.x, stats);
  if (dtype == DFK_BF16)
    hipLaunchKernelGGL((conv0_apply<bf16raw, RAGGED>), grid, dim3(256), 0, s, wave, w, (long)S, T0, stats, gamma, beta,
                       eps, (bf16raw*)out, len);
  else
    hipLaunchKernelGGL((conv0_apply<float, RAGGED>), grid, dim3(256), 0, s, wave, w, (long)S, T0, stats, gamma, beta,
                       eps, (float*)out, len);
}

template <bool RAGGED>
void conv0_bwd_launch(const float* wave, int64_t B, int64_t S, const float* w, const float* gamma, const float* beta,
                      float eps, const float* stats, const void* dout, int dtype, float* scratch, float* dw,
                      float* dgamma, float* dbeta, const int64_t* len, hipStream_t s) {
  const int T0 = (int)((S - KW) / KS + 1);
  const dim3 grid(dfk_cdiv(T0, TB), (unsigned)B);
  const dim3 gdw(conv0_dw_blocks(B, T0), (unsigned)B);
  float* part = scratch + B * CH * 2;   // [B * gdw.x][CH * KW] slab after the [B, CH, 2] reductions
  (void)hipMemsetAsync(scratch, 0, sizeof(float) * B * CH * 2, s);
  if (dtype == DFK_BF16) {
    hipLaunchKernelGGL((conv0_bwd_stats<bf16raw, RAGGED>), grid, dim3(256), 0, s, wave, w, (long)S, T0, stats, gamma,
                       beta, eps, (const bf16raw*)dout, scratch, len);
    hipLaunchKernelGGL((conv0_bwd_dw<bf16raw, RAGGED>), gdw, dim3(256), 0, s, wave, w, (long)S, T0, stats, gamma, beta,
                       eps, (const bf16raw*)dout, scratch, part, len);
  } else {
    hipLaunchKernelGGL((conv0_bwd_stats<float, RAGGED>), grid, dim3(256), 0, s, wave, w, (long)S, T0, stats, gamma,
                       beta, eps, (const float*)dout, scratch, len);
    hipLaunchKernelGGL((conv0_bwd_dw<float, RAGGED>), gdw, dim3(256), 0, s, wave, w, (long)S, T0, stats, gamma, beta,
                       eps, (const float*)dout, scratch, part, len);
  }
  hipLaunchKernelGGL(dw_slab_sum, dim3(dfk_cdiv(CH * KW, 64), dfk_cdiv(B * gdw.x, 128)), dim3(256), 0, s, part,
                     (int)(B * gdw.x), dw);
  if (dgamma || dbeta)
    hipLaunchKernelGGL(gn_affine_grad, dim3(dfk_cdiv(CH, 256)), dim3(256), 0, s, scratch, (int)B, dgamma, dbeta);
}

// the argument rules of the ragged entry points: B is a grid dimension, T0 an int
bool conv0_ragged_shape_ok(int64_t B, int64_t S, int dtype) {
  return B > 0 && B <= 65535 && S >= KW && S <= ((int64_t)1 << 31) && (dtype == DFK_F32 || dtype == DFK_BF16);
}

}  // namespace

extern "C" int dfk_w2v_conv0_fwd(const float* wave, int64_t B, int64_t S, const float* w, const float* gamma,
                                 const float* beta, float eps, float* stats, void* out, int dtype, float* ws,
                                 hipStream_t s) {
  if (!wave || !w || !gamma || !beta || !stats || !out || !ws || S < KW) return DFK_EINVAL;
  conv0_fwd_launch<false>(wave, B, S, w, gamma, beta, eps, stats, out, dtype, ws, nullptr, s);
  DFK_CHECK_LAUNCH();
  return 0;
}

extern "C" int dfk_w2v_conv0_bwd(const float* wave, int64_t B, int64_t S, const float* w, const float* gamma,
                                 const float* beta, float eps, const float* stats, const void* dout, int dtype,
                                 float* scratch, int64_t scratch_bytes, float* dw, float* dgamma, float* dbeta,
                                 hipStream_t s) {
  if (!wave || !w || !gamma || !beta || !stats || !dout || !scratch || !dw || S < KW) return DFK_EINVAL;
  if (scratch_bytes < dfk_w2v_conv0_bwd_workspace(B, S)) return DFK_EINVAL;   // the dw slab is sized per launch
  conv0_bwd_launch<false>(wave, B, S, w, gamma, beta, eps, stats, dout, dtype, scratch, dw, dgamma, dbeta, nullptr, s);
  DFK_CHECK_LAUNCH();
  return 0;
}

extern "C" int dfk_w2v_conv0_ragged_fwd(const float* wave, int64_t B, int64_t S, const float* w, const float* gamma,
                                        const float* beta, float eps, float* stats, void* out, int dtype, float* ws,
                                        const int64_t* len, hipStream_t s) {
  if (!wave || !w || !gamma || !beta || !stats || !out || !ws || !len) return DFK_EINVAL;
  if (!conv0_ragged_shape_ok(B, S, dtype)) return DFK_EINVAL;
  conv0_fwd_launch<true>(wave, B, S, w, gamma, beta, eps, stats, out, dtype, ws, len, s);
  DFK_CHECK_LAUNCH();
  return 0;
}

extern "C" int dfk_w2v_conv0_ragged_bwd(const float* wave, int64_t B, int64_t S, const float* w, const float* gamma,
                                        const float* beta, float eps, const float* stats, const void* dout, int dtype,
                                        float* scratch, int64_t scratch_bytes, float* dw, float* dgamma, float* dbeta,
                                        const int64_t* len, hipStream_t s) {
  if (!wave || !w || !gamma || !beta || !stats || !dout || !scratch || !dw || !len) return DFK_EINVAL;
  if (!conv0_ragged_shape_ok(B, S, dtype)) return DFK_EINVAL;
  if (scratch_bytes < dfk_w2v_conv0_bwd_workspace(B, S)) return DFK_EINVAL;   // the dw slab is sized per launch
  conv0_bwd_launch<true>(wave, B, S, w, gamma, beta, eps, stats, dout, dtype, scratch, dw, dgamma, dbeta, len, s);
  DFK_CHECK_LAUNCH();
  return 0;
}

// ---------------------------------------------------------------------------------------------------------
// Layer-norm feature encoder (HF modeling_wav2vec2.py:275-299, Wav2Vec2LayerNormConvLayer; feat_extract_norm ==
// "layer": wav2vec2-large-lv60, XLS-R, HuBERT-large):
//   y[b,t,:] = conv1d(x)[b,:,t] (+ bias);  z = LayerNorm_512(y[b,t,:]; gamma, beta);  out = gelu(z)
// LayerNorm is per frame, so one wave owns one frame row: a lane holds 8 consecutive channels (512 = 64 x 8),
// mean and variance are wave reductions in the fp32 two-pass form, and the row leaves as one 16-B store per
// lane (bf16).  Layer 0 computes the 10-tap conv in the same pass (a lane's 8 x 10 weights stay in registers
// across the frames its wave walks; the 10 samples of a frame are wave-uniform LDS reads); layers 1..6 run the
// same row code on the conv GEMM's [rows, 512] output.  All four kernels are HBM streams: 1 KB (bf16) written
// per frame forward, 1 KB read backward for layer 0, twice that for the others.
// The backward kernels keep their parameter-gradient partials in registers over the rows a wave walks, fold
// the workgroup's waves through LDS in a fixed order, write one slab row per workgroup, and ln_slab_sum adds
// the rows in a fixed order into the sinks: no float atomics, so the gradients are bitwise repeatable.
namespace {

constexpr int LN_WAVES = 4;                    // waves per workgroup
constexpr int CPL = CH / 64;                   // consecutive channels per lane
constexpr int NR0 = CPL * KW + 3 * CPL;        // conv0 backward: per-lane partials (dw | dbias | dgamma | dbeta)
constexpr int NR1 = 3 * CPL;                   // ln_gelu backward: per-lane partials (dbias | dgamma | dbeta)
constexpr int LN_COLS0 = CH * KW + 3 * CH;     // conv0 slab row
constexpr int LN_COLS1 = 3 * CH;               // ln_gelu slab row

template <typename T> __device__ __forceinline__ float gelu_t(float z) { return sizeof(T) == 2 ? gelu_bf(z) : gelu_f(z); }
template <typename T> __device__ __forceinline__ float dgelu_t(float z) { return sizeof(T) == 2 ? dgelu_bf(z) : dgelu_f(z); }

__device__ __forceinline__ void ld8f(const float* p, float* v) { ld8<float>(p, v); }

// mean and 1/sqrt(var + eps) of the wave's 512-channel row (two-pass; the same value in every lane)
__device__ __forceinline__ void row_stats(const float* y, float eps, float& mean, float& rstd) {
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < CPL; ++j) s += y[j];
  mean = wave_sum(s) * (1.f / CH);
  float q = 0.f;
#pragma unroll
  for (int j = 0; j < CPL; ++j) q = fmaf(y[j] - mean, y[j] - mean, q);
  rstd = rsqrtf(wave_sum(q) * (1.f / CH) + eps);
}

// the waveform samples of time block t0 of clip b -> LDS; nothing at or past sample S is read
__device__ __forceinline__ void stage_wave(const float* __restrict__ x, long S, int b, int t0, float* xs) {
  const long off = (long)t0 * KS;
  for (int i = threadIdx.x; i < TB * KS + KW; i += 64 * LN_WAVES) xs[i] = (off + i < S) ? x[(long)b * S + off + i] : 0.f;
}

// this lane's 8 x 10 conv weights (80 consecutive floats of w [512][10]) and y = conv (+ bias) of one frame
__device__ __forceinline__ void load_w(const float* __restrict__ w, int lane, float (&wr)[CPL][KW]) {
  const float4* p = reinterpret_cast<const float4*>(w + lane * (CPL * KW));
  float* f = &wr[0][0];
#pragma unroll
  for (int i = 0; i < CPL * KW / 4; ++i) {
    const float4 v = p[i];
    f[4 * i] = v.x; f[4 * i + 1] = v.y; f[4 * i + 2] = v.z; f[4 * i + 3] = v.w;
  }
}
__device__ __forceinline__ void conv_row(const float (&wr)[CPL][KW], const float* bi, const float* xv, float* y) {
#pragma unroll
  for (int j = 0; j < CPL; ++j) {
    float a = bi[j];
#pragma unroll
    for (int k = 0; k < KW; ++k) a = fmaf(wr[j][k], xv[k], a);
    y[j] = a;
  }
}

template <typename T>
__global__ __launch_bounds__(64 * LN_WAVES) void conv0_ln_fwd(const float* __restrict__ x, const float* __restrict__ w,
                                                              const float* __restrict__ bias,
                                                              const float* __restrict__ gamma,
                                                              const float* __restrict__ beta, long S, int T0, float eps,
                                                              float* __restrict__ stats, T* __restrict__ out) {
  __shared__ float xs[TB * KS + KW];
  const int b = blockIdx.y, t0 = blockIdx.x * TB;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  stage_wave(x, S, b, t0, xs);
  float wr[CPL][KW], g[CPL], be[CPL], bi[CPL];
  load_w(w, lane, wr);
  ld8f(gamma + lane * CPL, g);
  ld8f(beta + lane * CPL, be);
  if (bias) ld8f(bias + lane * CPL, bi);
  else {
#pragma unroll
    for (int j = 0; j < CPL; ++j) bi[j] = 0.f;
  }
  __syncthreads();
  const int nt = min(TB, T0 - t0);
  for (int tl = wv; tl < nt; tl += LN_WAVES) {
    float xv[KW], y[CPL], mean, rstd;
#pragma unroll
    for (int k = 0; k < KW; ++k) xv[k] = xs[tl * KS + k];
    conv_row(wr, bi, xv, y);
    row_stats(y, eps, mean, rstd);
#pragma unroll
    for (int j = 0; j < CPL; ++j) y[j] = gelu_t<T>(fmaf((y[j] - mean) * rstd, g[j], be[j]));
    const long row = (long)b * T0 + t0 + tl;
    st8<T>(out + row * CH + lane * CPL, y);
    if (lane == 0) *reinterpret_cast<float2*>(stats + row * 2) = make_float2(mean, rstd);
  }
}

// LayerNorm + GELU backward of one row held 8 channels per lane: xh = xhat, d = dout on entry; on exit d = the
// gradient of the LayerNorm input.  dgamma / dbeta partials are accumulated into pg / pb.
template <typename T>
__device__ __forceinline__ void row_bwd(const float* xh, float* d, const float* g, const float* be, float rstd,
                                        float* pg, float* pb) {
  float s1 = 0.f, s2 = 0.f;
#pragma unroll
  for (int j = 0; j < CPL; ++j) {
    const float dz = d[j] * dgelu_t<T>(fmaf(xh[j], g[j], be[j]));
    pg[j] = fmaf(dz, xh[j], pg[j]);
    pb[j] += dz;
    d[j] = dz * g[j];
    s1 += d[j];
    s2 = fmaf(d[j], xh[j], s2);
  }
  s1 = wave_sum(s1) * (1.f / CH);
  s2 = wave_sum(s2) * (1.f / CH);
#pragma unroll
  for (int j = 0; j < CPL; ++j) d[j] = rstd * (d[j] - s1 - xh[j] * s2);
}

// fold the per-lane partials v[NR] of the workgroup's waves into wave 0, in the fixed order ((w3 + w2) + w1) + w0
template <int NR>
__device__ __forceinline__ void fold_waves(float (&v)[NR], float* red, int lane, int wv) {
  for (int src = LN_WAVES - 1; src >= 1; --src) {
    if (wv == src) {
#pragma unroll
      for (int r = 0; r < NR; ++r) red[r * 64 + lane] = v[r];
    }
    __syncthreads();
    if (wv == src - 1) {
#pragma unroll
      for (int r = 0; r < NR; ++r) v[r] += red[r * 64 + lane];
    }
    __syncthreads();
  }
}

__device__ __forceinline__ void st8f(float* p, const float* v) { st8<float>(p, v); }

template <typename T>
__global__ __launch_bounds__(64 * LN_WAVES) void conv0_ln_bwd(const float* __restrict__ x, const float* __restrict__ w,
                                                              const float* __restrict__ bias,
                                                              const float* __restrict__ gamma,
                                                              const float* __restrict__ beta, long S, int T0,
                                                              const float* __restrict__ stats,
                                                              const T* __restrict__ dout, float* __restrict__ part) {
  __shared__ float xs[TB * KS + KW];
  __shared__ float red[NR0 * 64];
  const int b = blockIdx.y;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  float wr[CPL][KW], g[CPL], be[CPL], bi[CPL];
  load_w(w, lane, wr);
  ld8f(gamma + lane * CPL, g);
  ld8f(beta + lane * CPL, be);
  if (bias) ld8f(bias + lane * CPL, bi);
  else {
#pragma unroll
    for (int j = 0; j < CPL; ++j) bi[j] = 0.f;
  }
  float v[NR0];   // [0, 80): dw[j][k]; then dbias[j], dgamma[j], dbeta[j]
#pragma unroll
  for (int r = 0; r < NR0; ++r) v[r] = 0.f;
  const int ntb = (T0 + TB - 1) / TB;
  for (int tb = blockIdx.x; tb < ntb; tb += gridDim.x) {
    const int t0 = tb * TB;
    __syncthreads();
    stage_wave(x, S, b, t0, xs);
    __syncthreads();
    const int nt = min(TB, T0 - t0);
    for (int tl = wv; tl < nt; tl += LN_WAVES) {
      const long row = (long)b * T0 + t0 + tl;
      const float2 st = *reinterpret_cast<const float2*>(stats + row * 2);
      float xv[KW], xh[CPL], d[CPL];
      ld8<T>(dout + row * CH + lane * CPL, d);
#pragma unroll
      for (int k = 0; k < KW; ++k) xv[k] = xs[tl * KS + k];
      conv_row(wr, bi, xv, xh);
#pragma unroll
      for (int j = 0; j < CPL; ++j) xh[j] = (xh[j] - st.x) * st.y;
      row_bwd<T>(xh, d, g, be, st.y, v + CPL * KW + CPL, v + CPL * KW + 2 * CPL);
#pragma unroll
      for (int j = 0; j < CPL; ++j) {
        v[CPL * KW + j] += d[j];
#pragma unroll
        for (int k = 0; k < KW; ++k) v[j * KW + k] = fmaf(d[j], xv[k], v[j * KW + k]);
      }
    }
  }
  fold_waves<NR0>(v, red, lane, wv);
  if (wv == 0) {
    float* row = part + ((long)blockIdx.y * gridDim.x + blockIdx.x) * LN_COLS0;
#pragma unroll
    for (int i = 0; i < CPL * KW / 4; ++i)
      *reinterpret_cast<float4*>(row + lane * (CPL * KW) + 4 * i) = make_float4(v[4 * i], v[4 * i + 1], v[4 * i + 2], v[4 * i + 3]);
#pragma unroll
    for (int q = 0; q < 3; ++q) st8f(row + CH * KW + q * CH + lane * CPL, v + CPL * KW + q * CPL);
  }
}

template <typename T>
__global__ __launch_bounds__(64 * LN_WAVES) void ln_gelu_fwd(const T* __restrict__ x, long rows,
                                                             const float* __restrict__ gamma,
                                                             const float* __restrict__ beta, float eps,
                                                             float* __restrict__ stats, T* __restrict__ out) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  float g[CPL], be[CPL];
  ld8f(gamma + lane * CPL, g);
  ld8f(beta + lane * CPL, be);
  for (long row = (long)blockIdx.x * LN_WAVES + wv; row < rows; row += (long)gridDim.x * LN_WAVES) {
    float y[CPL], mean, rstd;
    ld8<T>(x + row * CH + lane * CPL, y);
    row_stats(y, eps, mean, rstd);
#pragma unroll
    for (int j = 0; j < CPL; ++j) y[j] = gelu_t<T>(fmaf((y[j] - mean) * rstd, g[j], be[j]));
    st8<T>(out + row * CH + lane * CPL, y);
    if (lane == 0) *reinterpret_cast<float2*>(stats + row * 2) = make_float2(mean, rstd);
  }
}

template <typename T>
__global__ __launch_bounds__(64 * LN_WAVES) void ln_gelu_bwd(const T* __restrict__ dy, const T* __restrict__ x, long rows,
                                                             const float* __restrict__ gamma,
                                                             const float* __restrict__ beta,
                                                             const float* __restrict__ stats, T* __restrict__ dx,
                                                             float* __restrict__ part) {
  __shared__ float red[NR1 * 64];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  float g[CPL], be[CPL];
  ld8f(gamma + lane * CPL, g);
  ld8f(beta + lane * CPL, be);
  float v[NR1];   // dbias[j], dgamma[j], dbeta[j]
#pragma unroll
  for (int r = 0; r < NR1; ++r) v[r] = 0.f;
  for (long row = (long)blockIdx.x * LN_WAVES + wv; row < rows; row += (long)gridDim.x * LN_WAVES) {
    const float2 st = *reinterpret_cast<const float2*>(stats + row * 2);
    float xh[CPL], d[CPL];
    ld8<T>(x + row * CH + lane * CPL, xh);
    ld8<T>(dy + row * CH + lane * CPL, d);
#pragma unroll
    for (int j = 0; j < CPL; ++j) xh[j] = (xh[j] - st.x) * st.y;
    row_bwd<T>(xh, d, g, be, st.y, v + CPL, v + 2 * CPL);
#pragma unroll
    for (int j = 0; j < CPL; ++j) v[j] += d[j];
    st8<T>(dx + row * CH + lane * CPL, d);
  }
  fold_waves<NR1>(v, red, lane, wv);
  if (wv == 0) {
    float* row = part + (long)blockIdx.x * LN_COLS1;
#pragma unroll
    for (int q = 0; q < 3; ++q) st8f(row + q * CH + lane * CPL, v + q * CPL);
  }
}

// sinks += column sums of the slab part[rows][ncol], every column by one lane group in a fixed order (4
// interleaved row phases, then (p0 + p1) + (p2 + p3)).  Columns [0, n0) go to d0, then three runs of CH columns
// to d1, d2, d3; a null sink is skipped.
__global__ __launch_bounds__(256) void ln_slab_sum(const float* __restrict__ part, int rows, int ncol, int n0,
                                                   float* __restrict__ d0, float* __restrict__ d1,
                                                   float* __restrict__ d2, float* __restrict__ d3) {
  __shared__ float red[4][64];
  const int lane = threadIdx.x & 63, ph = threadIdx.x >> 6;
  const int i = blockIdx.x * 64 + lane;
  float a[4] = {0.f, 0.f, 0.f, 0.f};
  if (i < ncol) {
    const float* src = part + i;
    int r = ph;
    for (; r + 12 < rows; r += 16) {
#pragma unroll
      for (int u = 0; u < 4; ++u) a[u] += src[(long)(r + 4 * u) * ncol];
    }
    for (; r < rows; r += 4) a[0] += src[(long)r * ncol];
  }
  red[ph][lane] = (a[0] + a[1]) + (a[2] + a[3]);
  __syncthreads();
  if (ph == 0 && i < ncol) {
    const float s = (red[0][lane] + red[1][lane]) + (red[2][lane] + red[3][lane]);
    float* d = d0;
    int o = i;
    if (i >= n0) {
      const int q = (i - n0) / CH;
      o = (i - n0) % CH;
      d = q == 0 ? d1 : (q == 1 ? d2 : d3);
    }
    if (d) d[o] += s;
  }
}

// workgroups per clip of the conv0 backward: about two per CU over the batch
int conv0_ln_blocks(long B, int T0) { return std::min(dfk_cdiv(T0, TB), std::max(1, (int)(512 / B))); }
// workgroups of the ln_gelu kernels (each wave strides over the rows)
int ln_gelu_fwd_blocks(long rows) { return (int)std::min<long>((rows + LN_WAVES - 1) / LN_WAVES, 2048); }
int ln_gelu_bwd_blocks(long rows) { return (int)std::min<long>((rows + LN_WAVES - 1) / LN_WAVES, 512); }

bool al(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

}  // namespace

extern "C" int64_t dfk_w2v_conv0_ln_bwd_workspace(int64_t B, int64_t S) {
  if (B <= 0 || B > 65535 || S < KW || S > ((int64_t)1 << 31)) return 0;
  const int T0 = (int)((S - KW) / KS + 1);
  return (int64_t)4 * B * conv0_ln_blocks(B, T0) * LN_COLS0;
}

extern "C" int dfk_w2v_conv0_ln_fwd(const float* wave, int64_t B, int64_t S, const float* w, const float* bias,
                                    const float* gamma, const float* beta, float eps, float* stats, void* out,
                                    int dtype, hipStream_t s) {
  if (!wave || !w || !gamma || !beta || !stats || !out) return DFK_EINVAL;
  if (B <= 0 || B > 65535 || S < KW || S > ((int64_t)1 << 31) || (dtype != DFK_F32 && dtype != DFK_BF16)) return DFK_EINVAL;
  if (!al(wave, 4) || !al(w, 16) || !al(gamma, 16) || !al(beta, 16) || !al(bias, 16) || !al(stats, 8) || !al(out, 16))
    return DFK_EINVAL;
  const int T0 = (int)((S - KW) / KS + 1);
  const dim3 grid(dfk_cdiv(T0, TB), (unsigned)B);
  if (dtype == DFK_BF16)
    hipLaunchKernelGGL(conv0_ln_fwd<bf16raw>, grid, dim3(64 * LN_WAVES), 0, s, wave, w, bias, gamma, beta, (long)S, T0,
                       eps, stats, (bf16raw*)out);
  else
    hipLaunchKernelGGL(conv0_ln_fwd<float>, grid, dim3(64 * LN_WAVES), 0, s, wave, w, bias, gamma, beta, (long)S, T0, eps,
                       stats, (float*)out);
  DFK_CHECK_LAUNCH();
  return 0;
}

extern "C" int dfk_w2v_conv0_ln_bwd(const float* wave, int64_t B, int64_t S, const float* w, const float* bias,
                                    const float* gamma, const float* beta, const float* stats, const void* dout,
                                    int dtype, float* scratch, int64_t scratch_bytes, float* dw, float* dbias,
                                    float* dgamma, float* dbeta, hipStream_t s) {
  if (!wave || !w || !gamma || !beta || !stats || !dout || !scratch || !dw) return DFK_EINVAL;
  if (B <= 0 || B > 65535 || S < KW || S > ((int64_t)1 << 31) || (dtype != DFK_F32 && dtype != DFK_BF16)) return DFK_EINVAL;
  if ((bias == nullptr) != (dbias == nullptr)) return DFK_EINVAL;   // a bias gradient needs the bias, and the reverse
  if (!al(wave, 4) || !al(w, 16) || !al(gamma, 16) || !al(beta, 16) || !al(bias, 16) || !al(stats, 8) ||
      !al(dout, 16) || !al(scratch, 16) || !al(dw, 4) || !al(dbias, 4) || !al(dgamma, 4) || !al(dbeta, 4))
    return DFK_EINVAL;
  if (scratch_bytes < dfk_w2v_conv0_ln_bwd_workspace(B, S)) return DFK_EINVAL;   // the slab is sized per launch
  const int T0 = (int)((S - KW) / KS + 1);
  const dim3 grid(conv0_ln_blocks(B, T0), (unsigned)B);
  if (dtype == DFK_BF16)
    hipLaunchKernelGGL(conv0_ln_bwd<bf16raw>, grid, dim3(64 * LN_WAVES), 0, s, wave, w, bias, gamma, beta, (long)S, T0,
                       stats, (const bf16raw*)dout, scratch);
  else
    hipLaunchKernelGGL(conv0_ln_bwd<float>, grid, dim3(64 * LN_WAVES), 0, s, wave, w, bias, gamma, beta, (long)S, T0,
                       stats, (const float*)dout, scratch);
  hipLaunchKernelGGL(ln_slab_sum, dim3(LN_COLS0 / 64), dim3(256), 0, s, scratch, (int)(B * grid.x), LN_COLS0, CH * KW,
                     dw, dbias, dgamma, dbeta);
  DFK_CHECK_LAUNCH();
  return 0;
}

extern "C" int64_t dfk_w2v_ln_gelu_bwd_workspace(int64_t rows) {
  if (rows <= 0) return 0;
  return (int64_t)4 * ln_gelu_bwd_blocks(rows) * LN_COLS1;
}

extern "C" int dfk_w2v_ln_gelu_fwd(const void* x, int64_t rows, int64_t C, const float* gamma, const float* beta,
                                   float eps, float* stats, void* out, int dtype, hipStream_t s) {
  if (!x || !gamma || !beta || !stats || !out) return DFK_EINVAL;
  if (rows <= 0 || C != CH || (dtype != DFK_F32 && dtype != DFK_BF16)) return DFK_EINVAL;
  if (!al(x, 16) || !al(out, 16) || !al(gamma, 16) || !al(beta, 16) || !al(stats, 8)) return DFK_EINVAL;
  const dim3 grid(ln_gelu_fwd_blocks(rows));
  if (dtype == DFK_BF16)
    hipLaunchKernelGGL(ln_gelu_fwd<bf16raw>, grid, dim3(64 * LN_WAVES), 0, s, (const bf16raw*)x, (long)rows, gamma, beta,
                       eps, stats, (bf16raw*)out);
  else
    hipLaunchKernelGGL(ln_gelu_fwd<float>, grid, dim3(64 * LN_WAVES), 0, s, (const float*)x, (long)rows, gamma, beta, eps,
                       stats, (float*)out);
  DFK_CHECK_LAUNCH();
  return 0;
}

extern "C" int dfk_w2v_ln_gelu_bwd(const void* dy, const void* x, int64_t rows, int64_t C, const float* gamma,
                                   const float* beta, const float* stats, void* dx, int dtype, float* scratch,
                                   int64_t scratch_bytes, float* dgamma, float* dbeta, float* dbias, hipStream_t s) {
  if (!dy || !x || !gamma || !beta || !stats || !dx || !scratch) return DFK_EINVAL;
  if (rows <= 0 || C != CH || (dtype != DFK_F32 && dtype != DFK_BF16)) return DFK_EINVAL;
  if (!al(dy, 16) || !al(x, 16) || !al(dx, 16) || !al(gamma, 16) || !al(beta, 16) || !al(stats, 8) ||
      !al(scratch, 16) || !al(dgamma, 4) || !al(dbeta, 4) || !al(dbias, 4))
    return DFK_EINVAL;
  if (scratch_bytes < dfk_w2v_ln_gelu_bwd_workspace(rows)) return DFK_EINVAL;
  const dim3 grid(ln_gelu_bwd_blocks(rows));
  if (dtype == DFK_BF16)
    hipLaunchKernelGGL(ln_gelu_bwd<bf16raw>, grid, dim3(64 * LN_WAVES), 0, s, (const bf16raw*)dy, (const bf16raw*)x,
                       (long)rows, gamma, beta, stats, (bf16raw*)dx, scratch);
  else
    hipLaunchKernelGGL(ln_gelu_bwd<float>, grid, dim3(64 * LN_WAVES), 0, s, (const float*)dy, (const float*)x, (long)rows,
                       gamma, beta, stats, (float*)dx, scratch);
  hipLaunchKernelGGL(ln_slab_sum, dim3(LN_COLS1 / 64), dim3(256), 0, s, scratch, (int)grid.x, LN_COLS1, 0,
                     (float*)nullptr, dbias, dgamma, dbeta);
  DFK_CHECK_LAUNCH();
  return 0;
}
