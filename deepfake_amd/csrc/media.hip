// Media front end on the device: the per-clip transforms the reference runs on the host
// before the model sees a batch.
//
//  * mel-spectrogram image — generate_mel_spectrogram (src/utils.py:63-87):
//      librosa.feature.melspectrogram(y, sr, n_mels) (n_fft 2048, hop 512, periodic Hann, center=True with zero
//      padding, power 2, Slaney-normalised Slaney-scale filterbank) -> librosa.power_to_db(S, ref=np.max)
//      (amin 1e-10, top_db 80) -> cv2.normalize(NORM_MINMAX, 0, 255) -> astype(uint8) (truncation) ->
//      cv2.resize(target, INTER_LINEAR) (uint8 fixed point, 11-bit coefficients).
//    The STFT runs as one fp32 MFMA GEMM per batch (dfk_gemm: frames of the padded waveform, a strided
//    overlapping view with row stride = hop, times a window-folded cos | -sin basis); power, filterbank and dB
//    in mel_power_kernel; per-clip min/max, quantisation and the resize in mel_image_kernel (image in LDS).
//    The JPEG round trip of the reference's cached images (data_process.py:83-93,162) is not reproduced (a
//    lossy codec outside the hot path).
//  * resampling — librosa.load's 16 kHz -> 22.05 kHz step in front of the mel spectrogram (src/utils.py:70):
//    a polyphase Kaiser-windowed sinc (table built on the host, media.resample_taps; up / down = L / M in lowest
//    terms), y[n] = sum_j x[i_n + j] H[p_n][j] with n M = i_n L + p_n.  A run of L outputs uses every phase once
//    and spans M inputs, so a workgroup takes whole periods of one clip, stages their input span plus the filter
//    halo in LDS and each thread makes one output at a time from LDS.  dfk_resample writes [B][S_out];
//    dfk_mel_image_resampled lets the same kernel write straight into the centre-padded STFT buffer (in place of
//    mel_pad_kernel), so the 22.05 kHz waveform makes no round trip of its own.  The filter is this build's
//    own: parity with librosa's soxr_hq is unpinned.
//  * ragged batches — the reference builds each clip's image from its own track at its own length
//    (data/data_process.py:82-93): dfk_resample_ragged / dfk_mel_image_ragged take a padded [B][S] batch and a
//    device array of per-clip lengths, and give every clip what the uniform entry points give it alone.
//  * gray image -> model input — Image.convert('RGB') + T.ToTensor() + T.Normalize (data_process.py:55-69,162):
//    uint8 [N, H, W] -> fp32 [N, 3, H, W], (x / 255 - mean[c]) / std[c].
//  * frame / mel-image transform — torchvision's T.Resize / RandomHorizontalFlip / RandomVerticalFlip /
//    RandomRotation(90) / ToTensor / Normalize as the reference runs them, on PIL images (data_process.py:55-69,
//    162; src/utils.py:32-33): PIL's antialiased BILINEAR resize (width pass, then height pass fused with the flips,
//    the NEAREST rotation's fixed-point inverse map and the normalisation).  Random flips / angles are per image.
#include "common.h"

namespace {

// Ragged batches (RAGGED kernels below): lengths int64 [B] on the device, clip b holds lengths[b] samples of its
// row of S, the rest of the row is padding that is never read.  Every kernel clamps the value into [1, S] first, so
// nothing in that array can take an index outside the row.
__device__ __forceinline__ long clip_len(const int64_t* __restrict__ lengths, long b, long S) {
  return (long)min(max(lengths[b], (int64_t)1), (int64_t)S);
}

template <bool RAGGED>
__global__ __launch_bounds__(256) void mel_pad_kernel(const float* __restrict__ y, long S, int half, long Lp,
                                                      float* __restrict__ yp, const int64_t* __restrict__ lengths) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long b = blockIdx.y;
  if (i >= Lp) return;
  const long s = i - half;
  const long n = RAGGED ? clip_len(lengths, b, S) : S;
  yp[b * Lp + i] = (s >= 0 && s < n) ? y[b * S + s] : 0.f;
}

// Polyphase resampler.  taps [ntaps][L] in period order: taps[jj][r] = H[(r M) mod L][jj], so the threads of
// consecutive outputs read consecutive entries.  Workgroup (blockIdx.x, clip blockIdx.y) owns `per` periods:
// outputs [q0 L, (q0 + per) L) from inputs [q0 M - Z + 1, (q0 + per - 1) M + (M - 1) + Z], Z = ntaps / 2, staged in
// LDS (zero outside [0, S_in)).  Sample indices are formed per period in 64 bit (n M passes 2^32 on long clips).
// The output row b starts at y + b ldy + pad; with pad > 0 (the STFT buffer) the first workgroup of each clip
// also zeroes the pad floats on either side of the S_out samples.
// RAGGED: the clip ends at n_in = lengths[b] of the row's S_in samples: the staging reads zero from there on,
// outputs below m = ceil(n_in L / M) are formed exactly as a clip of n_in samples alone would form them, and
// [m, S_out) is written as zero (workgroups wholly past m write zeros only); the grid covers the row.
template <bool RAGGED>
__global__ __launch_bounds__(256) void resample_kernel(const float* __restrict__ x, long S_in,
                                                       const float* __restrict__ taps, int L, int M, int ntaps,
                                                       int per, float* __restrict__ y, long S_out, long ldy, int pad,
                                                       const int64_t* __restrict__ lengths) {
  extern __shared__ float xs[];
  const long b = blockIdx.y, q0 = (long)blockIdx.x * per;
  const long n_in = RAGGED ? clip_len(lengths, b, S_in) : S_in;
  const long m_out = RAGGED ? (n_in * L + M - 1) / M : S_out;
  const int span = per * M + ntaps - 1;
  const long i0 = q0 * M - (ntaps / 2 - 1);
  const float* xb = x + b * S_in;
  for (int k = threadIdx.x; k < span; k += blockDim.x) {
    const long i = i0 + k;
    xs[k] = (i >= 0 && i < n_in) ? xb[i] : 0.f;
  }
  float* yb = y + b * ldy;
  if (pad > 0 && blockIdx.x == 0) {
    for (int k = threadIdx.x; k < pad; k += blockDim.x) {
      yb[k] = 0.f;
      yb[pad + S_out + k] = 0.f;
    }
  }
  __syncthreads();
  const long n0 = q0 * L;
  for (int o = threadIdx.x; o < per * L; o += blockDim.x) {
    const long n = n0 + o;
    if (n >= S_out) break;
    if (RAGGED && n >= m_out) {
      yb[pad + n] = 0.f;
      continue;
    }
    const int qq = o / L, r = o - qq * L;
    const float* xw = xs + qq * M + (int)(((long)r * M) / L);
    const float* h = taps + r;
    float acc = 0.f;
#pragma unroll 8
    for (int j = 0; j < ntaps; ++j) acc = fmaf(xw[j], h[(long)j * L], acc);
    yb[pad + n] = acc;
  }
}

// one workgroup per (clip, frame): |X[f]|^2 into LDS, then mel[m] = sum_f fb[m][f] |X[f]|^2 (fp32, the
// filterbank row streamed once per frame), written [clip][m][frame] (the reference's S layout)
__global__ __launch_bounds__(256) void mel_power_kernel(const float* __restrict__ X, long ldx, int nbin, int T,
                                                        const float* __restrict__ fb, int n_mels,
                                                        float* __restrict__ S) {
  extern __shared__ float pw[];
  const int t = blockIdx.x, b = blockIdx.y;
  const float* xr = X + ((long)b * T + t) * ldx;
  for (int f = threadIdx.x; f < nbin; f += blockDim.x) {
    const float re = xr[f], im = xr[nbin + f];
    pw[f] = re * re + im * im;
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
  for (int m = w; m < n_mels; m += nw) {   // one wave per mel band: lanes stride the bins, then a wave sum
    const float* row = fb + (long)m * nbin;
    float acc = 0.f;
    for (int f = lane; f < nbin; f += 64) acc += row[f] * pw[f];
    acc = wave_sum(acc);
    if (lane == 0) S[((long)b * n_mels + m) * T + t] = acc;
  }
}

__device__ __forceinline__ float block_max(float v, float* red) {
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) red[w] = v;
  __syncthreads();
  float t = red[0];
  for (int i = 1; i < (int)(blockDim.x >> 6); ++i) t = fmaxf(t, red[i]);
  return t;
}

// cv2 INTER_LINEAR tap for destination index d: (source index, 11-bit weights)
__device__ __forceinline__ void cv_tap(int d, double scale, int sn, int& s0, int& a0, int& a1) {
  float fx = (float)((d + 0.5) * scale - 0.5);
  int sx = (int)floorf(fx);
  fx -= (float)sx;
  if (sx < 0) { fx = 0.f; sx = 0; }
  if (sx >= sn - 1) { fx = 0.f; sx = sn - 1; }
  s0 = sx;
  a0 = (int)rintf((1.f - fx) * 2048.f);
  a1 = (int)rintf(fx * 2048.f);
}

// one workgroup per clip: power_to_db(ref=max, top_db 80), cv2 min-max to [0, 255], uint8 truncation into an
// LDS image [n_mels][T], then the cv2 fixed-point bilinear resize to [oh][ow]
// RAGGED: S keeps its [n_mels][Tmax] stride, but the clip has only T = 1 + m / hop frames (m = ceil(n_in L / M)
// samples at the filterbank's rate, n_in = lengths[b] of the row's S_in; L = M = 1 without the resampler).  Frames
// from T on still overlap the clip's tail, so they are not silent: they are left out of the max, the dB range and
// the image, which is built [n_mels][T] and resized from T columns, as for a clip of n_in samples alone.
template <bool RAGGED>
__global__ __launch_bounds__(1024) void mel_image_kernel(const float* __restrict__ S, int n_mels, int Tmax, int oh,
                                                         int ow, uint8_t* __restrict__ out,
                                                         const int64_t* __restrict__ lengths, long S_in, int L, int M,
                                                         int hop) {
  extern __shared__ uint8_t img[];
  __shared__ float red[16];
  const int b = blockIdx.x;
  const float* sb = S + (long)b * n_mels * Tmax;
  const int T = RAGGED ? min(Tmax, (int)(1 + ((clip_len(lengths, b, S_in) * L + M - 1) / M) / hop)) : Tmax;
  const long n = (long)n_mels * T;
  // element i of the clip's own [n_mels][T] spectrum (n_mels Tmax fits the LDS image, so 32-bit division does)
  auto s = [&](long i) { return RAGGED ? sb[((int)i / T) * Tmax + (int)i % T] : sb[i]; };
  float mx = -INFINITY;
  for (long i = threadIdx.x; i < n; i += blockDim.x) mx = fmaxf(mx, s(i));
  mx = block_max(mx, red);
  const float amin = 1e-10f;
  const float refdb = 10.f * log10f(fmaxf(amin, mx));
  // dB values, their max (0 up to rounding) and min after the top_db floor
  float dmx = -INFINITY, dmn = INFINITY;
  for (long i = threadIdx.x; i < n; i += blockDim.x) {
    const float v = 10.f * log10f(fmaxf(amin, s(i))) - refdb;
    dmx = fmaxf(dmx, v);
    dmn = fminf(dmn, v);
  }
  dmx = block_max(dmx, red);
  dmn = -block_max(-dmn, red);
  const float floor_db = dmx - 80.f;
  const float lo = fmaxf(dmn, floor_db), hi = dmx;
  const double scale = hi > lo ? 255.0 / ((double)hi - (double)lo) : 0.0;
  const double shift = -(double)lo * scale;
  for (long i = threadIdx.x; i < n; i += blockDim.x) {
    float v = 10.f * log10f(fmaxf(amin, s(i))) - refdb;
    v = fmaxf(v, floor_db);
    const float q = (float)((double)v * scale + shift);   // cv2 convertTo (double scale / shift), float result
    img[i] = (uint8_t)fminf(fmaxf(q, 0.f), 255.f);        // astype(np.uint8): truncation
  }
  __syncthreads();
  const double sx = (double)T / ow, sy = (double)n_mels / oh;
  for (int p = threadIdx.x; p < oh * ow; p += blockDim.x) {
    const int dy = p / ow, dx = p % ow;
    int x0, ax0, ax1, y0, by0, by1;
    cv_tap(dx, sx, T, x0, ax0, ax1);
    cv_tap(dy, sy, n_mels, y0, by0, by1);
    const int x1 = min(x0 + 1, T - 1), y1 = min(y0 + 1, n_mels - 1);
    const int r0 = img[y0 * T + x0] * ax0 + img[y0 * T + x1] * ax1;
    const int r1 = img[y1 * T + x0] * ax0 + img[y1 * T + x1] * ax1;
    const int v = (by0 * r0 + by1 * r1 + (1 << 21)) >> 22;
    out[(long)b * oh * ow + p] = (uint8_t)min(max(v, 0), 255);
  }
}

// gray uint8 [N, HW] -> fp32 [N, 3, HW]: the RGB conversion replicates the channel, then ToTensor + Normalize
__global__ __launch_bounds__(256) void gray_norm_kernel(const uint8_t* __restrict__ src, float* __restrict__ dst, long n,
                                                        int HW, float m0, float m1, float m2, float s0, float s1,
                                                        float s2) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const long f = i / HW, o = i % HW;
  const float x = (float)src[i] / 255.f;
  float* out = dst + f * 3 * (long)HW + o;
  out[0] = (x - m0) / s0;
  out[HW] = (x - m1) / s1;
  out[2 * (long)HW] = (x - m2) / s2;
}

// ---- train-time frame transform, PIL semantics (data_process.py:62-69 on PIL images, src/utils.py:32-33) ----
// T.Resize((h, w)) on a PIL image is Image.resize(BILINEAR): PIL's two-pass separable resampling — a triangle
// filter whose support grows with the downscale factor (antialiased), coefficients normalised per output
// pixel and rounded to 22-bit fixed point (precompute_coeffs + normalize_coeffs_8bpc; built on the host,
// media.pil_bilinear_coeffs), the width pass first into uint8, then the height pass, each output rounded
// (+2^21) and clipped to uint8.  Flips are exact; T.RandomRotation on a PIL image is Image.rotate(NEAREST,
// fill 0): the 16.16 fixed-point inverse affine walk of PIL's affine_fixed (matrix built on the host exactly as
// PIL builds it, media.pil_rotate_fixed).  Then ToTensor + Normalize.
struct PilArgs {
  int H, W, cin, oh, ow, kx, ky;
  float m[3], sd[3];
};

// width pass: src [f][H][W][cin] -> tmp [f][H][ow][cin] (uint8); one thread per output pixel of a row
__global__ __launch_bounds__(256) void pil_resize_w_kernel(const uint8_t* __restrict__ src, long frames, PilArgs a,
                                                           const int* __restrict__ xb, const int* __restrict__ xk,
                                                           uint8_t* __restrict__ tmp) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long n = frames * a.H * a.ow;
  if (i >= n) return;
  const int x = (int)(i % a.ow);
  const long fr = i / a.ow;   // (frame, row)
  const int x0 = xb[2 * x], cnt = xb[2 * x + 1];
  const int* k = xk + (long)x * a.kx;
  const uint8_t* row = src + fr * a.W * a.cin;
  int s0 = 1 << 21, s1 = 1 << 21, s2 = 1 << 21;
  for (int t = 0; t < cnt; ++t) {
    const uint8_t* px = row + (long)(x0 + t) * a.cin;
    s0 += (int)px[0] * k[t];
    if (a.cin == 3) {
      s1 += (int)px[1] * k[t];
      s2 += (int)px[2] * k[t];
    }
  }
  uint8_t* o = tmp + i * a.cin;
  o[0] = (uint8_t)min(max(s0 >> 22, 0), 255);
  if (a.cin == 3) {
    o[1] = (uint8_t)min(max(s1 >> 22, 0), 255);
    o[2] = (uint8_t)min(max(s2 >> 22, 0), 255);
  }
}

// height pass of the resized pixel (y, x) fused with flips, rotation, ToTensor and Normalize
__global__ __launch_bounds__(256) void pil_augment_kernel(const uint8_t* __restrict__ tmp, long frames, PilArgs a,
                                                          const int* __restrict__ yb, const int* __restrict__ yk,
                                                          const int* __restrict__ flips, const int* __restrict__ aff,
                                                          float* __restrict__ dst) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long per = (long)a.oh * a.ow;
  if (i >= frames * per) return;
  const long f = i / per;
  const int p = (int)(i % per), y = p / a.ow, x = p % a.ow;
  int iy = y, ix = x;
  bool in = true;
  if (aff && aff[8 * f]) {   // PIL affine_fixed: xx = a2 + x a0 + y a1, yy = a5 + x a3 + y a4 (16.16), >> 16
    const int* m = aff + 8 * f;
    const int xx = m[3] + x * m[1] + y * m[2], yy = m[6] + x * m[4] + y * m[5];
    ix = xx >> 16;
    iy = yy >> 16;
    in = ix >= 0 && ix < a.ow && iy >= 0 && iy < a.oh;
  }
  const int fl = flips ? flips[f] : 0;
  if (fl & 2) iy = a.oh - 1 - iy;   // vertical flip (applied before the rotation)
  if (fl & 1) ix = a.ow - 1 - ix;   // horizontal flip (first)
  float* out = dst + f * 3 * per + p;
  int v[3] = {0, 0, 0};
  if (in) {
    const int y0 = yb[2 * iy], cnt = yb[2 * iy + 1];
    const int* k = yk + (long)iy * a.ky;
    const uint8_t* col = tmp + (f * a.H * a.ow + ix) * a.cin;
    int s0 = 1 << 21, s1 = 1 << 21, s2 = 1 << 21;
    for (int t = 0; t < cnt; ++t) {
      const uint8_t* px = col + (long)(y0 + t) * a.ow * a.cin;
      s0 += (int)px[0] * k[t];
      if (a.cin == 3) {
        s1 += (int)px[1] * k[t];
        s2 += (int)px[2] * k[t];
      }
    }
    v[0] = min(max(s0 >> 22, 0), 255);
    v[1] = a.cin == 3 ? min(max(s1 >> 22, 0), 255) : v[0];
    v[2] = a.cin == 3 ? min(max(s2 >> 22, 0), 255) : v[0];
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) out[(long)c * per] = ((float)v[c] / 255.f - a.m[c]) / a.sd[c];
}

}  // namespace

extern "C" int64_t dfk_mel_workspace(int64_t B, int64_t S, int32_t n_fft, int32_t hop, int32_t n_mels) {
  if (B <= 0 || S <= 0 || n_fft <= 0 || hop <= 0 || n_mels <= 0) return -1;
  const long T = 1 + S / hop, Lp = S + n_fft, ldx = ((2 * (n_fft / 2 + 1) + 3) / 4) * 4;
  return 4 * (B * Lp + B * T * ldx + B * (long)n_mels * T) + 64;
}

// ceil(S_in up / down), or -1 where it is undefined or does not fit
static int64_t resample_len(int64_t S_in, int32_t up, int32_t down) {
  if (S_in <= 0 || up <= 0 || down <= 0 || S_in > (INT64_MAX - down) / up) return -1;
  return (S_in * up + down - 1) / down;
}

// periods per workgroup (about 1024 outputs) and the LDS bytes of their input span; 0 where one period's span
// does not fit the default 64 KB of dynamic LDS
static int resample_plan(int32_t up, int32_t down, int32_t ntaps, size_t* lds) {
  const int per = 1024 / up > 1 ? 1024 / up : 1;
  const long bytes = 4 * ((long)per * down + ntaps);
  *lds = (size_t)bytes;
  return bytes <= 64 * 1024 ? per : 0;
}

// lengths: null for whole rows, else the per-clip input lengths of the ragged kernel
static int resample_launch(const float* x, int64_t B, int64_t S_in, const float* taps, int32_t up, int32_t down,
                           int32_t ntaps, float* y, int64_t S_out, int64_t ldy, int pad, hipStream_t s,
                           const int64_t* lengths = nullptr) {
  size_t lds;
  const int per = resample_plan(up, down, ntaps, &lds);
  const long nblk = (S_out + (long)per * up - 1) / ((long)per * up);
  const dim3 grid((unsigned)nblk, (unsigned)B);
  if (lengths)
    hipLaunchKernelGGL(resample_kernel<true>, grid, dim3(256), lds, s, x, (long)S_in, taps, up, down, ntaps, per, y,
                       (long)S_out, (long)ldy, pad, lengths);
  else
    hipLaunchKernelGGL(resample_kernel<false>, grid, dim3(256), lds, s, x, (long)S_in, taps, up, down, ntaps, per, y,
                       (long)S_out, (long)ldy, pad, lengths);
  DFK_CHECK_LAUNCH();
  return 0;
}

static bool resample_args_ok(const float* x, int64_t B, int64_t S_in, const float* taps, int32_t up, int32_t down,
                             int32_t ntaps, int64_t S_out) {
  if (!x || !taps || B <= 0 || B > 65535 || S_in <= 0 || up <= 0 || down <= 0 || ntaps <= 0 || ntaps % 2) return false;
  if (S_out <= 0 || S_out != resample_len(S_in, up, down)) return false;
  size_t lds;
  if (!resample_plan(up, down, ntaps, &lds)) return false;
  return (S_out + 511) / 512 < (1L << 24);   // a workgroup makes more than 512 outputs: the grid stays below 2^32 threads
}

extern "C" int dfk_resample(const float* x, int64_t B, int64_t S_in, const float* taps, int32_t up, int32_t down,
                            int32_t ntaps, float* y, int64_t S_out, hipStream_t s) {
  if (!y || !resample_args_ok(x, B, S_in, taps, up, down, ntaps, S_out)) return DFK_EINVAL;
  return resample_launch(x, B, S_in, taps, up, down, ntaps, y, S_out, S_out, 0, s);
}

extern "C" int dfk_resample_ragged(const float* x, int64_t B, int64_t S_in, const int64_t* lengths, const float* taps,
                                   int32_t up, int32_t down, int32_t ntaps, float* y, int64_t S_out, hipStream_t s) {
  if (!y || !lengths || !resample_args_ok(x, B, S_in, taps, up, down, ntaps, S_out)) return DFK_EINVAL;
  return resample_launch(x, B, S_in, taps, up, down, ntaps, y, S_out, S_out, 0, s, lengths);
}

template <bool RAGGED>
static void mel_image_launch(const float* Sm, int64_t B, int32_t n_mels, long T, int32_t out_h, int32_t out_w,
                             uint8_t* out, const int64_t* lengths, int64_t S_in, int32_t up, int32_t down, int32_t hop,
                             hipStream_t s) {
  static bool lds_attr = false;   // the uint8 image may take up to 160 KB of dynamic LDS (clips past ~12 s)
  if (!lds_attr) {
    // (160 KB minus the kernel's static reduction scratch: the attribute counts dynamic LDS only)
    (void)hipFuncSetAttribute((const void*)mel_image_kernel<RAGGED>, hipFuncAttributeMaxDynamicSharedMemorySize,
                              160 * 1024 - 256);
    lds_attr = true;
  }
  hipLaunchKernelGGL(mel_image_kernel<RAGGED>, dim3((unsigned)B), dim3(1024), (size_t)n_mels * T, s, Sm, n_mels,
                     (int)T, out_h, out_w, out, lengths, (long)S_in, up, down, hop);
}

// The mel pipeline behind the entry points: argument and LDS-limit checks, `front` fills the centre-padded
// waveform yp [B][S + n_fft] (S samples at the filterbank's rate), then STFT GEMM, mel power, dB image + resize.
// lengths (ragged batches, else null): per-clip lengths of rows of S_in samples that up / down take to the
// filterbank's rate; the STFT and the mel power run over the row's T frames, the image keeps each clip's own.
template <typename Front>
static int mel_pipeline(int64_t B, int64_t S, const float* basis, const float* fbank, int32_t n_fft, int32_t hop,
                        int32_t n_mels, int32_t out_h, int32_t out_w, void* ws, int64_t ws_bytes, uint8_t* out,
                        hipStream_t s, Front front, const int64_t* lengths = nullptr, int64_t S_in = 0, int32_t up = 1,
                        int32_t down = 1) {
  if (!basis || !fbank || !ws || !out || B <= 0 || S <= 0 || n_fft <= 0 || n_fft % 4 || hop <= 0 ||
      hop % 4 || n_mels <= 0 || out_h <= 0 || out_w <= 0)
    return DFK_EINVAL;
  if (ws_bytes < dfk_mel_workspace(B, S, n_fft, hop, n_mels)) return DFK_EINVAL;
  const long T = 1 + S / hop, Lp = S + n_fft, nbin = n_fft / 2 + 1, ldx = ((2 * nbin + 3) / 4) * 4;
  if ((long)n_mels * T > 160 * 1024 - 256) return DFK_EINVAL;   // the uint8 image lives in LDS
  float* yp = reinterpret_cast<float*>(ws);
  float* X = yp + B * Lp;
  float* Sm = X + B * T * ldx;
  const int rf = front(yp, Lp);
  if (rf) return rf;
  // STFT: X[b][t][j] = sum_n yp[b][t*hop + n] basis[n][j]  (rows overlap: a strided view with ld = hop)
  dfk_gemm_args g = {};
  g.a.ptr = yp; g.a.ld = hop; g.a.bs0 = Lp;
  g.b.ptr = basis; g.b.ld = ldx;
  g.c = X; g.ldc = ldx; g.cbs0 = T * ldx;
  g.M = (int)T; g.N = (int)ldx; g.K = n_fft;
  g.dtype = DFK_F32; g.a_kmajor = 0; g.b_kmajor = 1; g.c_f32 = 1;
  g.nz0 = (int)B; g.nz1 = 1; g.splitk = 1;
  const int r = dfk_gemm(&g, s);
  if (r) return r;
  hipLaunchKernelGGL(mel_power_kernel, dim3((unsigned)T, (unsigned)B), dim3(256), 4 * nbin, s, X, ldx, (int)nbin,
                     (int)T, fbank, n_mels, Sm);
  if (lengths) mel_image_launch<true>(Sm, B, n_mels, T, out_h, out_w, out, lengths, S_in, up, down, hop, s);
  else mel_image_launch<false>(Sm, B, n_mels, T, out_h, out_w, out, nullptr, S, 1, 1, hop, s);
  DFK_CHECK_LAUNCH();
  return 0;
}

extern "C" int dfk_mel_image(const float* wave, int64_t B, int64_t S, const float* basis, const float* fbank,
                             int32_t n_fft, int32_t hop, int32_t n_mels, int32_t out_h, int32_t out_w, void* ws,
                             int64_t ws_bytes, uint8_t* out, hipStream_t s) {
  if (!wave) return DFK_EINVAL;
  return mel_pipeline(B, S, basis, fbank, n_fft, hop, n_mels, out_h, out_w, ws, ws_bytes, out, s,
                      [&](float* yp, long Lp) {
                        hipLaunchKernelGGL(mel_pad_kernel<false>, dim3((unsigned)dfk_cdiv(Lp, 256), (unsigned)B),
                                           dim3(256), 0, s, wave, (long)S, n_fft / 2, Lp, yp, (const int64_t*)nullptr);
                        DFK_CHECK_LAUNCH();
                        return 0;
                      });
}

extern "C" int64_t dfk_mel_resampled_workspace(int64_t B, int64_t S_in, int32_t up, int32_t down, int32_t n_fft,
                                               int32_t hop, int32_t n_mels) {
  const int64_t S = resample_len(S_in, up, down);
  return S < 0 ? -1 : dfk_mel_workspace(B, S, n_fft, hop, n_mels);
}

extern "C" int dfk_mel_image_resampled(const float* wave, int64_t B, int64_t S_in, const float* taps, int32_t up,
                                       int32_t down, int32_t ntaps, int64_t S_out, const float* basis,
                                       const float* fbank, int32_t n_fft, int32_t hop, int32_t n_mels, int32_t out_h,
                                       int32_t out_w, void* ws, int64_t ws_bytes, uint8_t* out, hipStream_t s) {
  if (!resample_args_ok(wave, B, S_in, taps, up, down, ntaps, S_out)) return DFK_EINVAL;
  return mel_pipeline(B, S_out, basis, fbank, n_fft, hop, n_mels, out_h, out_w, ws, ws_bytes, out, s,
                      [&](float* yp, long Lp) {
                        return resample_launch(wave, B, S_in, taps, up, down, ntaps, yp, S_out, Lp, n_fft / 2, s);
                      });
}

extern "C" int dfk_mel_image_ragged(const float* wave, int64_t B, int64_t S, const int64_t* lengths, const float* taps,
                                    int32_t up, int32_t down, int32_t ntaps, const float* basis, const float* fbank,
                                    int32_t n_fft, int32_t hop, int32_t n_mels, int32_t out_h, int32_t out_w, void* ws,
                                    int64_t ws_bytes, uint8_t* out, hipStream_t s) {
  if (!wave || !lengths || B > 65535) return DFK_EINVAL;
  if (!taps) {   // plain path: the rows are at the filterbank's rate
    if (up != 1 || down != 1 || ntaps != 0) return DFK_EINVAL;
    return mel_pipeline(
        B, S, basis, fbank, n_fft, hop, n_mels, out_h, out_w, ws, ws_bytes, out, s,
        [&](float* yp, long Lp) {
          hipLaunchKernelGGL(mel_pad_kernel<true>, dim3((unsigned)dfk_cdiv(Lp, 256), (unsigned)B), dim3(256), 0, s,
                             wave, (long)S, n_fft / 2, Lp, yp, lengths);
          DFK_CHECK_LAUNCH();
          return 0;
        },
        lengths, S, 1, 1);
  }
  const int64_t S_out = resample_len(S, up, down);
  if (!resample_args_ok(wave, B, S, taps, up, down, ntaps, S_out)) return DFK_EINVAL;
  return mel_pipeline(
      B, S_out, basis, fbank, n_fft, hop, n_mels, out_h, out_w, ws, ws_bytes, out, s,
      [&](float* yp, long Lp) {
        return resample_launch(wave, B, S, taps, up, down, ntaps, yp, S_out, Lp, n_fft / 2, s, lengths);
      },
      lengths, S, up, down);
}

extern "C" int dfk_gray_normalize(const uint8_t* src, float* dst, int64_t n_img, int32_t H, int32_t W, const float* mean3,
                                  const float* std3, hipStream_t s) {
  if (!src || !dst || !mean3 || !std3 || H <= 0 || W <= 0) return DFK_EINVAL;
  const long n = n_img * (long)H * W;
  if (n <= 0) return 0;
  hipLaunchKernelGGL(gray_norm_kernel, dim3((unsigned)dfk_cdiv(n, 256)), dim3(256), 0, s, src, dst, n, H * W, mean3[0],
                     mean3[1], mean3[2], std3[0], std3[1], std3[2]);
  DFK_CHECK_LAUNCH();
  return 0;
}

extern "C" int dfk_frame_augment(const uint8_t* src, int64_t frames, const dfk_pil_resize* rs, const int32_t* flips,
                                 const int32_t* affine, const float* mean3, const float* std3, uint8_t* tmp, float* dst,
                                 hipStream_t s) {
  if (!src || !rs || !dst || !tmp || !mean3 || !std3) return DFK_EINVAL;
  const dfk_pil_resize& r = *rs;
  if (r.H <= 0 || r.W <= 0 || r.out_h <= 0 || r.out_w <= 0 || (r.cin != 1 && r.cin != 3)) return DFK_EINVAL;
  if (!r.xb || !r.xk || !r.yb || !r.yk || r.kx <= 0 || r.ky <= 0) return DFK_EINVAL;
  if (frames <= 0) return 0;
  PilArgs a;
  a.H = r.H; a.W = r.W; a.cin = r.cin; a.oh = r.out_h; a.ow = r.out_w; a.kx = r.kx; a.ky = r.ky;
  for (int c = 0; c < 3; ++c) { a.m[c] = mean3[c]; a.sd[c] = std3[c]; }
  const long nw = frames * (long)r.H * r.out_w;
  hipLaunchKernelGGL(pil_resize_w_kernel, dim3((unsigned)dfk_cdiv(nw, 256)), dim3(256), 0, s, src, (long)frames, a,
                     r.xb, r.xk, tmp);
  const long n = frames * (long)r.out_h * r.out_w;
  hipLaunchKernelGGL(pil_augment_kernel, dim3((unsigned)dfk_cdiv(n, 256)), dim3(256), 0, s, tmp, (long)frames, a,
                     r.yb, r.yk, flips, affine, dst);
  DFK_CHECK_LAUNCH();
  return 0;
}
