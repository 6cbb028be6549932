// The optimizer: fused SGD and AdamW steps over the flat fp32 parameter store (one run per launch, or every run of
// the step in one launch through a by-value run table, also with a learning-rate multiplier and a weight decay per
// parameter group looked up per quad) and global gradient-norm clipping.  All HBM-bound: 16-B
// quads of the fp32 buffers, 8-B quads of the bf16 ones, the n % 4 tail of a run one element at a time.
// Shared by every kernel here:
//   gate: a LayerDrop-skipped layer (*gate == 0) is left untouched, as torch skips grad=None parameters.
//   Data-parallel fold (gscale, gbf): the gradient read is the all-reduced SUM — the fp32 buffer itself, or the
//   bf16 bucket copy RCCL summed (gbf != NULL) — times gscale = 1 / world, so no separate averaging / cast-back
//   pass over the flat gradient runs between the last all-reduce and the step (ddp.py GradBucketer.finish(fold)).
//   CLIP (the dfk_*_clip entry points): the gradient is also multiplied by coef = *clip, the global-norm
//   coefficient grad_clip_coef_kernel wrote (torch.nn.utils.clip_grad_norm_ on the mean gradient).
#include <math.h>

#include <initializer_list>

#include "common.h"

namespace {

// All runs of one step in one launch (the *_runs entry points): the run table travels by value in the kernel
// arguments (no device table to keep alive across graph replays); a workgroup owns kRunBlock consecutive elements
// of one run (two quads per thread, so each wave keeps 2x the bytes of the one-run kernels in flight).
constexpr int kRunBlock = 2048;
constexpr int kMaxRuns = 64;
struct RunTable {
  int64_t start[kMaxRuns], n[kMaxRuns];
  const float* gate[kMaxRuns];
  int32_t prefix[kMaxRuns + 1];       // first workgroup of each run; prefix[nruns] = the grid
  int32_t nruns;
};
struct SgdRuns : RunTable {
  uint64_t first;                     // bit r: run r takes its first momentum step
};
struct AdamwRuns : RunTable {
  uint8_t cls[kMaxRuns];              // gate class of each run (its pair in corr)
};
static_assert(sizeof(SgdRuns) + 128 <= 4096 && sizeof(AdamwRuns) + 128 <= 4096,
              "run table + the other arguments must fit the kernel-argument block");

// The table of the host array runs[nruns][4] = {start, n, gate pointer, the caller's own field}, 1 <= nruns <=
// kMaxRuns.  False for a run that is empty or does not start on a non-negative multiple of 4 elements, or when the
// workgroups do not fit an int32 grid.
bool fill_run_table(RunTable& T, const int64_t* runs, int32_t nruns) {
  T.nruns = nruns;
  int64_t blocks = 0;
  for (int r = 0; r < nruns; ++r) {
    const int64_t* e = runs + 4 * r;
    if (e[1] <= 0 || e[0] < 0 || (e[0] & 3)) return false;
    T.start[r] = e[0];
    T.n[r] = e[1];
    T.gate[r] = reinterpret_cast<const float*>(e[2]);
    T.prefix[r] = (int32_t)blocks;
    blocks += (e[1] + kRunBlock - 1) / kRunBlock;
    if (blocks > 0x7fffffffL) return false;
  }
  T.prefix[nruns] = (int32_t)blocks;
  return true;
}

// The alignment the quads need: 16 B for the fp32 buffers, 8 B for the bf16 ones (NULL, an absent buffer, passes)
bool misaligned(std::initializer_list<const void*> f32, std::initializer_list<const void*> b16) {
  uintptr_t a = 0, b = 0;
  for (const void* p : f32) a |= reinterpret_cast<uintptr_t>(p);
  for (const void* p : b16) b |= reinterpret_cast<uintptr_t>(p);
  return (a & 15) || (b & 7);
}

// the run r with prefix[r] <= block < prefix[r + 1]
__device__ __forceinline__ int find_run(const int32_t* prefix, int nruns, int block) {
  int lo = 0, hi = nruns - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (prefix[mid] <= block) lo = mid; else hi = mid - 1;
  }
  return lo;
}

__device__ __forceinline__ float4 ld_grad4(const float* grad, const bf16raw* gbf, long i) {
  if (gbf) {
    const uint2 u = *reinterpret_cast<const uint2*>(gbf + i);
    return make_float4(__uint_as_float(u.x << 16), __uint_as_float(u.x & 0xffff0000u), __uint_as_float(u.y << 16),
                       __uint_as_float(u.y & 0xffff0000u));
  }
  return *reinterpret_cast<const float4*>(grad + i);
}

__device__ __forceinline__ void st_shadow4(bf16raw* shadow, long i, const float4& p) {
  const float* pp = reinterpret_cast<const float*>(&p);
  uint2 w;
  bf16raw* e = reinterpret_cast<bf16raw*>(&w);
#pragma unroll
  for (int k = 0; k < 4; ++k) e[k] = f2bf(pp[k]);
  *reinterpret_cast<uint2*>(shadow + i) = w;
}

// torch.optim.SGD semantics (momentum, dampening 0, weight decay, no nesterov):
//   g = grad * gscale + wd*p ; buf = first ? g : mom*buf + g ; p -= lr*buf ; shadow = bf16(p)
// The gradient is one fma onto the rounded wd * p, g = fma(grad, gmul, round(wd * p)) with gmul = gscale.  It is
// spelled out: left to contraction, the compiler chooses per call site which product of grad * gscale + wd * p it
// fuses, or neither (a packed multiply and an add in the tail), and the one-run, the one-launch and the CLIP kernels
// must agree bit for bit.  CLIP: the product gscale * coef is rounded once per workgroup and is gmul, so with
// coef == 1 the CLIP kernels give the non-clip kernels' bits at every gscale.
// Non-temporal stores of p / buf / shadow were tried and had no measurable effect on the step or on the next step's
// patch embedding (profiles/step/r4p_conv3d_instep_diagnosis.txt).
struct SgdRun {                       // the buffers of one run and its per-step scalars
  float* p;
  const float* grad;
  float* buf;
  bf16raw* shadow;
  const bf16raw* gbf;
  long n;
  float lr, mom, wd;
  float gmul;                         // gscale, times the clip coefficient in the CLIP kernels
  int first;
};

struct SgdQuad {
  float4 p, g, b;
};

__device__ __forceinline__ void sgd_elem(float& p, float& b, float g, const SgdRun& r) {
  g = __builtin_fmaf(g, r.gmul, r.wd * p);
  b = r.first ? g : r.mom * b + g;
  p -= r.lr * b;
}

// 4 elements at i (i + 4 <= n): the 16-B loads, then the update and the 16-B stores (8-B for the shadow)
__device__ __forceinline__ void sgd_load4(const SgdRun& r, long i, SgdQuad& q) {
  q.p = *reinterpret_cast<const float4*>(r.p + i);
  q.g = ld_grad4(r.grad, r.gbf, i);
  q.b = r.first ? make_float4(0, 0, 0, 0) : *reinterpret_cast<const float4*>(r.buf + i);
}

__device__ __forceinline__ void sgd_update4(const SgdRun& r, long i, SgdQuad& q) {
  float* pp = reinterpret_cast<float*>(&q.p);
  const float* gg = reinterpret_cast<const float*>(&q.g);
  float* bb = reinterpret_cast<float*>(&q.b);
#pragma unroll
  for (int k = 0; k < 4; ++k) sgd_elem(pp[k], bb[k], gg[k], r);
  *reinterpret_cast<float4*>(r.p + i) = q.p;
  *reinterpret_cast<float4*>(r.buf + i) = q.b;
  if (r.shadow) st_shadow4(r.shadow, i, q.p);
}

// the run's last n - i < 4 elements, one by one
__device__ __forceinline__ void sgd_tail(const SgdRun& r, long i) {
  for (; i < r.n; ++i) {
    sgd_elem(r.p[i], r.buf[i], r.gbf ? bf2f(r.gbf[i]) : r.grad[i], r);
    if (r.shadow) r.shadow[i] = f2bf(r.p[i]);
  }
}

// one run
template <bool CLIP>
__global__ void sgd_kernel(float* __restrict__ p, const float* __restrict__ grad, float* __restrict__ buf,
                           bf16raw* __restrict__ shadow, long n, const float* __restrict__ lr_dev, float lr_host,
                           float mom, float wd, int first, const float* __restrict__ gate, float gscale,
                           const bf16raw* __restrict__ gbf, const float* __restrict__ clip) {
  const long i0 = ((long)blockIdx.x * blockDim.x + threadIdx.x) * 4;
  if (i0 >= n) return;
  if (gate && *gate == 0.f) return;
  const float lr = lr_dev ? *lr_dev : lr_host;
  float gmul = gscale;
  if constexpr (CLIP) gmul = gscale * *clip;
  const SgdRun r{p, grad, buf, shadow, gbf, n, lr, mom, wd, gmul, first};
  if (i0 + 4 <= n) {
    SgdQuad q;
    sgd_load4(r, i0, q);
    sgd_update4(r, i0, q);
  } else {
    sgd_tail(r, i0);
  }
}

template <bool CLIP>
__global__ __launch_bounds__(256) void sgd_runs_kernel(float* __restrict__ P, const float* __restrict__ G,
                                                       float* __restrict__ Bf, bf16raw* __restrict__ S,
                                                       const SgdRuns R, const float* __restrict__ lr_dev,
                                                       float lr_host, float mom, float wd, float gscale,
                                                       const bf16raw* __restrict__ GB,
                                                       const float* __restrict__ clip) {
  const int b = blockIdx.x;
  const int run = find_run(R.prefix, R.nruns, b);
  const long start = R.start[run], n = R.n[run];
  const float* gate = R.gate[run];
  const int first = (int)((R.first >> run) & 1);
  if (gate && *gate == 0.f) return;
  const float lr = lr_dev ? *lr_dev : lr_host;
  float gmul = gscale;
  if constexpr (CLIP) gmul = gscale * *clip;
  const SgdRun r{P + start, G + start, Bf + start, S ? S + start : nullptr, GB ? GB + start : nullptr, n, lr, mom, wd,
                 gmul, first};
  const long base = (long)(b - R.prefix[run]) * kRunBlock;
  const long idx[2] = {base + threadIdx.x * 4, base + 1024 + threadIdx.x * 4};
  SgdQuad q[2];
  bool full[2];
#pragma unroll
  for (int u = 0; u < 2; ++u) {     // both quads' loads in flight before the first update
    full[u] = idx[u] + 4 <= n;
    if (full[u]) sgd_load4(r, idx[u], q[u]);
  }
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    if (full[u]) sgd_update4(r, idx[u], q[u]);
    else sgd_tail(r, idx[u]);                  // empty when idx[u] >= n
  }
}

// torch.optim.AdamW semantics (amsgrad / maximize off), per element with g = grad * gscale:
//   p *= 1 - lr*wd ; m = m + (1-b1)(g - m) ; v = b2*v + ((1-b2) g) g ; p -= (lr*c1) m / (sqrt(v)*c2 + eps)
// c1 = 1/(1-b1^t), c2 = 1/sqrt(1-b2^t) come from adamw_prelude_kernel (evaluated in double, stored fp32, one pair
// per gate class).  The roundings follow torch's CPU kernels (lerp_ as one fma, addcmul_ as one fma onto the
// rounded b2*v, then separate multiply / divide / add): an fp32 emulation of this sequence reproduces torch's m and
// v bit for bit, and p except where the fp32 lr * c1 rounds differently from torch's double lr / (1-b1^t).
// Contraction is off so that the compiler forms no further fma.
// CLIP: g = (grad * gscale) * coef, two rounded multiplies as torch's clip_grad_norm_ leaves grad.mul_(coef)
// behind; coef == 1 gives the non-clip kernels' bits.
struct AdamwHyper {
  float omb1, b2, omb2, eps, wd, gscale;   // 1-b1 and 1-b2 are rounded from double on the host
};

template <bool CLIP>
__device__ __forceinline__ void adamw_elem(float& p, float& m, float& v, float g, float decay, float step, float c2,
                                           float coef, const AdamwHyper& h) {
#pragma clang fp contract(off)
  g = g * h.gscale;
  if constexpr (CLIP) g = g * coef;
  p = p * decay;
  m = __builtin_fmaf(h.omb1, g - m, m);
  const float vb = v * h.b2;
  v = __builtin_fmaf(h.omb2 * g, g, vb);
  const float den = __builtin_sqrtf(v) * c2 + h.eps;
  p = p - (step * m) / den;
}

// The buffers of one run and its per-step scalars
struct AdamwRun {
  float* p;
  const float* grad;
  float *m, *v;
  bf16raw* shadow;
  const bf16raw* gbf;
  long n;
  float decay, step, c2;
  float coef;   // the clip coefficient (CLIP kernels only)
};

struct AdamwQuad {
  float4 p, g, m, v;
};

// as sgd_load4 / sgd_update4 / sgd_tail
__device__ __forceinline__ void adamw_load4(const AdamwRun& r, long i, AdamwQuad& q) {
  q.p = *reinterpret_cast<const float4*>(r.p + i);
  q.g = ld_grad4(r.grad, r.gbf, i);
  q.m = *reinterpret_cast<const float4*>(r.m + i);
  q.v = *reinterpret_cast<const float4*>(r.v + i);
}

template <bool CLIP>
__device__ __forceinline__ void adamw_update4(const AdamwRun& r, long i, AdamwQuad& q, const AdamwHyper& h) {
  float* pp = reinterpret_cast<float*>(&q.p);
  const float* gg = reinterpret_cast<const float*>(&q.g);
  float* mm = reinterpret_cast<float*>(&q.m);
  float* vq = reinterpret_cast<float*>(&q.v);
#pragma unroll
  for (int k = 0; k < 4; ++k) adamw_elem<CLIP>(pp[k], mm[k], vq[k], gg[k], r.decay, r.step, r.c2, r.coef, h);
  *reinterpret_cast<float4*>(r.p + i) = q.p;
  *reinterpret_cast<float4*>(r.m + i) = q.m;
  *reinterpret_cast<float4*>(r.v + i) = q.v;
  if (r.shadow) st_shadow4(r.shadow, i, q.p);
}

template <bool CLIP>
__device__ __forceinline__ void adamw_tail(const AdamwRun& r, long i, const AdamwHyper& h) {
  for (; i < r.n; ++i) {
    float pe = r.p[i], me = r.m[i], ve = r.v[i];
    adamw_elem<CLIP>(pe, me, ve, r.gbf ? bf2f(r.gbf[i]) : r.grad[i], r.decay, r.step, r.c2, r.coef, h);
    r.p[i] = pe;
    r.m[i] = me;
    r.v[i] = ve;
    if (r.shadow) r.shadow[i] = f2bf(pe);
  }
}

// Step counts and bias corrections, once per optimizer step ahead of the update kernels: thread i owns class
// C.cls[i]; unless the class is gated off (*gate == 0) its counter advances, t = ++counters[cls], and
// corr[2 cls] = 1/(1-b1^t), corr[2 cls + 1] = 1/sqrt(1-b2^t) in double through -expm1(t log b) (1 - 0.999^t formed
// in fp32 keeps three digits at small t).  A gated-off class keeps its counter and its (unused) corrections.
constexpr int kAdamwMaxClasses = 64;
struct AdamwClasses {
  const float* gate[kAdamwMaxClasses];
  int32_t cls[kAdamwMaxClasses];
  int32_t n;
};

__global__ void adamw_prelude_kernel(int32_t* __restrict__ counters, float* __restrict__ corr, const AdamwClasses C,
                                     double log_b1, double log_b2) {
  const int i = threadIdx.x;
  if (i >= C.n) return;
  const float* gate = C.gate[i];
  if (gate && *gate == 0.f) return;
  const int c = C.cls[i];
  const int t = counters[c] + 1;
  counters[c] = t;
  corr[2 * c] = (float)(1.0 / -expm1((double)t * log_b1));
  corr[2 * c + 1] = (float)(1.0 / sqrt(-expm1((double)t * log_b2)));
}

// one run; corr points at its class's {c1, c2}
template <bool CLIP>
__global__ void adamw_kernel(float* __restrict__ p, const float* __restrict__ grad, float* __restrict__ m,
                             float* __restrict__ v, bf16raw* __restrict__ shadow, long n,
                             const float* __restrict__ lr_dev, float lr_host, const AdamwHyper h,
                             const float* __restrict__ corr, const float* __restrict__ gate,
                             const bf16raw* __restrict__ gbf, const float* __restrict__ clip) {
  const long i0 = ((long)blockIdx.x * blockDim.x + threadIdx.x) * 4;
  if (i0 >= n) return;
  if (gate && *gate == 0.f) return;
  const float lr = lr_dev ? *lr_dev : lr_host;
  float coef = 1.f;
  if constexpr (CLIP) coef = *clip;
  const AdamwRun r{p, grad, m, v, shadow, gbf, n, (float)(1.0 - (double)lr * (double)h.wd), lr * corr[0], corr[1],
                   coef};
  if (i0 + 4 <= n) {
    AdamwQuad q;
    adamw_load4(r, i0, q);
    adamw_update4<CLIP>(r, i0, q, h);
  } else {
    adamw_tail<CLIP>(r, i0, h);
  }
}

template <bool CLIP>
__global__ __launch_bounds__(256) void adamw_runs_kernel(float* __restrict__ P, const float* __restrict__ G,
                                                         float* __restrict__ M, float* __restrict__ V,
                                                         bf16raw* __restrict__ S, const AdamwRuns R,
                                                         const float* __restrict__ lr_dev, float lr_host,
                                                         const AdamwHyper h, const float* __restrict__ corr,
                                                         const bf16raw* __restrict__ GB,
                                                         const float* __restrict__ clip) {
  const int b = blockIdx.x;
  const int run = find_run(R.prefix, R.nruns, b);
  const long start = R.start[run], n = R.n[run];
  const float* gate = R.gate[run];
  if (gate && *gate == 0.f) return;
  const float* cr = corr + 2 * R.cls[run];
  const float lr = lr_dev ? *lr_dev : lr_host;
  float coef = 1.f;
  if constexpr (CLIP) coef = *clip;
  const AdamwRun r{P + start, G + start, M + start, V + start, S ? S + start : nullptr, GB ? GB + start : nullptr,
                   n, (float)(1.0 - (double)lr * (double)h.wd), lr * cr[0], cr[1], coef};
  const long base = (long)(b - R.prefix[run]) * kRunBlock;
  const long idx[2] = {base + threadIdx.x * 4, base + 1024 + threadIdx.x * 4};
  AdamwQuad q[2];
  bool full[2];
#pragma unroll
  for (int u = 0; u < 2; ++u) {     // both quads' loads in flight before the first update
    full[u] = idx[u] + 4 <= n;
    if (full[u]) adamw_load4(r, idx[u], q[u]);
  }
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    if (full[u]) adamw_update4<CLIP>(r, idx[u], q[u], h);
    else adamw_tail<CLIP>(r, idx[u], h);       // empty when idx[u] >= n
  }
}

// Parameter groups (the dfk_*_step_runs_groups entry points): the twins of sgd_runs_kernel / adamw_runs_kernel with
// the learning-rate multiplier and the weight decay looked up per quad instead of taken from the launch arguments, so
// that groups which alternate tensor by tensor along the store do not split the runs.
//   map:   one byte per 8 elements of the store (every parameter starts on a multiple of 8, run starts and quads on
//          multiples of 4: a quad lies in one cell; alignment padding shares the byte of the tensor it follows and
//          holds p = g = m = v = 0, which stays 0 under any pair).  The byte is clamped to the table's last row: no
//          value in that device array can take a read outside `hyper`.
//   hyper: fp32 [ngroups][2] = {lr_mult, weight_decay} in device memory, read at every launch (a value changed
//          between two replays of a captured step takes effect).
// lr_e = lr * lr_mult is one rounded multiply (lr_mult == 1 gives lr's bits); given equal scalars the per-element
// sequence is the plain kernels' own (the same *_load4 / *_update4 / *_tail), so one group is bit-equal to the twin.
// The map bytes are issued ahead of the 16-B streams (with no branch around them, so nothing waits in between) and
// the pair loads they select behind the streams.  As compiled, the per-quad branches around the streams make the wait
// in front of the pair loads cover most of the streams too; a whole-block path without those branches, where the
// pairs go out under the streams, measured the same on the C2 store (profiles/optim/groups_timing.md).
struct GroupTab {
  const uint8_t* map;
  const float* hyper;
  int32_t last;                       // ngroups - 1
};

__device__ __forceinline__ float2 group_pair(const GroupTab& T, int byte) {
  return *reinterpret_cast<const float2*>(T.hyper + 2 * min(byte, T.last));
}

__device__ __forceinline__ float group_lr(float lr, float mult) {
#pragma clang fp contract(off)
  return lr * mult;
}

__device__ __forceinline__ SgdRun sgd_group_run(SgdRun r, float lr, float2 hy) {
  r.lr = group_lr(lr, hy.x);
  r.wd = hy.y;
  return r;
}

template <bool CLIP>
__global__ __launch_bounds__(256) void sgd_runs_groups_kernel(float* __restrict__ P, const float* __restrict__ G,
                                                              float* __restrict__ Bf, bf16raw* __restrict__ S,
                                                              const SgdRuns R, const float* __restrict__ lr_dev,
                                                              float lr_host, float mom, float gscale,
                                                              const bf16raw* __restrict__ GB,
                                                              const float* __restrict__ clip, const GroupTab T) {
  const int b = blockIdx.x;
  const int run = find_run(R.prefix, R.nruns, b);
  const long start = R.start[run], n = R.n[run];
  const float* gate = R.gate[run];
  const int first = (int)((R.first >> run) & 1);
  if (gate && *gate == 0.f) return;
  const float lr = lr_dev ? *lr_dev : lr_host;
  float gmul = gscale;
  if constexpr (CLIP) gmul = gscale * *clip;
  const SgdRun r{P + start, G + start, Bf + start, S ? S + start : nullptr, GB ? GB + start : nullptr, n, 0.f, mom,
                 0.f, gmul, first};                      // lr and wd come per quad
  const long base = (long)(b - R.prefix[run]) * kRunBlock;
  const long idx[2] = {base + threadIdx.x * 4, base + 1024 + threadIdx.x * 4};
  SgdQuad q[2];
  bool full[2];
  int byte[2];
  float2 hy[2];
#pragma unroll
  for (int u = 0; u < 2; ++u) {     // the map bytes, then both quads' loads, then the pairs the bytes select
    full[u] = idx[u] + 4 <= n;
    byte[u] = T.map[(start + (full[u] ? idx[u] : 0)) >> 3];   // no branch around it: the run's first cell otherwise
  }
#pragma unroll
  for (int u = 0; u < 2; ++u)
    if (full[u]) sgd_load4(r, idx[u], q[u]);
#pragma unroll
  for (int u = 0; u < 2; ++u)
    if (full[u]) hy[u] = group_pair(T, byte[u]);
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    if (full[u]) {
      sgd_update4(sgd_group_run(r, lr, hy[u]), idx[u], q[u]);
    } else {
      for (long i = idx[u]; i < n; ++i) {        // the tail: each element takes the byte of its own index
        SgdRun e = sgd_group_run(r, lr, group_pair(T, T.map[(start + i) >> 3]));
        e.n = i + 1;
        sgd_tail(e, i);
      }
    }
  }
}

__device__ __forceinline__ AdamwRun adamw_group_run(AdamwRun r, float lr, float c1, float2 hy) {
#pragma clang fp contract(off)
  const float lr_e = group_lr(lr, hy.x);
  r.decay = (float)(1.0 - (double)lr_e * (double)hy.y);
  r.step = lr_e * c1;
  return r;
}

template <bool CLIP>
__global__ __launch_bounds__(256) void adamw_runs_groups_kernel(float* __restrict__ P, const float* __restrict__ G,
                                                                float* __restrict__ M, float* __restrict__ V,
                                                                bf16raw* __restrict__ S, const AdamwRuns R,
                                                                const float* __restrict__ lr_dev, float lr_host,
                                                                const AdamwHyper h, const float* __restrict__ corr,
                                                                const bf16raw* __restrict__ GB,
                                                                const float* __restrict__ clip, const GroupTab T) {
  const int b = blockIdx.x;
  const int run = find_run(R.prefix, R.nruns, b);
  const long start = R.start[run], n = R.n[run];
  const float* gate = R.gate[run];
  if (gate && *gate == 0.f) return;
  const float* cr = corr + 2 * R.cls[run];
  const float lr = lr_dev ? *lr_dev : lr_host;
  const float c1 = cr[0];
  float coef = 1.f;
  if constexpr (CLIP) coef = *clip;
  const AdamwRun r{P + start, G + start, M + start, V + start, S ? S + start : nullptr, GB ? GB + start : nullptr,
                   n, 1.f, 0.f, cr[1], coef};            // decay and step come per quad
  const long base = (long)(b - R.prefix[run]) * kRunBlock;
  const long idx[2] = {base + threadIdx.x * 4, base + 1024 + threadIdx.x * 4};
  AdamwQuad q[2];
  bool full[2];
  int byte[2];
  float2 hy[2];
#pragma unroll
  for (int u = 0; u < 2; ++u) {     // as sgd_runs_groups_kernel
    full[u] = idx[u] + 4 <= n;
    byte[u] = T.map[(start + (full[u] ? idx[u] : 0)) >> 3];
  }
#pragma unroll
  for (int u = 0; u < 2; ++u)
    if (full[u]) adamw_load4(r, idx[u], q[u]);
#pragma unroll
  for (int u = 0; u < 2; ++u)
    if (full[u]) hy[u] = group_pair(T, byte[u]);
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    if (full[u]) {
      adamw_update4<CLIP>(adamw_group_run(r, lr, c1, hy[u]), idx[u], q[u], h);
    } else {
      for (long i = idx[u]; i < n; ++i) {
        AdamwRun e = adamw_group_run(r, lr, c1, group_pair(T, T.map[(start + i) >> 3]));
        e.n = i + 1;
        adamw_tail<CLIP>(e, i, h);
      }
    }
  }
}

// Global gradient norm (torch.nn.utils.clip_grad_norm_, norm_type 2), stage 1: sum of (g * gscale)^2 over the
// runs of the step, g read as the update kernels read it (fp32, or the bf16 bucket copy).  A fixed grid of
// kGnormPartials persistent workgroups; workgroup w owns the kRunBlock-element blocks w, w + kGnormPartials, ...
// of the step's block list (the blocks of run 0, then of run 1, ...: sgd_runs_kernel's numbering), two 16-B quads
// (8-B with bf16) per thread and block, both loads issued before the arithmetic.  Every element is converted to
// double, scaled and accumulated with one fp64 fma; lanes, waves and workgroups are summed in double in a fixed
// order, and each workgroup stores exactly one partial — zero when it had no block — so the slab never holds a
// value of an earlier call and the result does not depend on scheduling.  A run whose gate reads 0 is not read.
constexpr int kGnormPartials = DFK_GNORM_PARTIALS;

__device__ __forceinline__ double sq_acc(float x, double gs, double acc) {
  const double d = (double)x * gs;
  return __builtin_fma(d, d, acc);
}

template <bool BF>   // BF: the gradient is the bf16 bucket copy
__global__ __launch_bounds__(256) void grad_sqnorm_runs_kernel(const float* __restrict__ G,
                                                               const bf16raw* __restrict__ GB, const RunTable R,
                                                               float gscale, double* __restrict__ partials) {
  __shared__ double red[4];
  const long total = R.prefix[R.nruns];
  const double gs = (double)gscale;
  double acc = 0.0;
  int lo = -1;
  long first = 0, next = 0, n = 0;                 // the current run's first block, the next run's, its length
  const float* grad = G;
  const bf16raw* gbf = GB;
  bool open = false;
  for (long b = blockIdx.x; b < total; b += kGnormPartials) {
    if (b >= next) {                               // blocks ascend: the run index only moves forward
      do ++lo; while (b >= R.prefix[lo + 1]);
      first = R.prefix[lo];
      next = R.prefix[lo + 1];
      n = R.n[lo];
      grad = G + R.start[lo];
      gbf = GB + R.start[lo];                      // used only when BF
      const float* gate = R.gate[lo];
      open = !(gate && *gate == 0.f);
    }
    if (!open) continue;
    const long base = (b - first) * kRunBlock;
    const long idx[2] = {base + threadIdx.x * 4, base + 1024 + threadIdx.x * 4};
    if (base + kRunBlock <= n) {                   // a whole block: both loads in flight, no per-quad branch
      const float4 v0 = ld_grad4(grad, BF ? gbf : nullptr, idx[0]);
      const float4 v1 = ld_grad4(grad, BF ? gbf : nullptr, idx[1]);
      acc = sq_acc(v0.x, gs, acc);
      acc = sq_acc(v0.y, gs, acc);
      acc = sq_acc(v0.z, gs, acc);
      acc = sq_acc(v0.w, gs, acc);
      acc = sq_acc(v1.x, gs, acc);
      acc = sq_acc(v1.y, gs, acc);
      acc = sq_acc(v1.z, gs, acc);
      acc = sq_acc(v1.w, gs, acc);
      continue;
    }
#pragma unroll
    for (int u = 0; u < 2; ++u) {                  // the run's last block: quads while they fit, then the n % 4 tail
      if (idx[u] + 4 <= n) {
        const float4 v = ld_grad4(grad, BF ? gbf : nullptr, idx[u]);
        acc = sq_acc(v.x, gs, acc);
        acc = sq_acc(v.y, gs, acc);
        acc = sq_acc(v.z, gs, acc);
        acc = sq_acc(v.w, gs, acc);
      } else {
        for (long i = idx[u]; i < n; ++i) acc = sq_acc(BF ? bf2f(gbf[i]) : grad[i], gs, acc);
      }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) partials[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// Stage 2, one workgroup: the n partials summed in a fixed order in double, then in fp32 as torch does it
// norm = sqrt(sum), coef = min(1, max_norm / (norm + 1e-6)).  No special case for a non-finite norm: an infinite
// one gives coef 0, a NaN one stays NaN through the comparison (torch.clamp keeps NaN where fminf would return 1).
__global__ __launch_bounds__(256) void grad_clip_coef_kernel(const double* __restrict__ partials, int n,
                                                             float max_norm, float* __restrict__ out) {
  __shared__ double red[256];
  const int t = threadIdx.x;
  double s = 0.0;
  for (int i = t; i < n; i += 256) s += partials[i];
  red[t] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (t < o) red[t] += red[t + o];
    __syncthreads();
  }
  if (t == 0) {
    const float norm = (float)sqrt(red[0]);
    const float c = max_norm / (norm + 1e-6f);
    out[0] = norm;
    out[1] = c > 1.f ? 1.f : c;
  }
}

// ---- host side.  clip: the coefficient of a _clip entry point, NULL from the plain one (which launches the non-clip
// kernels).  A plain entry point passes straight through; its _clip twin first applies its own stricter rules. ----
int sgd_step_impl(float* param, const float* grad, float* momentum_buf, void* bf16_shadow, int64_t n,
                  const float* lr_dev, float lr, float momentum, float weight_decay, int first_step,
                  const float* gate, float grad_scale, const void* grad_bf16, const float* clip, hipStream_t s) {
  if (!param || !grad || !momentum_buf) return DFK_EINVAL;
  if (misaligned({param, grad, momentum_buf}, {grad_bf16, bf16_shadow})) return DFK_EINVAL;
  if (n <= 0) return 0;
  const long threads = (n + 3) / 4;
  hipLaunchKernelGGL(clip ? sgd_kernel<true> : sgd_kernel<false>, dim3((unsigned)((threads + 255) / 256)), dim3(256),
                     0, s, param, grad, momentum_buf, (bf16raw*)bf16_shadow, (long)n, lr_dev, lr, momentum,
                     weight_decay, first_step, gate, grad_scale, (const bf16raw*)grad_bf16, clip);
  DFK_CHECK_LAUNCH();
  return 0;
}

int sgd_step_runs_impl(float* param, const float* grad, float* momentum_buf, void* bf16_shadow, const int64_t* runs,
                       int32_t nruns, const float* lr_dev, float lr, float momentum, float weight_decay,
                       float grad_scale, const void* grad_bf16, const float* clip, hipStream_t s) {
  if (!param || !grad || !momentum_buf || !runs || nruns <= 0) return DFK_EINVAL;
  if (nruns > kMaxRuns) return DFK_ENOTSUP;
  if (misaligned({param, grad, momentum_buf}, {grad_bf16, bf16_shadow})) return DFK_EINVAL;
  SgdRuns R{};
  if (!fill_run_table(R, runs, nruns)) return DFK_EINVAL;
  for (int r = 0; r < nruns; ++r)
    if (runs[4 * r + 3]) R.first |= 1ull << r;          // the fourth field: first_step
  hipLaunchKernelGGL(clip ? sgd_runs_kernel<true> : sgd_runs_kernel<false>, dim3((unsigned)R.prefix[nruns]),
                     dim3(256), 0, s, param, grad, momentum_buf, (bf16raw*)bf16_shadow, R, lr_dev, lr, momentum,
                     weight_decay, grad_scale, (const bf16raw*)grad_bf16, clip);
  DFK_CHECK_LAUNCH();
  return 0;
}

bool adamw_hyper(double b1, double b2, float eps, float wd, float gscale, AdamwHyper* h) {
  if (!(b1 >= 0.0 && b1 < 1.0) || !(b2 >= 0.0 && b2 < 1.0) || !(eps > 0.f)) return false;
  *h = AdamwHyper{(float)(1.0 - b1), (float)b2, (float)(1.0 - b2), eps, wd, gscale};
  return true;
}

int adamw_step_impl(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, void* bf16_shadow, int64_t n,
                    const float* lr_dev, float lr, double b1, double b2, float eps, float weight_decay,
                    const float* corr, const float* gate, float grad_scale, const void* grad_bf16, const float* clip,
                    hipStream_t s) {
  AdamwHyper h;
  if (!param || !grad || !exp_avg || !exp_avg_sq || !corr) return DFK_EINVAL;
  if (!adamw_hyper(b1, b2, eps, weight_decay, grad_scale, &h)) return DFK_EINVAL;
  if (misaligned({param, grad, exp_avg, exp_avg_sq}, {grad_bf16, bf16_shadow})) return DFK_EINVAL;
  if (n <= 0) return 0;
  const long threads = (n + 3) / 4;
  if ((threads + 255) / 256 > 0x7fffffffL) return DFK_EINVAL;
  hipLaunchKernelGGL(clip ? adamw_kernel<true> : adamw_kernel<false>, dim3((unsigned)((threads + 255) / 256)),
                     dim3(256), 0, s, param, grad, exp_avg, exp_avg_sq, (bf16raw*)bf16_shadow, (long)n, lr_dev, lr, h,
                     corr, gate, (const bf16raw*)grad_bf16, clip);
  DFK_CHECK_LAUNCH();
  return 0;
}

int adamw_step_runs_impl(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, void* bf16_shadow,
                         const int64_t* runs, int32_t nruns, const float* lr_dev, float lr, double b1, double b2,
                         float eps, float weight_decay, const float* corr, int32_t nclass, float grad_scale,
                         const void* grad_bf16, const float* clip, hipStream_t s) {
  AdamwHyper h;
  if (!param || !grad || !exp_avg || !exp_avg_sq || !corr || !runs || nruns <= 0 || nclass <= 0) return DFK_EINVAL;
  if (!adamw_hyper(b1, b2, eps, weight_decay, grad_scale, &h)) return DFK_EINVAL;
  if (nruns > kMaxRuns || nclass > kAdamwMaxClasses) return DFK_ENOTSUP;
  if (misaligned({param, grad, exp_avg, exp_avg_sq}, {grad_bf16, bf16_shadow})) return DFK_EINVAL;
  AdamwRuns R{};
  if (!fill_run_table(R, runs, nruns)) return DFK_EINVAL;
  for (int r = 0; r < nruns; ++r) {
    const int64_t c = runs[4 * r + 3];                  // the fourth field: class index
    if (c < 0 || c >= nclass) return DFK_EINVAL;
    R.cls[r] = (uint8_t)c;
  }
  hipLaunchKernelGGL(clip ? adamw_runs_kernel<true> : adamw_runs_kernel<false>, dim3((unsigned)R.prefix[nruns]),
                     dim3(256), 0, s, param, grad, exp_avg, exp_avg_sq, (bf16raw*)bf16_shadow, R, lr_dev, lr, h, corr,
                     (const bf16raw*)grad_bf16, clip);
  DFK_CHECK_LAUNCH();
  return 0;
}

// The groups arguments of a *_runs_groups entry point (the run table already filled): false for a NULL or, for the
// pairs, not 8-B aligned table, ngroups outside 1..256, or a map shorter than the runs reach
bool fill_group_tab(GroupTab& T, const RunTable& R, const uint8_t* group_map, int64_t map_len,
                    const float* group_hyper, int32_t ngroups) {
  if (!group_map || !group_hyper || ngroups < 1 || ngroups > 256) return false;
  if (reinterpret_cast<uintptr_t>(group_hyper) & 7) return false;
  int64_t end = 0;
  for (int r = 0; r < R.nruns; ++r)
    if (R.start[r] + R.n[r] > end) end = R.start[r] + R.n[r];
  if (map_len < (end + 7) / 8) return false;
  T = GroupTab{group_map, group_hyper, ngroups - 1};
  return true;
}

}  // namespace

extern "C" int dfk_sgd_step(float* param, const float* grad, float* momentum_buf, void* bf16_shadow, int64_t n,
                            const float* lr_dev, float lr, float momentum, float weight_decay, int first_step,
                            const float* gate, float grad_scale, const void* grad_bf16, hipStream_t s) {
  return sgd_step_impl(param, grad, momentum_buf, bf16_shadow, n, lr_dev, lr, momentum, weight_decay, first_step,
                       gate, grad_scale, grad_bf16, nullptr, s);
}

extern "C" int dfk_sgd_step_clip(float* param, const float* grad, float* momentum_buf, void* bf16_shadow, int64_t n,
                                 const float* lr_dev, float lr, float momentum, float weight_decay, int first_step,
                                 const float* gate, float grad_scale, const void* grad_bf16, const float* clip_coef,
                                 hipStream_t s) {
  if (!clip_coef || n < 0) return DFK_EINVAL;
  return sgd_step_impl(param, grad, momentum_buf, bf16_shadow, n, lr_dev, lr, momentum, weight_decay, first_step,
                       gate, grad_scale, grad_bf16, clip_coef, s);
}

extern "C" int dfk_sgd_step_runs(float* param, const float* grad, float* momentum_buf, void* bf16_shadow,
                                 const int64_t* runs, int32_t nruns, const float* lr_dev, float lr, float momentum,
                                 float weight_decay, float grad_scale, const void* grad_bf16, hipStream_t s) {
  return sgd_step_runs_impl(param, grad, momentum_buf, bf16_shadow, runs, nruns, lr_dev, lr, momentum, weight_decay,
                            grad_scale, grad_bf16, nullptr, s);
}

extern "C" int dfk_sgd_step_runs_clip(float* param, const float* grad, float* momentum_buf, void* bf16_shadow,
                                      const int64_t* runs, int32_t nruns, const float* lr_dev, float lr,
                                      float momentum, float weight_decay, float grad_scale, const void* grad_bf16,
                                      const float* clip_coef, hipStream_t s) {
  if (!clip_coef || nruns < 1 || nruns > kMaxRuns) return DFK_EINVAL;
  return sgd_step_runs_impl(param, grad, momentum_buf, bf16_shadow, runs, nruns, lr_dev, lr, momentum, weight_decay,
                            grad_scale, grad_bf16, clip_coef, s);
}

extern "C" int dfk_sgd_step_runs_groups(float* param, const float* grad, float* momentum_buf, void* bf16_shadow,
                                        const int64_t* runs, int32_t nruns, const float* lr_dev, float lr,
                                        float momentum, const uint8_t* group_map, int64_t map_len,
                                        const float* group_hyper, int32_t ngroups, float grad_scale,
                                        const void* grad_bf16, const float* clip_coef, hipStream_t s) {
  if (!param || !grad || !momentum_buf || !runs || nruns <= 0) return DFK_EINVAL;
  if (nruns > kMaxRuns) return DFK_ENOTSUP;
  if (misaligned({param, grad, momentum_buf}, {grad_bf16, bf16_shadow})) return DFK_EINVAL;
  SgdRuns R{};
  GroupTab T{};
  if (!fill_run_table(R, runs, nruns) || !fill_group_tab(T, R, group_map, map_len, group_hyper, ngroups))
    return DFK_EINVAL;
  for (int r = 0; r < nruns; ++r)
    if (runs[4 * r + 3]) R.first |= 1ull << r;
  hipLaunchKernelGGL(clip_coef ? sgd_runs_groups_kernel<true> : sgd_runs_groups_kernel<false>,
                     dim3((unsigned)R.prefix[nruns]), dim3(256), 0, s, param, grad, momentum_buf,
                     (bf16raw*)bf16_shadow, R, lr_dev, lr, momentum, grad_scale, (const bf16raw*)grad_bf16, clip_coef,
                     T);
  DFK_CHECK_LAUNCH();
  return 0;
}

extern "C" int dfk_adamw_prelude(int32_t* counters, float* corr, int32_t nclass, const int64_t* classes, int32_t n,
                                 double b1, double b2, hipStream_t s) {
  if (!counters || !corr || !classes || nclass <= 0 || n <= 0 || n > nclass) return DFK_EINVAL;
  if (!(b1 >= 0.0 && b1 < 1.0) || !(b2 >= 0.0 && b2 < 1.0)) return DFK_EINVAL;
  if (nclass > kAdamwMaxClasses) return DFK_ENOTSUP;
  AdamwClasses C{};
  C.n = n;
  for (int i = 0; i < n; ++i) {
    const int64_t* e = classes + 2 * i;       // {class index, gate pointer}
    if (e[0] < 0 || e[0] >= nclass) return DFK_EINVAL;
    for (int j = 0; j < i; ++j)
      if (C.cls[j] == e[0]) return DFK_EINVAL;   // a class advances once per step
    C.cls[i] = (int32_t)e[0];
    C.gate[i] = reinterpret_cast<const float*>(e[1]);
  }
  hipLaunchKernelGGL(adamw_prelude_kernel, dim3(1), dim3(kAdamwMaxClasses), 0, s, counters, corr, C, log(b1),
                     log(b2));
  DFK_CHECK_LAUNCH();
  return 0;
}

extern "C" int dfk_adamw_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, void* bf16_shadow,
                              int64_t n, const float* lr_dev, float lr, double b1, double b2, float eps,
                              float weight_decay, const float* corr, const float* gate, float grad_scale,
                              const void* grad_bf16, hipStream_t s) {
  return adamw_step_impl(param, grad, exp_avg, exp_avg_sq, bf16_shadow, n, lr_dev, lr, b1, b2, eps, weight_decay, corr,
                         gate, grad_scale, grad_bf16, nullptr, s);
}

extern "C" int dfk_adamw_step_clip(float* param, const float* grad, float* exp_avg, float* exp_avg_sq,
                                   void* bf16_shadow, int64_t n, const float* lr_dev, float lr, double b1, double b2,
                                   float eps, float weight_decay, const float* corr, const float* gate,
                                   float grad_scale, const void* grad_bf16, const float* clip_coef, hipStream_t s) {
  if (!clip_coef || n < 0) return DFK_EINVAL;
  return adamw_step_impl(param, grad, exp_avg, exp_avg_sq, bf16_shadow, n, lr_dev, lr, b1, b2, eps, weight_decay, corr,
                         gate, grad_scale, grad_bf16, clip_coef, s);
}

extern "C" int dfk_adamw_step_runs(float* param, const float* grad, float* exp_avg, float* exp_avg_sq,
                                   void* bf16_shadow, const int64_t* runs, int32_t nruns, const float* lr_dev,
                                   float lr, double b1, double b2, float eps, float weight_decay, const float* corr,
                                   int32_t nclass, float grad_scale, const void* grad_bf16, hipStream_t s) {
  return adamw_step_runs_impl(param, grad, exp_avg, exp_avg_sq, bf16_shadow, runs, nruns, lr_dev, lr, b1, b2, eps,
                              weight_decay, corr, nclass, grad_scale, grad_bf16, nullptr, s);
}

extern "C" int dfk_adamw_step_runs_clip(float* param, const float* grad, float* exp_avg, float* exp_avg_sq,
                                        void* bf16_shadow, const int64_t* runs, int32_t nruns, const float* lr_dev,
                                        float lr, double b1, double b2, float eps, float weight_decay,
                                        const float* corr, int32_t nclass, float grad_scale, const void* grad_bf16,
                                        const float* clip_coef, hipStream_t s) {
  if (!clip_coef || nruns < 1 || nruns > kMaxRuns) return DFK_EINVAL;
  return adamw_step_runs_impl(param, grad, exp_avg, exp_avg_sq, bf16_shadow, runs, nruns, lr_dev, lr, b1, b2, eps,
                              weight_decay, corr, nclass, grad_scale, grad_bf16, clip_coef, s);
}

extern "C" int dfk_adamw_step_runs_groups(float* param, const float* grad, float* exp_avg, float* exp_avg_sq,
                                          void* bf16_shadow, const int64_t* runs, int32_t nruns, const float* lr_dev,
                                          float lr, double b1, double b2, float eps, const float* corr,
                                          int32_t nclass, const uint8_t* group_map, int64_t map_len,
                                          const float* group_hyper, int32_t ngroups, float grad_scale,
                                          const void* grad_bf16, const float* clip_coef, hipStream_t s) {
  AdamwHyper h;
  if (!param || !grad || !exp_avg || !exp_avg_sq || !corr || !runs || nruns <= 0 || nclass <= 0) return DFK_EINVAL;
  if (!adamw_hyper(b1, b2, eps, 0.f, grad_scale, &h)) return DFK_EINVAL;     // the decay comes from group_hyper
  if (nruns > kMaxRuns || nclass > kAdamwMaxClasses) return DFK_ENOTSUP;
  if (misaligned({param, grad, exp_avg, exp_avg_sq}, {grad_bf16, bf16_shadow})) return DFK_EINVAL;
  AdamwRuns R{};
  GroupTab T{};
  if (!fill_run_table(R, runs, nruns) || !fill_group_tab(T, R, group_map, map_len, group_hyper, ngroups))
    return DFK_EINVAL;
  for (int r = 0; r < nruns; ++r) {
    const int64_t c = runs[4 * r + 3];
    if (c < 0 || c >= nclass) return DFK_EINVAL;
    R.cls[r] = (uint8_t)c;
  }
  hipLaunchKernelGGL(clip_coef ? adamw_runs_groups_kernel<true> : adamw_runs_groups_kernel<false>,
                     dim3((unsigned)R.prefix[nruns]), dim3(256), 0, s, param, grad, exp_avg, exp_avg_sq,
                     (bf16raw*)bf16_shadow, R, lr_dev, lr, h, corr, (const bf16raw*)grad_bf16, clip_coef, T);
  DFK_CHECK_LAUNCH();
  return 0;
}

// Global gradient-norm clipping (torch.nn.utils.clip_grad_norm_(params, max_norm, 2.0, error_if_nonfinite=False) on
// the mean gradient): the sum of squares over one chunk of <= 64 runs into its own slab of DFK_GNORM_PARTIALS doubles
extern "C" int dfk_grad_sqnorm_runs(const float* grad, const void* grad_bf16, const int64_t* runs, int32_t nruns,
                                    float grad_scale, double* partials, hipStream_t s) {
  if (!grad || !runs || !partials || nruns < 1 || nruns > kMaxRuns) return DFK_EINVAL;
  if (misaligned({grad}, {grad_bf16, partials})) return DFK_EINVAL;
  RunTable R{};
  if (!fill_run_table(R, runs, nruns)) return DFK_EINVAL;   // the fourth field is not read
  hipLaunchKernelGGL(grad_bf16 ? grad_sqnorm_runs_kernel<true> : grad_sqnorm_runs_kernel<false>, dim3(kGnormPartials),
                     dim3(256), 0, s, grad, (const bf16raw*)grad_bf16, R, grad_scale, partials);
  DFK_CHECK_LAUNCH();
  return 0;
}

extern "C" int dfk_grad_clip_coef(const double* partials, int32_t n, float max_norm, float* out, hipStream_t s) {
  if (!partials || !out || n <= 0) return DFK_EINVAL;
  if (!(max_norm > 0.f) || !(max_norm <= 3.402823466e38f)) return DFK_EINVAL;   // <= 0, NaN, Inf
  if ((reinterpret_cast<uintptr_t>(partials) & 7) || (reinterpret_cast<uintptr_t>(out) & 3)) return DFK_EINVAL;
  hipLaunchKernelGGL(grad_clip_coef_kernel, dim3(1), dim3(256), 0, s, partials, (int)n, max_norm, out);
  DFK_CHECK_LAUNCH();
  return 0;
}
