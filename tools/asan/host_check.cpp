// Host-side checks of libdfk under AddressSanitizer (CPU only; no kernel is launched).  Exercises the C ABI's
// host code: workspace planners (GEMM split-K, attention table / backward scratch, LayerNorm slab, wav2vec2
// conv0 on both the group-norm (with and without per-clip lengths) and the layer-norm path, mel with and without the resampler), argument validation on malformed inputs (null pointers, bad strides / shapes, unsupported head
// dims, the SGD and AdamW entry points' buffers / run table / hyper-parameters, the gradient-clipping entry points' slab /
// coefficient / max_norm / run table, the parameter-group entry points' map / pairs / group count, the weight-EMA entry points' buffers / decay), which must return DFK_EINVAL before touching
// the device.  Built and run by tools/asan/run.sh.
#include <cstdio>
#include <cstring>
#include <initializer_list>

#include "../../include/dfk.h"

static int fails = 0;
#define EXPECT(c)                                                      \
  do {                                                                 \
    if (!(c)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); ++fails; } \
  } while (0)

int main() {
  // GEMM workspace: a small-M grid asks for split-K slabs, a large one for none
  dfk_gemm_args g;
  std::memset(&g, 0, sizeof(g));
  g.M = 1592; g.N = 3072; g.K = 768; g.dtype = DFK_BF16; g.nz0 = g.nz1 = 1; g.splitk = 1;
  g.a.ld = 768; g.b.ld = 768; g.ldc = 3072;
  const int64_t ws_small = dfk_gemm_workspace(&g);
  EXPECT(ws_small >= 0);
  g.M = 401408; g.N = 288; g.K = 96;
  EXPECT(dfk_gemm_workspace(&g) == 0);
  EXPECT(dfk_gemm_workspace(nullptr) < 0);
  // dfk_gemm rejects missing operands and contradictory epilogues before any launch
  EXPECT(dfk_gemm(&g, nullptr) != 0);                       // null A / B / C
  g.a.ptr = g.b.ptr = reinterpret_cast<void*>(0x1000); g.c = reinterpret_cast<void*>(0x2000);
  g.act = 2;                                                // dGELU without aux
  EXPECT(dfk_gemm(&g, nullptr) != 0);
  g.act = 7;
  EXPECT(dfk_gemm(&g, nullptr) != 0);
  g.act = 0; g.atomic = 1; g.c_f32 = 0;                     // atomics need an fp32 C
  EXPECT(dfk_gemm(&g, nullptr) != 0);
  // attention planners and validation
  dfk_wattn_args a;
  std::memset(&a, 0, sizeof(a));
  a.B = 8; a.D = 16; a.H = 56; a.W = 56; a.wd = 8; a.wh = 7; a.ww = 7; a.fd = 8; a.fh = 7; a.fw = 7;
  a.sd = 4; a.sh = 3; a.sw = 3; a.heads = 3; a.hd = 32; a.scale = 0.1767767f; a.dtype = DFK_BF16;
  a.ld_qkv = 288; a.ld_out = 96;
  a.q = a.k = a.v = reinterpret_cast<void*>(0x1000); a.out = reinterpret_cast<void*>(0x2000);
  EXPECT(dfk_wattn_table_workspace(&a) > 0);
  EXPECT(dfk_wattn_bwd_workspace(&a) == 0);                 // no RPB: no dRPB scratch
  a.rpb = reinterpret_cast<const float*>(0x3000);
  EXPECT(dfk_wattn_bwd_workspace(&a) > 0);
  a.rpb = nullptr;
  a.hd = 48;                                                // unsupported head dim
  EXPECT(dfk_wattn_fwd(&a, nullptr) != 0);
  a.hd = 32; a.sd = 8;                                      // shift >= window
  EXPECT(dfk_wattn_fwd(&a, nullptr) != 0);
  EXPECT(dfk_wattn_fwd(nullptr, nullptr) != 0);
  // other planners
  EXPECT(dfk_layernorm_bwd_workspace(401408, 96) > 0);
  EXPECT(dfk_layernorm_bwd_workspace(6272, 768) > 0);
  EXPECT(dfk_layernorm_bwd_workspace(0, 96) == 0);
  EXPECT(dfk_w2v_conv0_fwd_workspace(8, 64000) > 0);
  EXPECT(dfk_w2v_conv0_bwd_workspace(8, 64000) > 0);
  EXPECT(dfk_w2v_conv0_fwd_workspace(8, 5) == 0);
  EXPECT(dfk_mel_workspace(8, 88200, 2048, 512, 128) > 0);
  // resampler in front of the mel pipeline: 4 s at 16 kHz -> 88200 samples at 22.05 kHz, the same plan
  EXPECT(dfk_mel_resampled_workspace(8, 64000, 441, 320, 2048, 512, 128) > 0);
  EXPECT(dfk_mel_resampled_workspace(8, 64000, 441, 320, 2048, 512, 128) == dfk_mel_workspace(8, 88200, 2048, 512, 128));
  EXPECT(dfk_mel_resampled_workspace(8, 0, 441, 320, 2048, 512, 128) == -1);
  EXPECT(dfk_mel_resampled_workspace(8, 64000, 0, 320, 2048, 512, 128) == -1);
  EXPECT(dfk_mel_resampled_workspace(8, 64000, 441, -1, 2048, 512, 128) == -1);
  EXPECT(dfk_mel_resampled_workspace(0, 64000, 441, 320, 2048, 512, 128) == -1);
  EXPECT(dfk_mel_resampled_workspace(8, INT64_MAX / 2, 441, 320, 2048, 512, 128) == -1);   // S_in * up overflows
  {
    const float* fx = reinterpret_cast<const float*>(0x1000);
    float* fy = reinterpret_cast<float*>(0x2000);
    void* ws = reinterpret_cast<void*>(0x3000);
    uint8_t* img = reinterpret_cast<uint8_t*>(0x4000);
    const int64_t wsb = dfk_mel_resampled_workspace(8, 64000, 441, 320, 2048, 512, 128);
    // malformed calls return DFK_EINVAL with no launch: null operands, odd ntaps, a wrong S_out, bad sizes
    EXPECT(dfk_resample(nullptr, 8, 64000, fx, 441, 320, 64, fy, 88200, nullptr) == DFK_EINVAL);
    EXPECT(dfk_resample(fx, 8, 64000, nullptr, 441, 320, 64, fy, 88200, nullptr) == DFK_EINVAL);
    EXPECT(dfk_resample(fx, 8, 64000, fx, 441, 320, 64, nullptr, 88200, nullptr) == DFK_EINVAL);
    EXPECT(dfk_resample(fx, 8, 64000, fx, 441, 320, 63, fy, 88200, nullptr) == DFK_EINVAL);
    EXPECT(dfk_resample(fx, 8, 64000, fx, 441, 320, 64, fy, 88199, nullptr) == DFK_EINVAL);
    EXPECT(dfk_resample(fx, 8, 64000, fx, 441, 320, 64, fy, 88201, nullptr) == DFK_EINVAL);
    EXPECT(dfk_resample(fx, 8, 1000, fx, 441, 320, 64, fy, 1378, nullptr) == DFK_EINVAL);   // ceil is 1379
    EXPECT(dfk_resample(fx, 0, 64000, fx, 441, 320, 64, fy, 88200, nullptr) == DFK_EINVAL);
    EXPECT(dfk_resample(fx, 8, 64000, fx, 0, 320, 64, fy, 88200, nullptr) == DFK_EINVAL);
    EXPECT(dfk_resample(fx, 8, 64000, fx, 441, 320, 0, fy, 88200, nullptr) == DFK_EINVAL);
    EXPECT(dfk_mel_image_resampled(nullptr, 8, 64000, fx, 441, 320, 64, 88200, fx, fx, 2048, 512, 128, 224, 224, ws, wsb,
                                   img, nullptr) == DFK_EINVAL);
    EXPECT(dfk_mel_image_resampled(fx, 8, 64000, nullptr, 441, 320, 64, 88200, fx, fx, 2048, 512, 128, 224, 224, ws, wsb,
                                   img, nullptr) == DFK_EINVAL);
    EXPECT(dfk_mel_image_resampled(fx, 8, 64000, fx, 441, 320, 64, 88200, nullptr, fx, 2048, 512, 128, 224, 224, ws, wsb,
                                   img, nullptr) == DFK_EINVAL);
    EXPECT(dfk_mel_image_resampled(fx, 8, 64000, fx, 441, 320, 64, 88200, fx, nullptr, 2048, 512, 128, 224, 224, ws, wsb,
                                   img, nullptr) == DFK_EINVAL);
    EXPECT(dfk_mel_image_resampled(fx, 8, 64000, fx, 441, 320, 64, 88200, fx, fx, 2048, 512, 128, 224, 224, nullptr, wsb,
                                   img, nullptr) == DFK_EINVAL);
    EXPECT(dfk_mel_image_resampled(fx, 8, 64000, fx, 441, 320, 64, 88200, fx, fx, 2048, 512, 128, 224, 224, ws, wsb,
                                   nullptr, nullptr) == DFK_EINVAL);
    EXPECT(dfk_mel_image_resampled(fx, 8, 64000, fx, 441, 320, 64, 88199, fx, fx, 2048, 512, 128, 224, 224, ws, wsb,
                                   img, nullptr) == DFK_EINVAL);
    EXPECT(dfk_mel_image_resampled(fx, 8, 64000, fx, 441, 320, 64, 88200, fx, fx, 2048, 512, 128, 224, 224, ws, wsb - 1,
                                   img, nullptr) == DFK_EINVAL);
    // the unchanged 22.05 kHz entry point keeps its checks
    EXPECT(dfk_mel_image(nullptr, 8, 88200, fx, fx, 2048, 512, 128, 224, 224, ws, wsb, img, nullptr) == DFK_EINVAL);
    EXPECT(dfk_mel_image(fx, 8, 88200, fx, fx, 2048, 512, 128, 224, 224, ws, wsb - 1, img, nullptr) == DFK_EINVAL);
    // ragged batches: null lengths, null operands and every size the uniform entry points reject
    const int64_t* len = reinterpret_cast<const int64_t*>(0x5000);
    EXPECT(dfk_resample_ragged(fx, 8, 64000, nullptr, fx, 441, 320, 64, fy, 88200, nullptr) == DFK_EINVAL);
    EXPECT(dfk_resample_ragged(nullptr, 8, 64000, len, fx, 441, 320, 64, fy, 88200, nullptr) == DFK_EINVAL);
    EXPECT(dfk_resample_ragged(fx, 8, 64000, len, nullptr, 441, 320, 64, fy, 88200, nullptr) == DFK_EINVAL);
    EXPECT(dfk_resample_ragged(fx, 8, 64000, len, fx, 441, 320, 64, nullptr, 88200, nullptr) == DFK_EINVAL);
    EXPECT(dfk_resample_ragged(fx, 8, 64000, len, fx, 441, 320, 63, fy, 88200, nullptr) == DFK_EINVAL);
    EXPECT(dfk_resample_ragged(fx, 8, 64000, len, fx, 441, 320, 64, fy, 88199, nullptr) == DFK_EINVAL);
    EXPECT(dfk_resample_ragged(fx, 8, 1000, len, fx, 441, 320, 64, fy, 1378, nullptr) == DFK_EINVAL);   // ceil is 1379
    EXPECT(dfk_resample_ragged(fx, 0, 64000, len, fx, 441, 320, 64, fy, 88200, nullptr) == DFK_EINVAL);
    EXPECT(dfk_resample_ragged(fx, 65536, 64000, len, fx, 441, 320, 64, fy, 88200, nullptr) == DFK_EINVAL);
    EXPECT(dfk_resample_ragged(fx, 8, 64000, len, fx, 0, 320, 64, fy, 88200, nullptr) == DFK_EINVAL);
    // resampled path (taps given)
    EXPECT(dfk_mel_image_ragged(fx, 8, 64000, nullptr, fx, 441, 320, 64, fx, fx, 2048, 512, 128, 224, 224, ws, wsb, img,
                                nullptr) == DFK_EINVAL);
    EXPECT(dfk_mel_image_ragged(nullptr, 8, 64000, len, fx, 441, 320, 64, fx, fx, 2048, 512, 128, 224, 224, ws, wsb, img,
                                nullptr) == DFK_EINVAL);
    EXPECT(dfk_mel_image_ragged(fx, 8, 64000, len, fx, 441, 320, 64, nullptr, fx, 2048, 512, 128, 224, 224, ws, wsb, img,
                                nullptr) == DFK_EINVAL);
    EXPECT(dfk_mel_image_ragged(fx, 8, 64000, len, fx, 441, 320, 64, fx, nullptr, 2048, 512, 128, 224, 224, ws, wsb, img,
                                nullptr) == DFK_EINVAL);
    EXPECT(dfk_mel_image_ragged(fx, 8, 64000, len, fx, 441, 320, 64, fx, fx, 2048, 512, 128, 224, 224, nullptr, wsb, img,
                                nullptr) == DFK_EINVAL);
    EXPECT(dfk_mel_image_ragged(fx, 8, 64000, len, fx, 441, 320, 64, fx, fx, 2048, 512, 128, 224, 224, ws, wsb, nullptr,
                                nullptr) == DFK_EINVAL);
    EXPECT(dfk_mel_image_ragged(fx, 8, 64000, len, fx, 441, 320, 63, fx, fx, 2048, 512, 128, 224, 224, ws, wsb, img,
                                nullptr) == DFK_EINVAL);
    EXPECT(dfk_mel_image_ragged(fx, 8, 64000, len, fx, 441, 0, 64, fx, fx, 2048, 512, 128, 224, 224, ws, wsb, img,
                                nullptr) == DFK_EINVAL);
    EXPECT(dfk_mel_image_ragged(fx, 8, 64000, len, fx, 441, 320, 64, fx, fx, 2048, 512, 128, 224, 224, ws, wsb - 1, img,
                                nullptr) == DFK_EINVAL);
    EXPECT(dfk_mel_image_ragged(fx, 8, 64000, len, fx, 441, 320, 64, fx, fx, 2046, 512, 128, 224, 224, ws, wsb, img,
                                nullptr) == DFK_EINVAL);
    EXPECT(dfk_mel_image_ragged(fx, 8, 0, len, fx, 441, 320, 64, fx, fx, 2048, 512, 128, 224, 224, ws, wsb, img,
                                nullptr) == DFK_EINVAL);
    EXPECT(dfk_mel_image_ragged(fx, 65536, 64000, len, fx, 441, 320, 64, fx, fx, 2048, 512, 128, 224, 224, ws, wsb, img,
                                nullptr) == DFK_EINVAL);
    // plain path (taps == NULL needs up = down = 1, ntaps = 0; wsb is dfk_mel_workspace(8, 88200, ...))
    EXPECT(dfk_mel_image_ragged(fx, 8, 88200, nullptr, nullptr, 1, 1, 0, fx, fx, 2048, 512, 128, 224, 224, ws, wsb, img,
                                nullptr) == DFK_EINVAL);
    EXPECT(dfk_mel_image_ragged(nullptr, 8, 88200, len, nullptr, 1, 1, 0, fx, fx, 2048, 512, 128, 224, 224, ws, wsb, img,
                                nullptr) == DFK_EINVAL);
    EXPECT(dfk_mel_image_ragged(fx, 8, 88200, len, nullptr, 441, 320, 0, fx, fx, 2048, 512, 128, 224, 224, ws, wsb, img,
                                nullptr) == DFK_EINVAL);
    EXPECT(dfk_mel_image_ragged(fx, 8, 88200, len, nullptr, 1, 1, 64, fx, fx, 2048, 512, 128, 224, 224, ws, wsb, img,
                                nullptr) == DFK_EINVAL);
    EXPECT(dfk_mel_image_ragged(fx, 8, 88200, len, nullptr, 1, 1, 0, fx, fx, 2048, 512, 128, 224, 224, ws, wsb - 1, img,
                                nullptr) == DFK_EINVAL);
    EXPECT(dfk_mel_image_ragged(fx, 8, 88200, len, nullptr, 1, 1, 0, fx, fx, 2048, 510, 128, 224, 224, ws, wsb, img,
                                nullptr) == DFK_EINVAL);
    EXPECT(dfk_mel_image_ragged(fx, 8, 88200, len, nullptr, 1, 1, 0, fx, fx, 2048, 512, 128, 0, 224, ws, wsb, img,
                                nullptr) == DFK_EINVAL);
  }
  // validation of the other entry points
  EXPECT(dfk_layernorm_fwd(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 10, 96, 1e-5f, DFK_BF16, nullptr,
                           nullptr, nullptr) != 0);
  EXPECT(dfk_sgd_step(nullptr, nullptr, nullptr, nullptr, 10, nullptr, 0.1f, 0.9f, 0.f, 0, nullptr, 1.f, nullptr,
                      nullptr) != 0);
  {
    // SGD: the run table, its limits and the alignment rules of dfk_sgd_step_runs (the rows AdamW has below)
    float* fx = reinterpret_cast<float*>(0x10000);
    float* odd = reinterpret_cast<float*>(0x10004);
    int64_t runs[65 * 4];
    for (int r = 0; r < 65; ++r) { runs[4 * r] = 64 * r; runs[4 * r + 1] = 40; runs[4 * r + 2] = 0; runs[4 * r + 3] = 0; }
    EXPECT(dfk_sgd_step_runs(fx, fx, fx, nullptr, nullptr, 2, fx, 0.f, 0.9f, 0.f, 1.f, nullptr, nullptr) == DFK_EINVAL);
    EXPECT(dfk_sgd_step_runs(fx, fx, fx, nullptr, runs, 0, fx, 0.f, 0.9f, 0.f, 1.f, nullptr, nullptr) == DFK_EINVAL);
    EXPECT(dfk_sgd_step_runs(fx, fx, fx, nullptr, runs, -1, fx, 0.f, 0.9f, 0.f, 1.f, nullptr, nullptr) == DFK_EINVAL);
    EXPECT(dfk_sgd_step_runs(fx, fx, fx, nullptr, runs, 65, fx, 0.f, 0.9f, 0.f, 1.f, nullptr, nullptr) == DFK_ENOTSUP);
    runs[5] = 0;                                                           // an empty run
    EXPECT(dfk_sgd_step_runs(fx, fx, fx, nullptr, runs, 2, fx, 0.f, 0.9f, 0.f, 1.f, nullptr, nullptr) == DFK_EINVAL);
    runs[5] = 40; runs[4] = -64;                                           // negative start
    EXPECT(dfk_sgd_step_runs(fx, fx, fx, nullptr, runs, 2, fx, 0.f, 0.9f, 0.f, 1.f, nullptr, nullptr) == DFK_EINVAL);
    runs[4] = 66;                                                          // run start not a multiple of 4
    EXPECT(dfk_sgd_step_runs(fx, fx, fx, nullptr, runs, 2, fx, 0.f, 0.9f, 0.f, 1.f, nullptr, nullptr) == DFK_EINVAL);
    runs[4] = 64;
    EXPECT(dfk_sgd_step_runs(odd, fx, fx, nullptr, runs, 2, fx, 0.f, 0.9f, 0.f, 1.f, nullptr, nullptr) == DFK_EINVAL);
    EXPECT(dfk_sgd_step_runs(fx, fx, fx, odd, runs, 2, fx, 0.f, 0.9f, 0.f, 1.f, nullptr, nullptr) == DFK_EINVAL);
    EXPECT(dfk_sgd_step_runs(fx, fx, fx, nullptr, runs, 2, fx, 0.f, 0.9f, 0.f, 1.f, odd, nullptr) == DFK_EINVAL);
    // the one-run entry point writes the shadow in 8-B quads too
    EXPECT(dfk_sgd_step(fx, fx, fx, odd, 16, fx, 0.f, 0.9f, 0.f, 0, nullptr, 1.f, nullptr, nullptr) == DFK_EINVAL);
  }
  {
    // AdamW: malformed calls return before any launch (fx: a fake 16-B aligned device pointer, never touched)
    float* fx = reinterpret_cast<float*>(0x10000);
    float* odd = reinterpret_cast<float*>(0x10004);
    int32_t* cnt = reinterpret_cast<int32_t*>(0x20000);
    EXPECT(dfk_adamw_step(nullptr, fx, fx, fx, nullptr, 16, fx, 0.f, 0.9, 0.999, 1e-8f, 0.f, fx, nullptr, 1.f, nullptr,
                          nullptr) == DFK_EINVAL);
    EXPECT(dfk_adamw_step(fx, nullptr, fx, fx, nullptr, 16, fx, 0.f, 0.9, 0.999, 1e-8f, 0.f, fx, nullptr, 1.f, nullptr,
                          nullptr) == DFK_EINVAL);
    EXPECT(dfk_adamw_step(fx, fx, nullptr, fx, nullptr, 16, fx, 0.f, 0.9, 0.999, 1e-8f, 0.f, fx, nullptr, 1.f, nullptr,
                          nullptr) == DFK_EINVAL);
    EXPECT(dfk_adamw_step(fx, fx, fx, nullptr, nullptr, 16, fx, 0.f, 0.9, 0.999, 1e-8f, 0.f, fx, nullptr, 1.f, nullptr,
                          nullptr) == DFK_EINVAL);
    EXPECT(dfk_adamw_step(fx, fx, fx, fx, nullptr, 16, fx, 0.f, 0.9, 0.999, 1e-8f, 0.f, nullptr, nullptr, 1.f, nullptr,
                          nullptr) == DFK_EINVAL);                         // no corrections
    EXPECT(dfk_adamw_step(odd, fx, fx, fx, nullptr, 16, fx, 0.f, 0.9, 0.999, 1e-8f, 0.f, fx, nullptr, 1.f, nullptr,
                          nullptr) == DFK_EINVAL);                         // misaligned parameter
    EXPECT(dfk_adamw_step(fx, fx, fx, odd, nullptr, 16, fx, 0.f, 0.9, 0.999, 1e-8f, 0.f, fx, nullptr, 1.f, nullptr,
                          nullptr) == DFK_EINVAL);                         // misaligned exp_avg_sq
    EXPECT(dfk_adamw_step(fx, fx, fx, fx, odd, 16, fx, 0.f, 0.9, 0.999, 1e-8f, 0.f, fx, nullptr, 1.f, nullptr,
                          nullptr) == DFK_EINVAL);                         // shadow not 8-B aligned
    EXPECT(dfk_adamw_step(fx, fx, fx, fx, nullptr, 16, fx, 0.f, 0.9, 0.999, 1e-8f, 0.f, fx, nullptr, 1.f, odd,
                          nullptr) == DFK_EINVAL);                         // grad_bf16 not 8-B aligned
    EXPECT(dfk_adamw_step(fx, fx, fx, fx, nullptr, 16, fx, 0.f, 1.0, 0.999, 1e-8f, 0.f, fx, nullptr, 1.f, nullptr,
                          nullptr) == DFK_EINVAL);                         // b1 = 1
    EXPECT(dfk_adamw_step(fx, fx, fx, fx, nullptr, 16, fx, 0.f, 0.9, -0.1, 1e-8f, 0.f, fx, nullptr, 1.f, nullptr,
                          nullptr) == DFK_EINVAL);                         // b2 < 0
    EXPECT(dfk_adamw_step(fx, fx, fx, fx, nullptr, 16, fx, 0.f, 0.9, 0.999, 0.f, 0.f, fx, nullptr, 1.f, nullptr,
                          nullptr) == DFK_EINVAL);                         // eps = 0
    EXPECT(dfk_adamw_step(fx, fx, fx, fx, nullptr, -4, fx, 0.f, 0.9, 0.999, 1e-8f, 0.f, fx, nullptr, 1.f, nullptr,
                          nullptr) == 0);                                  // n <= 0: nothing to do, as dfk_sgd_step
    int64_t runs[65 * 4];
    for (int r = 0; r < 65; ++r) { runs[4 * r] = 64 * r; runs[4 * r + 1] = 40; runs[4 * r + 2] = 0; runs[4 * r + 3] = 0; }
    EXPECT(dfk_adamw_step_runs(fx, fx, fx, fx, nullptr, runs, 0, fx, 0.f, 0.9, 0.999, 1e-8f, 0.f, fx, 1, 1.f, nullptr,
                               nullptr) == DFK_EINVAL);
    EXPECT(dfk_adamw_step_runs(fx, fx, fx, fx, nullptr, runs, 65, fx, 0.f, 0.9, 0.999, 1e-8f, 0.f, fx, 1, 1.f, nullptr,
                               nullptr) == DFK_ENOTSUP);
    EXPECT(dfk_adamw_step_runs(fx, fx, fx, fx, nullptr, nullptr, 2, fx, 0.f, 0.9, 0.999, 1e-8f, 0.f, fx, 1, 1.f,
                               nullptr, nullptr) == DFK_EINVAL);
    EXPECT(dfk_adamw_step_runs(nullptr, fx, fx, fx, nullptr, runs, 2, fx, 0.f, 0.9, 0.999, 1e-8f, 0.f, fx, 1, 1.f,
                               nullptr, nullptr) == DFK_EINVAL);
    EXPECT(dfk_adamw_step_runs(fx, fx, odd, fx, nullptr, runs, 2, fx, 0.f, 0.9, 0.999, 1e-8f, 0.f, fx, 1, 1.f,
                               nullptr, nullptr) == DFK_EINVAL);
    EXPECT(dfk_adamw_step_runs(fx, fx, fx, fx, nullptr, runs, 2, fx, 0.f, 0.9, 1.5, 1e-8f, 0.f, fx, 1, 1.f, nullptr,
                               nullptr) == DFK_EINVAL);
    EXPECT(dfk_adamw_step_runs(fx, fx, fx, fx, nullptr, runs, 2, fx, 0.f, 0.9, 0.999, -1.f, 0.f, fx, 1, 1.f, nullptr,
                               nullptr) == DFK_EINVAL);
    runs[4] = 66;                                                          // run start not a multiple of 4
    EXPECT(dfk_adamw_step_runs(fx, fx, fx, fx, nullptr, runs, 2, fx, 0.f, 0.9, 0.999, 1e-8f, 0.f, fx, 1, 1.f, nullptr,
                               nullptr) == DFK_EINVAL);
    runs[4] = 64; runs[5] = -8;                                            // negative n
    EXPECT(dfk_adamw_step_runs(fx, fx, fx, fx, nullptr, runs, 2, fx, 0.f, 0.9, 0.999, 1e-8f, 0.f, fx, 1, 1.f, nullptr,
                               nullptr) == DFK_EINVAL);
    runs[5] = 40; runs[7] = 1;                                             // class index beyond nclass
    EXPECT(dfk_adamw_step_runs(fx, fx, fx, fx, nullptr, runs, 2, fx, 0.f, 0.9, 0.999, 1e-8f, 0.f, fx, 1, 1.f, nullptr,
                               nullptr) == DFK_EINVAL);
    EXPECT(dfk_adamw_step_runs(fx, fx, fx, fx, nullptr, runs, 2, fx, 0.f, 0.9, 0.999, 1e-8f, 0.f, fx, 65, 1.f, nullptr,
                               nullptr) == DFK_ENOTSUP);
    int64_t cls[6] = {0, 0, 1, 0, 1, 0};
    EXPECT(dfk_adamw_prelude(nullptr, fx, 2, cls, 2, 0.9, 0.999, nullptr) == DFK_EINVAL);
    EXPECT(dfk_adamw_prelude(cnt, nullptr, 2, cls, 2, 0.9, 0.999, nullptr) == DFK_EINVAL);
    EXPECT(dfk_adamw_prelude(cnt, fx, 2, nullptr, 2, 0.9, 0.999, nullptr) == DFK_EINVAL);
    EXPECT(dfk_adamw_prelude(cnt, fx, 2, cls, 0, 0.9, 0.999, nullptr) == DFK_EINVAL);
    EXPECT(dfk_adamw_prelude(cnt, fx, 2, cls, 3, 0.9, 0.999, nullptr) == DFK_EINVAL);   // more entries than classes
    EXPECT(dfk_adamw_prelude(cnt, fx, 1, cls, 1, 0.9, 1.0, nullptr) == DFK_EINVAL);
    EXPECT(dfk_adamw_prelude(cnt, fx, 1, cls + 2, 1, 0.9, 0.999, nullptr) == DFK_EINVAL);   // class 1 of 1
    EXPECT(dfk_adamw_prelude(cnt, fx, 3, cls + 2, 2, 0.9, 0.999, nullptr) == DFK_EINVAL);   // class 1 listed twice
    EXPECT(dfk_adamw_prelude(cnt, fx, 65, cls, 2, 0.9, 0.999, nullptr) == DFK_ENOTSUP);
  }
  {
    // gradient-norm clipping: the norm / coefficient entry points and the _clip twins reject malformed calls
    float* fx = reinterpret_cast<float*>(0x10000);
    float* odd = reinterpret_cast<float*>(0x10004);
    double* part = reinterpret_cast<double*>(0x30000);
    int64_t runs[65 * 4];
    for (int r = 0; r < 65; ++r) { runs[4 * r] = 64 * r; runs[4 * r + 1] = 40; runs[4 * r + 2] = 0; runs[4 * r + 3] = 0; }
    EXPECT(dfk_grad_sqnorm_runs(fx, nullptr, runs, 2, 1.f, nullptr, nullptr) == DFK_EINVAL);      // no slab
    EXPECT(dfk_grad_sqnorm_runs(nullptr, nullptr, runs, 2, 1.f, part, nullptr) == DFK_EINVAL);
    EXPECT(dfk_grad_sqnorm_runs(fx, nullptr, nullptr, 2, 1.f, part, nullptr) == DFK_EINVAL);
    EXPECT(dfk_grad_sqnorm_runs(fx, nullptr, runs, 0, 1.f, part, nullptr) == DFK_EINVAL);
    EXPECT(dfk_grad_sqnorm_runs(fx, nullptr, runs, -1, 1.f, part, nullptr) == DFK_EINVAL);
    EXPECT(dfk_grad_sqnorm_runs(fx, nullptr, runs, 65, 1.f, part, nullptr) == DFK_EINVAL);
    EXPECT(dfk_grad_sqnorm_runs(odd, nullptr, runs, 2, 1.f, part, nullptr) == DFK_EINVAL);        // misaligned grad
    EXPECT(dfk_grad_sqnorm_runs(fx, odd, runs, 2, 1.f, part, nullptr) == DFK_EINVAL);             // grad_bf16 not 8-B
    EXPECT(dfk_grad_sqnorm_runs(fx, nullptr, runs, 2, 1.f, reinterpret_cast<double*>(odd), nullptr) == DFK_EINVAL);
    runs[4] = 66;                                                          // run start not a multiple of 4
    EXPECT(dfk_grad_sqnorm_runs(fx, nullptr, runs, 2, 1.f, part, nullptr) == DFK_EINVAL);
    EXPECT(dfk_sgd_step_runs_clip(fx, fx, fx, nullptr, runs, 2, fx, 0.f, 0.9f, 0.f, 1.f, nullptr, fx, nullptr) ==
           DFK_EINVAL);
    runs[4] = 64; runs[5] = -8;                                            // negative n
    EXPECT(dfk_grad_sqnorm_runs(fx, nullptr, runs, 2, 1.f, part, nullptr) == DFK_EINVAL);
    EXPECT(dfk_adamw_step_runs_clip(fx, fx, fx, fx, nullptr, runs, 2, fx, 0.f, 0.9, 0.999, 1e-8f, 0.f, fx, 1, 1.f,
                                    nullptr, fx, nullptr) == DFK_EINVAL);
    runs[5] = 40;
    const float inf = 1.f / 0.f, nan = inf - inf;
    EXPECT(dfk_grad_clip_coef(nullptr, 2048, 1.f, fx, nullptr) == DFK_EINVAL);
    EXPECT(dfk_grad_clip_coef(part, 2048, 1.f, nullptr, nullptr) == DFK_EINVAL);
    EXPECT(dfk_grad_clip_coef(part, 0, 1.f, fx, nullptr) == DFK_EINVAL);
    EXPECT(dfk_grad_clip_coef(part, -2048, 1.f, fx, nullptr) == DFK_EINVAL);
    EXPECT(dfk_grad_clip_coef(part, 2048, 0.f, fx, nullptr) == DFK_EINVAL);
    EXPECT(dfk_grad_clip_coef(part, 2048, -1.f, fx, nullptr) == DFK_EINVAL);
    EXPECT(dfk_grad_clip_coef(part, 2048, inf, fx, nullptr) == DFK_EINVAL);
    EXPECT(dfk_grad_clip_coef(part, 2048, nan, fx, nullptr) == DFK_EINVAL);
    // the twins: no coefficient, then their twins' own rules
    EXPECT(dfk_sgd_step_clip(fx, fx, fx, nullptr, 16, fx, 0.f, 0.9f, 0.f, 0, nullptr, 1.f, nullptr, nullptr, nullptr) ==
           DFK_EINVAL);
    EXPECT(dfk_sgd_step_clip(fx, fx, fx, nullptr, -4, fx, 0.f, 0.9f, 0.f, 0, nullptr, 1.f, nullptr, fx, nullptr) ==
           DFK_EINVAL);                                                    // negative length
    EXPECT(dfk_sgd_step_clip(odd, fx, fx, nullptr, 16, fx, 0.f, 0.9f, 0.f, 0, nullptr, 1.f, nullptr, fx, nullptr) ==
           DFK_EINVAL);
    EXPECT(dfk_sgd_step_clip(fx, fx, fx, nullptr, 16, fx, 0.f, 0.9f, 0.f, 0, nullptr, 1.f, odd, fx, nullptr) ==
           DFK_EINVAL);
    EXPECT(dfk_sgd_step_runs_clip(fx, fx, fx, nullptr, runs, 2, fx, 0.f, 0.9f, 0.f, 1.f, nullptr, nullptr, nullptr) ==
           DFK_EINVAL);
    EXPECT(dfk_sgd_step_runs_clip(fx, fx, fx, nullptr, runs, 0, fx, 0.f, 0.9f, 0.f, 1.f, nullptr, fx, nullptr) ==
           DFK_EINVAL);
    EXPECT(dfk_sgd_step_runs_clip(fx, fx, fx, nullptr, runs, 65, fx, 0.f, 0.9f, 0.f, 1.f, nullptr, fx, nullptr) ==
           DFK_EINVAL);
    EXPECT(dfk_sgd_step_runs_clip(fx, fx, odd, nullptr, runs, 2, fx, 0.f, 0.9f, 0.f, 1.f, nullptr, fx, nullptr) ==
           DFK_EINVAL);
    EXPECT(dfk_adamw_step_clip(fx, fx, fx, fx, nullptr, 16, fx, 0.f, 0.9, 0.999, 1e-8f, 0.f, fx, nullptr, 1.f, nullptr,
                               nullptr, nullptr) == DFK_EINVAL);
    EXPECT(dfk_adamw_step_clip(fx, fx, fx, fx, nullptr, -4, fx, 0.f, 0.9, 0.999, 1e-8f, 0.f, fx, nullptr, 1.f, nullptr,
                               fx, nullptr) == DFK_EINVAL);
    EXPECT(dfk_adamw_step_clip(fx, fx, fx, odd, nullptr, 16, fx, 0.f, 0.9, 0.999, 1e-8f, 0.f, fx, nullptr, 1.f, nullptr,
                               fx, nullptr) == DFK_EINVAL);
    EXPECT(dfk_adamw_step_clip(fx, fx, fx, fx, nullptr, 16, fx, 0.f, 0.9, 0.999, 0.f, 0.f, fx, nullptr, 1.f, nullptr,
                               fx, nullptr) == DFK_EINVAL);                // eps = 0
    EXPECT(dfk_adamw_step_runs_clip(fx, fx, fx, fx, nullptr, runs, 2, fx, 0.f, 0.9, 0.999, 1e-8f, 0.f, fx, 1, 1.f,
                                    nullptr, nullptr, nullptr) == DFK_EINVAL);
    EXPECT(dfk_adamw_step_runs_clip(fx, fx, fx, fx, nullptr, runs, 65, fx, 0.f, 0.9, 0.999, 1e-8f, 0.f, fx, 1, 1.f,
                                    nullptr, fx, nullptr) == DFK_EINVAL);
    EXPECT(dfk_adamw_step_runs_clip(fx, fx, fx, fx, nullptr, runs, 2, fx, 0.f, 0.9, 0.999, 1e-8f, 0.f, fx, 1, 1.f,
                                    odd, fx, nullptr) == DFK_EINVAL);      // grad_bf16 not 8-B aligned
  }
  {
    // parameter groups: the *_runs_groups entry points reject a missing / misaligned table, a group count outside
    // 1..256 and a map shorter than the runs reach, and keep their twins' run-table / alignment / hyper-parameter rules
    float* fx = reinterpret_cast<float*>(0x10000);
    float* odd = reinterpret_cast<float*>(0x10004);
    const uint8_t* gm = reinterpret_cast<const uint8_t*>(0x40001);         // the map needs no alignment
    int64_t runs[65 * 4];
    for (int r = 0; r < 65; ++r) { runs[4 * r] = 64 * r; runs[4 * r + 1] = 40; runs[4 * r + 2] = 0; runs[4 * r + 3] = 0; }
    // two runs end at element 104: 13 map bytes
    EXPECT(dfk_sgd_step_runs_groups(fx, fx, fx, nullptr, runs, 2, fx, 0.f, 0.9f, nullptr, 13, fx, 3, 1.f, nullptr,
                                    nullptr, nullptr) == DFK_EINVAL);
    EXPECT(dfk_sgd_step_runs_groups(fx, fx, fx, nullptr, runs, 2, fx, 0.f, 0.9f, gm, 13, nullptr, 3, 1.f, nullptr,
                                    nullptr, nullptr) == DFK_EINVAL);
    EXPECT(dfk_sgd_step_runs_groups(fx, fx, fx, nullptr, runs, 2, fx, 0.f, 0.9f, gm, 13, odd, 3, 1.f, nullptr,
                                    nullptr, nullptr) == DFK_EINVAL);      // pairs not 8-B aligned
    for (int32_t bad : {0, -1, 257})
      EXPECT(dfk_sgd_step_runs_groups(fx, fx, fx, nullptr, runs, 2, fx, 0.f, 0.9f, gm, 13, fx, bad, 1.f, nullptr,
                                      nullptr, nullptr) == DFK_EINVAL);
    for (int64_t bad : {(int64_t)12, (int64_t)0, (int64_t)-1})
      EXPECT(dfk_sgd_step_runs_groups(fx, fx, fx, nullptr, runs, 2, fx, 0.f, 0.9f, gm, bad, fx, 3, 1.f, nullptr,
                                      nullptr, nullptr) == DFK_EINVAL);    // map shorter than ceil(104 / 8)
    EXPECT(dfk_sgd_step_runs_groups(fx, fx, fx, nullptr, runs, 65, fx, 0.f, 0.9f, gm, 1024, fx, 3, 1.f, nullptr,
                                    nullptr, nullptr) == DFK_ENOTSUP);
    EXPECT(dfk_sgd_step_runs_groups(fx, fx, fx, nullptr, runs, 65, fx, 0.f, 0.9f, gm, 1024, fx, 3, 1.f, nullptr, fx,
                                    nullptr) == DFK_ENOTSUP);              // with a clip coefficient too
    EXPECT(dfk_sgd_step_runs_groups(fx, fx, fx, nullptr, runs, 0, fx, 0.f, 0.9f, gm, 13, fx, 3, 1.f, nullptr, nullptr,
                                    nullptr) == DFK_EINVAL);
    EXPECT(dfk_sgd_step_runs_groups(fx, fx, fx, nullptr, nullptr, 2, fx, 0.f, 0.9f, gm, 13, fx, 3, 1.f, nullptr,
                                    nullptr, nullptr) == DFK_EINVAL);
    EXPECT(dfk_sgd_step_runs_groups(nullptr, fx, fx, nullptr, runs, 2, fx, 0.f, 0.9f, gm, 13, fx, 3, 1.f, nullptr,
                                    nullptr, nullptr) == DFK_EINVAL);
    EXPECT(dfk_sgd_step_runs_groups(fx, fx, odd, nullptr, runs, 2, fx, 0.f, 0.9f, gm, 13, fx, 3, 1.f, nullptr, nullptr,
                                    nullptr) == DFK_EINVAL);
    EXPECT(dfk_sgd_step_runs_groups(fx, fx, fx, odd, runs, 2, fx, 0.f, 0.9f, gm, 13, fx, 3, 1.f, nullptr, nullptr,
                                    nullptr) == DFK_EINVAL);               // shadow not 8-B aligned
    EXPECT(dfk_sgd_step_runs_groups(fx, fx, fx, nullptr, runs, 2, fx, 0.f, 0.9f, gm, 13, fx, 3, 1.f, odd, nullptr,
                                    nullptr) == DFK_EINVAL);               // grad_bf16 not 8-B aligned
    EXPECT(dfk_adamw_step_runs_groups(fx, fx, fx, fx, nullptr, runs, 2, fx, 0.f, 0.9, 0.999, 1e-8f, fx, 1, nullptr, 13,
                                      fx, 3, 1.f, nullptr, nullptr, nullptr) == DFK_EINVAL);
    EXPECT(dfk_adamw_step_runs_groups(fx, fx, fx, fx, nullptr, runs, 2, fx, 0.f, 0.9, 0.999, 1e-8f, fx, 1, gm, 13,
                                      nullptr, 3, 1.f, nullptr, nullptr, nullptr) == DFK_EINVAL);
    EXPECT(dfk_adamw_step_runs_groups(fx, fx, fx, fx, nullptr, runs, 2, fx, 0.f, 0.9, 0.999, 1e-8f, fx, 1, gm, 13,
                                      odd, 3, 1.f, nullptr, nullptr, nullptr) == DFK_EINVAL);
    for (int32_t bad : {0, -1, 257})
      EXPECT(dfk_adamw_step_runs_groups(fx, fx, fx, fx, nullptr, runs, 2, fx, 0.f, 0.9, 0.999, 1e-8f, fx, 1, gm, 13,
                                        fx, bad, 1.f, nullptr, nullptr, nullptr) == DFK_EINVAL);
    EXPECT(dfk_adamw_step_runs_groups(fx, fx, fx, fx, nullptr, runs, 2, fx, 0.f, 0.9, 0.999, 1e-8f, fx, 1, gm, 12, fx,
                                      3, 1.f, nullptr, nullptr, nullptr) == DFK_EINVAL);
    EXPECT(dfk_adamw_step_runs_groups(fx, fx, fx, fx, nullptr, runs, 2, fx, 0.f, 0.9, 0.999, 1e-8f, fx, 1, gm, 12, fx,
                                      3, 1.f, nullptr, fx, nullptr) == DFK_EINVAL);
    EXPECT(dfk_adamw_step_runs_groups(fx, fx, fx, fx, nullptr, runs, 65, fx, 0.f, 0.9, 0.999, 1e-8f, fx, 1, gm, 1024,
                                      fx, 3, 1.f, nullptr, nullptr, nullptr) == DFK_ENOTSUP);
    EXPECT(dfk_adamw_step_runs_groups(fx, fx, fx, fx, nullptr, runs, 2, fx, 0.f, 0.9, 0.999, 1e-8f, fx, 65, gm, 13, fx,
                                      3, 1.f, nullptr, nullptr, nullptr) == DFK_ENOTSUP);
    EXPECT(dfk_adamw_step_runs_groups(fx, fx, fx, fx, nullptr, runs, 2, fx, 0.f, 0.9, 0.999, 1e-8f, nullptr, 1, gm, 13,
                                      fx, 3, 1.f, nullptr, nullptr, nullptr) == DFK_EINVAL);   // no corrections
    EXPECT(dfk_adamw_step_runs_groups(fx, fx, fx, fx, nullptr, runs, 2, fx, 0.f, 1.0, 0.999, 1e-8f, fx, 1, gm, 13, fx,
                                      3, 1.f, nullptr, nullptr, nullptr) == DFK_EINVAL);       // b1 = 1
    EXPECT(dfk_adamw_step_runs_groups(fx, fx, fx, fx, nullptr, runs, 2, fx, 0.f, 0.9, 0.999, 0.f, fx, 1, gm, 13, fx, 3,
                                      1.f, nullptr, nullptr, nullptr) == DFK_EINVAL);          // eps = 0
    EXPECT(dfk_adamw_step_runs_groups(fx, fx, odd, fx, nullptr, runs, 2, fx, 0.f, 0.9, 0.999, 1e-8f, fx, 1, gm, 13, fx,
                                      3, 1.f, nullptr, nullptr, nullptr) == DFK_EINVAL);
    runs[7] = 1;                                                           // class index beyond nclass
    EXPECT(dfk_adamw_step_runs_groups(fx, fx, fx, fx, nullptr, runs, 2, fx, 0.f, 0.9, 0.999, 1e-8f, fx, 1, gm, 13, fx,
                                      3, 1.f, nullptr, nullptr, nullptr) == DFK_EINVAL);
    runs[7] = 0; runs[4] = 66;                                             // run start not a multiple of 4
    EXPECT(dfk_adamw_step_runs_groups(fx, fx, fx, fx, nullptr, runs, 2, fx, 0.f, 0.9, 0.999, 1e-8f, fx, 1, gm, 14, fx,
                                      3, 1.f, nullptr, nullptr, nullptr) == DFK_EINVAL);
    EXPECT(dfk_sgd_step_runs_groups(fx, fx, fx, nullptr, runs, 2, fx, 0.f, 0.9f, gm, 14, fx, 3, 1.f, nullptr, nullptr,
                                    nullptr) == DFK_EINVAL);
  }
  {
    // weight EMA: the prelude, the update and the swap reject malformed calls; an empty buffer is a no-op
    float* fx = reinterpret_cast<float*>(0x10000);
    float* fy = reinterpret_cast<float*>(0x20000);
    float* odd = reinterpret_cast<float*>(0x10004);
    int32_t* cnt = reinterpret_cast<int32_t*>(0x30000);
    void* sh = reinterpret_cast<void*>(0x40000);
    const double inf = 1.0 / 0.0, nan = inf - inf;
    EXPECT(dfk_ema_prelude(nullptr, fx, 0.9, 0, nullptr) == DFK_EINVAL);
    EXPECT(dfk_ema_prelude(cnt, nullptr, 0.9, 0, nullptr) == DFK_EINVAL);
    EXPECT(dfk_ema_prelude(cnt, odd, 0.9, 0, nullptr) == DFK_EINVAL);                     // weight not 16-B aligned
    EXPECT(dfk_ema_prelude(reinterpret_cast<int32_t*>(0x30002), fx, 0.9, 0, nullptr) == DFK_EINVAL);
    for (double bad : {-0.1, 1.0, 1.5, inf, -inf, nan}) EXPECT(dfk_ema_prelude(cnt, fx, bad, 1, nullptr) == DFK_EINVAL);
    EXPECT(dfk_ema_update(nullptr, fy, 16, fx, nullptr) == DFK_EINVAL);
    EXPECT(dfk_ema_update(fx, nullptr, 16, fx, nullptr) == DFK_EINVAL);
    EXPECT(dfk_ema_update(fx, fy, 16, nullptr, nullptr) == DFK_EINVAL);
    EXPECT(dfk_ema_update(fx, fx, 16, fy, nullptr) == DFK_EINVAL);                        // param and ema alias
    EXPECT(dfk_ema_update(fx, fy, -4, fx, nullptr) == DFK_EINVAL);
    EXPECT(dfk_ema_update(odd, fy, 16, fx, nullptr) == DFK_EINVAL);
    EXPECT(dfk_ema_update(fx, odd, 16, fy, nullptr) == DFK_EINVAL);
    EXPECT(dfk_ema_update(fx, fy, 16, odd, nullptr) == DFK_EINVAL);
    EXPECT(dfk_ema_update(fx, fy, (int64_t)1 << 43, fx, nullptr) == DFK_EINVAL);          // grid beyond int32
    EXPECT(dfk_ema_update(fx, fy, 0, fx, nullptr) == 0);
    EXPECT(dfk_ema_swap(nullptr, fy, sh, 16, nullptr) == DFK_EINVAL);
    EXPECT(dfk_ema_swap(fx, nullptr, sh, 16, nullptr) == DFK_EINVAL);
    EXPECT(dfk_ema_swap(fx, fx, sh, 16, nullptr) == DFK_EINVAL);
    EXPECT(dfk_ema_swap(fx, fy, sh, -4, nullptr) == DFK_EINVAL);
    EXPECT(dfk_ema_swap(odd, fy, sh, 16, nullptr) == DFK_EINVAL);
    EXPECT(dfk_ema_swap(fx, odd, nullptr, 16, nullptr) == DFK_EINVAL);
    EXPECT(dfk_ema_swap(fx, fy, odd, 16, nullptr) == DFK_EINVAL);                         // shadow not 8-B aligned
    EXPECT(dfk_ema_swap(fx, fy, nullptr, (int64_t)1 << 43, nullptr) == DFK_EINVAL);
    EXPECT(dfk_ema_swap(fx, fy, nullptr, 0, nullptr) == 0);
  }
  {
    // wav2vec2 layer-norm feature encoder: planners, then null operands, B <= 0, S < 10, rows <= 0, a channel
    // count other than 512, misaligned pointers, a bad dtype, a short scratch: all before any launch
    float* fx = reinterpret_cast<float*>(0x10000);
    float* odd = reinterpret_cast<float*>(0x10004);
    void* vx = reinterpret_cast<void*>(0x20000);
    void* vodd = reinterpret_cast<void*>(0x20008);
    const int64_t ws0 = dfk_w2v_conv0_ln_bwd_workspace(8, 64000);
    EXPECT(ws0 > 0 && ws0 % 16 == 0);
    EXPECT(dfk_w2v_conv0_ln_bwd_workspace(8, 9) == 0);
    EXPECT(dfk_w2v_conv0_ln_bwd_workspace(0, 64000) == 0);
    EXPECT(dfk_w2v_conv0_ln_bwd_workspace(2, 14) == (int64_t)4 * 2 * (512 * 10 + 3 * 512));   // T0 = 1: one workgroup per clip
    const int64_t ws1 = dfk_w2v_ln_gelu_bwd_workspace(51192);
    EXPECT(ws1 > 0 && ws1 % 16 == 0);
    EXPECT(dfk_w2v_ln_gelu_bwd_workspace(0) == 0);
    EXPECT(dfk_w2v_ln_gelu_bwd_workspace(-3) == 0);
    EXPECT(dfk_w2v_ln_gelu_bwd_workspace(1) == (int64_t)4 * 3 * 512);
    // conv0 forward
    EXPECT(dfk_w2v_conv0_ln_fwd(nullptr, 8, 64000, fx, fx, fx, fx, 1e-5f, fx, vx, DFK_BF16, nullptr) == DFK_EINVAL);
    EXPECT(dfk_w2v_conv0_ln_fwd(fx, 8, 64000, nullptr, fx, fx, fx, 1e-5f, fx, vx, DFK_BF16, nullptr) == DFK_EINVAL);
    EXPECT(dfk_w2v_conv0_ln_fwd(fx, 8, 64000, fx, fx, nullptr, fx, 1e-5f, fx, vx, DFK_BF16, nullptr) == DFK_EINVAL);
    EXPECT(dfk_w2v_conv0_ln_fwd(fx, 8, 64000, fx, fx, fx, nullptr, 1e-5f, fx, vx, DFK_BF16, nullptr) == DFK_EINVAL);
    EXPECT(dfk_w2v_conv0_ln_fwd(fx, 8, 64000, fx, fx, fx, fx, 1e-5f, nullptr, vx, DFK_BF16, nullptr) == DFK_EINVAL);
    EXPECT(dfk_w2v_conv0_ln_fwd(fx, 8, 64000, fx, fx, fx, fx, 1e-5f, fx, nullptr, DFK_BF16, nullptr) == DFK_EINVAL);
    EXPECT(dfk_w2v_conv0_ln_fwd(fx, 0, 64000, fx, fx, fx, fx, 1e-5f, fx, vx, DFK_BF16, nullptr) == DFK_EINVAL);
    EXPECT(dfk_w2v_conv0_ln_fwd(fx, -1, 64000, fx, fx, fx, fx, 1e-5f, fx, vx, DFK_BF16, nullptr) == DFK_EINVAL);
    EXPECT(dfk_w2v_conv0_ln_fwd(fx, 65536, 64000, fx, fx, fx, fx, 1e-5f, fx, vx, DFK_BF16, nullptr) == DFK_EINVAL);
    EXPECT(dfk_w2v_conv0_ln_fwd(fx, 8, 9, fx, fx, fx, fx, 1e-5f, fx, vx, DFK_BF16, nullptr) == DFK_EINVAL);
    EXPECT(dfk_w2v_conv0_ln_fwd(fx, 8, 64000, fx, fx, fx, fx, 1e-5f, fx, vx, 7, nullptr) == DFK_EINVAL);
    EXPECT(dfk_w2v_conv0_ln_fwd(fx, 8, 64000, odd, fx, fx, fx, 1e-5f, fx, vx, DFK_BF16, nullptr) == DFK_EINVAL);
    EXPECT(dfk_w2v_conv0_ln_fwd(fx, 8, 64000, fx, odd, fx, fx, 1e-5f, fx, vx, DFK_BF16, nullptr) == DFK_EINVAL);
    EXPECT(dfk_w2v_conv0_ln_fwd(fx, 8, 64000, fx, fx, odd, fx, 1e-5f, fx, vx, DFK_BF16, nullptr) == DFK_EINVAL);
    EXPECT(dfk_w2v_conv0_ln_fwd(fx, 8, 64000, fx, fx, fx, odd, 1e-5f, fx, vx, DFK_BF16, nullptr) == DFK_EINVAL);
    EXPECT(dfk_w2v_conv0_ln_fwd(fx, 8, 64000, fx, fx, fx, fx, 1e-5f, odd, vx, DFK_BF16, nullptr) == DFK_EINVAL);
    EXPECT(dfk_w2v_conv0_ln_fwd(fx, 8, 64000, fx, fx, fx, fx, 1e-5f, fx, vodd, DFK_BF16, nullptr) == DFK_EINVAL);
    // conv0 backward
    EXPECT(dfk_w2v_conv0_ln_bwd(nullptr, 8, 64000, fx, fx, fx, fx, fx, vx, DFK_BF16, fx, ws0, fx, fx, fx, fx, nullptr) ==
           DFK_EINVAL);
    EXPECT(dfk_w2v_conv0_ln_bwd(fx, 8, 64000, fx, fx, fx, fx, nullptr, vx, DFK_BF16, fx, ws0, fx, fx, fx, fx, nullptr) ==
           DFK_EINVAL);
    EXPECT(dfk_w2v_conv0_ln_bwd(fx, 8, 64000, fx, fx, fx, fx, fx, nullptr, DFK_BF16, fx, ws0, fx, fx, fx, fx, nullptr) ==
           DFK_EINVAL);
    EXPECT(dfk_w2v_conv0_ln_bwd(fx, 8, 64000, fx, fx, fx, fx, fx, vx, DFK_BF16, nullptr, ws0, fx, fx, fx, fx, nullptr) ==
           DFK_EINVAL);
    EXPECT(dfk_w2v_conv0_ln_bwd(fx, 8, 64000, fx, fx, fx, fx, fx, vx, DFK_BF16, fx, ws0, nullptr, fx, fx, fx, nullptr) ==
           DFK_EINVAL);                                                    // no dw sink
    EXPECT(dfk_w2v_conv0_ln_bwd(fx, 8, 64000, fx, fx, fx, fx, fx, vx, DFK_BF16, fx, ws0, fx, nullptr, fx, fx, nullptr) ==
           DFK_EINVAL);                                                    // a bias without its sink
    EXPECT(dfk_w2v_conv0_ln_bwd(fx, 8, 64000, fx, nullptr, fx, fx, fx, vx, DFK_BF16, fx, ws0, fx, fx, fx, fx, nullptr) ==
           DFK_EINVAL);                                                    // a bias sink without the bias
    EXPECT(dfk_w2v_conv0_ln_bwd(fx, 8, 64000, fx, fx, fx, fx, fx, vx, DFK_BF16, fx, ws0 - 1, fx, fx, fx, fx, nullptr) ==
           DFK_EINVAL);                                                    // short scratch
    EXPECT(dfk_w2v_conv0_ln_bwd(fx, 8, 64000, fx, fx, fx, fx, fx, vx, DFK_BF16, odd, ws0, fx, fx, fx, fx, nullptr) ==
           DFK_EINVAL);                                                    // scratch not 16-B aligned
    EXPECT(dfk_w2v_conv0_ln_bwd(fx, 8, 64000, fx, fx, fx, fx, fx, vodd, DFK_BF16, fx, ws0, fx, fx, fx, fx, nullptr) ==
           DFK_EINVAL);
    EXPECT(dfk_w2v_conv0_ln_bwd(fx, 0, 64000, fx, fx, fx, fx, fx, vx, DFK_BF16, fx, ws0, fx, fx, fx, fx, nullptr) ==
           DFK_EINVAL);
    EXPECT(dfk_w2v_conv0_ln_bwd(fx, 8, 5, fx, fx, fx, fx, fx, vx, DFK_BF16, fx, ws0, fx, fx, fx, fx, nullptr) ==
           DFK_EINVAL);
    EXPECT(dfk_w2v_conv0_ln_bwd(fx, 8, 64000, fx, fx, fx, fx, fx, vx, -1, fx, ws0, fx, fx, fx, fx, nullptr) == DFK_EINVAL);
    // row kernels
    EXPECT(dfk_w2v_ln_gelu_fwd(nullptr, 100, 512, fx, fx, 1e-5f, fx, vx, DFK_BF16, nullptr) == DFK_EINVAL);
    EXPECT(dfk_w2v_ln_gelu_fwd(vx, 100, 512, nullptr, fx, 1e-5f, fx, vx, DFK_BF16, nullptr) == DFK_EINVAL);
    EXPECT(dfk_w2v_ln_gelu_fwd(vx, 100, 512, fx, nullptr, 1e-5f, fx, vx, DFK_BF16, nullptr) == DFK_EINVAL);
    EXPECT(dfk_w2v_ln_gelu_fwd(vx, 100, 512, fx, fx, 1e-5f, nullptr, vx, DFK_BF16, nullptr) == DFK_EINVAL);
    EXPECT(dfk_w2v_ln_gelu_fwd(vx, 100, 512, fx, fx, 1e-5f, fx, nullptr, DFK_BF16, nullptr) == DFK_EINVAL);
    EXPECT(dfk_w2v_ln_gelu_fwd(vx, 0, 512, fx, fx, 1e-5f, fx, vx, DFK_BF16, nullptr) == DFK_EINVAL);
    EXPECT(dfk_w2v_ln_gelu_fwd(vx, -5, 512, fx, fx, 1e-5f, fx, vx, DFK_BF16, nullptr) == DFK_EINVAL);
    for (int64_t badc : {(int64_t)0, (int64_t)256, (int64_t)768, (int64_t)1024})
      EXPECT(dfk_w2v_ln_gelu_fwd(vx, 100, badc, fx, fx, 1e-5f, fx, vx, DFK_BF16, nullptr) == DFK_EINVAL);
    EXPECT(dfk_w2v_ln_gelu_fwd(vx, 100, 512, fx, fx, 1e-5f, fx, vx, 2, nullptr) == DFK_EINVAL);
    EXPECT(dfk_w2v_ln_gelu_fwd(vodd, 100, 512, fx, fx, 1e-5f, fx, vx, DFK_BF16, nullptr) == DFK_EINVAL);
    EXPECT(dfk_w2v_ln_gelu_fwd(vx, 100, 512, odd, fx, 1e-5f, fx, vx, DFK_BF16, nullptr) == DFK_EINVAL);
    EXPECT(dfk_w2v_ln_gelu_fwd(vx, 100, 512, fx, fx, 1e-5f, odd, vx, DFK_BF16, nullptr) == DFK_EINVAL);
    EXPECT(dfk_w2v_ln_gelu_fwd(vx, 100, 512, fx, fx, 1e-5f, fx, vodd, DFK_BF16, nullptr) == DFK_EINVAL);
    EXPECT(dfk_w2v_ln_gelu_bwd(nullptr, vx, 100, 512, fx, fx, fx, vx, DFK_BF16, fx, ws1, fx, fx, fx, nullptr) == DFK_EINVAL);
    EXPECT(dfk_w2v_ln_gelu_bwd(vx, nullptr, 100, 512, fx, fx, fx, vx, DFK_BF16, fx, ws1, fx, fx, fx, nullptr) == DFK_EINVAL);
    EXPECT(dfk_w2v_ln_gelu_bwd(vx, vx, 100, 512, fx, fx, nullptr, vx, DFK_BF16, fx, ws1, fx, fx, fx, nullptr) == DFK_EINVAL);
    EXPECT(dfk_w2v_ln_gelu_bwd(vx, vx, 100, 512, fx, fx, fx, nullptr, DFK_BF16, fx, ws1, fx, fx, fx, nullptr) == DFK_EINVAL);
    EXPECT(dfk_w2v_ln_gelu_bwd(vx, vx, 100, 512, fx, fx, fx, vx, DFK_BF16, nullptr, ws1, fx, fx, fx, nullptr) == DFK_EINVAL);
    EXPECT(dfk_w2v_ln_gelu_bwd(vx, vx, 0, 512, fx, fx, fx, vx, DFK_BF16, fx, ws1, fx, fx, fx, nullptr) == DFK_EINVAL);
    EXPECT(dfk_w2v_ln_gelu_bwd(vx, vx, 100, 511, fx, fx, fx, vx, DFK_BF16, fx, ws1, fx, fx, fx, nullptr) == DFK_EINVAL);
    EXPECT(dfk_w2v_ln_gelu_bwd(vx, vx, 100, 512, fx, fx, fx, vx, DFK_BF16, fx, 100, fx, fx, fx, nullptr) == DFK_EINVAL);
    EXPECT(dfk_w2v_ln_gelu_bwd(vodd, vx, 100, 512, fx, fx, fx, vx, DFK_BF16, fx, ws1, fx, fx, fx, nullptr) == DFK_EINVAL);
    EXPECT(dfk_w2v_ln_gelu_bwd(vx, vx, 100, 512, fx, fx, fx, vodd, DFK_BF16, fx, ws1, fx, fx, fx, nullptr) == DFK_EINVAL);
    EXPECT(dfk_w2v_ln_gelu_bwd(vx, vx, 100, 512, fx, fx, fx, vx, DFK_BF16, odd, ws1, fx, fx, fx, nullptr) == DFK_EINVAL);
    EXPECT(dfk_w2v_ln_gelu_bwd(vx, vx, 100, 512, fx, fx, fx, vx, 9, fx, ws1, fx, fx, fx, nullptr) == DFK_EINVAL);
  }
  {
    // wav2vec2 group-norm conv0 with per-clip lengths: null operands (the lengths included), B <= 0 or past the
    // grid, S < 10, a bad dtype, a short scratch: all before any launch
    float* fx = reinterpret_cast<float*>(0x10000);
    void* vx = reinterpret_cast<void*>(0x20000);
    const int64_t* ln = reinterpret_cast<const int64_t*>(0x30000);
    const int64_t ws0 = dfk_w2v_conv0_bwd_workspace(8, 64000);
    EXPECT(ws0 > 0);
    EXPECT(dfk_w2v_conv0_ragged_fwd(nullptr, 8, 64000, fx, fx, fx, 1e-5f, fx, vx, DFK_BF16, fx, ln, nullptr) == DFK_EINVAL);
    EXPECT(dfk_w2v_conv0_ragged_fwd(fx, 8, 64000, nullptr, fx, fx, 1e-5f, fx, vx, DFK_BF16, fx, ln, nullptr) == DFK_EINVAL);
    EXPECT(dfk_w2v_conv0_ragged_fwd(fx, 8, 64000, fx, nullptr, fx, 1e-5f, fx, vx, DFK_BF16, fx, ln, nullptr) == DFK_EINVAL);
    EXPECT(dfk_w2v_conv0_ragged_fwd(fx, 8, 64000, fx, fx, nullptr, 1e-5f, fx, vx, DFK_BF16, fx, ln, nullptr) == DFK_EINVAL);
    EXPECT(dfk_w2v_conv0_ragged_fwd(fx, 8, 64000, fx, fx, fx, 1e-5f, nullptr, vx, DFK_BF16, fx, ln, nullptr) == DFK_EINVAL);
    EXPECT(dfk_w2v_conv0_ragged_fwd(fx, 8, 64000, fx, fx, fx, 1e-5f, fx, nullptr, DFK_BF16, fx, ln, nullptr) == DFK_EINVAL);
    EXPECT(dfk_w2v_conv0_ragged_fwd(fx, 8, 64000, fx, fx, fx, 1e-5f, fx, vx, DFK_BF16, nullptr, ln, nullptr) == DFK_EINVAL);
    EXPECT(dfk_w2v_conv0_ragged_fwd(fx, 8, 64000, fx, fx, fx, 1e-5f, fx, vx, DFK_BF16, fx, nullptr, nullptr) == DFK_EINVAL);
    EXPECT(dfk_w2v_conv0_ragged_fwd(fx, 0, 64000, fx, fx, fx, 1e-5f, fx, vx, DFK_BF16, fx, ln, nullptr) == DFK_EINVAL);
    EXPECT(dfk_w2v_conv0_ragged_fwd(fx, -1, 64000, fx, fx, fx, 1e-5f, fx, vx, DFK_BF16, fx, ln, nullptr) == DFK_EINVAL);
    EXPECT(dfk_w2v_conv0_ragged_fwd(fx, 65536, 64000, fx, fx, fx, 1e-5f, fx, vx, DFK_BF16, fx, ln, nullptr) == DFK_EINVAL);
    EXPECT(dfk_w2v_conv0_ragged_fwd(fx, 8, 9, fx, fx, fx, 1e-5f, fx, vx, DFK_BF16, fx, ln, nullptr) == DFK_EINVAL);
    EXPECT(dfk_w2v_conv0_ragged_fwd(fx, 8, ((int64_t)1 << 31) + 1, fx, fx, fx, 1e-5f, fx, vx, DFK_BF16, fx, ln, nullptr) ==
           DFK_EINVAL);
    EXPECT(dfk_w2v_conv0_ragged_fwd(fx, 8, 64000, fx, fx, fx, 1e-5f, fx, vx, 7, fx, ln, nullptr) == DFK_EINVAL);
    EXPECT(dfk_w2v_conv0_ragged_fwd(fx, 8, 64000, fx, fx, fx, 1e-5f, fx, vx, -1, fx, ln, nullptr) == DFK_EINVAL);
    EXPECT(dfk_w2v_conv0_ragged_bwd(nullptr, 8, 64000, fx, fx, fx, 1e-5f, fx, vx, DFK_BF16, fx, ws0, fx, fx, fx, ln, nullptr) ==
           DFK_EINVAL);
    EXPECT(dfk_w2v_conv0_ragged_bwd(fx, 8, 64000, nullptr, fx, fx, 1e-5f, fx, vx, DFK_BF16, fx, ws0, fx, fx, fx, ln, nullptr) ==
           DFK_EINVAL);
    EXPECT(dfk_w2v_conv0_ragged_bwd(fx, 8, 64000, fx, nullptr, fx, 1e-5f, fx, vx, DFK_BF16, fx, ws0, fx, fx, fx, ln, nullptr) ==
           DFK_EINVAL);
    EXPECT(dfk_w2v_conv0_ragged_bwd(fx, 8, 64000, fx, fx, nullptr, 1e-5f, fx, vx, DFK_BF16, fx, ws0, fx, fx, fx, ln, nullptr) ==
           DFK_EINVAL);
    EXPECT(dfk_w2v_conv0_ragged_bwd(fx, 8, 64000, fx, fx, fx, 1e-5f, nullptr, vx, DFK_BF16, fx, ws0, fx, fx, fx, ln, nullptr) ==
           DFK_EINVAL);
    EXPECT(dfk_w2v_conv0_ragged_bwd(fx, 8, 64000, fx, fx, fx, 1e-5f, fx, nullptr, DFK_BF16, fx, ws0, fx, fx, fx, ln, nullptr) ==
           DFK_EINVAL);
    EXPECT(dfk_w2v_conv0_ragged_bwd(fx, 8, 64000, fx, fx, fx, 1e-5f, fx, vx, DFK_BF16, nullptr, ws0, fx, fx, fx, ln, nullptr) ==
           DFK_EINVAL);
    EXPECT(dfk_w2v_conv0_ragged_bwd(fx, 8, 64000, fx, fx, fx, 1e-5f, fx, vx, DFK_BF16, fx, ws0, nullptr, fx, fx, ln, nullptr) ==
           DFK_EINVAL);                                                    // no dw sink
    EXPECT(dfk_w2v_conv0_ragged_bwd(fx, 8, 64000, fx, fx, fx, 1e-5f, fx, vx, DFK_BF16, fx, ws0, fx, fx, fx, nullptr, nullptr) ==
           DFK_EINVAL);                                                    // no lengths
    EXPECT(dfk_w2v_conv0_ragged_bwd(fx, 8, 64000, fx, fx, fx, 1e-5f, fx, vx, DFK_BF16, fx, ws0 - 1, fx, fx, fx, ln, nullptr) ==
           DFK_EINVAL);                                                    // short scratch
    EXPECT(dfk_w2v_conv0_ragged_bwd(fx, 8, 64000, fx, fx, fx, 1e-5f, fx, vx, DFK_BF16, fx, 0, fx, fx, fx, ln, nullptr) ==
           DFK_EINVAL);
    EXPECT(dfk_w2v_conv0_ragged_bwd(fx, 0, 64000, fx, fx, fx, 1e-5f, fx, vx, DFK_BF16, fx, ws0, fx, fx, fx, ln, nullptr) ==
           DFK_EINVAL);
    EXPECT(dfk_w2v_conv0_ragged_bwd(fx, -3, 64000, fx, fx, fx, 1e-5f, fx, vx, DFK_BF16, fx, ws0, fx, fx, fx, ln, nullptr) ==
           DFK_EINVAL);
    EXPECT(dfk_w2v_conv0_ragged_bwd(fx, 65536, 64000, fx, fx, fx, 1e-5f, fx, vx, DFK_BF16, fx, INT64_MAX, fx, fx, fx, ln,
                                    nullptr) == DFK_EINVAL);
    EXPECT(dfk_w2v_conv0_ragged_bwd(fx, 8, 5, fx, fx, fx, 1e-5f, fx, vx, DFK_BF16, fx, ws0, fx, fx, fx, ln, nullptr) ==
           DFK_EINVAL);
    EXPECT(dfk_w2v_conv0_ragged_bwd(fx, 8, 64000, fx, fx, fx, 1e-5f, fx, vx, 2, fx, ws0, fx, fx, fx, ln, nullptr) ==
           DFK_EINVAL);
  }
  EXPECT(dfk_cpb_bias_fwd(nullptr, nullptr, nullptr, nullptr, nullptr, 169, 512, 64, nullptr) != 0);
  std::printf("host_check: %s (%d failures)\n", fails ? "FAILED" : "ok", fails);
  return fails ? 1 : 0;
}
