"""Device time of the layer-norm wav2vec2 feature encoder against the group-norm one (the yardstick, code this
path leaves alone), at B = 8 clips of 4 s (S = 64000, T0 = 12799, conv1: 6399 frames), bf16 compute:

  conv0 forward / backward          dfk_w2v_conv0_fwd / _bwd (GroupNorm: 3 + 4 launches) against
                                    dfk_w2v_conv0_ln_fwd / _bwd (LayerNorm: 1 + 2 launches)
  conv1 forward / forward+backward  ConvGeluFn against ConvLNGeluFn (bias, LayerNorm)
  large fwd+bwd                     one forward + backward of the 24-layer w2v_large_config.json model (regularisers
                                    off), and of the 12-layer base model for orientation

HIP events on the op's stream around `inner` back-to-back calls, median over `reps` repeats after a warm-up, the
cases interleaved in each repeat (as tools/optim_bench.py).  The bytes model of conv0: 1 KB written per frame
forward (bf16), 1 KB read backward.  Prints one JSON line.
Usage: python tools/w2v_ln_bench.py [reps] [inner] [--no-model]"""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from deepfake_amd import functional as Fn  # noqa: E402
from deepfake_amd import kernels as K  # noqa: E402
from deepfake_amd.models import set_compute_dtype  # noqa: E402
from deepfake_amd.models import wav2vec2 as W  # noqa: E402

MODELS = os.path.join(os.path.dirname(os.path.abspath(W.__file__)))


def timed(fn, inner):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(inner):
        fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) / inner


def interleaved(cases, reps, inner, warm=3):
    for fn in cases.values():
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in cases}
    for _ in range(reps):
        for k, fn in cases.items():
            ms[k].append(timed(fn, inner))
    return ms


def summary(ms):
    return {k: {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
            for k, v in ms.items()}


def model_case(path, dt, wave):
    cfg = W.Wav2Vec2Config.from_json_file(os.path.join(MODELS, path)).deterministic()
    torch.manual_seed(0)
    m = set_compute_dtype(W.Wav2Vec2Model(cfg), dt).cuda().train()

    def run():
        h = m(wave)["last_hidden_state"]
        h.backward(torch.ones_like(h))
        for p in m.parameters():
            p.grad = None
    return run


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    reps = int(args[0]) if len(args) > 0 else 30
    inner = int(args[1]) if len(args) > 1 else 20
    if not torch.cuda.is_available():
        raise SystemExit("w2v_ln_bench: needs the GPU (no CPU timing)")
    dev, dt, B, S = "cuda", torch.bfloat16, 8, 64000
    g = torch.Generator(device=dev).manual_seed(0)
    wave = torch.randn(B, S, device=dev, generator=g)
    w = (0.3 * torch.randn(512, 10, device=dev, generator=g))
    bias, beta = (0.1 * torch.randn(512, device=dev, generator=g) for _ in range(2))
    gamma = 1 + 0.1 * torch.randn(512, device=dev, generator=g)
    y_gn, st_gn = K.w2v_conv0_fwd(wave, w, gamma, beta, 1e-5, dt)
    y_ln, st_ln = K.w2v_conv0_ln_fwd(wave, w, bias, gamma, beta, 1e-5, dt)
    dy = torch.randn(y_ln.shape, device=dev, generator=g).to(dt)
    sinks = [torch.zeros_like(t) for t in (w, bias, gamma, beta)]
    x1 = y_ln.detach().clone().requires_grad_(True)
    w1 = (torch.randn(512, 512, 3, device=dev, generator=g) / 40).requires_grad_(True)
    b1, g1, be1 = (t.clone().requires_grad_(True) for t in (bias, gamma, beta))
    T1 = (y_ln.shape[1] - 3) // 2 + 1
    dy1 = torch.randn(B, T1, 512, device=dev, generator=g).to(dt)

    def fb(fn):
        def run():
            fn().backward(dy1)
            x1.grad = w1.grad = b1.grad = g1.grad = be1.grad = None
        return run
    cases = {
        "conv0_gn_fwd": lambda: K.w2v_conv0_fwd(wave, w, gamma, beta, 1e-5, dt),
        "conv0_ln_fwd": lambda: K.w2v_conv0_ln_fwd(wave, w, bias, gamma, beta, 1e-5, dt),
        "conv0_gn_bwd": lambda: K.w2v_conv0_bwd(wave, w, gamma, beta, 1e-5, st_gn, dy, sinks[0], sinks[2], sinks[3]),
        "conv0_ln_bwd": lambda: K.w2v_conv0_ln_bwd(wave, w, bias, gamma, beta, st_ln, dy, *sinks),
        "conv1_gelu_fwd": lambda: Fn.ConvGeluFn.apply(x1.detach(), w1.detach(), 2),
        "conv1_ln_gelu_fwd": lambda: Fn.ConvLNGeluFn.apply(x1.detach(), w1.detach(), b1.detach(), g1.detach(),
                                                           be1.detach(), 2, 1e-5),
        "conv1_gelu_fwd_bwd": fb(lambda: Fn.ConvGeluFn.apply(x1, w1, 2)),
        "conv1_ln_gelu_fwd_bwd": fb(lambda: Fn.ConvLNGeluFn.apply(x1, w1, b1, g1, be1, 2, 1e-5)),
    }
    out = {"B": B, "S": S, "T0": y_ln.shape[1], "T1": T1, "dtype": "bf16", "reps": reps, "inner": inner,
           "ms": summary(interleaved(cases, reps, inner)), "device": torch.cuda.get_device_name(0)}
    frames = B * y_ln.shape[1]
    for k in ("conv0_gn_fwd", "conv0_ln_fwd", "conv0_gn_bwd", "conv0_ln_bwd"):
        out.setdefault("conv0_TB_per_s", {})[k] = round(frames * 1024 / (out["ms"][k]["median"] * 1e-3) / 1e12, 3)
    if "--no-model" not in sys.argv:
        models = {"base_12_fwd_bwd": model_case("w2v_base_config.json", dt, wave),
                  "large_24_fwd_bwd": model_case("w2v_large_config.json", dt, wave)}
        out["model_ms"] = summary(interleaved(models, max(reps // 3, 3), max(inner // 10, 1), warm=2))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
