"""Device time of the wav2vec2 attention core on long clips: bf16, B = 8, 16 heads, hd 64, forward and backward timed
separately.  Cases:
  (a) T = 199 and (b) T = 499: the resident forward v3 (the default) against the streaming forward v3s
      (dfk_wattn_fwd_policy version 7), same process, interleaved — the only sizes where both run, so they decide
      where v3s takes over from v3;
  (c) T = 799 (16 s) and (d) T = 1499 (30 s): v3s only (v3's K / V image does not fit LDS: nothing to compare against),
      without klen and with klen uniform in [T / 2, T].
The backward is wattn_bwd3_kernel in query chunks at every size; it is timed from the default forward's outputs.
HIP events on the op's stream around `inner` back-to-back calls, median over `reps` repeats, after a warm-up of every
case; the cases are timed interleaved in each repeat.  FLOP: 4 kn^2 hd per (clip, head) forward, 10 kn^2 hd backward
(kn = T without klen); the fraction is of the 2516.6 TFLOP/s dense bf16 matrix peak.  Prints one JSON line, then a
markdown table.  Extra resident sizes (v3 against v3s, to place the crossover between (a) and (b)) can be
appended as a comma-separated list of T.
Usage: python tools/wattn_long_bench.py [reps] [inner] [T,T,...]"""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from deepfake_amd import kernels as K  # noqa: E402

B, HEADS, HD = 8, 16, 64
PEAK_TFLOPS = 2516.6   # MI355X dense bf16 MFMA, spec
SHAPES = [("a", 199, True), ("b", 499, True), ("c", 799, False), ("d", 1499, False)]   # (case, T, v3 can run it)


def timed(fn, inner):
    """Milliseconds per call: events recorded on the current stream around `inner` calls."""
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(inner):
        fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) / inner


def make_case(T, g, klen):
    C = HEADS * HD
    qkv = (0.5 * torch.randn(B * T, 3 * C, generator=g)).cuda().to(torch.bfloat16)
    do = torch.randn(B * T, C, generator=g).cuda().to(torch.bfloat16)
    dqkv = torch.empty_like(qkv)
    dims, win, shift, scale = (B, 1, 1, T), (1, 1, T), (0, 0, 0), HD ** -0.5
    kw = {} if klen is None else {"klen": klen}

    def fwd(version):
        def run():
            K.wattn_fwd_policy(version, -1)
            return K.wattn_fwd(qkv, qkv[:, C:], qkv[:, 2 * C:], qkv.stride(0), dims, win, win, shift, HEADS, HD, scale,
                               **kw)
        return run

    out, lse = fwd(6)()

    def bwd():
        K.wattn_bwd((qkv, qkv[:, C:], qkv[:, 2 * C:], out, lse, qkv.stride(0), dims, win, win, shift, HEADS, HD, scale,
                     None, None), do, dqkv, dqkv[:, C:], dqkv[:, 2 * C:], qkv.stride(0), **kw)

    return fwd, bwd


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 30
    inner = int(sys.argv[2]) if len(sys.argv) > 2 else 10
    if not torch.cuda.is_available():
        raise SystemExit("wattn_long_bench: needs the GPU (no CPU timing)")
    extra = [int(t) for t in sys.argv[3].split(",")] if len(sys.argv) > 3 else []
    if any(4 * (-(-t // 32) * 32) * HD > 160 * 1024 for t in extra):
        raise SystemExit("wattn_long_bench: the extra sizes are resident ones (T <= 640)")
    g = torch.Generator().manual_seed(0)
    cases, work, lens_used = {}, {}, {}
    try:
        for name, T, resident in SHAPES + [("x", t, True) for t in extra]:
            variants = [("", None)]
            if not resident:
                lens = torch.randint(T // 2, T + 1, (B,), generator=g).to(torch.int32)
                lens_used[name] = lens.tolist()
                variants.append(("_klen", lens.cuda()))
            for tag, klen in variants:
                fwd, bwd = make_case(T, g, klen)
                kn2 = float(B * T * T) if klen is None else float(sum(int(n) ** 2 for n in klen.tolist()))
                key = f"{name}_T{T}{tag}"
                if resident:
                    cases[key + "_fwd_v3"] = fwd(6)
                cases[key + "_fwd_v3s"] = fwd(7) if resident else fwd(6)   # past the limit the default is v3s
                cases[key + "_bwd"] = bwd
                for k, mult in (("_fwd_v3", 4), ("_fwd_v3s", 4), ("_bwd", 10)):
                    work[key + k] = mult * kn2 * HD * HEADS
        for fn in cases.values():          # warm-up: code objects, the LDS attribute, the allocator's blocks
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in cases}
        for _ in range(reps):
            for k, fn in cases.items():
                ms[k].append(timed(fn, inner))
    finally:
        K.wattn_fwd_policy(6, -1)
    med = {k: statistics.median(v) for k, v in ms.items()}
    tflops = {k: work[k] / (med[k] * 1e-3) / 1e12 for k in cases}
    out = {"B": B, "heads": HEADS, "hd": HD, "dtype": "bf16", "reps": reps, "inner": inner,
           "ms_median": {k: round(v, 4) for k, v in med.items()},
           "ms_min": {k: round(min(v), 4) for k, v in ms.items()},
           "ms_max": {k: round(max(v), 4) for k, v in ms.items()},
           "tflops": {k: round(v, 1) for k, v in tflops.items()},
           "peak_fraction": {k: round(v / PEAK_TFLOPS, 4) for k, v in tflops.items()},
           "peak_tflops": PEAK_TFLOPS, "klen": lens_used, "device": torch.cuda.get_device_name(0)}
    print(json.dumps(out), flush=True)
    print("\n| case | median ms | min | max | TFLOP/s | of bf16 peak |\n|---|---|---|---|---|---|")
    for k in cases:
        print(f"| {k} | {med[k]:.4f} | {min(ms[k]):.4f} | {max(ms[k]):.4f} | {tflops[k]:.1f} | "
              f"{100 * tflops[k] / PEAK_TFLOPS:.2f} % |")


if __name__ == "__main__":
    main()
