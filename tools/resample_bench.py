"""Device time of the audio resampler and of the mel pipeline with and without it, at B = 8 clips of 4 s:
media.resample alone (16 kHz -> 22.05 kHz), media.mel_image from a 22.05 kHz input (the yardstick: unchanged by
the resampler), media.mel_image(..., sr_in=16000) (the resample kernel writing the STFT's padded buffer), and the
ragged path of the last (lengths= on the device): with every length full — the same work as the uniform call, so
their difference is the cost of the length-aware kernels — and with lengths uniform in [2 s, 4 s].
HIP events on the op's stream around `inner` back-to-back calls, median over `reps` repeats, after a warm-up of
every shape; the cases are timed interleaved in each repeat.  Prints one JSON line.
Usage: python tools/resample_bench.py [reps] [inner]"""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from deepfake_amd import media  # noqa: E402

B, SECONDS = 8, 4


def timed(fn, inner):
    """Milliseconds per call: events recorded on the current stream around `inner` calls."""
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(inner):
        fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) / inner


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 30
    inner = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    if not torch.cuda.is_available():
        raise SystemExit("resample_bench: needs the GPU (no CPU timing)")
    g = torch.Generator().manual_seed(0)
    x16 = (0.1 * torch.randn(B, 16000 * SECONDS, generator=g)).cuda()
    x22 = media.resample(x16)
    cases = {"resample": lambda: media.resample(x16),
             "mel_image_22k": lambda: media.mel_image(x22),
             "mel_image_from_16k": lambda: media.mel_image(x16, sr_in=16000)}
    S = x16.shape[1]
    n_full = torch.full((B,), S, dtype=torch.int64).cuda()
    n_rag = torch.randint(S // 2, S + 1, (B,), generator=g).cuda()
    cases["mel_image_from_16k_ragged_full"] = lambda: media.mel_image(x16, sr_in=16000, lengths=n_full)
    cases["mel_image_from_16k_ragged_2to4s"] = lambda: media.mel_image(x16, sr_in=16000, lengths=n_rag)
    for fn in cases.values():          # warm-up: code objects, constants, the allocator's blocks
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in cases}
    for _ in range(reps):
        for k, fn in cases.items():
            ms[k].append(timed(fn, inner))
    med = {k: statistics.median(v) for k, v in ms.items()}
    out = {"B": B, "seconds": SECONDS, "reps": reps, "inner": inner,
           "ms_median": {k: round(v, 4) for k, v in med.items()},
           "ms_min": {k: round(min(v), 4) for k, v in ms.items()},
           "ms_max": {k: round(max(v), 4) for k, v in ms.items()},
           "fused_extra_ms": round(med["mel_image_from_16k"] - med["mel_image_22k"], 4),
           "ragged_full_extra_ms": round(med["mel_image_from_16k_ragged_full"] - med["mel_image_from_16k"], 4),
           "ragged_lengths": n_rag.tolist(),
           "device": torch.cuda.get_device_name(0)}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
