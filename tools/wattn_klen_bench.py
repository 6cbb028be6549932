"""Device time of the wav2vec2 attention core (forward + backward) with per-clip key lengths, at the 4 s training
shape: B = 8, T = 199, 16 heads, hd 64, bf16.  Three cases: (a) without klen (the yardstick: a path the key lengths
must leave alone), (b) klen = T for every clip (the same work through the length-aware instantiations, so b - a is
their cost) and (c) klen uniform in the frame counts of [2 s, 4 s].  On a build without klen only (a) runs.
HIP events on the op's stream around `inner` back-to-back forward + backward pairs, median over `reps` repeats,
after a warm-up of every case; the cases are timed interleaved in each repeat.  Prints one JSON line.
Usage: python tools/wattn_klen_bench.py [reps] [inner]"""
import inspect
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from deepfake_amd import kernels as K  # noqa: E402

B, T, HEADS, HD = 8, 199, 16, 64


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
        raise SystemExit("wattn_klen_bench: needs the GPU (no CPU timing)")
    C = HEADS * HD
    g = torch.Generator().manual_seed(0)
    qkv = (0.5 * torch.randn(B * T, 3 * C, generator=g)).cuda().to(torch.bfloat16)
    do = torch.randn(B * T, C, generator=g).cuda().to(torch.bfloat16)
    dqkv = torch.empty_like(qkv)
    dims, win, shift, scale = (B, 1, 1, T), (1, 1, T), (0, 0, 0), HD ** -0.5

    def pair(**kw):
        out, lse = K.wattn_fwd(qkv, qkv[:, C:], qkv[:, 2 * C:], qkv.stride(0), dims, win, win, shift, HEADS, HD, scale,
                               **kw)
        K.wattn_bwd((qkv, qkv[:, C:], qkv[:, 2 * C:], out, lse, qkv.stride(0), dims, win, win, shift, HEADS, HD, scale,
                     None, None), do, dqkv, dqkv[:, C:], dqkv[:, 2 * C:], qkv.stride(0), **kw)

    cases = {"no_klen": lambda: pair()}
    lens = None
    if "klen" in inspect.signature(K.wattn_fwd).parameters:
        full = torch.full((B,), T, dtype=torch.int32).cuda()
        lo = (2 * 16000 - 400) // 320 + 1   # frames of a 2 s clip
        lens = torch.randint(lo, T + 1, (B,), generator=g).to(torch.int32).cuda()
        cases["klen_full"] = lambda: pair(klen=full)
        cases["klen_2to4s"] = lambda: pair(klen=lens)
    for fn in cases.values():          # warm-up: code objects, the LDS attribute, the allocator's blocks
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in cases}
    for _ in range(reps):
        for k, fn in cases.items():
            ms[k].append(timed(fn, inner))
    out = {"B": B, "T": T, "heads": HEADS, "hd": HD, "dtype": "bf16", "reps": reps, "inner": inner,
           "ms_median": {k: round(statistics.median(v), 4) for k, v in ms.items()},
           "ms_min": {k: round(min(v), 4) for k, v in ms.items()},
           "ms_max": {k: round(max(v), 4) for k, v in ms.items()},
           "klen_2to4s": lens.tolist() if lens is not None else None,
           "device": torch.cuda.get_device_name(0)}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
