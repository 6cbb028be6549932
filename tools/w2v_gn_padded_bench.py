"""Device time of padded batches on the group-norm / post-LN wav2vec2 family (masked_group_norm) against the uniform
call of the same build (the yardstick: code this path leaves alone), at B = 8 clips of 4 s (S = 64000, T0 = 12799),
bf16 compute, in three cases each:

  uniform        no lengths                      dfk_w2v_conv0_fwd / _bwd, Wav2Vec2Model(wave)
  ragged_full    lengths = S for every clip      dfk_w2v_conv0_ragged_fwd / _bwd, Wav2Vec2Model(wave, lengths=)
  ragged_2to4s   lengths spread over [2 s, 4 s]  the same

for conv0 forward, conv0 backward and one forward + backward of the 12-layer base model (regularisers off).

The protocol is tools/w2v_ln_bench.py's: HIP events on the op's stream around `inner` back-to-back calls, median over
`reps` repeats after a warm-up, the cases interleaved in each repeat.  Prints one JSON line.
Usage: python tools/w2v_gn_padded_bench.py [reps] [inner] [--no-model]"""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from w2v_ln_bench import MODELS, interleaved, summary  # noqa: E402
from deepfake_amd import kernels as K  # noqa: E402
from deepfake_amd.models import set_compute_dtype  # noqa: E402
from deepfake_amd.models import wav2vec2 as W  # noqa: E402


def model_cases(dt, wave, lengths):
    """One model, its forward + backward without lengths and with each lengths tensor."""
    cfg = W.Wav2Vec2Config.from_json_file(os.path.join(MODELS, "w2v_base_masked_config.json")).deterministic()
    torch.manual_seed(0)
    m = set_compute_dtype(W.Wav2Vec2Model(cfg), dt).cuda().train()

    def case(n):
        def run():
            h = m(wave, lengths=n)["last_hidden_state"]
            h.backward(torch.ones_like(h))
            for p in m.parameters():
                p.grad = None
        return run
    return {"model_" + k: case(n) for k, n in lengths.items()}


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    reps = int(args[0]) if len(args) > 0 else 30
    inner = int(args[1]) if len(args) > 1 else 20
    if not torch.cuda.is_available():
        raise SystemExit("w2v_gn_padded_bench: needs the GPU (no CPU timing)")
    dev, dt, B, S = "cuda", torch.bfloat16, 8, 64000
    g = torch.Generator(device=dev).manual_seed(0)
    wave = torch.randn(B, S, device=dev, generator=g)
    w = (0.3 * torch.randn(512, 10, device=dev, generator=g))
    beta = 0.1 * torch.randn(512, device=dev, generator=g)
    gamma = 1 + 0.1 * torch.randn(512, device=dev, generator=g)
    spread = [S // 2 + (S // 2) * i // (B - 1) for i in range(B)]        # 32000 .. 64000 in equal steps
    lengths = {"uniform": None, "ragged_full": torch.full((B,), S, dtype=torch.int64, device=dev),
               "ragged_2to4s": torch.tensor(spread, dtype=torch.int64, device=dev)}
    cases = {}
    for k, n in lengths.items():
        y, st = K.w2v_conv0_fwd(wave, w, gamma, beta, 1e-5, dt, n)
        if k == "uniform":
            dy = torch.randn(y.shape, device=dev, generator=g).to(dt)
            sinks = [torch.zeros_like(t) for t in (w, gamma, beta)]
        cases["conv0_fwd_" + k] = lambda n=n: K.w2v_conv0_fwd(wave, w, gamma, beta, 1e-5, dt, n)
        cases["conv0_bwd_" + k] = lambda n=n, st=st: K.w2v_conv0_bwd(wave, w, gamma, beta, 1e-5, st, dy, *sinks, n)
    out = {"B": B, "S": S, "T0": (S - 10) // 5 + 1, "dtype": "bf16", "reps": reps, "inner": inner,
           "lengths_2to4s": spread, "ms": summary(interleaved(cases, reps, inner)),
           "device": torch.cuda.get_device_name(0)}
    if "--no-model" not in sys.argv:
        out["model_ms"] = summary(interleaved(model_cases(dt, wave, lengths), max(reps // 3, 3), max(inner // 10, 1),
                                              warm=2))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
