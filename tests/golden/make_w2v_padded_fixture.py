"""Golden vectors of a padded batch through the layer-norm / pre-norm wav2vec2 family: transformers' Wav2Vec2Model
on CPU (fp32) with an attention mask, on clips of unequal length normalised per clip over their own samples
(Wav2Vec2FeatureExtractor.zero_mean_unit_var_norm with a mask).

Run in the build container only (needs transformers 5.15.0):
    python tests/golden/make_w2v_padded_fixture.py
Writes tests/golden/w2v_ln_padded_2layer_1s.npz: the per-clip mean / rstd of the normalisation (float64 statistics),
last_hidden_state with the padded frames zeroed (HF leaves its final LayerNorm's output there), the mean over each
clip's own frames, the frame lengths, and the GRAD_KEYS sample of the parameter gradients under a seeded cotangent on
that pooled feature.  Config, weight fill and compression are make_w2v_ln_fixture's; weights are never stored.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import golden_cases as GC  # noqa: E402
import make_w2v_ln_fixture as LN  # noqa: E402
from oracle.fill import named_fill_, randn  # noqa: E402

NAME = "w2v_ln_padded_2layer_1s"
# T_b = 49 / 33 / 32 / 1 of T = 49 (Np = 64): full, one key into the second key block, exactly one block, one key
CASE = dict(B=4, S=16000, seed=231, layers=2, lengths=(16000, 10640, 10639, 400))
CONFIG, GRAD_KEYS = LN.CONFIG, LN.GRAD_KEYS


def wave_input():
    """[B, S] fp32 raw waveform with an offset and a scale per clip (so the normalisation has work to do); the
    samples past a clip's length are zero, as a collate pads them."""
    w = randn(CASE["seed"] + 1, (CASE["B"], CASE["S"]))
    w = w * torch.tensor([0.5, 2.0, 1.0, 3.0])[:, None] + torch.tensor([0.1, -0.3, 0.7, 0.0])[:, None]
    for b, n in enumerate(CASE["lengths"]):
        w[b, n:] = 0.0
    return w


def feature_cotangent(C):
    return randn(CASE["seed"] + 2, (CASE["B"], C))


def clip_stats(w):
    """float64 mean and 1 / sqrt(var + 1e-7) over each clip's own samples."""
    mean, rstd = [], []
    for b, n in enumerate(CASE["lengths"]):
        x = w[b, :n].double()
        mean.append(x.mean())
        rstd.append(1.0 / torch.sqrt(x.var(unbiased=False) + 1e-7))
    return torch.stack(mean), torch.stack(rstd)


def main():
    torch.set_num_threads(8)
    m = named_fill_(LN.hf_model(), seed=CASE["seed"])
    m.train()   # every stochastic piece is off (w2v_overrides)
    w = wave_input()
    n = torch.tensor(CASE["lengths"])
    mean, rstd = clip_stats(w)
    mask = (torch.arange(CASE["S"])[None, :] < n[:, None])
    x = torch.where(mask, ((w.double() - mean[:, None]) * rstd[:, None]).float(), torch.zeros(()))
    h = m(x, attention_mask=mask.long()).last_hidden_state
    flen = m._get_feat_extract_output_lengths(n)
    fm = (torch.arange(h.shape[1])[None, :] < flen[:, None])[:, :, None]
    y = torch.where(fm, h, torch.zeros(()))
    feat = y.sum(1) / flen[:, None].float()
    feat.backward(feature_cotangent(feat.shape[1]))
    arrays = {"mean": mean, "rstd": rstd, "y": y, "feat": feat, "flen": flen}
    for k, p in m.named_parameters():
        if p.grad is not None and any(s in k for s in GRAD_KEYS):
            arrays["g:" + k] = p.grad
    packed = {}
    for k, v in arrays.items():
        packed.update(GC.fixture_compress(k, v.detach().cpu().numpy()))
    np.savez_compressed(os.path.join(HERE, NAME + ".npz"), **packed)
    print(f"{NAME}: {len(packed)} arrays, T = {h.shape[1]}, frame lengths {flen.tolist()}")


if __name__ == "__main__":
    main()
