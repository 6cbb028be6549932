"""Golden vectors of the layer-norm / pre-norm wav2vec2 family (feat_extract_norm="layer", conv_bias,
do_stable_layer_norm: the wav2vec2-large-lv60 / XLS-R layout) from transformers' Wav2Vec2Model on CPU (fp32).

Run in the build container only (needs transformers 5.15.0):
    python tests/golden/make_w2v_ln_fixture.py
Writes tests/golden/w2v_ln_2layer_1s.npz (last_hidden_state, extract_features and a sample of the parameter
gradients under a seeded cotangent) and tests/golden/w2v_ln_keys.json (the HF model's state_dict keys and
shapes).  Weights are never stored: named_fill_ re-creates them per state_dict key.
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import golden_cases as GC  # noqa: E402
from oracle.fill import named_fill_, randn  # noqa: E402

NAME = "w2v_ln_2layer_1s"
CASE = dict(B=2, S=16000, seed=221, layers=2)
# the fields deepfake_amd.models.wav2vec2.Wav2Vec2Config reads, at the small size the tests run
CONFIG = dict(feat_extract_norm="layer", conv_bias=True, do_stable_layer_norm=True, hidden_size=256,
              num_attention_heads=4, intermediate_size=512, num_hidden_layers=2,
              conv_dim=[512] * 7, conv_kernel=[10, 3, 3, 3, 3, 2, 2], conv_stride=[5, 2, 2, 2, 2, 2, 2],
              num_conv_pos_embeddings=128, num_conv_pos_embedding_groups=16, layer_norm_eps=1e-5)
GRAD_KEYS = ("conv_layers.0.conv.weight", "conv_layers.0.conv.bias", "conv_layers.0.layer_norm",
             "conv_layers.3.conv.weight", "conv_layers.3.conv.bias", "conv_layers.3.layer_norm",
             "conv_layers.6.layer_norm", "feature_projection", "pos_conv_embed", "layers.0.attention.q_proj",
             "layers.0.layer_norm", "layers.1.feed_forward", "layers.1.final_layer_norm", "encoder.layer_norm")


def wave_input():
    """[B, S] fp32 waveform, roughly unit variance as a normalised clip (seeded Philox stream)."""
    return randn(CASE["seed"] + 1, (CASE["B"], CASE["S"]))


def hf_model():
    from transformers import Wav2Vec2Config, Wav2Vec2Model
    cfg = Wav2Vec2Config(**CONFIG)
    for k, v in GC.w2v_overrides(CASE["layers"]).items():
        setattr(cfg, k, v)
    cfg._attn_implementation = "eager"
    return Wav2Vec2Model(cfg)


def main():
    torch.set_num_threads(8)
    m = named_fill_(hf_model(), seed=CASE["seed"])
    m.train()   # every stochastic piece is off (w2v_overrides)
    out = m(wave_input())
    h = out.last_hidden_state
    h.backward(randn(CASE["seed"] + 2, h.shape))
    arrays = {"y": h, "extract": out.extract_features}
    for n, p in m.named_parameters():
        if p.grad is not None and any(s in n for s in GRAD_KEYS):
            arrays["g:" + n] = p.grad
    packed = {}
    for k, v in arrays.items():
        packed.update(GC.fixture_compress(k, v.detach().cpu().numpy()))
    np.savez_compressed(os.path.join(HERE, NAME + ".npz"), **packed)
    keys = {k: list(v.shape) for k, v in sorted(m.state_dict().items())}
    with open(os.path.join(HERE, "w2v_ln_keys.json"), "w") as f:
        json.dump(keys, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{NAME}: {len(packed)} arrays, {len(keys)} state_dict keys, T = {h.shape[1]}")


if __name__ == "__main__":
    main()
