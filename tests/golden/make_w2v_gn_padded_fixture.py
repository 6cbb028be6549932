"""Golden vectors of a padded batch through the group-norm / post-LN wav2vec2 family (wav2vec2-base): what every
clip gives ALONE in transformers' Wav2Vec2Model on CPU (fp32), normalised over its own samples.  That is the
contract of lengths= with masked_group_norm; transformers' own batched run is no reference here, because conv0's
GroupNorm takes its statistics over the whole padded row and no attention mask undoes that.

Run in the build container only (needs transformers 5.15.0):
    python tests/golden/make_w2v_gn_padded_fixture.py
Writes tests/golden/w2v_gn_padded_2layer_1s.npz: the per-clip mean / rstd of the normalisation (float64 statistics),
last_hidden_state of the four lone runs assembled into [B, T, C] with zeros past each clip's frames, the mean over
each clip's own frames, the frame lengths, and the GC.W2V_GRAD_KEYS sample of the parameter gradients summed over the
four lone runs under a seeded cotangent on that pooled feature.  The clips are make_w2v_padded_fixture's; weights are
never stored.
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
import make_w2v_padded_fixture as PD  # noqa: E402
from oracle.fill import named_fill_  # noqa: E402

NAME = "w2v_gn_padded_2layer_1s"
CASE = dict(PD.CASE, seed=241)   # the clips (B, S, lengths) of the layer-norm padded fixture, another weight seed
GRAD_KEYS = GC.W2V_GRAD_KEYS


def hf_model():
    from transformers import Wav2Vec2Config, Wav2Vec2Model
    cfg = Wav2Vec2Config.from_json_file(GC.W2V_CONFIG_JSON)
    for k, v in GC.w2v_overrides(CASE["layers"]).items():
        setattr(cfg, k, v)
    cfg._attn_implementation = "eager"
    return Wav2Vec2Model(cfg)


def lone_clips(w=None):
    """The clips as their lone runs see them: [1, n_b] fp32, normalised over their own samples (float64 statistics)."""
    w = PD.wave_input() if w is None else w
    mean, rstd = PD.clip_stats(w)
    return [((w[b, :n].double() - mean[b]) * rstd[b]).float()[None] for b, n in enumerate(CASE["lengths"])]


def run_alone(m, hidden):
    """y [B, T, C] (zeros past T_b), feat [B, C] and the frame counts of the lone runs of model m (a callable that
    returns last_hidden_state [1, T_b, C]); parameter gradients of sum_b <feat_b, cotangent_b> add up in .grad."""
    cot = PD.feature_cotangent(hidden)
    ys, feats, flen = [], [], []
    for b, x in enumerate(lone_clips()):
        h = m(x)[0]
        f = h.mean(0)
        (f * cot[b]).sum().backward()
        ys.append(h.detach())
        feats.append(f.detach())
        flen.append(h.shape[0])
    y = torch.zeros(len(ys), max(flen), hidden)
    for b, h in enumerate(ys):
        y[b, :h.shape[0]] = h
    return y, torch.stack(feats), torch.tensor(flen)


def main():
    torch.set_num_threads(8)
    m = named_fill_(hf_model(), seed=CASE["seed"])
    m.train()   # every stochastic piece is off (w2v_overrides)
    mean, rstd = PD.clip_stats(PD.wave_input())
    y, feat, flen = run_alone(lambda x: m(x).last_hidden_state, m.config.hidden_size)
    assert flen.tolist() == m._get_feat_extract_output_lengths(torch.tensor(CASE["lengths"])).tolist()
    arrays = {"mean": mean, "rstd": rstd, "y": y, "feat": feat, "flen": flen}
    for k, p in m.named_parameters():
        if p.grad is not None and any(s in k for s in GRAD_KEYS):
            arrays["g:" + k] = p.grad
    packed = {}
    for k, v in arrays.items():
        packed.update(GC.fixture_compress(k, v.detach().cpu().numpy()))
    np.savez_compressed(os.path.join(HERE, NAME + ".npz"), **packed)
    print(f"{NAME}: {len(packed)} arrays, T = {y.shape[1]}, frame lengths {flen.tolist()}")


if __name__ == "__main__":
    main()
