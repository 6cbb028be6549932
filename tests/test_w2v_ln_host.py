"""CPU: the layer-norm / pre-norm wav2vec2 family (feat_extract_norm="layer", conv_bias, do_stable_layer_norm)
constructs with transformers' state_dict keys and shapes, the base family's keys are what they were, --w2v_config
reaches the builders, and what stays unbuilt still raises.  No compute: there is no GPU here."""
import json
import os

import pytest
import torch

import golden_cases as GC
import make_w2v_ln_fixture as LN
from config import get_opt
from deepfake_amd.models import wav2vec2 as W
from deepfake_amd.models.fused import build_model

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
LARGE_JSON = os.path.join(os.path.dirname(W.__file__), "w2v_large_config.json")


def small_config(**kw):
    return W.Wav2Vec2Config(**{**LN.CONFIG, **GC.w2v_overrides(LN.CASE["layers"]), **kw})


def shapes(m):
    return {k: list(v.shape) for k, v in m.state_dict().items()}


def test_layer_norm_family_constructs_with_hf_keys():
    m = W.Wav2Vec2Model(small_config())
    assert isinstance(m.encoder, W.Wav2Vec2EncoderStableLayerNorm)
    assert all(isinstance(l, W.Wav2Vec2EncoderLayerStableLayerNorm) for l in m.encoder.layers)
    ref = json.load(open(os.path.join(GOLD, "w2v_ln_keys.json")))
    ours = shapes(m)
    assert sorted(ours) == sorted(ref)
    assert ours == ref
    # nn.LayerNorm's default eps at the conv layers (HF builds them without one), not config.layer_norm_eps
    m2 = W.Wav2Vec2Model(small_config(layer_norm_eps=1e-3))
    assert m2.feature_extractor.conv_layers[3].layer_norm.eps == 1e-5
    assert m2.encoder.layers[0].layer_norm.eps == 1e-3


def test_layer_norm_family_without_conv_bias():
    m = W.Wav2Vec2Model(small_config(conv_bias=False))
    keys = set(m.state_dict())
    ref = {k for k in json.load(open(os.path.join(GOLD, "w2v_ln_keys.json"))) if not k.endswith(".conv.bias")
           or "pos_conv_embed" in k}
    assert keys == ref


def test_base_family_keys_unchanged():
    """wav2vec2-base from the committed config: the reference's own keys and shapes, in its order (the C2 fused
    model's waveform slot in tests/golden/state_keys.json)."""
    m = W.Wav2Vec2Model(W.Wav2Vec2Config.from_json_file(GC.W2V_CONFIG_JSON).deterministic())
    assert type(m.encoder) is W.Wav2Vec2Encoder and type(m.encoder.layers[0]) is W.Wav2Vec2EncoderLayer
    pre = "paExtract.wav_model."
    ref = [(k[len(pre):], s) for k, s in json.load(open(os.path.join(GOLD, "state_keys.json")))["fused_c2"]
           if k.startswith(pre)]
    assert len(ref) == 210
    assert [(k, list(v.shape)) for k, v in m.state_dict().items()] == ref


def test_w2v_config_flag_reaches_build_model():
    a = get_opt(["--modality", "fused", "--config", "c1", "--deterministic"])
    assert a.w2v_config is None
    assert build_model(a).paudio_projection.in_features == 768
    a = get_opt(["--modality", "fused", "--config", "c1", "--deterministic", "--w2v_config", LARGE_JSON])
    m = build_model(a)
    assert m.paudio_projection.in_features == 1024
    w = m.paExtract.wav_model
    assert isinstance(w.encoder, W.Wav2Vec2EncoderStableLayerNorm) and len(w.encoder.layers) == 2   # c1: w2v_layers
    assert w.feature_extractor.conv_layers[6].conv.bias is not None
    a = get_opt(["--modality", "paudio", "--config", "c1", "--deterministic", "--w2v_config", LARGE_JSON])
    assert build_model(a).mlp.fc1.in_features == 1024


def test_large_config_json_fields():
    c = W.Wav2Vec2Config.from_json_file(LARGE_JSON)
    assert (c.feat_extract_norm, c.conv_bias, c.do_stable_layer_norm) == ("layer", True, True)
    assert (c.hidden_size, c.intermediate_size, c.num_attention_heads, c.num_hidden_layers) == (1024, 4096, 16, 24)
    assert (c.conv_dim, c.conv_kernel, c.conv_stride) == ([512] * 7, [10, 3, 3, 3, 3, 2, 2], [5, 2, 2, 2, 2, 2, 2])
    assert (c.num_conv_pos_embeddings, c.num_conv_pos_embedding_groups, c.layer_norm_eps) == (128, 16, 1e-5)
    assert (c.hidden_dropout, c.attention_dropout, c.activation_dropout, c.feat_proj_dropout, c.layerdrop) == \
        (0.1, 0.1, 0.1, 0.1, 0.1)
    assert (c.mask_time_prob, c.mask_time_length, c.mask_time_min_masks, c.apply_spec_augment) == (0.05, 10, 2, True)


def test_unbuilt_configurations_still_raise():
    with pytest.raises(NotImplementedError):
        W.Wav2Vec2Model(small_config(feat_extract_norm="group", conv_bias=True))
    for kw in (dict(conv_kernel=[8, 3, 3, 3, 3, 2, 2]), dict(conv_stride=[4, 2, 2, 2, 2, 2, 2]),
               dict(conv_dim=[256] + [512] * 6), dict(conv_dim=[512] * 6 + [768])):
        with pytest.raises(NotImplementedError):
            W.Wav2Vec2Model(small_config(**kw))
    # an encoder class built directly from the other family's config (Wav2Vec2Model picks by do_stable_layer_norm)
    with pytest.raises(NotImplementedError):
        W.Wav2Vec2Encoder(small_config())
    with pytest.raises(NotImplementedError):
        W.Wav2Vec2EncoderStableLayerNorm(small_config(do_stable_layer_norm=False))
    m = W.Wav2Vec2Model(small_config())
    with pytest.raises(NotImplementedError):
        m(torch.zeros(2, 400), attention_mask=torch.ones(2, 400, dtype=torch.long))


def test_param_gates_follow_layerdrop():
    enc = W.Wav2Vec2Model(small_config(layerdrop=0.5)).encoder
    gates = enc.param_gates()
    assert len(gates) == 2 and len(gates[0][0]) == len(list(enc.layers[0].parameters()))
    assert W.Wav2Vec2Model(small_config()).encoder.param_gates() == []
