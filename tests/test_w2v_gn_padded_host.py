"""CPU: the host side of padded batches on the group-norm / post-LN wav2vec2 family (masked_group_norm) — the config
field and its JSON, the start-up check, the length checks, and the fixture of the lone-clip runs
(tests/golden/w2v_gn_padded_2layer_1s.npz) pinned against the CPU oracle with no transformers import.  No compute on
the product's side: there is no GPU here."""
import json
import os

import pytest
import torch

import golden_cases as GC
import make_w2v_gn_padded_fixture as GP
import make_w2v_ln_fixture as LN
from config import get_opt
from deepfake_amd.models import wav2vec2 as W
from deepfake_amd.models.fused import build_model, check_paudio_lengths
from deepfake_amd.trainer import wave_samples
from fixtures import check, keys, load
from oracle import w2v as OW
from oracle.fill import named_fill_

MODELS = os.path.dirname(W.__file__)
BASE_JSON = os.path.join(MODELS, "w2v_base_config.json")
LARGE_JSON = os.path.join(MODELS, "w2v_large_config.json")
MASKED_JSON = os.path.join(MODELS, "w2v_base_masked_config.json")


def masked_config(**kw):
    return W.Wav2Vec2Config.from_json_file(GC.W2V_CONFIG_JSON, masked_group_norm=True,
                                           **{**GC.w2v_overrides(GP.CASE["layers"]), **kw})


def test_the_field_defaults_to_false():
    assert W.Wav2Vec2Config().masked_group_norm is False
    assert W.Wav2Vec2Config.from_json_file(BASE_JSON).masked_group_norm is False
    assert W.Wav2Vec2Config.from_json_file(LARGE_JSON).masked_group_norm is False
    assert W.Wav2Vec2Config.from_json_file(GC.W2V_CONFIG_JSON).masked_group_norm is False
    assert W.Wav2Vec2Config(masked_group_norm=True).masked_group_norm is True                 # from kwargs
    assert W.Wav2Vec2Config.from_json_file(BASE_JSON, masked_group_norm=True).masked_group_norm is True
    assert W.Wav2Vec2Config.from_json_file(MASKED_JSON).masked_group_norm is True             # from the JSON


def test_the_masked_json_is_the_base_json_plus_the_key():
    with open(BASE_JSON) as f:
        base = json.load(f)
    with open(MASKED_JSON) as f:
        masked = json.load(f)
    assert "masked_group_norm" not in base
    assert masked == {**base, "masked_group_norm": True}


def test_the_field_on_a_layer_norm_config_raises():
    with pytest.raises(ValueError):
        W.Wav2Vec2Config.from_json_file(LARGE_JSON, masked_group_norm=True)
    with pytest.raises(ValueError):
        W.Wav2Vec2Config(**{**LN.CONFIG, "masked_group_norm": True})
    with pytest.raises(ValueError):
        W.Wav2Vec2Config(feat_extract_norm="layer", masked_group_norm=True)
    assert W.Wav2Vec2Config(feat_extract_norm="layer", masked_group_norm=False).masked_group_norm is False


@pytest.mark.parametrize("modality", ["paudio", "fused"])
def test_build_model_with_the_masked_json(modality):
    a = get_opt(["--modality", modality, "--config", "c1", "--deterministic", "--paudio_lengths", "--w2v_config",
                 MASKED_JSON])
    assert a.paudio_lengths is True and wave_samples(a) == 16000
    m = build_model(a)
    wav = m.wav_model if modality == "paudio" else next(x for x in m.modules() if isinstance(x, W.Wav2Vec2Model))
    assert type(wav.encoder) is W.Wav2Vec2Encoder
    assert wav.config.masked_group_norm is True and not wav.feature_extractor.layer_norm_path


def test_the_start_up_check_names_both_configs():
    a = get_opt(["--modality", "paudio", "--config", "c1", "--deterministic", "--paudio_lengths"])
    check_paudio_lengths(a, W.Wav2Vec2Config.from_json_file(MASKED_JSON))
    check_paudio_lengths(a, W.Wav2Vec2Config.from_json_file(LARGE_JSON))
    with pytest.raises(ValueError, match="layer-norm") as e:
        check_paudio_lengths(a, W.Wav2Vec2Config.from_json_file(BASE_JSON))
    assert "w2v_base_masked_config.json" in str(e.value)
    off = get_opt(["--modality", "paudio", "--config", "c1", "--deterministic"])
    check_paudio_lengths(off, W.Wav2Vec2Config.from_json_file(BASE_JSON))      # flag off: nothing to check


def test_good_host_lengths_become_int64():
    m = W.Wav2Vec2Model(masked_config(num_hidden_layers=1))
    n = m.sample_lengths(torch.zeros(2, 16000), [400, 16000])
    assert n.dtype == torch.int64 and n.tolist() == [400, 16000]
    n = m.sample_lengths(torch.zeros(2, 16000), torch.tensor([400, 16000], dtype=torch.int32))
    assert n.dtype == torch.int64 and n.tolist() == [400, 16000]


@pytest.mark.parametrize("bad", [
    [16000],                                  # wrong shape: one length for two clips
    [[16000, 8000]],                          # wrong shape: 2-D
    torch.tensor([16000.0, 8000.0]),          # wrong dtype
    [16000, 399],                             # below one frame's receptive field
    [16001, 8000],                            # above the padded length
    torch.tensor([0, 16000]),
])
def test_bad_host_lengths_raise_value_error(bad):
    m = W.Wav2Vec2Model(masked_config(num_hidden_layers=1))
    with pytest.raises(ValueError):
        m(torch.zeros(2, 16000), lengths=bad)


def test_other_configs_and_attention_mask_keep_raising():
    plain = W.Wav2Vec2Model(W.Wav2Vec2Config.from_json_file(GC.W2V_CONFIG_JSON, **GC.w2v_overrides(1)))
    with pytest.raises(NotImplementedError):
        plain.sample_lengths(torch.zeros(2, 16000), [16000, 8000])
    m = W.Wav2Vec2Model(masked_config(num_hidden_layers=1))
    with pytest.raises(NotImplementedError):
        m(torch.zeros(2, 16000), attention_mask=torch.ones(2, 16000))


def test_frame_lengths_match_the_fixture():
    fx = load(GP.NAME)
    cfg = masked_config()
    assert W.frame_lengths(list(GP.CASE["lengths"]), cfg) == fx["flen"].tolist() == [49, 33, 32, 1]
    t = W.frame_lengths(torch.tensor(GP.CASE["lengths"]), cfg)
    assert t.dtype == torch.int64 and t.tolist() == fx["flen"].tolist()


def test_fixture_against_the_oracle_alone():
    """The oracle with the fixture's seed and per-key fill, run on each clip alone: hidden states, pooled feature and
    the sampled gradients (summed over the clips) within 1e-4, the bar the base fixture is pinned at."""
    fx = load(GP.NAME)
    c = GP.CASE
    m = named_fill_(OW.Wav2Vec2Model(OW.W2VConfig(GC.W2V_CONFIG_JSON, num_hidden_layers=c["layers"])), c["seed"])
    y, feat, flen = GP.run_alone(lambda x: m(x)["last_hidden_state"], m.config.hidden)
    assert flen.tolist() == fx["flen"].tolist()
    assert tuple(y.shape) == (c["B"], 49, m.config.hidden)
    check(fx, "y", y, 1e-4)
    check(fx, "feat", feat, 1e-4)
    names = dict(m.named_parameters())
    gk = keys(fx, "g:")
    assert gk and all(any(s in k for k in gk) for s in GP.GRAD_KEYS)
    for k in gk:
        check(fx, k, names[k[2:]].grad, 1e-4, what=f"[{k}] ")
