"""CPU: the host side of wav2vec2 padded batches (lengths=) — frame lengths against transformers' fixture and the
closed form, the argument checks, pad_longest(pad_to=) and the --paudio_lengths flag.  No compute: there is no GPU
here."""
import os

import pytest
import torch

import golden_cases as GC
import make_w2v_ln_fixture as LN
import make_w2v_padded_fixture as PD
from config import get_opt
from deepfake_amd.models import wav2vec2 as W
from deepfake_amd.models.fused import build_model
from deepfake_amd.trainer import pad_longest, wave_samples
from fixtures import load

LARGE_JSON = os.path.join(os.path.dirname(W.__file__), "w2v_large_config.json")


def small_config(**kw):
    return W.Wav2Vec2Config(**{**LN.CONFIG, **GC.w2v_overrides(LN.CASE["layers"]), **kw})


def test_frame_lengths_match_the_fixture():
    fx = load(PD.NAME)
    cfg = small_config()
    assert W.frame_lengths(list(PD.CASE["lengths"]), cfg) == fx["flen"].tolist() == [49, 33, 32, 1]
    t = W.frame_lengths(torch.tensor(PD.CASE["lengths"]), cfg)
    assert t.dtype == torch.int64 and t.tolist() == fx["flen"].tolist()
    assert W.receptive_field(cfg) == 400


@pytest.mark.parametrize("j", [0, 1, 31, 32, 48, 198])
def test_frame_lengths_closed_form_at_the_frame_edges(j):
    """n = 400 + 320 j is the first sample count that gives j + 1 frames: one sample less gives j."""
    cfg = small_config()
    n = 400 + 320 * j
    for v in (n - 1, n, n + 1, n + 319, n + 320):
        want = (v - 400) // 320 + 1
        assert W.frame_lengths(v, cfg) == want
        assert int(W.frame_lengths(torch.tensor([v]), cfg)) == want
    assert W.frame_lengths(n, cfg) == j + 1 and W.frame_lengths(n - 1, cfg) == j


def test_lengths_on_the_group_norm_family_raise():
    m = W.Wav2Vec2Model(W.Wav2Vec2Config.from_json_file(GC.W2V_CONFIG_JSON, num_hidden_layers=1).deterministic())
    with pytest.raises(NotImplementedError):
        m(torch.zeros(2, 16000), lengths=[16000, 8000])
    with pytest.raises(NotImplementedError):   # HF's argument still raises, on both families
        W.Wav2Vec2Model(small_config())(torch.zeros(2, 16000), attention_mask=torch.ones(2, 16000))


@pytest.mark.parametrize("bad", [
    [16000],                                  # wrong shape: one length for two clips
    [[16000, 8000]],                          # wrong shape: 2-D
    torch.tensor([16000.0, 8000.0]),          # wrong dtype
    [16000, 399],                             # below one frame's receptive field
    [16001, 8000],                            # above the padded length
    torch.tensor([0, 16000]),
])
def test_bad_host_lengths_raise_value_error(bad):
    m = W.Wav2Vec2Model(small_config())
    with pytest.raises(ValueError):
        m(torch.zeros(2, 16000), lengths=bad)


def test_good_host_lengths_become_int64():
    m = W.Wav2Vec2Model(small_config())
    n = m.sample_lengths(torch.zeros(2, 16000), [400, 16000])
    assert n.dtype == torch.int64 and n.tolist() == [400, 16000]
    n = m.sample_lengths(torch.zeros(2, 16000), torch.tensor([400, 16000], dtype=torch.int32))
    assert n.dtype == torch.int64 and n.tolist() == [400, 16000]


def test_pad_longest_pad_to():
    waves = [torch.arange(3.0), torch.arange(5.0)]
    out, n = pad_longest(waves, return_lengths=True, pad_to=8)
    assert out.shape == (2, 8) and n.tolist() == [3, 5] and n.dtype == torch.int64
    assert torch.equal(out[:, :5], pad_longest(waves)) and not out[:, 5:].any()
    assert torch.equal(pad_longest(waves, pad_to=5), pad_longest(waves))
    with pytest.raises(ValueError):
        pad_longest(waves, pad_to=4)
    stacked = torch.ones(2, 6)
    out, n = pad_longest(stacked, return_lengths=True, pad_to=8)
    assert out.shape == (2, 8) and n.tolist() == [6, 6] and not out[:, 6:].any() and out[:, :6].all()
    with pytest.raises(ValueError):
        pad_longest(stacked, pad_to=5)


def test_paudio_lengths_flag():
    assert get_opt([]).paudio_lengths is False and wave_samples(get_opt([])) is None
    a = get_opt(["--modality", "paudio", "--config", "c1", "--deterministic", "--paudio_lengths", "--w2v_config",
                 LARGE_JSON])
    assert a.paudio_lengths is True and wave_samples(a) == 16000
    assert isinstance(build_model(a).wav_model.encoder, W.Wav2Vec2EncoderStableLayerNorm)
    for modality in ("paudio", "fused"):      # the base family has no padded-batch path: fail at start-up
        with pytest.raises(ValueError, match="layer-norm"):
            build_model(get_opt(["--modality", modality, "--config", "c1", "--deterministic", "--paudio_lengths"]))
