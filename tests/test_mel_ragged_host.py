"""CPU: the host side of per-clip lengths in the mel pipeline — padding with lengths, the collate functions'
stack-or-list rule, the seeded per-clip length draw, the exact output lengths of the resampler, the validation of
host-side lengths, the loud failure on CPU waveforms and the operators' fake shapes.  (The header / binding
agreement of the two new C entry points is held by tests/test_clib.py.)"""
import types

import numpy as np
import pytest
import torch
from torch._subclasses.fake_tensor import FakeTensorMode

import deepfake_amd.ops as O
from config import clip_seconds, get_opt
from deepfake_amd import media
from deepfake_amd.data import DeepFake, fusion_collate, fusion_collate_test
from deepfake_amd.trainer import pad_longest


def test_pad_longest_returns_lengths():
    waves = [np.arange(5, dtype=np.float32), torch.arange(3).float(), np.ones(7, dtype=np.float32)]
    out, n = pad_longest(waves, return_lengths=True)
    assert out.shape == (3, 7) and out.dtype == torch.float32
    assert n.dtype == torch.int64 and n.tolist() == [5, 3, 7]
    assert torch.equal(out, pad_longest(waves))                         # the padded batch is the one it always gave
    assert out[0, 5:].eq(0).all() and out[1, 3:].eq(0).all() and torch.equal(out[0, :5], torch.arange(5).float())
    stacked = torch.ones(2, 9)
    out, n = pad_longest(stacked, return_lengths=True)
    assert torch.equal(out, stacked) and n.tolist() == [9, 9] and n.dtype == torch.int64


def _ds(seconds, source="wave16k", n=6, seed=3, split="train"):
    args = types.SimpleNamespace(modality="fused", num_frames=2)
    return DeepFake(args, split, n=n, seed=seed, T=2, H=8, W=8, seconds=seconds, mel_source=source)


def test_collate_stacks_equal_and_lists_ragged():
    items = [_ds(0.01)[i] for i in range(3)]
    feat, labels, names = fusion_collate(items)
    assert torch.is_tensor(feat["Audio"]) and feat["Audio"].shape == (3, 160)            # unchanged: stacked
    assert torch.is_tensor(feat["Video"]) and isinstance(feat["PAudio"], list) and labels.shape == (3,)
    tfeat, _ = fusion_collate_test([(f, name) for f, _, name in items])
    assert torch.equal(tfeat["Audio"], feat["Audio"])

    ragged = _ds((0.01, 0.05))
    items = [ragged[i] for i in range(6)]
    lens = [it[0]["Audio"].numel() for it in items]
    assert len(set(lens)) > 1, lens
    feat, _, _ = fusion_collate(items)
    assert isinstance(feat["Audio"], list) and [a.numel() for a in feat["Audio"]] == lens
    for a, p in zip(feat["Audio"], feat["PAudio"]):                                        # wave16k: the same samples
        assert a.dim() == 1 and np.array_equal(a.numpy(), p)
    tfeat, _ = fusion_collate_test([(f, name) for f, _, name in items])
    assert isinstance(tfeat["Audio"], list) and all(torch.equal(a, b) for a, b in zip(tfeat["Audio"], feat["Audio"]))
    # images (not 1-D waveforms) are always stacked
    imgs = [_ds((0.01, 0.05), source="uint8")[i] for i in range(3)]
    assert fusion_collate(imgs)[0]["Audio"].shape == (3, 224, 224)


def test_seeded_length_draw():
    lo, hi = 0.01, 0.05
    a, b = _ds((lo, hi)), _ds((lo, hi))
    lens = [a[i][0]["PAudio"].shape[0] for i in range(6)]
    assert lens == [b[i][0]["PAudio"].shape[0] for i in range(6)]                          # reproducible
    assert all(int(16000 * lo) <= n <= int(16000 * hi) for n in lens) and len(set(lens)) > 1
    for i in range(3):
        assert np.array_equal(a[i][0]["PAudio"], b[i][0]["PAudio"])
    assert [_ds((lo, hi), seed=4)[i][0]["PAudio"].shape[0] for i in range(6)] != lens      # the seed decides
    w = _ds((lo, hi), source="wave")[0][0]                                                 # the 22.05 kHz source follows
    assert w["Audio"].numel() == w["PAudio"].shape[0] * 22050 // 16000
    assert _ds((0.02, 0.02))[0][0]["PAudio"].shape[0] == 320                               # lo == hi: one length
    with pytest.raises(ValueError):
        _ds((0.05, 0.01))[0]


def test_fixed_length_clips_are_unchanged():
    """A fixed length makes no extra draw: the clip is what the seeded stream gave before lengths could vary."""
    from deepfake_amd.data import _rng
    for source in ("wave16k", "wave"):
        feat, label, _ = _ds(0.01, source=source, seed=5)[2]
        g = _rng(5, 2)
        want_label = float(g.uniform() < 0.5)
        g.integers(0, 256, size=(2, 8, 8, 3), dtype=np.uint8)
        if source == "wave":
            mel = (0.1 * g.standard_normal(int(22050 * 0.01))).astype(np.float32)
            assert np.array_equal(feat["Audio"].numpy(), mel)
        wave = (0.1 * g.standard_normal(160)).astype(np.float32)
        assert float(label) == want_label and np.array_equal(feat["PAudio"], wave)


def test_audio_seconds_min_flag():
    cfg = {"seconds": 4}
    assert get_opt([]).audio_seconds_min is None and clip_seconds(get_opt([]), cfg) == 4
    assert clip_seconds(get_opt(["--audio_seconds_min", "1.5"]), cfg) == (1.5, 4)
    assert clip_seconds(types.SimpleNamespace(), cfg) == 4
    for bad in ("0", "-1", "4.5"):
        with pytest.raises(ValueError):
            clip_seconds(get_opt(["--audio_seconds_min", bad]), cfg)


def test_resample_lengths_exact_ceil():
    ns = [1, 2, 319, 320, 321, 1113, 1114, 1115, 64000, 10_000_000, 2 ** 40 + 1]
    want = [-((-n * 441) // 320) for n in ns]
    assert media.resample_lengths(ns) == want and all(isinstance(v, int) for v in media.resample_lengths(ns))
    t = media.resample_lengths(torch.tensor(ns))
    assert t.dtype == torch.int64 and t.tolist() == want
    assert media.resample_lengths(torch.tensor(ns[:8], dtype=torch.int32)).tolist() == want[:8]
    assert media.resample_lengths([257], 16000, 24000) == [386] and media.resample_lengths([7], 16000, 16000) == [7]
    assert media.resample_lengths((1115, 1114)) == [1537, 1536]


@pytest.mark.parametrize("fn", [media.mel_image, media.resample])
def test_host_lengths_validated(fn):
    x = torch.zeros(2, 1000)
    for bad in ([1000], [1000, 1000, 1000], [0, 1000], [1000, 1001], [-5, 10], [[1000, 1000]], [0.5, 1.0],
                torch.tensor([1000]), torch.tensor([0, 1000]), torch.tensor([1, 1001]), torch.tensor([1.0, 2.0]),
                torch.tensor([True, True])):
        with pytest.raises(ValueError):
            fn(x, lengths=bad)


@pytest.mark.parametrize("fn", [media.mel_image, media.resample])
def test_cpu_wave_raises(fn):
    x = torch.zeros(2, 1000)
    for ok in ([1000, 1], (5, 999), torch.tensor([7, 8]), torch.tensor([7, 8], dtype=torch.int32)):
        with pytest.raises(RuntimeError, match="device tensors only"):
            fn(x, lengths=ok)
    with pytest.raises(RuntimeError, match="GPU only"):
        torch.ops.dfk.mel_image_ragged(x, torch.tensor([7, 8]))
    with pytest.raises(RuntimeError, match="GPU only"):
        torch.ops.dfk.resample_ragged(x, torch.tensor([7, 8]))


def test_ragged_ops_registered_with_fake_shapes():
    assert "resample_ragged" in O.OPS and "mel_image_ragged" in O.OPS
    assert str(torch.ops.dfk.resample_ragged.default._schema) == \
        "dfk::resample_ragged(Tensor wave, Tensor lengths, SymInt sr_in=16000, SymInt sr_out=22050) -> Tensor"
    with FakeTensorMode():
        x = torch.empty(3, 64000, device="cuda")
        n = torch.empty(3, dtype=torch.int64, device="cuda")
        y = torch.ops.dfk.resample_ragged(x, n)
        assert y.shape == (3, 88200) and y.dtype == torch.float32
        assert torch.ops.dfk.resample_ragged(torch.empty(3, 1000, device="cuda"), n).shape == (3, 1379)
        img = torch.ops.dfk.mel_image_ragged(x, n)
        assert img.shape == (3, 224, 224) and img.dtype == torch.uint8
        img = torch.ops.dfk.mel_image_ragged(x, n, 16000, 22050, 2048, 512, 128, 128, 9)
        assert img.shape == (3, 128, 9) and img.dtype == torch.uint8
