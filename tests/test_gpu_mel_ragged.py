"""GPU: per-clip lengths in the device mel pipeline (csrc/media.hip, the RAGGED kernels): a padded batch with
`lengths` gives every clip, bit for bit, what the unchanged uniform code gives that clip alone,

    mel_image(wave, lengths=n, ...)[b] == mel_image(wave[b:b+1, :n_b].contiguous(), ...)[0]        (uint8)
    resample(wave, lengths=n)[b, :m_b] == resample(wave[b:b+1, :n_b])[0],   == 0.0 on [m_b, S_out)

whatever the padding wave[b, n_b:] holds (zeros, NaN, 1e6: it is never read into arithmetic).  The right-hand sides
are the code the earlier tests pin (test_gpu_media.py, test_gpu_resample.py), so no tolerance appears here except
the resampler's derived bound against tests/resample_ref.py, ntaps * 2^-23 * sum |x h| (as in test_gpu_resample.py).

Frame counts: T_b = 1 + m_b / hop with m_b = n_b (plain) or ceil(n_b 441 / 320) (from 16 kHz).  Frames from T_b on
still overlap the clip's tail (they are not silent), so the lengths sit on both sides of frame-count boundaries."""
import types

import numpy as np
import pytest
import torch

import deepfake_amd.ops  # noqa: F401  (registers torch.ops.dfk)
from resample_ref import out_len, resample_ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
SIZES = ((224, 224), (9, 128))
PADS = (0.0, float("nan"), 1e6)

PLAIN_S, PLAIN_N = 4096, [4096, 3000, 1536, 1535, 700]              # T_b = 9, 6, 4, 3, 2
RES_S, RES_N = 3000, [3000, 2177, 1115, 1114, 1113, 320]            # m_b = 4135, 3001, 1537, 1536, 1534, 441


def _batch(S, lengths, seed):
    """Gaussian noise x 0.1, one row per clip (host); only row[:n_b] belongs to clip b."""
    return 0.1 * torch.randn(len(lengths), S, generator=torch.Generator().manual_seed(seed))


def _padded(x, lengths, fill):
    y = x.clone()
    for b, n in enumerate(lengths):
        y[b, n:] = fill
    return y.to(DEV)


def _per_clip(x, lengths, **kw):
    """The contract's right-hand side: every clip alone through today's uniform path."""
    from deepfake_amd import media
    return torch.stack([media.mel_image(x[b:b + 1, :n].contiguous().to(DEV), **kw)[0] for b, n in enumerate(lengths)])


@pytest.fixture(scope="module")
def plain():
    x = _batch(PLAIN_S, PLAIN_N, 11)
    return x, {size: _per_clip(x, PLAIN_N, size=size) for size in SIZES}


@pytest.fixture(scope="module")
def res():
    x = _batch(RES_S, RES_N, 12)
    return x, {size: _per_clip(x, RES_N, size=size, sr_in=16000) for size in SIZES}


def test_frame_counts_cover_the_boundaries():
    assert [1 + n // 512 for n in PLAIN_N] == [9, 6, 4, 3, 2]
    m = [out_len(n, 441, 320) for n in RES_N]
    assert m == [4135, 3001, 1537, 1536, 1534, 441]
    assert [1 + v // 512 for v in m] == [9, 6, 4, 4, 3, 1]


@pytest.mark.parametrize("size", SIZES)
def test_plain_ragged_equals_per_clip(plain, size):
    from deepfake_amd import media
    x, want = plain
    outs = [media.mel_image(_padded(x, PLAIN_N, fill), lengths=PLAIN_N, size=size) for fill in PADS]
    for fill, got in zip(PADS, outs):
        assert got.shape == (len(PLAIN_N), size[1], size[0]) and got.dtype == torch.uint8
        for b, n in enumerate(PLAIN_N):
            diff = (got[b].int() - want[size][b].int()).abs()
            print(f"plain pad={fill} n={n}: {int((diff != 0).sum())} pixels differ, max {int(diff.max())}")
            assert torch.equal(got[b], want[size][b]), (fill, n)
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])


@pytest.mark.parametrize("size", SIZES)
def test_resampled_ragged_equals_per_clip(res, size):
    from deepfake_amd import media
    x, want = res
    outs = [media.mel_image(_padded(x, RES_N, fill), lengths=RES_N, size=size, sr_in=16000) for fill in PADS]
    for fill, got in zip(PADS, outs):
        assert got.shape == (len(RES_N), size[1], size[0]) and got.dtype == torch.uint8
        for b, n in enumerate(RES_N):
            diff = (got[b].int() - want[size][b].int()).abs()
            print(f"resampled pad={fill} n={n}: {int((diff != 0).sum())} pixels differ, max {int(diff.max())}")
            assert torch.equal(got[b], want[size][b]), (fill, n)
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    # the fused pipeline is the composition of its ragged parts
    for fill in PADS:
        y = media.resample(_padded(x, RES_N, fill), lengths=RES_N)
        two = media.mel_image(y, lengths=media.resample_lengths(RES_N), size=size)
        assert torch.equal(two, outs[0]), fill


def test_resample_lengths_rows():
    """Every row against the float64 sum on x[b, :n_b] (derived bound), bit-equal to the single-row call, exact
    zeros past the clip's end; NaN padding in the input."""
    from deepfake_amd import media
    H, L, M = media.resample_taps(16000, 22050)
    ntaps = H.shape[1]
    S, lengths = 1000, [1, 50, 320, 321, 1000]
    x = torch.randn(len(lengths), S, generator=torch.Generator().manual_seed(5))
    xd = _padded(x, lengths, float("nan"))
    y = media.resample(xd, lengths=lengths)
    S_out = out_len(S, L, M)
    assert y.shape == (len(lengths), S_out) and y.dtype == torch.float32
    assert media.resample_lengths(lengths) == [out_len(n, L, M) for n in lengths]
    got = y.cpu()
    for b, n in enumerate(lengths):
        m = out_len(n, L, M)
        ref, scale = resample_ref(x[b, :n].numpy(), H, L, M, with_abs=True)
        err = np.abs(got[b, :m].numpy().astype(np.float64) - ref)
        bound = ntaps * 2.0 ** -23 * scale
        print(f"n={n}: worst error = {float((err / np.maximum(bound, 1e-300)).max()):.3f} of the bound")
        assert (err <= bound).all(), (n, float(err.max()))
        alone = media.resample(x[b:b + 1, :n].contiguous().to(DEV))[0].cpu()
        assert alone.shape == (m,) and torch.equal(got[b, :m], alone), n
        tail = got[b, m:]
        assert tail.numel() == S_out - m and bool((tail == 0).all()) and not bool(torch.signbit(tail).any()), n


def test_full_lengths_are_the_uniform_path(plain, res):
    from deepfake_amd import media
    for (x, _), S, kw in ((plain, PLAIN_S, {}), (res, RES_S, {"sr_in": 16000})):
        xd = x.to(DEV)
        full = [S] * x.shape[0]
        for size in SIZES:
            assert torch.equal(media.mel_image(xd, lengths=full, size=size, **kw), media.mel_image(xd, size=size, **kw))
    xd = res[0].to(DEV)
    assert torch.equal(media.resample(xd, lengths=[RES_S] * xd.shape[0]), media.resample(xd))


def test_device_lengths_and_clamp(plain, res):
    """Lengths that live on the device are passed through unread; the kernels clamp them into [1, S]."""
    from deepfake_amd import media
    for (x, want), S, lengths, kw in ((plain, PLAIN_S, PLAIN_N, {}), (res, RES_S, RES_N, {"sr_in": 16000})):
        xd = _padded(x, lengths, float("nan"))
        for dtype in (torch.int64, torch.int32):
            got = media.mel_image(xd, lengths=torch.tensor(lengths, dtype=dtype, device=DEV), **kw)
            assert torch.equal(got, want[(224, 224)])
        assert torch.equal(media.mel_image(xd, lengths=torch.tensor(lengths), **kw), want[(224, 224)])   # CPU tensor
        two = x[:2].to(DEV)   # whole rows of noise: S + 7 clamps to a length whose samples are all real
        wild = torch.tensor([0, S + 7], dtype=torch.int64, device=DEV)
        assert torch.equal(media.mel_image(two, lengths=wild, **kw), media.mel_image(two, lengths=[1, S], **kw))
        if kw:
            assert torch.equal(media.resample(two, lengths=wild), media.resample(two, lengths=[1, S]))
    # the operator library's entries are the same calls
    xd, n = _padded(res[0], RES_N, 0.0), torch.tensor(RES_N, device=DEV)
    assert torch.equal(torch.ops.dfk.mel_image_ragged(xd, n, 16000), res[1][(224, 224)])
    assert torch.equal(torch.ops.dfk.resample_ragged(xd, n), media.resample(xd, lengths=RES_N))
    xd = _padded(plain[0], PLAIN_N, 0.0)
    assert torch.equal(torch.ops.dfk.mel_image_ragged(xd, torch.tensor(PLAIN_N, device=DEV)), plain[1][(224, 224)])


def test_host_lengths_are_validated_on_device_waves():
    from deepfake_amd import media
    x = torch.zeros(2, 1000, device=DEV)
    for bad in ([1000], [1000, 1000, 1000], [0, 1000], [1000, 1001], [[1000, 1000]], [0.5, 1.0]):
        with pytest.raises(ValueError):
            media.mel_image(x, lengths=bad)
        with pytest.raises(ValueError):
            media.resample(x, lengths=bad)
    with pytest.raises(ValueError):
        media.mel_image(x, lengths=torch.zeros(3, dtype=torch.int64, device=DEV))   # a device tensor's shape is known


def test_trainer_and_inference_path_ragged_wave16k():
    """seconds=(lo, hi): clips of unequal length; fusion_collate keeps the mel slot a list (the same samples as
    PAudio); prepare_mel, Trainer._features and SubmitCtl._features give gray_normalize of the per-clip images."""
    from deepfake_amd import media
    from deepfake_amd.data import DeepFake, fusion_collate, fusion_collate_test
    from deepfake_amd.models.fused import CONFIGS
    from deepfake_amd.submit import SubmitCtl
    from deepfake_amd.trainer import Trainer, mel_sample_rate, pad_longest, prepare_mel
    c = CONFIGS["c1"]
    args = types.SimpleNamespace(modality="fused", num_frames=c["T"], batch_size=3, log_step=1, mel_source="wave16k")
    ds = DeepFake(args, "train", n=3, seed=3, T=c["T"], H=c["H"], W=c["W"], seconds=(0.05, 0.2), mel_source="wave16k")
    items = [ds[i] for i in range(3)]
    feat, _, _ = fusion_collate(items)
    audio = feat["Audio"]
    assert isinstance(audio, list) and len(audio) == 3
    lens = [a.numel() for a in audio]
    assert len(set(lens)) > 1 and all(800 <= n <= 3200 for n in lens), lens
    for a, p in zip(audio, feat["PAudio"]):
        assert a.dim() == 1 and a.dtype == torch.float32 and np.array_equal(a.numpy(), p)
    imgs = torch.stack([media.mel_image(a[None].to(DEV), sr_in=16000)[0] for a in audio])
    want = media.gray_normalize(imgs)
    m = prepare_mel(audio, DEV, sr=16000)
    assert m.shape == (3, 3, 224, 224) and m.dtype == torch.float32 and torch.equal(m, want)
    padded, n = pad_longest(audio, return_lengths=True)
    assert torch.equal(prepare_mel(padded, DEV, sr=16000, lengths=n), want)
    assert torch.equal(prepare_mel(padded, DEV, sr=16000, lengths=n.to(DEV)), want)

    tfeat, _ = fusion_collate_test([(f, name) for f, _, name in items])
    assert isinstance(tfeat["Audio"], list)

    class _Set:
        def test_dataloader(self):
            return [(tfeat, ["a", "b", "c"])]

    sub = SubmitCtl(torch.nn.Identity(), args, torch.device(DEV), _Set())
    assert torch.equal(sub._features(tfeat)[1], want)
    tr = types.SimpleNamespace(augment=False, model=torch.nn.Identity(), modality="fused", device=torch.device(DEV),
                               mel_sr=mel_sample_rate(args))
    assert torch.equal(Trainer._features(tr, feat)[1], want)
