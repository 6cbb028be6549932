"""CPU: the resampler in the dfk operator library (deepfake_amd/ops.py) — registration, shape propagation through
the fake implementations, and the loud failure on CPU tensors."""
import pytest
import torch
from torch._subclasses.fake_tensor import FakeTensorMode

import deepfake_amd.ops as O


def test_resample_ops_registered():
    assert hasattr(torch.ops.dfk, "resample") and hasattr(torch.ops.dfk, "mel_image_resampled")
    assert "resample" in O.OPS and "mel_image_resampled" in O.OPS
    assert str(torch.ops.dfk.resample.default._schema) == \
        "dfk::resample(Tensor wave, SymInt sr_in=16000, SymInt sr_out=22050) -> Tensor"


def test_resample_fake_shapes():
    with FakeTensorMode():
        x = torch.empty(2, 64000, device="cuda")
        y = torch.ops.dfk.resample(x)
        assert y.shape == (2, 88200) and y.dtype == torch.float32
        assert torch.ops.dfk.resample(torch.empty(3, 1000, device="cuda")).shape == (3, 1379)
        assert torch.ops.dfk.resample(torch.empty(1, 257, device="cuda"), 16000, 24000).shape == (1, 386)
        img = torch.ops.dfk.mel_image_resampled(x)
        assert img.shape == (2, 224, 224) and img.dtype == torch.uint8


def test_resample_cpu_tensor_fails_loudly():
    with pytest.raises(RuntimeError, match="GPU only"):
        torch.ops.dfk.resample(torch.zeros(2, 1000))
    with pytest.raises(RuntimeError, match="GPU only"):
        torch.ops.dfk.mel_image_resampled(torch.zeros(2, 1000))
