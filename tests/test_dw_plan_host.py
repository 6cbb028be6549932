"""CPU: the host policies of the Python op layer that are pure functions of integers — the split plan of a
weight-gradient GEMM (kernels.dw_plan) and the slab / atomic choice of the LayerNorm backward's dw/db partials —
and the set of DFK_* environment variables the package still reads.

The expected dW triples were recorded from the commit before the plan was pulled out of _dw_args (9b06211): that
commit's kernels._dw_args, no DFK_* variable set, called on stand-in tensor objects (shape, stride, dtype, data_ptr,
is_cuda), reading (splitk, atomic) from the dfk_gemm_args it returned and the workgroup count beside it.  The
LayerNorm values are that commit's rule `_ln_bwd_blocks(rows, C) >= 64 and not rows <= 4096` at its defaults.  None
of them were taken from the code under test.
"""
import os
import re

import pytest

from deepfake_amd import kernels as K

# ((M, N, K), (splitk, atomic, workgroups)) of dw[N, K] += dy[M, N]^T x[M, K]
DW_CASES = [
    ((25088, 512, 128), (24, True, 96)),        # SwinV2 stage-1 fc1: capped by the partial bytes, rounded 30 -> 24
    ((50176, 96, 96), (98, True, 98)),
    ((40000, 384, 96), (64, True, 192)),
    ((401408, 96, 96), (256, True, 256)),
    ((1568, 2048, 512), (3, True, 192)),
    ((1592, 768, 3072), (1, False, 576)),
    ((1592, 2304, 768), (1, False, 432)),
    ((3, 512, 1024), (1, False, 32)),
    ((64, 1536, 512), (1, False, 48)),
    ((2000, 1536, 1024), (1, False, 384)),      # 384 64x64 tiles: the first unsplit grid
    ((2000, 1472, 1024), (2, True, 192)),       # 368 tiles: still split, on 128x128 tiles
    ((30000, 256, 128), (40, True, 80)),        # two tiles, 43 splits rounded to a multiple of 8 (XCD grouping)
    ((30000, 128, 128), (58, True, 58)),        # one tile: 58 splits stay unrounded
]

# ((rows, C), slab partials)
LN_CASES = [((1568, 512), False), ((392, 1024), False), ((4096, 512), False), ((4097, 512), True),
            ((4100, 96), True), ((6272, 768), True), ((401408, 96), True)]


@pytest.mark.parametrize("mnk,expect", DW_CASES, ids=["x".join(map(str, c[0])) for c in DW_CASES])
def test_dw_plan(mnk, expect):
    assert K.dw_plan(*mnk) == expect


class _Stop(Exception):
    pass


@pytest.mark.parametrize("shape,expect", LN_CASES, ids=["x".join(map(str, c[0])) for c in LN_CASES])
def test_layernorm_bwd_slab_choice(shape, expect, monkeypatch):
    """layernorm_bwd asks for the partial slab's workspace exactly when it chose slab partials; the stand-in
    library stops the call there (no device)."""
    asked = []

    class Lib:
        @staticmethod
        def dfk_layernorm_bwd_workspace(rows, C):
            asked.append((rows, C))
            raise _Stop

        @staticmethod
        def dfk_layernorm_bwd(*a):
            raise _Stop

    class T:
        is_cuda = True
        device = "cpu"

        def __init__(self, *shape):
            self.shape = shape

        def data_ptr(self):
            return 0x7F0000000000

    monkeypatch.setattr(K.L, "lib", lambda: Lib)
    monkeypatch.setattr(K.L, "dt", lambda t: K.L.BF16)
    monkeypatch.setattr(K.L, "drop", lambda spec, device: None)
    monkeypatch.setattr(K.L, "stream", lambda: None)
    rows, C = shape
    x = T(rows, C)
    with pytest.raises(_Stop):
        K.layernorm_bwd(x, x, T(C), T(rows), T(rows), T(C), T(C), dx=x)
    assert asked == ([shape] if expect else [])


KEPT = {"DFK_LIB", "DFK_DDP_FORCE", "DFK_WGRAD", "DFK_INLAUNCH_COMBINE"}


def test_environment_reads():
    """The DFK_* variables read from the environment anywhere in the package: os.environ in the Python sources,
    getenv in csrc/."""
    root = os.path.dirname(os.path.abspath(K.__file__))
    found = set()
    for d, _, files in os.walk(root):
        for f in files:
            if f.endswith(".py"):
                pat = r"""(?:os\.environ(?:\.get\(|\[|\.pop\(|\.setdefault\()|os\.getenv\()\s*["'](DFK_\w+)["']"""
            elif os.path.basename(d) == "csrc" and f.endswith((".hip", ".h", ".cpp")):
                pat = r"""getenv\(\s*"(DFK_\w+)"\s*\)"""
            else:
                continue
            with open(os.path.join(d, f), encoding="utf-8") as fh:
                found |= set(re.findall(pat, fh.read()))
    assert found == KEPT
