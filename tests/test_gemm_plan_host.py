"""CPU: the host-side decisions of dfk_gemm that show in dfk_gemm_workspace (automatic split count, slab size,
bias-gradient partials, which launches take the LDS-DMA vector path).  dfk_gemm_workspace touches no device, so
the library is called here with made-up operand addresses.

The expected byte counts were recorded from the library of the commit before the dispatch was folded (069bc1d),
built from that commit's sources; they were never taken from the code under test.
"""
import os

import pytest

from deepfake_amd import _lib as L

P = 0x7F0000000000   # a 16-byte aligned made-up address


def case(M, N, K, dtype=L.BF16, ak=0, bk=0, splitk=1, atomic=0, rowsum=0, c_f32=0, nz=(1, 1), a_ld=None, b_ld=None,
         a_ptr=P, a_conv=None, b_conv=None, bs=(0, 0)):
    g = L.GemmArgs()
    g.a.ptr, g.b.ptr, g.c = a_ptr, P + (1 << 36), P + (2 << 36)
    g.a.ld = a_ld if a_ld is not None else (M if ak else K)
    g.b.ld = b_ld if b_ld is not None else (N if bk else K)
    g.a.bs0, g.a.bs1 = bs
    for v, conv in ((g.a, a_conv), (g.b, b_conv)):
        if conv:
            v.conv_cg, v.conv_stride, v.conv_pad, v.conv_rows = conv
    g.ldc = N
    g.M, g.N, g.K, g.dtype = M, N, K, dtype
    g.a_kmajor, g.b_kmajor, g.c_f32 = ak, bk, c_f32
    g.nz0, g.nz1 = nz
    g.splitk, g.atomic = splitk, atomic
    g.beta = 1.0 if c_f32 else 0.0
    g.rowsum = P + (3 << 36) if rowsum else None
    return g


DW = dict(ak=1, bk=1, c_f32=1)
# (name, arguments, workspace bytes of the parent commit's library)
CASES = [
    # automatic splits, the four layouts, bf16 and fp32
    ("bf16_nn_1568x512x2048", case(1568, 512, 2048), 6422528),
    ("bf16_nk_1568x512x2048", case(1568, 512, 2048, bk=1), 6422528),
    ("bf16_kn_1568x512x2048", case(1568, 512, 2048, ak=1), 6422528),
    ("bf16_kk_1568x512x2048", case(1568, 512, 2048, ak=1, bk=1), 6422528),
    ("f32_nn_1568x512x2048", case(1568, 512, 2048, dtype=L.F32), 12845056),
    ("f32_nk_1568x512x2048", case(1568, 512, 2048, dtype=L.F32, bk=1), 12845056),
    ("f32_kn_1568x512x2048", case(1568, 512, 2048, dtype=L.F32, ak=1), 12845056),
    ("f32_kk_1568x512x2048", case(1568, 512, 2048, dtype=L.F32, ak=1, bk=1), 12845056),
    ("bf16_1592x768x3072", case(1592, 768, 3072), 14671872),
    ("f32_1592x768x3072", case(1592, 768, 3072, dtype=L.F32), 14671872),
    ("bf16_1000x288x96", case(1000, 288, 96), 0),
    ("bf16_8200x4104x200", case(8200, 4104, 200), 0),
    ("bf16_64x1536x512", case(64, 1536, 512), 0),
    ("f32_64x1536x512", case(64, 1536, 512, dtype=L.F32), 0),
    ("bf16_64x1536x4096", case(64, 1536, 4096), 1966080),
    ("bf16_3x512x1024", case(3, 512, 1024), 0),
    ("bf16_batched_2x3_64x64x2048", case(64, 64, 2048, nz=(2, 3), bs=(3 * 64 * 2048, 64 * 2048)), 196608),
    # extents that are no multiple of 8
    ("bf16_40000x100x96", case(40000, 100, 96), 0),
    ("bf16_40000x96x100", case(40000, 96, 100), 0),
    ("bf16_kk_100x96x40000_rs32", case(100, 96, 40000, splitk=32, atomic=1, rowsum=1, **DW), 0),
    # caller splits through slabs
    ("bf16_nn_split4", case(1568, 512, 2048, splitk=4), 12845056),
    ("bf16_dw_slab16_rs", case(96, 96, 50176, splitk=16, rowsum=1, **DW), 589824),
    ("bf16_dw_slab32_rs", case(96, 96, 50176, splitk=32, rowsum=1, **DW), 1191936),
    ("bf16_dw_slab32", case(96, 96, 50176, splitk=32, **DW), 1179648),
    ("f32_dw_slab32_rs", case(96, 96, 50176, dtype=L.F32, splitk=32, rowsum=1, **DW), 1179648),
    # weight gradients: unsplit, atomic splits below and at 32, with and without the fused bias gradient
    ("bf16_dw_unsplit_rs", case(96, 96, 50176, rowsum=1, **DW), 2421120),
    ("bf16_dw_atomic8_rs", case(96, 96, 50176, splitk=8, atomic=1, rowsum=1, **DW), 0),
    ("bf16_dw_atomic31_rs", case(96, 96, 50176, splitk=31, atomic=1, rowsum=1, **DW), 0),
    ("bf16_dw_atomic32_rs", case(96, 96, 50176, splitk=32, atomic=1, rowsum=1, **DW), 12288),
    ("bf16_dw_atomic64", case(96, 96, 50176, splitk=64, atomic=1, **DW), 0),
    ("bf16_dw_2048x512x1568_atomic32_rs", case(2048, 512, 1568, splitk=32, atomic=1, rowsum=1, **DW), 262144),
    ("f32_dw_atomic32_rs", case(2048, 512, 1568, dtype=L.F32, splitk=32, atomic=1, rowsum=1, **DW), 0),
    # off the LDS-DMA vector path: an operand that is not 16-byte aligned, a view of 2 GB and more
    ("bf16_dw_atomic32_rs_unaligned", case(2048, 512, 1568, splitk=32, atomic=1, rowsum=1, a_ptr=P + 2, **DW), 0),
    ("bf16_dw_atomic32_rs_2gb", case(64, 64, 32768, splitk=32, atomic=1, rowsum=1, a_ld=40000, **DW), 0),
    # a wav2vec2 conv layer at batch 1 (512 channels, kernel 3, stride 2, 3199 -> 1599 frames): forward, weight gradient
    ("bf16_conv_fwd", case(1599, 512, 1536, a_ld=512, a_conv=(512, 2, 0, 3199)), 6549504),
    ("bf16_conv_dw", case(512, 1536, 1599, b_ld=512, b_conv=(512, 2, 0, 3199), **DW), 6291456),
]


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(L.LIB_PATH):
        pytest.skip("libdfk.so not built (run python -m deepfake_amd.build)")
    return L.lib()


@pytest.mark.parametrize("name,g,expect", CASES, ids=[c[0] for c in CASES])
def test_gemm_workspace_bytes(lib, name, g, expect):
    assert lib.dfk_gemm_workspace(g) == expect
