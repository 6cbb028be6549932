"""GPU: window-attention core vs a torch fp32 reference (gather formulation of oracle/vst.py)."""
import math

import pytest
import torch

from oracle import vst as OV

pytestmark = pytest.mark.gpu
if torch.cuda.is_available():
    from deepfake_amd import kernels as K

DEV = "cuda"

CASES = [
    # dims(B,D,H,W), window(clamped), full window, shift, heads, hd
    ((1, 4, 14, 14), (4, 7, 7), (4, 7, 7), (2, 3, 3), 2, 32),
    ((2, 8, 14, 14), (8, 7, 7), (8, 7, 7), (0, 0, 0), 3, 32),
    ((1, 4, 10, 10), (4, 7, 7), (4, 7, 7), (2, 3, 3), 2, 32),     # padded H/W
    ((2, 4, 4, 4), (4, 4, 4), (4, 7, 7), (0, 0, 0), 4, 32),       # Q3 clamped window
    ((3, 1, 1, 49), (1, 1, 49), (1, 1, 49), (0, 0, 0), 12, 64),   # wav2vec2 (T=49)
    ((2, 1, 1, 199), (1, 1, 199), (1, 1, 199), (0, 0, 0), 4, 64), # wav2vec2 (T=199)
]


def ref_attention(qkv, pads, dims, window, full_window, shift, heads, hd, scale, rpb):
    """fp32 torch: gather windows (pad with pad vectors, roll), softmax(q k^T s + rpb + mask) v, scatter."""
    B, D, H, W = dims
    C = heads * hd
    Dp, Hp, Wp = (math.ceil(n / w) * w for n, w in zip((D, H, W), window))
    x = torch.zeros(B, Dp, Hp, Wp, 3 * C, device=qkv.device)
    x[...] = torch.cat(pads).float()
    x[:, :D, :H, :W] = qkv.view(B, D, H, W, 3 * C).float()
    tok = OV.window_token_index(Dp, Hp, Wp, window).to(qkv.device)
    d, h, w = tok // (Hp * Wp), (tok // Wp) % Hp, tok % Wp
    src = (((d + shift[0]) % Dp) * Hp + (h + shift[1]) % Hp) * Wp + (w + shift[2]) % Wp
    nW, N = tok.shape
    win = x.view(B, -1, 3 * C)[:, src.reshape(-1)].view(B * nW, N, 3, heads, hd)
    q, k, v = (win[:, :, i].transpose(1, 2) for i in range(3))
    s = (q * scale) @ k.transpose(-1, -2)
    if rpb is not None:
        idx = OV.rpb_index(full_window, N).to(qkv.device)
        s = s + rpb[idx.reshape(-1)].view(N, N, heads).permute(2, 0, 1)[None]
    if any(sh > 0 for sh in shift):
        m = OV.shift_mask(Dp, Hp, Wp, window, shift).to(qkv.device)
        s = (s.view(B, nW, heads, N, N) + m[None, :, None]).view(B * nW, heads, N, N)
    o = (torch.softmax(s, -1) @ v).transpose(1, 2).reshape(B, nW * N, C)
    out = torch.zeros(B, Dp * Hp * Wp, C, device=qkv.device).index_copy(1, src.reshape(-1), o)
    return out.view(B, Dp, Hp, Wp, C)[:, :D, :H, :W].reshape(-1, C)


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("case", CASES, ids=[str(i) for i in range(len(CASES))])
def test_wattn_fwd(dt, case):
    dims, window, fw, shift, heads, hd = case
    g = torch.Generator(device=DEV).manual_seed(3)
    rows = dims[0] * dims[1] * dims[2] * dims[3]
    C = heads * hd
    qkv = torch.randn(rows, 3 * C, device=DEV, generator=g).to(dt)
    pads = [0.3 * torch.randn(C, device=DEV, generator=g).to(dt) for _ in range(3)]
    L = (2 * fw[0] - 1) * (2 * fw[1] - 1) * (2 * fw[2] - 1)
    rpb = torch.randn(L, heads, device=DEV, generator=g) * 0.5 if hd == 32 else None
    scale = hd ** -0.5
    out, lse = K.wattn_fwd(qkv, qkv[:, C:], qkv[:, 2 * C:], 3 * C, dims, window, fw, shift, heads, hd, scale,
                           rpb=rpb, pads=pads)
    ref = ref_attention(qkv, pads, dims, window, fw, shift, heads, hd, scale, rpb)
    err = ((out.float() - ref).abs().max() / ref.abs().max()).item()
    assert err < (2e-2 if dt == torch.bfloat16 else 1e-5), err


@pytest.mark.parametrize("table", [True, False], ids=["tab", "notab"])
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("case", CASES, ids=[str(i) for i in range(len(CASES))])
def test_wattn_bwd(dt, case, table):
    """bf16: with the forward's bias tables (table-driven kernels) and without (gather kernels)."""
    dims, window, fw, shift, heads, hd = case
    if dt == torch.float32 and not table:
        pytest.skip("fp32 parity mode has one kernel pair")
    g = torch.Generator(device=DEV).manual_seed(4)
    rows = dims[0] * dims[1] * dims[2] * dims[3]
    C = heads * hd
    qkv = torch.randn(rows, 3 * C, device=DEV, generator=g).to(dt)
    pads = [0.3 * torch.randn(C, device=DEV, generator=g).to(dt) for _ in range(3)]
    Lt = (2 * fw[0] - 1) * (2 * fw[1] - 1) * (2 * fw[2] - 1)
    rpb = torch.randn(Lt, heads, device=DEV, generator=g) * 0.5 if hd == 32 else None
    scale = hd ** -0.5
    out, lse, tab = K.wattn_fwd(qkv, qkv[:, C:], qkv[:, 2 * C:], 3 * C, dims, window, fw, shift, heads, hd, scale,
                                rpb=rpb, pads=pads, use_table=table, return_table=True)
    assert (tab is not None) == (table and dt == torch.bfloat16 and (rpb is not None or any(shift)))
    dout = torch.randn(rows, C, device=DEV, generator=g).to(dt)
    dqkv = torch.empty_like(qkv)
    drpb = torch.zeros(Lt, heads, device=DEV) if rpb is not None else None
    dpads = [torch.zeros(C, device=DEV) for _ in range(3)]
    K.wattn_bwd((qkv, qkv[:, C:], qkv[:, 2 * C:], out, lse, 3 * C, dims, window, fw, shift, heads, hd, scale, rpb,
                 pads), dout, dqkv, dqkv[:, C:], dqkv[:, 2 * C:], 3 * C, drpb=drpb, dpads=dpads, tab=tab)
    # reference
    qr = qkv.float().requires_grad_(True)
    pr = [p.float().requires_grad_(True) for p in pads]
    rr = rpb.clone().requires_grad_(True) if rpb is not None else None
    ref = ref_attention(qr, pr, dims, window, fw, shift, heads, hd, scale, rr)
    ref.backward(dout.float())
    t = 3e-2 if dt == torch.bfloat16 else 1e-4

    def chk(a, b, name):
        e = ((a.float() - b).abs().max() / b.abs().max().clamp_min(1e-6)).item()
        assert e < t, f"{name}: {e}"
    chk(dqkv, qr.grad, "dqkv")
    if rpb is not None:
        chk(drpb, rr.grad, "drpb")
    padded = any(n % w for n, w in zip(dims[1:], window))
    if padded:
        chk(torch.cat(dpads), torch.cat([p.grad for p in pr]), "dpad")


def test_wattn_bwd_query_chunks():
    """A window whose Q / dO / dQ exceed the LDS (wav2vec2 at 10 s: T = 499, hd 64 -> Np 512) runs the backward
    in query chunks, dK / dV accumulated across them (bf16, attention dropout off; the dropout-on case of the
    same geometry is test_gpu_regularize.py::test_attention_dropout[499-2-64])."""
    dims, window, fw, shift, heads, hd = (2, 1, 1, 499), (1, 1, 499), (1, 1, 499), (0, 0, 0), 2, 64
    g = torch.Generator(device=DEV).manual_seed(9)
    rows, C = 2 * 499, 2 * 64
    qkv = torch.randn(rows, 3 * C, device=DEV, generator=g).to(torch.bfloat16)
    out, lse = K.wattn_fwd(qkv, qkv[:, C:], qkv[:, 2 * C:], 3 * C, dims, window, fw, shift, heads, hd, hd ** -0.5)
    dout = torch.randn(rows, C, device=DEV, generator=g).to(torch.bfloat16)
    dqkv = torch.empty_like(qkv)
    K.wattn_bwd((qkv, qkv[:, C:], qkv[:, 2 * C:], out, lse, 3 * C, dims, window, fw, shift, heads, hd, hd ** -0.5,
                 None, None), dout, dqkv, dqkv[:, C:], dqkv[:, 2 * C:], 3 * C)
    qr = qkv.float().requires_grad_(True)
    ref = ref_attention(qr, [torch.zeros(C, device=DEV)] * 3, dims, window, fw, shift, heads, hd, hd ** -0.5, None)
    assert ((out.float() - ref).abs().max() / ref.abs().max()).item() < 2e-2
    ref.backward(dout.float())
    e = ((dqkv.float() - qr.grad).abs().max() / qr.grad.abs().max()).item()
    assert e < 3e-2, e


# v5 forward schedules: (dims, window, shift, heads) chosen for each (pairs % 4, tail) the balanced schedule takes
V5_CASES = [
    ((1, 8, 14, 14), (8, 7, 7), (4, 3, 3), 3),    # N 392: 13 query blocks, pairs 6 (R 2) + tail
    ((1, 6, 14, 14), (6, 7, 7), (3, 3, 3), 2),    # N 294: 10 blocks, pairs 5 (R 1), no tail
    ((1, 7, 14, 14), (7, 7, 7), (3, 3, 3), 2),    # N 343: 11 blocks, pairs 5 (R 1) + tail
    ((1, 5, 14, 14), (5, 7, 7), (2, 3, 3), 2),    # N 245: 8 blocks, pairs 4 (R 0), no tail
    ((1, 2, 24, 24), (2, 12, 12), (1, 6, 6), 2),  # N 288: 9 blocks, pairs 4 (R 0) + tail
    ((1, 3, 14, 14), (3, 7, 7), (1, 3, 3), 2),    # N 147: 5 blocks, pairs 2 (R 2) + tail
    ((1, 4, 14, 14), (4, 7, 7), (2, 3, 3), 2),    # N 196: 7 blocks, pairs 3 (R 3: simple schedule)
]
V5_POLICIES = [(5, 0), (5, 1 << 40), (4, -1), (6, 1 << 40)]   # v5 balanced / simple, v4, v6 (one schedule)


@pytest.mark.parametrize("policy", V5_POLICIES, ids=["v5bal", "v5", "v4", "v6"])
@pytest.mark.parametrize("extreme", ["normal", "huge", "tiny"])
@pytest.mark.parametrize("case", V5_CASES, ids=[str(i) for i in range(len(V5_CASES))])
def test_wattn_fwd_v5(case, extreme, policy):
    """bf16 table forward, every forward policy (v5 on both its schedules) against the fp32 reference.  'huge'
    scores (up to ~±600 log2 units) and 'tiny' rows (every score ~ -150 log2 units) are rejected by the fast
    path's l in [2^-80, 2^100] test and recomputed by the max-subtracted loop: the output is still the softmax."""
    dims, window, shift, heads = case
    hd = 32
    g = torch.Generator(device=DEV).manual_seed(11)
    rows = dims[0] * dims[1] * dims[2] * dims[3]
    C = heads * hd
    qkv = torch.randn(rows, 3 * C, device=DEV, generator=g)
    if extreme == "huge":
        qkv[:, :2 * C] *= 6.0
    qkv = qkv.to(torch.bfloat16)
    pads = [0.3 * torch.randn(C, device=DEV, generator=g).to(torch.bfloat16) for _ in range(3)]
    L = (2 * window[0] - 1) * (2 * window[1] - 1) * (2 * window[2] - 1)
    rpb = torch.randn(L, heads, device=DEV, generator=g) * 0.5
    if extreme == "tiny":
        rpb -= 100.0
    scale = hd ** -0.5
    K.wattn_fwd_policy(*policy)
    try:
        out, lse = K.wattn_fwd(qkv, qkv[:, C:], qkv[:, 2 * C:], 3 * C, dims, window, window, shift, heads, hd,
                               scale, rpb=rpb, pads=pads)
        K.wattn_fwd_policy(4, -1)
        out4, lse4 = K.wattn_fwd(qkv, qkv[:, C:], qkv[:, 2 * C:], 3 * C, dims, window, window, shift, heads, hd,
                                 scale, rpb=rpb, pads=pads)
    finally:
        K.wattn_fwd_policy(6, -2)   # the defaults (dfk_wattn_fwd_policy)
    torch.cuda.synchronize()
    if extreme == "normal":
        ref = ref_attention(qkv, pads, dims, window, window, shift, heads, hd, scale, rpb)
        err = ((out.float() - ref).abs().max() / ref.abs().max()).item()
        assert err < 2e-2, err
    # against v4 (the max-subtracted kernel, pinned to the reference at normal ranges; at extreme ranges the
    # bf16 bias table and the bf16 Q' quantise the logits, so the fp32 reference is not the yardstick there):
    # rejected blocks are recomputed by v4's own loop
    err4 = ((out.float() - out4.float()).abs().max() / out4.float().abs().max()).item()
    assert err4 < 1e-2, err4
    # the saved log-sum-exp (what the backward reads) agrees with v4's at every real query
    nW, N, Np = K.window_geometry(dims, window)
    d = (lse.view(-1, Np)[:, :N] - lse4.view(-1, Np)[:, :N]).abs().max().item()
    assert d < 1e-3 * max(1.0, lse4.view(-1, Np)[:, :N].abs().max().item()), d


GROUP_CASES = [
    ((4, 8, 14, 14), (8, 7, 7), (8, 7, 7), (4, 3, 3), 3, 32),   # 8 shift classes, ragged groups (2-window classes)
    ((3, 4, 14, 14), (4, 7, 7), (4, 7, 7), (2, 3, 3), 2, 32),
    ((5, 1, 14, 14), (1, 7, 7), (1, 7, 7), (0, 3, 3), 4, 32),   # SwinV2-shaped 49-token windows, 4 classes
]


@pytest.mark.parametrize("case", GROUP_CASES, ids=[str(i) for i in range(len(GROUP_CASES))])
def test_wattn_bwd_grouped_drpb(case):
    """The bf16 table backward with G windows of one (shift class, head) per workgroup summing their dS^T into one
    dRPB scratch slab (dfk_wattn_bwd_policy): dq / dk / dv are bit-identical to the ungrouped launch (the same
    arithmetic per window), dRPB within bf16 partial-sum rounding of it, and both match the fp32 reference."""
    dims, window, fw, shift, heads, hd = case
    g = torch.Generator(device=DEV).manual_seed(12)
    rows = dims[0] * dims[1] * dims[2] * dims[3]
    C = heads * hd
    qkv = torch.randn(rows, 3 * C, device=DEV, generator=g).to(torch.bfloat16)
    pads = [0.3 * torch.randn(C, device=DEV, generator=g).to(torch.bfloat16) for _ in range(3)]
    Lt = (2 * fw[0] - 1) * (2 * fw[1] - 1) * (2 * fw[2] - 1)
    rpb = torch.randn(Lt, heads, device=DEV, generator=g) * 0.5
    scale = hd ** -0.5
    out, lse, tab = K.wattn_fwd(qkv, qkv[:, C:], qkv[:, 2 * C:], 3 * C, dims, window, fw, shift, heads, hd, scale,
                                rpb=rpb, pads=pads, return_table=True)
    dout = torch.randn(rows, C, device=DEV, generator=g).to(torch.bfloat16)
    res = {}
    try:
        for G in (1, 2, 3, 8):
            K.wattn_bwd_policy(G)
            dqkv = torch.empty_like(qkv)
            drpb = torch.zeros(Lt, heads, device=DEV)
            dpads = [torch.zeros(C, device=DEV) for _ in range(3)]
            K.wattn_bwd((qkv, qkv[:, C:], qkv[:, 2 * C:], out, lse, 3 * C, dims, window, fw, shift, heads, hd, scale,
                         rpb, pads), dout, dqkv, dqkv[:, C:], dqkv[:, 2 * C:], 3 * C, drpb=drpb, dpads=dpads, tab=tab)
            res[G] = (dqkv, drpb, dpads)
    finally:
        K.wattn_bwd_policy(0)
    torch.cuda.synchronize()
    qr = qkv.float().requires_grad_(True)
    rr = rpb.clone().requires_grad_(True)
    ref = ref_attention(qr, [p.float() for p in pads], dims, window, fw, shift, heads, hd, scale, rr)
    ref.backward(dout.float())
    d1, r1, p1 = res[1]
    for G, (dq, dr, dp) in res.items():
        assert torch.equal(dq, d1), G
        for a, b in zip(dp, p1):
            assert torch.equal(a, b), G
        e1 = ((dr - r1).abs().max() / r1.abs().max()).item()
        assert e1 < 5e-3, (G, e1)
        e = ((dr - rr.grad).abs().max() / rr.grad.abs().max()).item()
        assert e < 3e-2, (G, e)
