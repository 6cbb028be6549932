"""GPU: dfk_gemm's kernel families, tiles, layouts, split-K mechanisms and epilogues against the float64 reference
of the dfk_gemm contract (tests/gemm_ref.py, pinned on the CPU by tests/test_gemm_ref_host.py), bit for bit.

Operands are integers with |v| <= 2; bias, residual and the old contents of C are integers with |v| <= 4; alpha and
beta are 1 or 0.5; K <= 4104.  Every partial sum of every launch is then an integer or half-integer below 2^15, so
every fp32 accumulation is exact in any order -- through k-tiles, split slabs and atomics -- and the kernel's output
must equal the reference's one round-to-nearest-even conversion (f2bf in csrc/common.h): no tolerance, and every
dropped, duplicated or misplaced element shows.  check() asserts that bound on the reference of each launch, so a
later edit of the inputs cannot silently leave the exact regime.  Only the outputs of act 1 / act 2 go through erf:
they are compared with the bound tests/test_gpu_ops.py uses for the same epilogues, against the float64 reference;
the pre-activation that act 1 saves is compared exactly.

Every output lies inside a wider buffer (ld > N, rows below, sometimes elements before) that is pre-filled with a
sentinel, and the WHOLE buffer is compared: an epilogue tail that writes past N or M changes the sentinel.

The launches go through kernels._gemm_args / _gemm_launch, i.e. raw kernels.gemm, with no routing knob touched.
Where a case relies on a split, the split count is asserted through dfk_gemm_workspace before the launch.

Why each shape reaches its leaf (launch() in csrc/gemm.hip):
  dma_vec     bf16, both bases 16-byte aligned, ld and batch strides % 8 == 0, contiguous extents % 8 == 0
              (K for a row-major operand, M / N for a k-major one): the LDS-DMA kernel, else the register-staged one
  views_vec   the same test with 8 (bf16) / 4 (fp32) on the register-staged kernel: vector or element-wise loaders
  pick_wt     atomic or splitk > 1: 64 (128x128 tiles); else 32 below kTiles128MinDma = 1024 128x128-tiles, which
              every shape here is
  pick_tile   wave tile 32, no conv view, A row-major, dma_vec: the 8-wave 128x64 (M >= N) / 64x128 (M < N); else
              the square 64x64 / 128x128
  auto_splitk splitk == 1, not atomic: min(K // (12 k-tiles), ceil(768 / tiles)) splits; k-tile 64 (bf16), 32 (fp32)
  kchunk      ceil(K / splits) rounded up to whole k-tiles, so late splits can be short or empty
  kRsPartialMin = 32: from 32 splits on, the LDS-DMA kernel writes bias-gradient partials for rowsum_reduce_kernel
"""
import pytest
import torch

from gemm_ref import gemm_ref

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from deepfake_amd import _lib as L
    from deepfake_amd import kernels as K

BF, F32 = torch.bfloat16, torch.float32
SENT = 77.0          # the sentinel around every output: a bf16 number, neither zero nor a value a store leaves
EXACT_BOUND = 2 ** 15
OBSERVED = {}        # id -> largest rel of a toleranced GELU output (printed with -s)


def tol(dt):         # tests/test_gpu_ops.py's bound for the same epilogues
    return 2e-2 if dt == BF else 2e-5


class Gen:
    def __init__(self, seed):
        self.g = torch.Generator(device="cuda").manual_seed(seed)

    def ints(self, n, dt, lim=2):
        return torch.randint(-lim, lim + 1, (int(n),), device="cuda", generator=self.g).to(dt)


def storage(t):
    return torch.as_strided(t, (t.untyped_storage().nbytes() // t.element_size(),), (1,), 0)


def window(t, nz, M, N, ld, bs):
    """The [nz0, nz1, M, N] window of base tensor t, as a view."""
    return torch.as_strided(t, (nz[0], nz[1], M, N), (bs[0], bs[1], ld, 1), t.storage_offset())


def outbuf(gen, dt, nz, M, N, ld, bs, off=0, prefill=False, tail=0):
    """A sentinel-filled buffer holding the nz0 x nz1 windows of M x N at leading dimension ld, `off` elements
    before the base and two rows (+ tail) after the last window; prefill: the windows hold integers |v| <= 4.
    Returns the base tensor."""
    n = off + (nz[0] - 1) * bs[0] + (nz[1] - 1) * bs[1] + (M + 2) * ld + tail
    buf = torch.full((n,), SENT, device="cuda", dtype=dt)
    base = buf[off:]
    if prefill:
        w = window(base, nz, M, N, ld, bs)
        w.copy_(gen.ints(w.numel(), dt, 4).view(w.shape))
    return base


def check(name, pos, kw, slab=0, part=0, toleranced=False):
    """One launch against the reference: workspace bytes (the split count), the exact regime, then the whole of C,
    aux and rowsum."""
    a, _, _, _, _, _, M, N, Kd, c, ldc = pos
    nz = kw.get("nz", (1, 1))
    kw = dict(kw, dtype=L.dt(a))
    ref = gemm_ref(*pos, **kw)
    # the exact regime: any partial sum, in any order, is a (half-)integer below 2^15
    assert ref.bound < EXACT_BOUND, (name, ref.bound)
    if not toleranced:
        assert torch.equal(ref.c64 * 2, (ref.c64 * 2).round()), name
    g = K._gemm_args(*pos, **kw)
    ws = L.lib().dfk_gemm_workspace(g)
    assert ws == slab * nz[0] * nz[1] * M * N * 4 + part * M * 4, (name, ws, slab, part)
    K._gemm_launch(g, c)
    torch.cuda.synchronize()
    got = storage(c)
    if toleranced:
        mask = torch.zeros(got.shape, device="cuda", dtype=torch.bool)
        window(mask[c.storage_offset():], nz, M, N, ldc, kw.get("c_bs", (0, 0))).fill_(True)
        assert torch.equal(got[~mask], ref.c[~mask]), f"{name}: C changed outside its window"
        want = ref.c64[mask]
        r = ((got[mask].double() - want).abs().max() / want.abs().max().clamp_min(1e-12)).item()
        OBSERVED[name] = max(OBSERVED.get(name, 0.0), r)
        print(f"{name}: rel {r:.3e} (bound {tol(a.dtype):.0e})")
        assert r < tol(a.dtype), (name, r)
    else:
        same(name + " C", got, ref.c)
    if ref.aux is not None:
        same(name + " aux", storage(kw["aux"]), ref.aux)
    if ref.rowsum is not None:
        same(name + " rowsum", storage(kw["rowsum"]), ref.rowsum)


def same(what, got, want):
    if not torch.equal(got, want):
        bad = (got != want).nonzero().flatten()
        i = bad[:8].tolist()
        raise AssertionError(f"{what}: {bad.numel()} of {got.numel()} elements differ; flat offsets {i}: got "
                             f"{got[bad[:8]].tolist()}, want {want[bad[:8]].tolist()}")


def plain(lay, M, N, Kd, dt=None, epi="", beta=0.0, splitk=1, atomic=False, c_f32=False, rowsum=False, a_pad=0,
          b_pad=0, a_off=0, b_off=0, c_off=0, c_pad=None, nz=(1, 1), slab=0, part=0, seed=0):
    """A case of plain (non-conv) views.  lay: 'r' (row-major) or 'k' (k-major) for A and B.  epi: words of bias, res,
    gelu (act 1 + aux), dgelu (act 2), alpha (0.5), relu (act 3).  *_pad widens a leading dimension, *_off moves a
    base off its allocation by that many elements (8 keeps a bf16 base 16-byte aligned, 1 does not).  Batches
    (nz) are laid out one after another; B and the bias are per z1 (grouped weights)."""
    dt = dt or BF

    def run(name):
        gen = Gen(seed)
        ak, bk = lay[0] == "k", lay[1] == "k"
        vec = 8 if dt == BF else 4
        cdt = F32 if (c_f32 or atomic) else dt
        ar, ac = (Kd, M) if ak else (M, Kd)
        br, bc = (Kd, N) if bk else (N, Kd)
        a_ld, b_ld = ac + a_pad, bc + b_pad
        a_bs, b_bs = (nz[1] * ar * a_ld, ar * a_ld), (0, br * b_ld)
        a = gen.ints(a_off + nz[0] * nz[1] * ar * a_ld, dt)[a_off:]
        b = gen.ints(b_off + nz[1] * br * b_ld, dt)[b_off:]
        ldc = N + (vec if c_pad is None else c_pad)
        c_bs = (nz[1] * (M + 2) * ldc, (M + 2) * ldc)
        c = outbuf(gen, cdt, nz, M, N, ldc, c_bs, off=c_off, prefill=beta != 0.0 or atomic)
        kw = dict(nz=nz, a_bs=a_bs, b_bs=b_bs, c_bs=c_bs, splitk=splitk, atomic=atomic, c_f32=c_f32, beta=beta)
        words = epi.split()
        ldr = -(-N // vec) * vec + vec   # bias stride and residual ld: wider than N, and whole vectors
        if "bias" in words:
            kw.update(bias=gen.ints(nz[1] * ldr, dt, 4), bias_bs1=ldr)
        if "res" in words:
            kw.update(residual=gen.ints(nz[0] * nz[1] * M * ldr, dt, 4), ldr=ldr, r_bs=(nz[1] * M * ldr, M * ldr))
        if "gelu" in words:
            kw.update(act=1, aux=outbuf(gen, dt, nz, M, N, ldc, c_bs), ldaux=ldc)
        if "dgelu" in words:
            kw.update(act=2, aux=outbuf(gen, dt, nz, M, N, ldc, c_bs, prefill=True), ldaux=ldc)
        if "relu" in words:
            kw.update(act=3)
        if "alpha" in words:
            kw.update(alpha=0.5)
        if rowsum:
            rs = torch.full((M + 8,), SENT, device="cuda")
            rs[:M] = gen.ints(M, F32, 4)
            kw.update(rowsum=rs)
        check(name, (a, a_ld, ak, b, b_ld, bk, M, N, Kd, c, ldc), kw, slab=slab, part=part,
              toleranced="gelu" in words or "dgelu" in words)
    return run


def each(*runs):
    def run(name):
        for i, r in enumerate(runs):
            r(f"{name}[{i}]")
    return run


# the five epilogues of the issue's forward case; beta reads the sentinel-free pre-filled window
def epilogues(lay, M, N, Kd, **kw):
    return each(plain(lay, M, N, Kd, **kw),
                plain(lay, M, N, Kd, epi="bias res", **kw),
                plain(lay, M, N, Kd, epi="bias gelu", **kw),
                plain(lay, M, N, Kd, beta=1.0, **kw),
                plain(lay, M, N, Kd, epi="bias alpha res relu", beta=0.5, **kw))


def dx_variants(M, N, Kd, **kw):
    return each(plain("rk", M, N, Kd, **kw),
                plain("rk", M, N, Kd, epi="res", beta=1.0, **kw),
                plain("rk", M, N, Kd, epi="dgelu", **kw))


def dw(M, N, Kd, rowsum, **kw):
    """dW += dy^T x: k-major x k-major, fp32 C, beta = 1 or atomic, into non-zero C (and rowsum)."""
    beta = 0.0 if kw.get("atomic") else 1.0
    return plain("kk", M, N, Kd, c_f32=True, beta=beta, rowsum=rowsum, c_pad=4, **kw)


def dw_pair(M, N, Kd, part=0, **kw):
    return each(dw(M, N, Kd, False, **kw), dw(M, N, Kd, True, part=part, **kw))


# ---- implicit-conv views: the argument mappings of functional._conv1d_gemm_fwd/_bwd and _posconv_gemm_fwd/_bwd,
# ---- outputs moved into sentinel-padded buffers
def conv1d(dt):
    """Conv1d(Cin = 64 -> Cout = 72, kernel 3, stride 2) on 2 clips (nz0) of 37 -> 18 frames: forward with bias
    (M = 18, N = 72, K = 192, A a conv view), dW (b_conv, k-major x k-major, atomic splitk = 2 of K = 18 whose
    second split is empty, both clips adding into one dW), and the per-tap dX (beta = 1, C stepped by stride * Cin
    from a base offset by the tap)."""
    def run(name):
        gen = Gen(11)
        B, Tin, Cin, Cout, k, s = 2, 37, 64, 72, 3, 2
        Tout = (Tin - k) // s + 1
        vec = 8 if dt == BF else 4
        x, w2 = gen.ints(B * Tin * Cin, dt), gen.ints(Cout * k * Cin, dt)
        ldc = Cout + vec
        c_bs = ((Tout + 2) * ldc, 0)
        y = outbuf(gen, dt, (B, 1), Tout, Cout, ldc, c_bs)
        check(name + " fwd", (x, Cin, False, w2, k * Cin, False, Tout, Cout, k * Cin, y, ldc),
              dict(bias=gen.ints(Cout, dt, 4), nz=(B, 1), a_bs=(Tin * Cin, 0), c_bs=c_bs, a_conv=(Cin, s, 0, Tin)))
        dpre = gen.ints(B * Tout * Cout, dt)
        ldw = k * Cin + 4
        dw2 = outbuf(gen, F32, (1, 1), Cout, k * Cin, ldw, (0, 0), prefill=True)
        check(name + " dW", (dpre, Cout, True, x, Cin, True, Cout, k * Cin, Tout, dw2, ldw),
              dict(c_f32=True, atomic=True, splitk=2, nz=(B, 1), a_bs=(Tout * Cout, 0), b_bs=(Tin * Cin, 0),
                   b_conv=(Cin, s, 0, Tin)))
        # dx: [B][Tin + 1 rows][Cin], every row old integers (beta = 1 reads them); the extra row per clip and the
        # rows no tap reaches must come back unchanged
        dxb = gen.ints(B * (Tin + 1) * Cin, dt, 4)
        for kk in range(k):
            wk, ck = w2[kk * Cin:], dxb[kk * Cin:]
            check(f"{name} dX tap {kk}", (dpre, Cout, False, wk, k * Cin, True, Tout, Cin, Cout, ck, s * Cin),
                  dict(beta=1.0, nz=(B, 1), a_bs=(Tout * Cout, 0), c_bs=((Tin + 1) * Cin, 0)))
    return run


def posconv():
    """Grouped Conv1d(C = 16, groups = 2 as nz1, Cg = 8, k = 4, pad k // 2, last frame dropped) on 2 clips of T = 21
    frames -- a fifth of all taps fall in the padding: forward with bias_bs1, residual and act 1 (aux exact); dW
    with c_bs = (0, Cg*k*Cg), atomic splitk = 2 (second split empty); dX with pad k // 2 - 1 and beta = 1."""
    def run(name):
        gen = Gen(12)
        B, T, G, Cg, k = 2, 21, 2, 8, 4
        C = G * Cg
        x, w2, bias = gen.ints(B * T * C, BF), gen.ints(C * k * Cg, BF), gen.ints(C, BF, 4)
        c_bs = ((T + 2) * C, Cg)                      # two sentinel rows after every clip
        y = outbuf(gen, BF, (B, G), T, Cg, C, c_bs)
        pre = outbuf(gen, BF, (B, G), T, Cg, C, c_bs)
        conv = dict(nz=(B, G), a_bs=(T * C, Cg), b_bs=(0, Cg * k * Cg), c_bs=c_bs)
        check(name + " fwd", (x, C, False, w2, k * Cg, False, T, Cg, k * Cg, y, C),
              dict(conv, bias=bias, bias_bs1=Cg, act=1, aux=pre, ldaux=C, residual=x, ldr=C, r_bs=(T * C, Cg),
                   a_conv=(Cg, 1, k // 2, T)), toleranced=True)
        dpre = gen.ints(B * T * C, BF)
        dw2 = outbuf(gen, F32, (1, G), Cg, k * Cg, k * Cg, (0, Cg * k * Cg), prefill=True, tail=8)
        check(name + " dW", (dpre, C, True, x, C, True, Cg, k * Cg, T, dw2, k * Cg),
              dict(c_f32=True, atomic=True, splitk=2, nz=(B, G), a_bs=(T * C, Cg), b_bs=(T * C, Cg),
                   c_bs=(0, Cg * k * Cg), b_conv=(Cg, 1, k // 2, T)))
        dx = outbuf(gen, BF, (B, G), T, Cg, C, c_bs, prefill=True)
        check(name + " dX", (dpre, C, False, w2, k * Cg, False, T, Cg, k * Cg, dx, C),
              dict(conv, beta=1.0, a_conv=(Cg, 1, k // 2 - 1, T)))
    return run


MW = 16385   # the weight-resident kernel's floor is 16384 rows: one row into the last 128-row tile

CASES = [
    # ------------------------------------------------------------------ LDS-DMA kernel (bf16, dma_vec holds)
    # forward, row x row.  200 x 72 (M >= N): 128x64 tiles, a ragged second row tile (72 of 128 rows), a second
    # column tile of 8 columns, K = 136 = 2 k-tiles + an 8-element tail.  auto_splitk: 136 // 768 = 0, no split.
    ("dma_fwd_128x64", epilogues("rr", 200, 72, 136)),
    # the same extents with M < N: 64x128 tiles
    ("dma_fwd_64x128", epilogues("rr", 72, 200, 136)),
    # K = 8: one partial k-tile;  M = 3: fewer rows than one 16-row MFMA block
    ("dma_fwd_K8", each(plain("rr", 200, 72, 8, epi="bias res"), plain("rr", 72, 200, 8, epi="bias res"))),
    ("dma_fwd_M3", each(plain("rr", 3, 72, 136, epi="bias res"), plain("rr", 3, 200, 136, epi="bias gelu"))),
    # scalar epilogue (epi_vec false) while the operands stay on DMA: C (and nothing else) one element off a 16-byte
    # boundary with ldc % 8 == 0; ldc = N + 1
    ("dma_fwd_c_odd_base", each(plain("rr", 200, 72, 136, epi="bias res", c_off=1),
                                plain("rr", 72, 200, 136, epi="bias gelu", c_off=1),
                                plain("rr", 200, 72, 136, epi="bias alpha res relu", beta=0.5, c_off=1))),
    ("dma_fwd_ldc_odd", each(plain("rr", 200, 72, 136, epi="bias res", c_pad=1),
                             plain("rr", 72, 200, 136, beta=1.0, c_pad=1))),
    # N = 76: a partial 8-column group (4 columns) under the vector epilogue; row x row needs only K % 8 == 0
    ("dma_fwd_N76", each(plain("rr", 200, 76, 136, epi="bias res", c_pad=4),
                         plain("rr", 200, 76, 136, epi="bias gelu", c_pad=4),
                         plain("rr", 200, 76, 136, epi="bias alpha res relu", beta=0.5, c_pad=4))),
    # dX, row x k-major B (b_ld = N): the bf16 layout kernels.linear_dx sends to hipBLASLt; both 8-wave tiles
    ("dma_dx_128x64", dx_variants(200, 72, 136)),
    ("dma_dx_64x128", dx_variants(72, 200, 136)),
    # k-major A x row-major B: a_kmajor keeps the square 64x64 tile
    ("dma_kr_64x64", each(plain("kr", 136, 72, 200), plain("kr", 136, 72, 200, epi="bias res"))),
    # batched nz0 x nz1 with per-z1 weights and bias (bias_bs1), plain views
    ("dma_batched_bias_bs1", each(plain("rr", 40, 24, 72, nz=(2, 3), epi="bias res"),
                                  plain("rk", 40, 24, 72, nz=(2, 3), epi="bias", beta=1.0))),
    # 128x128 tiles: pick_wt returns 64 for splitk > 1.  K = 200, 2 splits of kchunk 128: 128 + 72.  The slabs go
    # through splitk_reduce_kernel (2 < 8 splits) with the whole epilogue, into bf16 C and into fp32 C
    ("dma_split2_128x128", each(plain("rr", 200, 136, 200, splitk=2, slab=2),
                                plain("rr", 200, 136, 200, splitk=2, slab=2, epi="bias res"),
                                plain("rk", 200, 136, 200, splitk=2, slab=2, epi="bias res"),
                                plain("rr", 200, 136, 200, splitk=2, slab=2, epi="bias res", c_f32=True, c_pad=4),
                                plain("rk", 200, 136, 200, splitk=2, slab=2, beta=1.0, c_f32=True, c_pad=4))),
    # K = 136, 4 splits: kchunk = ceil(34 / 64) * 64 = 64, so the splits hold 64, 64, 8 and nothing: the fourth
    # slab must read as zero
    ("dma_split4_last_empty", each(plain("rr", 200, 136, 136, splitk=4, slab=4, epi="bias res"),
                                   plain("rk", 200, 136, 136, splitk=4, slab=4))),
    # automatic split: 72 x 40 is 2 tiles of 64x64, K = 1544 allows 1544 // 768 = 2 splits: kchunk 832 -> 832 + 712
    ("dma_auto_split2", each(plain("rr", 72, 40, 1544, slab=2), plain("rr", 72, 40, 1544, slab=2, epi="bias res"))),
    # dW, k-major x k-major, fp32 C.  136 x 72 x 4104 with splitk = 1 is split automatically (6 tiles of 64x64,
    # 4104 // 768 = 5 splits of kchunk 832, the last one 776) and reduced by splitk_reduce_kernel with beta = 1
    ("dma_dw_auto5", dw_pair(136, 72, 4104, slab=5)),
    # truly unsplit (712 // 768 = 0): the fp32 epilogue of the 64x64 tile adds into C
    ("dma_dw_unsplit", dw_pair(136, 72, 712)),
    # atomic splits on 128x128 tiles (1 x 2 of them): 8 splits take the XCD-remap branch of gemm_dma_body
    # (splitk % 8 == 0, more than one tile), 3 splits the other one
    ("dma_dw_atomic8_xcd", dw_pair(136, 72, 4104, splitk=8, atomic=True)),
    ("dma_dw_atomic3", dw_pair(136, 72, 4104, splitk=3, atomic=True)),
    # 16 slabs, fp32 C, N % 4 == 0, no epilogue: slab_sum_f32_kernel.  kchunk = 320: 13 splits hold work, 3 are empty
    ("dma_dw_slab16", dw_pair(136, 72, 4104, splitk=16, slab=16)),
    # N = 76: N % 8 != 0 takes the k-major B off DMA -> gemm_kernel<bf16, 64, k-major, k-major, element-wise loads>
    # (rowsum by atomics); N % 4 == 0 keeps slab_sum_f32_kernel
    ("reg_dw_slab16_N76", dw_pair(136, 76, 4104, splitk=16, slab=16)),
    # 32 atomic splits of K = 2056: kchunk 128, 17 splits hold work; with rowsum the 32 x M partials (15 rows of them
    # from empty splits, which must be zero) go through rowsum_reduce_kernel
    ("dma_dw_atomic32_partials", dw_pair(136, 72, 2056, splitk=32, atomic=True, part=32)),
    # 32 slabs + partials behind them: slab_sum_f32_kernel and rowsum_reduce_kernel
    ("dma_dw_slab32_partials", dw_pair(136, 72, 2056, splitk=32, slab=32, part=32)),
    # conv views (CONV instantiations; pick_tile keeps the square tiles)
    ("dma_conv1d", conv1d(BF)),
    ("dma_posconv", posconv()),
    # ------------------------------------------------------------------ register-staged kernel, bf16, no vector path
    # one reason each: K = 100 (row-major extents % 8 != 0), ld = K + 1, a base one element off
    ("reg_bf16_K100", each(plain("rr", 200, 72, 100, epi="bias res", a_pad=4, b_pad=4),
                           plain("rk", 200, 72, 100, epi="res", beta=1.0, a_pad=4))),
    ("reg_bf16_ld_odd", each(plain("rr", 200, 72, 136, epi="bias gelu", a_pad=1),
                             plain("rk", 200, 72, 136, epi="bias alpha res relu", beta=0.5, a_pad=1),
                             dw(136, 72, 200, True, b_pad=1))),
    ("reg_bf16_base_odd", each(plain("rr", 200, 72, 136, epi="bias res", b_off=1),
                               plain("rk", 200, 72, 136, epi="dgelu", a_off=1),
                               dw(136, 72, 200, True, a_off=1))),
    # 128x128 tiles through splitk = 2: slabs (K = 100: 64 + 36) and atomics with the bias gradient
    ("reg_bf16_split2_128x128", each(plain("rr", 200, 136, 100, splitk=2, slab=2, epi="bias res", a_pad=4, b_pad=4),
                                     plain("rk", 200, 136, 100, splitk=2, slab=2, a_pad=4),
                                     dw(136, 72, 200, True, splitk=2, atomic=True, a_off=1))),
    # ------------------------------------------------------------------ register-staged kernel, fp32
    # vector loaders (extents % 4 == 0), K = 44: a tail of 12 inside the second 32-element k-tile
    ("f32_vec_four_layouts", each(plain("rr", 200, 72, 44, dt=F32, epi="bias res"),
                                  plain("rk", 200, 72, 44, dt=F32, epi="bias gelu"),
                                  plain("kr", 200, 72, 44, dt=F32, epi="bias alpha res relu", beta=0.5),
                                  dw(200, 72, 44, True, dt=F32))),
    # element-wise loaders: K = 45 (row-major), odd M = 201 (k-major A)
    ("f32_elementwise", each(plain("rr", 200, 72, 45, dt=F32, epi="bias res", c_pad=1),
                             plain("rk", 200, 72, 45, dt=F32, epi="dgelu"),
                             plain("kr", 201, 72, 45, dt=F32, beta=1.0),
                             dw(201, 72, 45, True, dt=F32))),
    ("f32_split2_128x128", each(plain("rr", 200, 136, 44, dt=F32, splitk=2, slab=2, epi="bias res"),
                                dw(200, 72, 44, True, dt=F32, splitk=2, atomic=True))),
    # automatic split: 8 tiles of 64x64, 776 // (12 * 32) = 2 splits
    ("f32_auto_split2", plain("rr", 200, 72, 776, dt=F32, slab=2, epi="bias res")),
    ("f32_conv1d", conv1d(F32)),
    # ------------------------------------------------------------------ weight-resident kernel (wres.hip)
    # M >= 16384, K % 32 == 0, N*K small: one 96-channel slice; 576 x 192 is three slices of 192.  M = 16385: the
    # last 128-row tile holds one row.  Forward with bias + residual, and the k-major-B dX form
    ("wres_96x96", each(plain("rr", MW, 96, 96, epi="bias res"), plain("rk", MW, 96, 96))),
    ("wres_576x192", each(plain("rr", MW, 576, 192, epi="bias res"), plain("rk", MW, 576, 192, epi="res"))),
]


@pytest.mark.parametrize("name,run", CASES, ids=[c[0] for c in CASES])
def test_gemm_exact(name, run):
    run(name)
