"""Op-level tests of the Inception conv family (csrc/conv2d.hip; ConvBNReLUFn, ResConvFn, Pool2dFn) against the
float64 CPU reference tests/conv2d_ref.py (itself checked by tests/test_conv2d_ref.py), at the geometries
InceptionResV2.py really runs: Cin = 3 (scalar im2col, GEMM K = 27), C > 256 BatchNorm, BatchNorm over 1 / 4 /
255 / 256 / 257 / 33001 rows, 1x1 maps, windows that lie mostly in the padding, max-pool ties, the residual
epilogue relu(x + alpha (acc + bias)), eval-mode backward, channel-slice views and accumulate.

Every input is drawn on the CPU from a seed, rounded to the dtype under test, and handed to both sides, so the
reference sees exactly the kernel's inputs.

Exact checks (torch.equal): im2col2d / col2im2d (data movement, or sums of <= 49 integers in [-4, 4] plus a
prefill in [-2, 2], |sum| < 256: exact in fp32 and bf16), max-pool forward, max-pool backward with integer dy.

Average pool: inputs are multiples of 1/8 and dy integers, so the fp32 window sum is exact and the forward is one
rounding: |err| <= u |ref| with u = 2^-24 (fp32) / 2^-8 (bf16).  The backward adds up to 9 quotients dy / cnt
(cnt >= 4, so |.| <= 1 and partial sums < 16) in fp32: 9 * 2^-25 for the quotients + 8 * 2^-21 for the additions
< 2^-17, on top of the output rounding u |ref|.

Inherited bounds (tests/test_gpu_inception.py's for the same quantities; error = max |a - b| / max |b|, bf16
gradients ||a - b|| / ||b||):
    fp32: y 2e-5, running statistics and gradients 1e-4;  bf16: y 3e-2, running statistics 2e-2, gradients 3e-2.
In the direct BatchNorm tests mean / rstd / running statistics / dgamma / dbeta are fp32 reductions of inputs the
reference shares bit for bit, in both dtypes, so they are held to the fp32 bound 1e-4 in bf16 too.

ReLU masks: a fp32 pre-activation within round-off of 0 could take the other side of the ReLU than in float64
and move a gradient by a whole dy.  Each fp32 case therefore first asserts, on the reference alone, that no
pre-activation lies within a margin of 0 (2e-6 for BatchNorm on given rows, 2e-5 behind a conv GEMM, 1e-5 scale
in ResConvFn, in bf16 too since its mask comes from the same fp32 accumulator: >= 10x the fp32 round-off of those
values); the seeds are chosen so that this holds.

Measured bounds.  Where a case is worse conditioned than the inherited bound allows, the bound is 4x the error
of an independent implementation against the same float64 reference on the same inputs, never of the kernels
under test: for fp32, torch's own device ops (F.conv2d + F.batch_norm + relu, autograd backward); for bf16, the
float64 pipeline with the conv output z and its gradient rounded to bf16 where ConvBNReLUFn stores them.
bound = max(inherited, 4 x measured).  All eight Conv -> BN -> ReLU cases, every BatchNorm shape and every
ResConvFn shape were measured; 4 x measured stays inside the inherited bound everywhere except in the entries
below (MEASURED in the code), which are the only bounds not inherited:
    case           dtype  quantity  measured  bound
    3x3s2-to-1x1   fp32   y         2.42e-5   9.68e-5     BatchNorm over N*1*1 = 2 rows: xhat is +-sqrt(var/(var+eps)),
    3x3s2-to-1x1   fp32   dx        2.53e-5   1.01e-4     and a channel whose two values nearly coincide (var ~ eps)
    3x3s2-to-1x1   fp32   dw        3.28e-5   1.31e-4     amplifies the round-off of z by rstd ~ 30
    3x3s2-to-1x1   bf16   y         3.98e-2   1.59e-1     (the same, on z rounded to bf16)
    3x3s2-to-1x1   bf16   dx        6.19e-2   2.48e-1
    3x3s2-to-1x1   bf16   dw        6.20e-2   2.48e-1
    3x3s2-to-1x1   bf16   dgamma    7.54e-3   3.02e-2
    1x3-on-1x1     bf16   y         8.87e-3   3.55e-2     BatchNorm over 4 rows
    1x1-2080       bf16   dx        3.73e-2   1.49e-1     BatchNorm over 4 rows
    1x1-2080       bf16   dw        3.73e-2   1.49e-1
    1x1-2080       bf16   dbeta     2.48e-2   9.92e-2
    stem           bf16   dx        1.60e-2   6.40e-2     K = 27
    stem           bf16   dw        1.51e-2   6.04e-2
    stem           bf16   dgamma    1.05e-2   4.20e-2
    stem           bf16   dbeta     2.61e-2   1.04e-1
"""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

import conv2d_ref as R

pytestmark = pytest.mark.gpu
if torch.cuda.is_available():
    from deepfake_amd import functional as Fn
    from deepfake_amd import kernels as K

DEV = "cuda"
F64 = torch.float64
DTS = [torch.float32, torch.bfloat16]
EPS, MOM = 1e-3, 0.1
U = {torch.float32: 2.0 ** -24, torch.bfloat16: 2.0 ** -8}      # unit round-off of the output type

# (quantity) -> inherited bound
INHERITED = {
    torch.float32: dict(y=2e-5, rm=1e-4, rv=1e-4, dx=1e-4, dw=1e-4, dg=1e-4, db=1e-4),
    torch.bfloat16: dict(y=3e-2, rm=2e-2, rv=2e-2, dx=3e-2, dw=3e-2, dg=3e-2, db=3e-2),
}
# (case, dtype) -> {quantity: error of the independent implementation}; see the docstring
MEASURED = {
    ("3x3s2-to-1x1", torch.float32): dict(y=2.42e-5, dx=2.53e-5, dw=3.28e-5),
    ("stem", torch.bfloat16): dict(dx=1.60e-2, dw=1.51e-2, dg=1.05e-2, db=2.61e-2),
    ("3x3s2-to-1x1", torch.bfloat16): dict(y=3.98e-2, dx=6.19e-2, dw=6.20e-2, dg=7.54e-3),
    ("1x3-on-1x1", torch.bfloat16): dict(y=8.87e-3),
    ("1x1-2080", torch.bfloat16): dict(dx=3.73e-2, dw=3.73e-2, db=2.48e-2),
}


def rel(a, b):
    a, b = a.detach().cpu().to(F64), b.detach().cpu().to(F64)
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


def nrm(a, b):
    a, b = a.detach().cpu().to(F64), b.detach().cpu().to(F64)
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def gmetric(dt):
    return rel if dt == torch.float32 else nrm


def bound(case, dt, q):
    return max(INHERITED[dt][q], 4 * MEASURED.get((case, dt), {}).get(q, 0.0))


class Report:
    """Print every figure, then fail on all that missed."""

    def __init__(self, tag):
        self.tag, self.bad = tag, []

    def __call__(self, q, err, limit):
        print(f"{self.tag} {q}: {err:.3e} (bound {limit:.1e})")
        if not err <= limit:
            self.bad.append((q, err, limit))

    def done(self):
        assert not self.bad, f"{self.tag}: {self.bad}"


def rn(shape, seed, dt, scale=1.0, shift=0.0):
    """randn on the CPU, rounded to dt, as fp32."""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale + shift).to(dt).float()


def uni(shape, seed, lo, hi):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(shape, generator=g) * (hi - lo) + lo


def dev(t, dt=None):
    return t.to(DEV, dt if dt is not None else t.dtype).contiguous()


def assert_clear_of_zero(pre, margin):
    assert pre.detach().abs().min().item() > margin, "a pre-activation sits on the ReLU's edge: pick another seed"


# ------------------------------------------------------------------ im2col2d / col2im2d, bit-exact
GEO_IDS = [f"{H}x{W}-k{k[0]}x{k[1]}-s{s[0]}-p{p[0]}{p[1]}" for (H, W, k, s, p) in R.IM2COL_GEOS]
geo_params = pytest.mark.parametrize("H,W,k,s,p", R.IM2COL_GEOS, ids=GEO_IDS)
SLICES = [(8, 24), (4, 20), (2, 18)]     # of a 24-channel buffer: aligned, 8 B off in bf16, 8 B off in fp32


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("C", R.C_LIST)
@geo_params
def test_im2col2d_exact(dt, C, H, W, k, s, p):
    x = rn((2, H, W, C), 1, dt)
    got = K.im2col2d(dev(x, dt), K.conv2d_geo(2, H, W, C, k, s, p))
    assert torch.equal(got.cpu().float(), R.im2col(x, k, s, p))


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("C", R.C_LIST)
@pytest.mark.parametrize("accumulate", [False, True])
@geo_params
def test_col2im2d_exact(dt, C, accumulate, H, W, k, s, p):
    g = K.conv2d_geo(2, H, W, C, k, s, p)
    dcols = R.ints((2 * g.Ho * g.Wo, k[0] * k[1] * C), -4, 4, 2)
    pre = R.ints((2, H, W, C), -2, 2, 3)
    want = R.col2im(dcols, (2, H, W, C), k, s, p) + (pre if accumulate else 0)
    assert want.abs().max().item() < 256
    dx = dev(pre, dt)
    K.col2im2d(dev(dcols, dt), g, dx, accumulate=accumulate)
    assert torch.equal(dx.cpu().float(), want)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("lo,hi", SLICES)
@geo_params
def test_im2col2d_channel_slice(dt, lo, hi, H, W, k, s, p):
    """x is a channel slice of a wider buffer (ldx = 24 != C = 16), whose first channel need not be 16-byte
    aligned: then the kernel may not take its 16-byte vector path."""
    buf = rn((2, H, W, 24), 4, dt)
    view = dev(buf, dt)[..., lo:hi]
    assert view.stride(2) == 24 and view.data_ptr() % 16 == (lo * view.element_size()) % 16
    got = K.im2col2d(view, K.conv2d_geo(2, H, W, hi - lo, k, s, p))
    assert torch.equal(got.cpu().float(), R.im2col(buf[..., lo:hi], k, s, p))


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("lo,hi", SLICES)
@pytest.mark.parametrize("accumulate", [False, True])
@geo_params
def test_col2im2d_channel_slice(dt, lo, hi, accumulate, H, W, k, s, p):
    C = hi - lo
    g = K.conv2d_geo(2, H, W, C, k, s, p)
    dcols = R.ints((2 * g.Ho * g.Wo, k[0] * k[1] * C), -4, 4, 5)
    want = torch.full((2, H, W, 24), -7.0)                            # the sentinel
    pre = R.ints((2, H, W, C), -2, 2, 6)
    want[..., lo:hi] = R.col2im(dcols, (2, H, W, C), k, s, p) + (pre if accumulate else 0)
    buf = torch.full((2, H, W, 24), -7.0)
    buf[..., lo:hi] = pre
    buf = dev(buf, dt)
    K.col2im2d(dev(dcols, dt), g, buf[..., lo:hi], accumulate=accumulate)
    assert torch.equal(buf.cpu().float(), want)


# ------------------------------------------------------------------ BatchNorm kernels on row views
BN_SHAPES = [(4, 2080), (1, 32), (255, 48), (256, 48), (257, 260), (33001, 8)]
BN_SEED = {33001: 120}      # rows -> seed (default 100): see "ReLU masks" in the docstring


def _bn_inputs(rows, C, dt, seed):
    return dict(x=rn((rows, C), seed, dt, 1.5, 0.3), dy=rn((rows, C), seed + 1, dt),
                gm=uni((C,), seed + 2, 0.5, 1.5), bt=uni((C,), seed + 3, -0.3, 0.3),
                rm=rn((C,), seed + 4, torch.float32, 0.1), rv=uni((C,), seed + 5, 0.5, 1.5),
                dg0=rn((C,), seed + 6, torch.float32), db0=rn((C,), seed + 7, torch.float32))


def _bn_ref(i, relu, training=True):
    x, gm, bt = (i[n].double().requires_grad_(True) for n in ("x", "gm", "bt"))
    y, mean, rstd, rm, rv = R.bn_rows(x, gm, bt, EPS, MOM, i["rm"].double(), i["rv"].double(), training, relu)
    if relu:
        assert_clear_of_zero((x - mean) * rstd * gm + bt, 2e-6)
    y.backward(i["dy"].double())
    return dict(y=y, mean=mean, rstd=rstd, rm=rm, rv=rv, dx=x.grad, dg=gm.grad + i["dg0"].double(),
                db=bt.grad + i["db0"].double())


def _bn_dev(i, dt, relu, pad=0):
    """bn2d_fwd + bn2d_bwd; pad: x, y, dy and dx are columns [pad:pad+C] of buffers 2*pad wider, pre-filled."""
    rows, C = i["x"].shape

    def view(t):
        if not pad:
            return dev(t, dt), None
        full = torch.full((rows, C + 2 * pad), -7.0)
        full[:, pad:pad + C] = t
        full = dev(full, dt)
        return full[:, pad:pad + C], full
    x, xf = view(i["x"])
    dy, dyf = view(i["dy"])
    y, yf = view(torch.zeros(rows, C))
    dx, dxf = view(torch.zeros(rows, C))
    gm, bt, rm, rv, dg, db = (dev(i[n]) for n in ("gm", "bt", "rm", "rv", "dg0", "db0"))
    mean, rstd = K.bn2d_fwd(x, y, gm, bt, EPS, MOM, relu, rm, rv)
    K.bn2d_bwd(dy, y, x, dx, mean, rstd, gm, relu, dg, db)
    out = dict(y=y, mean=mean, rstd=rstd, rm=rm, rv=rv, dx=dx, dg=dg, db=db)
    return out, [f for f in (xf, dyf, yf, dxf) if f is not None]


def _bn_check(tag, dt, got, ref):
    rep = Report(tag)
    rep("y", rel(got["y"], ref["y"]), INHERITED[dt]["y"])
    for q in ("mean", "rstd", "rm", "rv", "dg", "db"):
        rep(q, rel(got[q], ref[q]), 1e-4)
    rep("dx", gmetric(dt)(got["dx"], ref["dx"]), INHERITED[dt]["dx"])
    rep.done()


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("rows,C", BN_SHAPES)
def test_bn2d_rows(dt, relu, rows, C):
    i = _bn_inputs(rows, C, dt, BN_SEED.get(rows, 100))
    got, _ = _bn_dev(i, dt, relu)
    _bn_check(f"bn2d {rows}x{C} {dt} relu={relu}", dt, got, _bn_ref(i, relu))


@pytest.mark.parametrize("dt", DTS)
def test_bn2d_strided_views(dt):
    """x, y, dy and dx are the columns [8:56] of 64-wide buffers (ld = 64 != C = 48); the rest stays untouched."""
    i = _bn_inputs(257, 48, dt, 200)
    got, fulls = _bn_dev(i, dt, True, pad=8)
    assert got["y"].stride(0) == 64 and got["dx"].stride(0) == 64
    _bn_check(f"bn2d strided {dt}", dt, got, _bn_ref(i, True))
    for f in fulls:
        assert (f[:, :8] == -7).all() and (f[:, 56:] == -7).all()


def test_bn2d_two_pass_variance():
    """x = 100 + 0.01 randn: the variance (1e-4) is 1e-8 of E[x^2], so a one-pass E[x^2] - m^2 in fp32 loses it
    entirely (cancellation error ~1e-3, 10x the variance), while the two-pass sum the kernel documents keeps
    ~1e-5 relative.  momentum = 1 and zero running statistics read the mean and the unbiased variance out."""
    rows, C = 1000, 8
    x = rn((rows, C), 300, torch.float32, 0.01, 100.0)
    rm, rv = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
    y = torch.empty(rows, C, device=DEV)
    mean, rstd = K.bn2d_fwd(dev(x), y, torch.ones(C, device=DEV), torch.zeros(C, device=DEV), EPS, 1.0, False, rm, rv)
    xd = x.double()
    var = xd.var(0, unbiased=False)
    relel = lambda a, b: ((a.cpu().double() - b).abs() / b.abs()).max().item()  # noqa: E731
    rep = Report("bn2d conditioning")
    rep("rstd", relel(rstd, (var + EPS).rsqrt()), 1e-3)
    rep("running_var", relel(rv, xd.var(0, unbiased=True)), 1e-3)
    rep("running_mean", relel(rm, xd.mean(0)), 1e-6)
    rep("mean", relel(mean, xd.mean(0)), 1e-6)
    rep.done()


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("rows,C", [(4, 2080), (257, 260)])
def test_bn2d_apply_fixed_statistics(dt, relu, rows, C):
    """The eval-mode forward: y = relu?((x - mean) rstd gamma + beta) with given statistics."""
    i = _bn_inputs(rows, C, dt, 400)
    rstd = (i["rv"] + EPS).rsqrt()
    y = torch.empty(rows, C, device=DEV, dtype=dt)
    K.bn2d_apply(dev(i["x"], dt), y, dev(i["rm"]), dev(rstd), dev(i["gm"]), dev(i["bt"]), relu)
    ref = (i["x"].double() - i["rm"].double()) * rstd.double() * i["gm"].double() + i["bt"].double()
    err = rel(y, F.relu(ref) if relu else ref)
    print(f"bn2d_apply {rows}x{C} {dt}: {err:.3e}")
    assert err <= INHERITED[dt]["y"]


# ------------------------------------------------------------------ pooling
def _pool_x(shape, mode, dt, ties):
    if ties:
        return R.tie_input(shape, 21, dt).float()
    if mode == 1:
        return (R.ints(shape, -32, 32, 22) / 8).to(dt).float()      # window sums exact in fp32
    return rn(shape, 23, dt)


def _one_rounding(got, ref, dt, slack=0.0):
    err = (got.cpu().double() - ref).abs()
    lim = U[dt] * (1 + 2.0 ** -10) * ref.abs() + slack
    print(f"  worst error / allowance: {(err / lim.clamp_min(1e-300)).max().item():.3f}")
    return bool((err <= lim).all())


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("shape", R.POOL_SHAPES)
@pytest.mark.parametrize("mode,k,s,p", R.POOL_GEOS)
@pytest.mark.parametrize("ties", [False, True])
def test_pool2d(dt, shape, mode, k, s, p, ties):
    x = _pool_x(shape, mode, dt, ties)
    N, H, W, C = shape
    g = K.conv2d_geo(N, H, W, C, k, s, p)
    xr = x.double().requires_grad_(True)
    ref = R.pool(xr, k, s, p, mode)
    assert ref.shape == (N, g.Ho, g.Wo, C)
    dy = R.ints(tuple(ref.shape), -4, 4, 24)
    if mode == 0:
        if ties:      # the point of this input: most windows have several equal maxima
            frac = R.tie_fraction(x.double(), k, s)
            print(f"windows with a tied maximum: {frac:.2f}")
            assert frac >= 0.5
        dref = R.maxpool_bwd_first(x.double(), dy.double(), k, s)
    else:
        ref.backward(dy.double())
        dref = xr.grad
    xd = dev(x, dt)
    y = K.pool2d_fwd(xd, g, mode)
    dx = K.pool2d_bwd(xd, dev(dy, dt), g, mode)
    if mode == 0:
        assert torch.equal(y.cpu().double(), ref.detach())
        assert torch.equal(dx.cpu().double(), dref)
    else:
        assert _one_rounding(y, ref.detach(), dt)
        assert _one_rounding(dx, dref, dt, slack=2.0 ** -17)


@pytest.mark.parametrize("dt", DTS)
def test_pool2d_fn_ties_through_autograd(dt):
    """Pool2dFn end to end on a post-ReLU input: the gradient of a tied window goes to its first maximum."""
    shape = R.POOL_SHAPES[0]
    x = R.tie_input(shape, 25, dt).float()
    assert R.tie_fraction(x.double(), 3, 2) >= 0.5
    xi = dev(x, dt).requires_grad_(True)
    y = Fn.Pool2dFn.apply(xi, 3, 2, 0, 0)
    dy = R.ints(tuple(y.shape), -4, 4, 26)
    y.backward(dev(dy, dt))
    assert torch.equal(y.detach().cpu().double(), R.pool(x.double(), 3, 2, 0, 0))
    assert torch.equal(xi.grad.cpu().double(), R.maxpool_bwd_first(x.double(), dy.double(), 3, 2))


@pytest.mark.parametrize("mode", [2, -1])
def test_pool2d_bwd_rejects_unknown_mode(mode):
    x = torch.zeros(1, 3, 3, 8, device=DEV)
    g = K.conv2d_geo(1, 3, 3, 8, 3, 2, 0)
    with pytest.raises(RuntimeError):
        K.pool2d_fwd(x, g, mode)
    with pytest.raises(RuntimeError):
        K.pool2d_bwd(x, torch.zeros(1, 1, 1, 8, device=DEV), g, mode)


# ------------------------------------------------------------------ Conv -> BN -> ReLU at the model's shapes
CONV = {c[0]: c[1:] for c in R.CONV_CASES}
CONV_SEED = {**{name: 1000 for name in CONV}, "5x5": 1010}     # see "ReLU masks" in the docstring


def conv_inputs(name, dt):
    N, H, W, Cin, Cout, k, s, p = CONV[name]
    sd = CONV_SEED[name]
    Ho, Wo = R.out_hw(H, W, k, s, p)
    return dict(x=rn((N, H, W, Cin), sd, dt), w=rn((Cout, Cin, *k), sd + 1, dt, 1 / math.sqrt(Cin * k[0] * k[1])),
                gm=uni((Cout,), sd + 2, 0.5, 1.5), bt=uni((Cout,), sd + 3, -0.3, 0.3),
                rm=rn((Cout,), sd + 4, torch.float32, 0.1), rv=uni((Cout,), sd + 5, 0.5, 1.5),
                dy=rn((N, Ho, Wo, Cout), sd + 6, dt))


def conv_ref(name, i, training=True, z_dtype=None, margin=None):
    """float64 (y, running stats, dx, dW, dgamma, dbeta); z_dtype: see conv2d_ref.conv_bn_relu."""
    _, _, _, _, _, k, s, p = CONV[name]
    x, w, gm, bt = (i[n].double().requires_grad_(True) for n in ("x", "w", "gm", "bt"))
    y, mean, rstd, rm, rv = R.conv_bn_relu(x, w, gm, bt, EPS, MOM, i["rm"].double(), i["rv"].double(), training,
                                           k, s, p, z_dtype=z_dtype)
    if margin:
        assert_clear_of_zero((R.conv(x, w, k, s, p) - mean) * rstd * gm + bt, margin)
    y.backward(i["dy"].double())
    return dict(y=y.detach(), rm=rm, rv=rv, dx=x.grad, dw=w.grad, dg=gm.grad, db=bt.grad)


@functools.lru_cache(maxsize=None)
def _conv_ref_cached(name, dt, training):
    return conv_ref(name, conv_inputs(name, dt), training, margin=2e-5 if dt == torch.float32 else None)


def conv_dev(name, i, dt, training=True):
    _, _, _, _, Cout, k, s, p = CONV[name]
    bn = torch.nn.BatchNorm2d(Cout, eps=EPS, momentum=MOM).to(DEV)
    with torch.no_grad():
        bn.running_mean.copy_(i["rm"])
        bn.running_var.copy_(i["rv"])
    x = dev(i["x"], dt).requires_grad_(True)
    w, gm, bt = (dev(i[n]).requires_grad_(True) for n in ("w", "gm", "bt"))
    y = Fn.ConvBNReLUFn.apply(x, w, gm, bt, bn, k, s, p, training)
    y.backward(dev(i["dy"], dt))
    return dict(y=y.detach(), rm=bn.running_mean, rv=bn.running_var, dx=x.grad, dw=w.grad, dg=gm.grad, db=bt.grad)


def _conv_check(tag, name, dt, got, ref):
    rep = Report(tag)
    for q in ("y", "rm", "rv"):
        rep(q, rel(got[q], ref[q]), bound(name, dt, q))
    for q in ("dx", "dw", "dg", "db"):
        assert got[q].shape == ref[q].shape
        rep(q, gmetric(dt)(got[q], ref[q]), bound(name, dt, q))
    rep.done()


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("name", list(CONV))
def test_conv_bn_relu_model_shapes(dt, name):
    i = conv_inputs(name, dt)
    _conv_check(f"conv_bn_relu {name} {dt}", name, dt, conv_dev(name, i, dt), _conv_ref_cached(name, dt, True))


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("name", ["1x1", "5x5", "stem"])
def test_conv_bn_relu_eval_backward(dt, name):
    """forward(training=False) normalises with the running statistics, which are constants: the backward is
    dz = gamma rstd dy (y > 0) with no batch-mean terms, dgamma / dbeta use the running-stat xhat, and the
    running statistics stay as they were.  Reference: torch's Conv2d -> BatchNorm2d.eval() -> ReLU in float64."""
    _, _, _, Cin, Cout, k, s, p = CONV[name]
    i = conv_inputs(name, dt)
    conv = torch.nn.Conv2d(Cin, Cout, k, stride=s, padding=p, bias=False).double()
    bn = torch.nn.BatchNorm2d(Cout, eps=EPS, momentum=MOM).double().eval()
    with torch.no_grad():
        conv.weight.copy_(i["w"]), bn.weight.copy_(i["gm"]), bn.bias.copy_(i["bt"])
        bn.running_mean.copy_(i["rm"]), bn.running_var.copy_(i["rv"])
    xr = i["x"].double().permute(0, 3, 1, 2).requires_grad_(True)
    pre = bn(conv(xr))
    if dt == torch.float32:
        assert_clear_of_zero(pre, 2e-5)
    yr = F.relu(pre).permute(0, 2, 3, 1)
    yr.backward(i["dy"].double())
    ref = dict(y=yr.detach(), rm=i["rm"], rv=i["rv"], dx=xr.grad.permute(0, 2, 3, 1), dw=conv.weight.grad,
               dg=bn.weight.grad, db=bn.bias.grad)
    got = conv_dev(name, i, dt, training=False)
    assert torch.equal(got["rm"].cpu(), i["rm"]) and torch.equal(got["rv"].cpu(), i["rv"])
    rep = Report(f"conv_bn_relu eval {name} {dt}")
    rep("y", rel(got["y"], ref["y"]), INHERITED[dt]["y"])
    for q in ("dx", "dw", "dg", "db"):
        rep(q, gmetric(dt)(got[q], ref[q]), INHERITED[dt][q])
    rep.done()


# ------------------------------------------------------------------ ResConvFn
RES_SHAPES = {98: (2, 7, 7), 18: (2, 3, 3), 4: (4, 1, 1)}
RES_SEED = {98: 2010, 18: 2000, 4: 2000}


def res_inputs(rows, Cin, C, dt, scale):
    N, H, W = RES_SHAPES[rows]
    sd = RES_SEED[rows]
    return dict(xres=rn((N, H, W, Cin), sd, dt), w=rn((C, Cin, 1, 1), sd + 1, dt, 1 / math.sqrt(Cin)),
                b=rn((C,), sd + 2, dt, 0.1), x=rn((N, H, W, C), sd + 3, dt, scale), dy=rn((N, H, W, C), sd + 4, dt))


def res_ref(i, scale, relu, margin=None):
    xres, w, b, x = (i[n].double().requires_grad_(True) for n in ("xres", "w", "b", "x"))
    C, Cin = w.shape[:2]
    if relu:
        pre = R.res_conv(xres.reshape(-1, Cin), w, b, x.reshape(-1, C), scale, False)
        neg = (pre < 0).double().mean().item()
        assert 0.35 < neg < 0.65, f"{neg:.2f} of the pre-ReLU values are negative: the mask would not matter"
        if margin:
            assert_clear_of_zero(pre, margin)
    y = R.res_conv(xres.reshape(-1, Cin), w, b, x.reshape(-1, C), scale, relu).reshape(x.shape)
    y.backward(i["dy"].double())
    return dict(y=y.detach(), dxres=xres.grad, dx=x.grad, dw=w.grad, db=b.grad)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("scale", [0.17, 1.0])
@pytest.mark.parametrize("rows,Cin,C", [(98, 128, 320), (18, 384, 1088), (4, 448, 2080)])
def test_res_conv(dt, relu, scale, rows, Cin, C):
    """relu?(x + scale (conv1x1(xres) + bias)): the GEMM epilogue act = 3 with alpha.  x is drawn at the branch's
    own magnitude (scale), so about half the pre-ReLU values are negative and the mask decides the gradients."""
    i = res_inputs(rows, Cin, C, dt, scale)
    ref = res_ref(i, scale, relu, margin=1e-5 * scale)
    xres, x = (dev(i[n], dt).requires_grad_(True) for n in ("xres", "x"))
    w, b = (dev(i[n]).requires_grad_(True) for n in ("w", "b"))
    y = Fn.ResConvFn.apply(xres, w, b, x, scale, relu)
    y.backward(dev(i["dy"], dt))
    rep = Report(f"res_conv {rows}x{Cin}->{C} scale={scale} relu={relu} {dt}")
    rep("y", rel(y, ref["y"]), INHERITED[dt]["y"])
    for q, t in (("dxres", xres.grad), ("dx", x.grad), ("dw", w.grad), ("db", b.grad)):
        assert t.shape == ref[q].shape
        rep(q, gmetric(dt)(t, ref[q]), INHERITED[dt]["dx"])
    rep.done()
