"""Test helper (not a test): float64 CPU reference of the 2-D convolution family of csrc/conv2d.hip and the
autograd functions built on it (ConvBNReLUFn, ResConvFn, Pool2dFn), on channels-last [N, H, W, C] activations.

Everything is plain torch, differentiable, so backward references come from autograd.  im2col / col2im are
F.unfold / F.fold permuted to the project's column order, tap-major and channel-fastest:

    cols[(n*Ho + oh)*Wo + ow, (ky*kw + kx)*C + c] = x[n, oh*sh - ph + ky, ow*sw - pw + kx, c]   (0 outside)

tests/test_conv2d_ref.py checks these against F.conv2d, the adjoint identity and torch's max-pool index on the
CPU, so the GPU tests' oracle is itself tested without a GPU.
"""
import torch
import torch.nn.functional as F

# (H, W, k, s, p): what the kernels are called with directly (N = 2, C in C_LIST) ...
IM2COL_GEOS = [
    (7, 5, (3, 3), (2, 2), (0, 0)),
    (7, 5, (3, 3), (1, 1), (1, 1)),
    (7, 5, (5, 5), (1, 1), (2, 2)),
    (7, 5, (1, 7), (1, 1), (0, 3)),
    (7, 5, (7, 1), (1, 1), (3, 0)),
    (1, 1, (1, 3), (1, 1), (0, 1)),
    (1, 1, (3, 1), (1, 1), (1, 0)),
    (3, 3, (3, 3), (2, 2), (0, 0)),
]
C_LIST = [3, 8, 20, 40]

# ... and (name, N, H, W, Cin, Cout, k, s, p): the Conv -> BN -> ReLU blocks of InceptionResV2.py at the sizes a
# 75 x 75 frame gives them
CONV_CASES = [
    ("stem", 2, 15, 13, 3, 32, (3, 3), (2, 2), (0, 0)),
    ("1x1", 2, 5, 5, 80, 192, (1, 1), (1, 1), (0, 0)),
    ("1x7", 2, 3, 3, 128, 160, (1, 7), (1, 1), (0, 3)),
    ("7x1", 2, 3, 3, 160, 192, (7, 1), (1, 1), (3, 0)),
    ("3x3s2-to-1x1", 2, 3, 3, 256, 288, (3, 3), (2, 2), (0, 0)),
    ("1x3-on-1x1", 4, 1, 1, 192, 224, (1, 3), (1, 1), (0, 1)),
    ("1x1-2080", 4, 1, 1, 2080, 1536, (1, 1), (1, 1), (0, 0)),
    ("5x5", 2, 7, 7, 48, 64, (5, 5), (1, 1), (2, 2)),
]

POOL_SHAPES = [(2, 7, 5, 20), (2, 3, 3, 8), (1, 4, 6, 264)]
# (mode, k, s, p): the model's max pool, the same with overlapping windows, the model's average pool
POOL_GEOS = [(0, 3, 2, 0), (0, 3, 1, 0), (1, 3, 1, 1)]


def out_hw(H, W, k, s, p):
    return (H + 2 * p[0] - k[0]) // s[0] + 1, (W + 2 * p[1] - k[1]) // s[1] + 1


def im2col(x, k, s, p):
    """x [N, H, W, C] -> [N*Ho*Wo, kh*kw*C] in the project's column order."""
    N, H, W, C = x.shape
    u = F.unfold(x.permute(0, 3, 1, 2), k, padding=p, stride=s)          # [N, C*kh*kw (channel-major), L]
    L = u.shape[-1]
    return u.reshape(N, C, k[0] * k[1], L).permute(0, 3, 2, 1).reshape(N * L, k[0] * k[1] * C)


def col2im(dcols, shape, k, s, p):
    """The adjoint of im2col: dcols [N*Ho*Wo, kh*kw*C] -> dx of `shape` = [N, H, W, C]."""
    N, H, W, C = shape
    L = dcols.shape[0] // N
    d = dcols.reshape(N, L, k[0] * k[1], C).permute(0, 3, 2, 1).reshape(N, C * k[0] * k[1], L)
    return F.fold(d, (H, W), k, padding=p, stride=s).permute(0, 2, 3, 1)


def weight2d(w):
    """[Cout, Cin, kh, kw] -> [Cout, kh*kw*Cin], the layout functional._conv_weight2d gives the GEMM."""
    return w.permute(0, 2, 3, 1).reshape(w.shape[0], -1)


def conv(x, w, k, s, p):
    """Conv2d(bias=False) as rows: [N*Ho*Wo, Cout]."""
    return im2col(x, k, s, p) @ weight2d(w).t()


def bn_rows(z, gamma, beta, eps, momentum, running_mean, running_var, training, relu=True):
    """BatchNorm over the rows of z [rows, C] (+ReLU).  Returns (y, mean, rstd, new running mean, new running
    var); training: batch statistics, running variance from the unbiased one (the biased one for a single row, as
    the kernel documents); eval: the running statistics, returned unchanged."""
    if training:
        n = z.shape[0]
        mean = z.mean(0)
        var = ((z - mean) ** 2).mean(0)
        with torch.no_grad():
            rm = (1 - momentum) * running_mean + momentum * mean
            rv = (1 - momentum) * running_var + momentum * var * (n / (n - 1) if n > 1 else 1.0)
    else:
        mean, var, rm, rv = running_mean, running_var, running_mean.clone(), running_var.clone()
    rstd = (var + eps).rsqrt()
    y = (z - mean) * rstd * gamma + beta
    return (F.relu(y) if relu else y), mean.detach(), rstd.detach(), rm, rv


class _RoundBoth(torch.autograd.Function):
    """Round to `dt` and back, forward and backward: a tensor (and its gradient) stored in a narrower type."""

    @staticmethod
    def forward(ctx, x, dt):
        ctx.dt = dt
        return x.to(dt).to(x.dtype)

    @staticmethod
    def backward(ctx, g):
        return g.to(ctx.dt).to(g.dtype), None


def stored_as(x, dt):
    return x if dt is None or dt == x.dtype else _RoundBoth.apply(x, dt)


def conv_bn_relu(x, w, gamma, beta, eps, momentum, running_mean, running_var, training, k, s, p, z_dtype=None):
    """Conv2d(bias=False) -> BatchNorm2d -> ReLU.  Returns (y [N, Ho, Wo, Cout], mean, rstd, running mean,
    running var).  z_dtype: round the conv output (and its gradient) to that type, as ConvBNReLUFn stores them."""
    N, H, W, _ = x.shape
    Ho, Wo = out_hw(H, W, k, s, p)
    z = stored_as(conv(x, w, k, s, p), z_dtype)
    y, mean, rstd, rm, rv = bn_rows(z, gamma, beta, eps, momentum, running_mean, running_var, training)
    return y.reshape(N, Ho, Wo, -1), mean, rstd, rm, rv


def res_conv(xres, w, bias, x, scale, relu):
    """relu?(x + scale * (conv1x1(xres) + bias)); w [C, Cin, 1, 1]."""
    y = x + scale * (xres @ w.reshape(w.shape[0], -1).t() + bias)
    return F.relu(y) if relu else y


def pool(x, k, s, p, mode):
    """mode 0: MaxPool2d(k, s, p); mode 1: AvgPool2d(k, s, p, count_include_pad=False)."""
    xc = x.permute(0, 3, 1, 2)
    y = F.max_pool2d(xc, k, s, p) if mode == 0 else F.avg_pool2d(xc, k, s, p, count_include_pad=False)
    return y.permute(0, 2, 3, 1)


def _windows(x, k, s):
    """Unpadded k x k windows: [N, C, k*k (row-major scan), L]."""
    N, H, W, C = x.shape
    return F.unfold(x.permute(0, 3, 1, 2), k, stride=s).reshape(N, C, k * k, -1)


def tie_fraction(x, k, s):
    """The share of max-pool windows whose maximum occurs more than once."""
    w = _windows(x, k, s)
    return ((w == w.amax(2, keepdim=True)).sum(2) > 1).double().mean().item()


def maxpool_bwd_first(x, dy, k, s):
    """Max-pool backward by definition: each window's dy goes to its first maximum in a row-major scan."""
    N, H, W, C = x.shape
    w = _windows(x, k, s)
    eq = w == w.amax(2, keepdim=True)
    first = eq & (eq.cumsum(2) == 1)
    d = first.to(dy.dtype) * dy.permute(0, 3, 1, 2).reshape(N, C, 1, -1)
    return F.fold(d.reshape(N, C * k * k, -1), (H, W), k, stride=s).permute(0, 2, 3, 1)


def tie_input(shape, seed, dtype=torch.float64):
    """relu of small integers: what a max pool after a ReLU sees, most windows with several equal maxima."""
    g = torch.Generator().manual_seed(seed)
    return F.relu(torch.randint(-2, 3, shape, generator=g).float()).to(dtype)


def ints(shape, lo, hi, seed, dtype=torch.float32):
    """Integers in [lo, hi] as `dtype`: sums of a few of them are exact in fp32 and bf16."""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(lo, hi + 1, shape, generator=g).to(dtype)
