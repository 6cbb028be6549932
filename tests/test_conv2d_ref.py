"""The float64 oracle of tests/test_gpu_conv2d.py (tests/conv2d_ref.py) checked against torch on the CPU:
im2col + GEMM is F.conv2d, col2im is im2col's exact adjoint, BatchNorm / the residual conv agree with torch's
modules, and torch's CPU max-pool index is the first maximum of a row-major window scan on inputs full of ties."""
import pytest
import torch
import torch.nn.functional as F

import conv2d_ref as R

F64 = torch.float64
GEOS = [(2, H, W, C, k, s, p) for (H, W, k, s, p) in R.IM2COL_GEOS for C in R.C_LIST] + \
       [(N, H, W, Cin, k, s, p) for (_, N, H, W, Cin, _, k, s, p) in R.CONV_CASES]


def _randn(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=F64)


@pytest.mark.parametrize("N,H,W,C,k,s,p", GEOS)
def test_im2col_gemm_is_conv2d(N, H, W, C, k, s, p):
    x, w = _randn((N, H, W, C), 1), _randn((5, C, *k), 2)
    ref = F.conv2d(x.permute(0, 3, 1, 2), w, stride=s, padding=p).permute(0, 2, 3, 1)
    got = R.conv(x, w, k, s, p).reshape(ref.shape)
    assert got.shape[1:3] == R.out_hw(H, W, k, s, p)
    assert (got - ref).abs().max().item() <= 1e-12 * max(1.0, ref.abs().max().item())


@pytest.mark.parametrize("N,H,W,C,k,s,p", GEOS)
def test_col2im_is_the_adjoint(N, H, W, C, k, s, p):
    """<im2col(x), d> == <x, col2im(d)>, exactly: integer data, so both sides are exact sums."""
    x = R.ints((N, H, W, C), -4, 4, 3, F64)
    cols = R.im2col(x, k, s, p)
    d = R.ints(cols.shape, -4, 4, 4, F64)
    dx = R.col2im(d, x.shape, k, s, p)
    assert dx.shape == x.shape
    assert (cols * d).sum().item() == (x * dx).sum().item()
    # and it is what autograd makes of im2col
    xa = x.clone().requires_grad_(True)
    R.im2col(xa, k, s, p).backward(d)
    assert torch.equal(xa.grad, dx)


def test_col2im_integer_sums_are_exact_in_bf16():
    """The bit-exact col2im test's premise: |sums| of dcols in [-4, 4] plus a prefill in [-2, 2] stay below 256,
    where every integer is a bf16 value."""
    worst = 0.0
    for (H, W, k, s, p) in R.IM2COL_GEOS:
        cols = R.im2col(torch.ones(1, H, W, 1, dtype=F64), k, s, p)
        worst = max(worst, R.col2im(torch.full_like(cols, 4.0), (1, H, W, 1), k, s, p).max().item() + 2)
    assert worst < 256
    i = torch.arange(-256, 257, dtype=torch.float32)
    assert torch.equal(i.to(torch.bfloat16).float(), i)


@pytest.mark.parametrize("training", [True, False])
def test_conv_bn_relu_is_torch(training):
    N, H, W, Cin, Cout, k, s, p = 3, 7, 5, 6, 10, (3, 3), (2, 2), (1, 1)
    x, w = _randn((N, H, W, Cin), 5).requires_grad_(True), _randn((Cout, Cin, *k), 6).requires_grad_(True)
    gm, bt = (_randn((Cout,), 7) + 2).requires_grad_(True), _randn((Cout,), 8).requires_grad_(True)
    rm, rv = _randn((Cout,), 9), _randn((Cout,), 10).abs() + 0.5
    y, mean, rstd, rm2, rv2 = R.conv_bn_relu(x, w, gm, bt, 1e-3, 0.1, rm, rv, training, k, s, p)
    bn = torch.nn.BatchNorm2d(Cout, eps=1e-3, momentum=0.1).double().train(training)
    with torch.no_grad():
        bn.weight.copy_(gm), bn.bias.copy_(bt), bn.running_mean.copy_(rm), bn.running_var.copy_(rv)
    xr, wr = x.detach().clone().requires_grad_(True), w.detach().clone().requires_grad_(True)
    z = F.conv2d(xr.permute(0, 3, 1, 2), wr, stride=s, padding=p)
    ref = F.relu(bn(z)).permute(0, 2, 3, 1)
    close = lambda a, b: (a - b).abs().max().item() <= 1e-12 * max(1.0, b.abs().max().item())  # noqa: E731
    assert close(y, ref) and close(rm2, bn.running_mean) and close(rv2, bn.running_var)
    if training:
        assert close(mean, z.mean((0, 2, 3))) and close(rstd, (z.var((0, 2, 3), unbiased=False) + 1e-3).rsqrt())
    else:
        assert torch.equal(rm2, rm) and torch.equal(rv2, rv) and torch.equal(mean, rm)
    dy = _randn(tuple(ref.shape), 11)
    y.backward(dy)
    ref.backward(dy)
    assert close(x.grad, xr.grad) and close(w.grad, wr.grad) and close(gm.grad, bn.weight.grad)
    assert close(bt.grad, bn.bias.grad)


def test_single_row_batchnorm_keeps_the_biased_variance():
    z = _randn((1, 4), 12)
    y, mean, rstd, rm, rv = R.bn_rows(z, torch.ones(4, dtype=F64), torch.zeros(4, dtype=F64), 1e-3, 1.0,
                                      torch.zeros(4, dtype=F64), torch.ones(4, dtype=F64), True, relu=False)
    assert torch.equal(mean, z[0]) and torch.equal(rm, z[0]) and torch.equal(rv, torch.zeros(4, dtype=F64))
    assert torch.equal(y, torch.zeros_like(y))


@pytest.mark.parametrize("relu", [True, False])
def test_res_conv_is_torch(relu):
    xres, x = _randn((2, 3, 3, 12), 13), _randn((2, 3, 3, 20), 14)
    w, b = _randn((20, 12, 1, 1), 15), _randn((20,), 16)
    ref = x.permute(0, 3, 1, 2) + 0.17 * F.conv2d(xres.permute(0, 3, 1, 2), w, b)
    ref = (F.relu(ref) if relu else ref).permute(0, 2, 3, 1)
    got = R.res_conv(xres.reshape(-1, 12), w, b, x.reshape(-1, 20), 0.17, relu).reshape(ref.shape)
    assert (got - ref).abs().max().item() <= 1e-12


def test_stored_as_rounds_value_and_gradient():
    x = _randn((64,), 17).requires_grad_(True)
    y = R.stored_as(x, torch.bfloat16)
    assert torch.equal(y.detach(), x.detach().to(torch.bfloat16).double())
    g = _randn((64,), 18)
    y.backward(g)
    assert torch.equal(x.grad, g.to(torch.bfloat16).double())


@pytest.mark.parametrize("shape", R.POOL_SHAPES)
@pytest.mark.parametrize("s", [2, 1])
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_torch_max_pool_index_is_the_first_maximum(shape, s, dt):
    """On the tie inputs of the GPU pooling test, autograd through torch's CPU max pool (NCHW and channels-last
    memory) routes each window's gradient to its first maximum: the definition maxpool_bwd_first spells out."""
    x = R.tie_input(shape, 21, dt).double()
    assert R.tie_fraction(x, 3, s) >= 0.5
    Ho, Wo = R.out_hw(shape[1], shape[2], (3, 3), (s, s), (0, 0))
    dy = R.ints((shape[0], Ho, Wo, shape[3]), -4, 4, 22, F64)
    want = R.maxpool_bwd_first(x, dy, 3, s)
    assert want.sum().item() == dy.sum().item()                 # every window's gradient lands exactly once
    for fmt in (torch.contiguous_format, torch.channels_last):
        xc = x.permute(0, 3, 1, 2).contiguous(memory_format=fmt).requires_grad_(True)
        F.max_pool2d(xc, 3, s, 0).backward(dy.permute(0, 3, 1, 2))
        assert torch.equal(xc.grad.permute(0, 2, 3, 1), want)
    xa = x.clone().requires_grad_(True)
    R.pool(xa, 3, s, 0, 0).backward(dy)
    assert torch.equal(xa.grad, want)


def test_avg_pool_excludes_padding():
    x = torch.ones(1, 3, 3, 2, dtype=F64)
    assert torch.equal(R.pool(x, 3, 1, 1, 1), x)
