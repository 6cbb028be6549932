"""CPU: the float64 dfk_gemm reference of tests/test_gpu_gemm_exact.py (tests/gemm_ref.py) pinned against torch in
float64: F.linear forward / dX / dW, the four operand layouts, F.conv1d through the argument mappings that
functional._conv1d_gemm_fwd/_bwd and _posconv_gemm_fwd/_bwd use (copied here argument for argument), batch strides,
bias_bs1, alpha, beta, act 3 and leading dimensions wider than the extents.  float64 against float64: 1e-10."""
import torch
import torch.nn.functional as F

from gemm_ref import dgelu, gelu, gemm_ref

TOL = 1e-10


def rnd(*shape, seed):
    return torch.randn(*shape, dtype=torch.float64, generator=torch.Generator().manual_seed(seed))


def close(got, want):
    err = (got - want).abs().max().item()
    assert got.shape == want.shape and err < TOL, err


def test_linear_forward_dx_dw():
    M, N, Kd = 13, 7, 11
    x, w, b = rnd(M, Kd, seed=1).requires_grad_(), rnd(N, Kd, seed=2).requires_grad_(), rnd(N, seed=3)
    dy = rnd(M, N, seed=4)
    y = F.linear(x, w, b)
    y.backward(dy)
    # kernels.linear / linear_dx / linear_dw
    r = gemm_ref(x.detach(), Kd, False, w.detach(), Kd, False, M, N, Kd, torch.zeros(M, N, dtype=torch.float64), N,
                 bias=b)
    close(r.c.view(M, N), y.detach())
    r = gemm_ref(dy, N, False, w.detach(), Kd, True, M, Kd, N, torch.zeros(M, Kd, dtype=torch.float64), Kd)
    close(r.c.view(M, Kd), x.grad)
    dw0, db0 = rnd(N, Kd, seed=5), rnd(N, seed=6)
    r = gemm_ref(dy, N, True, x.detach(), Kd, True, N, Kd, M, dw0.clone(), Kd, c_f32=False, beta=1.0,
                 rowsum=db0.clone())
    close(r.c.view(N, Kd), dw0 + w.grad)
    close(r.rowsum, db0 + dy.sum(0))
    r = gemm_ref(dy, N, True, x.detach(), Kd, True, N, Kd, M, dw0.clone(), Kd, atomic=True, splitk=3)
    close(r.c.view(N, Kd), dw0 + w.grad)


def test_four_layouts_with_wide_ld_and_offset_base():
    M, N, Kd = 9, 6, 10
    for ak in (False, True):
        for bk in (False, True):
            ar, ac = (Kd, M) if ak else (M, Kd)
            br, bc = (Kd, N) if bk else (N, Kd)
            abuf, bbuf = rnd(ar + 1, ac + 5, seed=7), rnd(br + 2, bc + 3, seed=8)
            a, b = abuf[1:, 2:], bbuf[2:, 1:]           # base pointers inside wider buffers
            A = a[:ar, :ac].t() if ak else a[:ar, :ac]
            B = b[:br, :bc] if bk else b[:br, :bc].t()
            cbuf = rnd(M + 2, N + 4, seed=9)
            r = gemm_ref(a, ac + 5, ak, b, bc + 3, bk, M, N, Kd, cbuf[1:, 3:], N + 4)
            want = cbuf.clone()
            want[1:M + 1, 3:N + 3] = A @ B
            close(r.c.view_as(cbuf), want)              # the window, and nothing outside it
            assert torch.equal(r.c.view_as(cbuf)[0], cbuf[0]) and torch.equal(r.c.view_as(cbuf)[:, :3], cbuf[:, :3])


def test_epilogue_order_batches_bias_bs1():
    nz0, nz1, M, N, Kd = 2, 3, 5, 4, 6
    a, b = rnd(nz0, nz1, M, Kd + 2, seed=10), rnd(nz1, N, Kd, seed=11)
    bias, res, c0 = rnd(nz1, N + 1, seed=12), rnd(nz0, nz1, M, N, seed=13), rnd(nz0, M, nz1 * N, seed=14)
    prod = torch.einsum("zgmk,gnk->zgmn", a[..., :Kd], b) + bias[:, :N].view(1, nz1, 1, N)
    kw = dict(nz=(nz0, nz1), a_bs=(nz1 * M * (Kd + 2), M * (Kd + 2)), b_bs=(0, N * Kd), c_bs=(M * nz1 * N, N),
              r_bs=(nz1 * M * N, M * N), bias=bias, bias_bs1=N + 1, residual=res, ldr=N)
    # groups side by side in C's rows, as the grouped conv writes its channels
    def grouped(v):
        return v.permute(0, 2, 1, 3).reshape(nz0, M, nz1 * N)
    r = gemm_ref(a, Kd + 2, False, b, Kd, False, M, N, Kd, c0.clone(), nz1 * N, alpha=0.5, act=3, beta=0.25, **kw)
    close(r.c.view_as(c0), grouped(torch.relu(0.5 * prod + res)) + 0.25 * c0)
    aux = torch.zeros_like(c0)
    r = gemm_ref(a, Kd + 2, False, b, Kd, False, M, N, Kd, c0.clone(), nz1 * N, act=1, aux=aux, ldaux=nz1 * N, **kw)
    close(r.aux.view_as(c0), grouped(prod))
    close(r.c.view_as(c0), grouped(F.gelu(prod) + res))
    pre = rnd(nz0, M, nz1 * N, seed=15)
    r = gemm_ref(a, Kd + 2, False, b, Kd, False, M, N, Kd, c0.clone(), nz1 * N, act=2, aux=pre, ldaux=nz1 * N, **kw)
    p = pre.clone().requires_grad_()
    F.gelu(p).sum().backward()
    close(r.c.view_as(c0), grouped(prod) * p.grad + grouped(res))
    close(gelu(pre), F.gelu(pre))
    close(dgelu(pre), p.grad)


def test_conv1d_stride2_kernel3_mapping():
    """functional._conv1d_gemm_fwd / _conv1d_gemm_bwd: forward, split-K dW summed over the clips, per-tap dX."""
    B, Tin, Cin, Cout, k, stride = 2, 11, 4, 5, 3, 2
    Tout = (Tin - k) // stride + 1
    x = rnd(B, Tin, Cin, seed=20).requires_grad_()
    weight, bias = rnd(Cout, Cin, k, seed=21).requires_grad_(), rnd(Cout, seed=22)
    y = F.conv1d(x.transpose(1, 2), weight, bias, stride=stride).transpose(1, 2)
    dpre = rnd(B, Tout, Cout, seed=23)
    y.backward(dpre)
    xd = x.detach()
    w2 = weight.detach().permute(0, 2, 1).reshape(Cout, k * Cin).contiguous()
    out = torch.zeros(B, Tout, Cout, dtype=torch.float64)
    r = gemm_ref(xd, Cin, False, w2, k * Cin, False, Tout, Cout, k * Cin, out, Cout, bias=bias, nz=(B, 1),
                 a_bs=(Tin * Cin, 0), c_bs=(Tout * Cout, 0), a_conv=(Cin, stride, 0, Tin))
    close(r.c.view_as(out), y.detach())
    dw2 = torch.zeros(Cout, k * Cin, dtype=torch.float64)
    r = gemm_ref(dpre, Cout, True, xd, Cin, True, Cout, k * Cin, Tout, dw2, k * Cin, c_f32=False, atomic=True,
                 splitk=2, nz=(B, 1), a_bs=(Tout * Cout, 0), b_bs=(Tin * Cin, 0), b_conv=(Cin, stride, 0, Tin))
    close(r.c.view(Cout, k, Cin).permute(0, 2, 1), weight.grad)
    dx = torch.zeros(B, Tin, Cin, dtype=torch.float64)
    for kk in range(k):
        r = gemm_ref(dpre, Cout, False, w2[:, kk * Cin:], k * Cin, True, Tout, Cin, Cout, dx[:, kk:], stride * Cin,
                     beta=1.0, nz=(B, 1), a_bs=(Tout * Cout, 0), c_bs=(Tin * Cin, 0))
        dx = r.c.view(B, Tin, Cin)
    close(dx, x.grad)


def test_grouped_conv_padding_mapping():
    """functional._posconv_gemm_fwd / _posconv_gemm_bwd: grouped conv, pad k//2, last frame dropped, + GELU +
    residual; the weight and input gradients of the conv from autograd."""
    B, T, G, Cg, k = 2, 9, 2, 3, 4
    C = G * Cg
    x = rnd(B, T, C, seed=30).requires_grad_()
    weight, bias = rnd(C, Cg, k, seed=31).requires_grad_(), rnd(C, seed=32)
    pre = F.conv1d(x.transpose(1, 2), weight, bias, padding=k // 2, groups=G)[:, :, :-1].transpose(1, 2)
    dpre = rnd(B, T, C, seed=33)
    pre.backward(dpre)
    xd = x.detach()
    w2 = weight.detach().permute(0, 2, 1).reshape(C, k * Cg).contiguous()
    y, aux = torch.zeros(B, T, C, dtype=torch.float64), torch.zeros(B, T, C, dtype=torch.float64)
    r = gemm_ref(xd, C, False, w2, k * Cg, False, T, Cg, k * Cg, y, C, bias=bias, bias_bs1=Cg, act=1, aux=aux,
                 ldaux=C, residual=xd, ldr=C, nz=(B, G), a_bs=(T * C, Cg), b_bs=(0, Cg * k * Cg), c_bs=(T * C, Cg),
                 r_bs=(T * C, Cg), a_conv=(Cg, 1, k // 2, T))
    close(r.aux.view_as(aux), pre.detach())
    close(r.c.view_as(y), xd + F.gelu(pre.detach()))
    dw2 = torch.zeros(C, k * Cg, dtype=torch.float64)
    r = gemm_ref(dpre, C, True, xd, C, True, Cg, k * Cg, T, dw2, k * Cg, c_f32=False, atomic=True, splitk=2,
                 nz=(B, G), a_bs=(T * C, Cg), b_bs=(T * C, Cg), c_bs=(0, Cg * k * Cg), b_conv=(Cg, 1, k // 2, T))
    close(r.c.view(C, k, Cg).permute(0, 2, 1), weight.grad)
    w3 = weight.detach().view(G, Cg, Cg, k).flip(3).permute(0, 2, 3, 1).reshape(C, k * Cg).contiguous()
    dy = rnd(B, T, C, seed=34)
    r = gemm_ref(dpre, C, False, w3, k * Cg, False, T, Cg, k * Cg, dy.clone(), C, beta=1.0, nz=(B, G),
                 a_bs=(T * C, Cg), b_bs=(0, Cg * k * Cg), c_bs=(T * C, Cg), a_conv=(Cg, 1, k // 2 - 1, T))
    close(r.c.view_as(dy), dy + x.grad)


def test_bf16_output_is_one_rne_rounding_and_bound():
    """bf16 tensors: the result is the float64 value rounded once to nearest even (257 -> 256, 259 -> 260), and
    bound is the sum of magnitudes."""
    a = torch.tensor([[2.0, 2.0, 1.0]], dtype=torch.bfloat16).repeat(1, 43)          # 129 elements
    b = torch.tensor([[2.0, -1.0, 1.0]], dtype=torch.bfloat16).repeat(1, 43)
    c = torch.tensor([[-2.0]], dtype=torch.bfloat16)
    r = gemm_ref(a, 129, False, b, 129, False, 1, 1, 129, c, 1, beta=1.0)
    assert r.v.item() == 43 * 3 and r.bound == 43 * 7 + 2
    assert r.c.item() == 127.0 and r.c.dtype == torch.bfloat16
    r = gemm_ref(a, 129, False, a, 129, False, 1, 1, 129, c, 1, residual=c, ldr=1)     # 43*9 - 2 = 385 -> 384
    assert r.v.item() == 385 and r.c.item() == 384.0
    r = gemm_ref(a, 129, False, a, 129, False, 1, 1, 129, c, 1, beta=-1.0)             # 387 + 2 = 389 -> 388 ... 390
    assert r.c.item() == 388.0   # 389 lies between 388 and 390: ties to the even mantissa
