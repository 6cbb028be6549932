"""float64 reference of the dfk_gemm contract (include/dfk.h), in plain torch: the oracle of
tests/test_gpu_gemm_exact.py, itself checked against torch on the CPU by tests/test_gemm_ref_host.py.

gemm_ref() takes the arguments of deepfake_amd.kernels._gemm_args (the tensors are base pointers, everything else
is element counts) and returns what the launch must leave in memory.  It imports nothing from the package, runs on
the tensors' own device and reads the operands through torch.as_strided, i.e. by the same address arithmetic as
the kernels' view_off():

  row-major view   V(r, c) = base[z0*bs0 + z1*bs1 + r*ld + c]
  conv view        V(r, c) = X[r*stride + c // cg - pad, c % cg], 0 where that row is outside [0, conv_rows)
  A(i, k) = a_kmajor ? a.V(k, i) : a.V(i, k);   B(k, j) = b_kmajor ? b.V(k, j) : b.V(j, k)

Epilogue, in order: sum; + bias[z1*bias_bs1 + j]; act 1: aux <- v, v = gelu(v) (erf form); act 2: v *= gelu'(aux);
* alpha (0 reads as 1); + residual; act 3: relu; + beta * C_old; one round-to-nearest-even conversion to C's type.
atomic: C += v.  rowsum[i] += sum_k A(i, k).  Dropout is left out (tests/test_gpu_regularize.py).

Batches are applied in z order onto one float64 image of C, so batches that share an output range (atomic weight
gradients summed over clips) add up as on the device.
"""
import math
from types import SimpleNamespace

import torch


def _storage(t):
    """The whole storage of t as a flat tensor (aliasing t)."""
    return torch.as_strided(t, (t.untyped_storage().nbytes() // t.element_size(),), (1,), 0)


def _plain(t, sizes, strides):
    return torch.as_strided(t, tuple(int(s) for s in sizes), tuple(int(s) for s in strides), t.storage_offset())


def _view(t, rows, cols, ld, nz, bs, conv):
    """[nz0, nz1, rows, cols] float64 of the operand view of base tensor t."""
    if not conv or conv[0] <= 0:
        return _plain(t, (nz[0], nz[1], rows, cols), (bs[0], bs[1], ld, 1)).double()
    cg, stride, pad, conv_rows = (int(v) for v in conv)
    r = torch.arange(rows, device=t.device).view(-1, 1)
    c = torch.arange(cols, device=t.device).view(1, -1)
    src = r * stride + c // cg - pad
    ok = (src >= 0) & (src < conv_rows)
    off = (src.clamp(0, conv_rows - 1) * int(ld) + c % cg).reshape(-1)
    flat = _plain(t, (nz[0], nz[1], (conv_rows - 1) * int(ld) + cg), (bs[0], bs[1], 1))
    v = flat[:, :, off].double().view(nz[0], nz[1], rows, cols)
    return v * ok.double()


def gelu(v):
    return 0.5 * v * (1.0 + torch.erf(v / math.sqrt(2.0)))


def dgelu(x):
    return 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def _round_to(v64, dtype):
    if dtype == torch.bfloat16:   # through fp32: values of the exact regime are fp32 numbers, nothing is lost there
        return v64.to(torch.float32).to(dtype)
    return v64.to(dtype)


def gemm_ref(a, a_ld, a_kmajor, b, b_ld, b_kmajor, M, N, K, c, ldc, *, dtype=None, c_f32=False, bias=None,
             residual=None, ldr=0, aux=None, ldaux=0, act=0, beta=0.0, atomic=False, splitk=1, nz=(1, 1),
             a_bs=(0, 0), b_bs=(0, 0), c_bs=(0, 0), r_bs=(0, 0), a_conv=None, b_conv=None, bias_bs1=0, rowsum=None,
             alpha=0.0):
    """Expected memory after dfk_gemm with these arguments.  Returns a namespace of
      c, aux, rowsum : the WHOLE storage behind each of those tensors (flat, in its own dtype; None where the
                       launch writes none), so that equality also says that nothing outside the window changed;
      c64            : c before the rounding, float64;
      v              : [nz0, nz1, M, N] float64, the value of each batch before beta / atomic and the rounding;
      bound          : the largest magnitude any partial sum of the launch can reach, in any order of summation
                       (sum of |terms|, old contents of C / rowsum included) -- the exactness tests assert it.
    dtype and splitk are accepted for the signature's sake: the tensors carry their types, and a split changes
    no value."""
    if a.dtype == torch.bfloat16:
        assert c.dtype == (torch.float32 if (c_f32 or atomic) else a.dtype), "C's tensor type must match c_f32"
    nz = (int(nz[0]), int(nz[1]))
    M, N, K = int(M), int(N), int(K)
    A = _view(a, K, M, a_ld, nz, a_bs, a_conv).transpose(2, 3) if a_kmajor else _view(a, M, K, a_ld, nz, a_bs, a_conv)
    B = _view(b, K, N, b_ld, nz, b_bs, b_conv) if b_kmajor else _view(b, N, K, b_ld, nz, b_bs, b_conv).transpose(2, 3)
    v = A @ B
    bound = A.abs() @ B.abs()
    if bias is not None:
        bz = _plain(bias, (nz[1], N), (bias_bs1, 1)).double().view(1, nz[1], 1, N)
        v = v + bz
        bound = bound + bz.abs()
    aux_out = None
    cs = (c_bs[0], c_bs[1], ldc, 1)
    if act == 1:
        if aux is not None:
            aux_out = _storage(aux).clone()
            win = torch.as_strided(aux_out, (nz[0], nz[1], M, N), (c_bs[0], c_bs[1], int(ldaux), 1),
                                   aux.storage_offset())
            for z0 in range(nz[0]):
                for z1 in range(nz[1]):
                    win[z0, z1] = _round_to(v[z0, z1], aux.dtype)
        v = gelu(v)
    elif act == 2:
        v = v * dgelu(_plain(aux, (nz[0], nz[1], M, N), (c_bs[0], c_bs[1], ldaux, 1)).double())
    if alpha != 0.0:
        v = v * float(alpha)
    if residual is not None:
        r = _plain(residual, (nz[0], nz[1], M, N), (r_bs[0], r_bs[1], ldr, 1)).double()
        v = v + r
        bound = bound + r.abs()
    if act == 3:
        v = v.clamp_min(0.0)
    c64 = _storage(c).to(torch.float64, copy=True)
    win = torch.as_strided(c64, (nz[0], nz[1], M, N), tuple(int(s) for s in cs), c.storage_offset())
    cb = 0.0
    for z0 in range(nz[0]):
        for z1 in range(nz[1]):
            if atomic or beta != 0.0:
                old = win[z0, z1].clone()
                cb = max(cb, float((bound[z0, z1] + old.abs()).max()))
                win[z0, z1] = v[z0, z1] + (1.0 if atomic else float(beta)) * old
            else:
                win[z0, z1] = v[z0, z1]
    out = SimpleNamespace(c=_round_to(c64, c.dtype), c64=c64, aux=aux_out, rowsum=None, v=v,
                          bound=max(float(bound.max()), cb))
    if rowsum is not None:
        assert nz == (1, 1)
        rs = _storage(rowsum).to(torch.float64, copy=True)
        w = torch.as_strided(rs, (M,), (1,), rowsum.storage_offset())
        out.bound = max(out.bound, float((A[0, 0].abs().sum(1) + w.abs()).max()))
        w += A[0, 0].sum(1)
        out.rowsum = _round_to(rs, rowsum.dtype)
    return out
