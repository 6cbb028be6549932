"""GPU: wav2vec2 attention past the resident forward's limit (4 Np hd > 160 KiB of LDS: 640 frames at hd 64, 1280 at
hd 32).  The streaming forward v3s (K / V through LDS in chunks of KC key blocks) gives the bits of the resident v3
wherever both run (dfk_wattn_fwd_policy version 7 selects v3s below the limit), and past the limit the forward and the
chunked backward agree with a torch fp32 masked softmax on the same bf16 inputs, with and without per-clip lengths and
attention dropout; the paths that cannot stream (bias tables, explicit masks, fp32) stay errors.

Bars are those of tests/test_gpu_w2v_padded.py for bf16: op forward 2e-2, op gradients 3e-2, model forward 5e-2, model
gradients 1e-1 (max|a-b| / max|b|)."""
import types

import pytest
import torch

import golden_cases as GC
import make_w2v_ln_fixture as LN
from oracle.fill import named_fill_, randn

pytestmark = pytest.mark.gpu
if torch.cuda.is_available():
    from deepfake_amd import functional as Fn
    from deepfake_amd import kernels as K
    from deepfake_amd import rng
    from deepfake_amd.models import set_compute_dtype
    from deepfake_amd.models import wav2vec2 as W
    from deepfake_amd.models.audioTransformer import Audio2D
    from deepfake_amd.trainer import normalize_wave

DEV = "cuda"
BF16 = torch.bfloat16
NAN = float("nan")
KC = 4            # wattn.hip kF3sKC: key blocks of 32 per staged chunk of the streaming forward
CHUNK = 32 * KC   # keys per chunk
OP_FWD, OP_BWD = 2e-2, 3e-2
MODEL_FWD, MODEL_BWD = 5e-2, 1e-1


def rel(a, b):
    return ((a.float() - b.float()).abs().max() / b.float().abs().max().clamp_min(1e-12)).item()


def i32(v):
    return torch.tensor(v, dtype=torch.int32, device=DEV)


def i64(v):
    return torch.tensor(v, dtype=torch.int64, device=DEV)


def _geo(B, T, heads, hd):
    return ((B, 1, 1, T), (1, 1, T), (1, 1, T), (0, 0, 0), heads, hd, hd ** -0.5)


def _attn_inputs(B, T, heads, hd, dt, seed):
    C = heads * hd
    g = torch.Generator(device=DEV).manual_seed(seed)
    qkv = (torch.randn(B * T, 3 * C, device=DEV, generator=g) * 0.5).to(dt)
    do = torch.randn(B * T, C, device=DEV, generator=g).to(dt)
    return qkv, do


def _attn_ref(qkv, do, B, T, heads, hd, klen, z=None):
    """fp32 softmax with -inf on the keys >= kn, restricted to the rows < kn (everything else zero): out, dqkv.
    z [B, heads, T, T]: a dropout mask on the probabilities (keep / (1 - p) or 0)."""
    C = heads * hd
    x = qkv.float().view(B, T, 3, heads, hd).requires_grad_(True)
    out = torch.zeros(B, T, heads, hd, device=DEV)
    for b, kn in enumerate(klen):
        q, k, v = (x[b, :kn, i].transpose(0, 1) for i in range(3))        # [heads, kn, hd]
        s = torch.softmax((q * hd ** -0.5) @ k.transpose(-1, -2), dim=-1)
        if z is not None:
            s = s * z[b, :, :kn, :kn]
        out[b, :kn] = (s @ v).transpose(0, 1)
    out = out.reshape(B * T, C)
    (gx,) = torch.autograd.grad(out, x, do.float())
    return out.detach(), gx.reshape(B * T, 3 * C)


def _raw(qkv, do, B, T, heads, hd, klen, drop=None):
    """out, lse, dq, dk, dv through the kernel wrappers (the lse is not an autograd output)."""
    C = heads * hd
    dims, win, shift = (B, 1, 1, T), (1, 1, T), (0, 0, 0)
    out, lse = K.wattn_fwd(qkv, qkv[:, C:], qkv[:, 2 * C:], qkv.stride(0), dims, win, win, shift, heads, hd, hd ** -0.5,
                           drop=drop, klen=klen)
    dqkv = torch.full_like(qkv, NAN)
    K.wattn_bwd((qkv, qkv[:, C:], qkv[:, 2 * C:], out, lse, qkv.stride(0), dims, win, win, shift, heads, hd,
                 hd ** -0.5, None, None), do, dqkv, dqkv[:, C:], dqkv[:, 2 * C:], qkv.stride(0), drop=drop, klen=klen)
    return out, lse, dqkv


def _rows_past(t, B, T, klen):
    """The rows >= kn of every clip of a [B*T, *] tensor, concatenated."""
    t = t.view(B, T, -1)
    return torch.cat([t[b, kn:].reshape(-1) for b, kn in enumerate(klen)])


def _check_against_torch(T, hd, klen, B, heads, seed, tag):
    C = heads * hd
    qkv, do = _attn_inputs(B, T, heads, hd, BF16, seed)
    kl = None if klen is None else i32(klen)
    out, lse, dqkv = _raw(qkv, do, B, T, heads, hd, kl)
    lens = [T] * B if klen is None else list(klen)
    ref, dref = _attn_ref(qkv, do, B, T, heads, hd, lens)
    errs = [rel(out, ref)] + [rel(dqkv[:, i * C:(i + 1) * C], dref[:, i * C:(i + 1) * C]) for i in range(3)]
    print(f"{tag} T={T} hd={hd} klen={klen}: fwd {errs[0]:.3e} dq {errs[1]:.3e} dk {errs[2]:.3e} dv {errs[3]:.3e}")
    Np = -(-T // 32) * 32
    assert torch.isfinite(out).all() and torch.isfinite(dqkv).all() and torch.isfinite(lse.view(-1, Np)[:, :T]).all()
    assert errs[0] < OP_FWD, errs
    assert max(errs[1:]) < OP_BWD, errs
    for name, t in (("out", out), ("dqkv", dqkv)):
        past = _rows_past(t, B, T, lens)
        assert past.numel() == 0 or (past == 0).all(), name


# ---------------------------------------------------------------- 1. the bits of the resident kernel
def _klen_sets(T):
    return [None, (T, T, T), (T, -(-T // 2) + 1, 1)]


@pytest.mark.parametrize("dropout", [False, True])
@pytest.mark.parametrize("hd", [32, 64])
@pytest.mark.parametrize("T", [33, 199, CHUNK, CHUNK + 1, 2 * CHUNK - 1, 499])
def test_streaming_forward_gives_the_resident_bits(T, hd, dropout):
    """out and lse[:, :T] of v3s (policy 7) are torch.equal to v3's (the default policy), and so is the backward run
    from either forward's outputs: without klen, with klen = T and with ragged klen, with and without dropout."""
    B, heads = 3, 2
    Np = -(-T // 32) * 32
    qkv, do = _attn_inputs(B, T, heads, hd, BF16, 21)
    try:
        for klen in _klen_sets(T):
            kl = None if klen is None else i32(klen)
            with rng.pinned(9, first_site=6200):
                drop = rng.Drop(0.1).spec() if dropout else None
                K.wattn_fwd_policy(6, -1)
                res = _raw(qkv, do, B, T, heads, hd, kl, drop)
                K.wattn_fwd_policy(7, -1)
                stream = _raw(qkv, do, B, T, heads, hd, kl, drop)
            for name, a, b in zip(("out", "lse", "dqkv"), res, stream):
                if name == "lse":   # the columns past T are never written
                    a, b = a.view(-1, Np)[:, :T], b.view(-1, Np)[:, :T]
                assert torch.isfinite(a).all() and torch.equal(a, b), (name, klen)
    finally:
        K.wattn_fwd_policy(6, -1)


# ---------------------------------------------------------------- 2. past the old limit, against torch
# ragged sets: kn inside the first chunk and exactly on a chunk boundary; one past that boundary and 1
LONG_CASES = [(641, 64, (97, 4 * CHUNK), (4 * CHUNK + 1, 1)),
              (700, 64, (97, 5 * CHUNK), (5 * CHUNK + 1, 1)),
              (1300, 32, (97, 10 * CHUNK), (10 * CHUNK + 1, 1))]


@pytest.mark.parametrize("which", ["none", "ragged_a", "ragged_b"])
@pytest.mark.parametrize("T,hd,ka,kb", LONG_CASES)
def test_long_clips_against_torch(T, hd, ka, kb, which):
    """Np 672 / 704 at hd 64 and 1312 at hd 32 (4 Np hd > 160 KiB: the resident forward cannot run them): forward and
    dq / dk / dv at the op bars, rows >= kn exactly zero, everything finite."""
    klen = {"none": None, "ragged_a": ka, "ragged_b": kb}[which]
    _check_against_torch(T, hd, klen, 2, 2, 22, "long")


# ---------------------------------------------------------------- 3. the padding is never read
def test_long_attention_never_reads_the_padding():
    """T = 700, hd 64: NaN in the rows >= kn of q / k / v and of dout — the rows < kn are bit-equal to those with
    zeros there, and everything is finite."""
    B, T, heads, hd = 3, 700, 2, 64
    klen = (5 * CHUNK + 1, 3 * CHUNK, 1)
    qkv, do = _attn_inputs(B, T, heads, hd, BF16, 23)
    keep = (torch.arange(T, device=DEV)[None, :] < i32(klen)[:, None]).reshape(B * T, 1)
    outs = []
    for fill in (0.0, NAN):
        q = torch.where(keep, qkv, torch.full_like(qkv, fill))
        d = torch.where(keep, do, torch.full_like(do, fill))
        out, _, dqkv = _raw(q, d, B, T, heads, hd, i32(klen))
        outs.append((out, dqkv))
    for name, a, b in zip(("out", "dqkv"), outs[0], outs[1]):
        assert torch.isfinite(b).all(), name
        assert torch.equal(a, b), name


# ---------------------------------------------------------------- 4. dropout past the limit
@pytest.mark.parametrize("T,hd", [(700, 64), (1300, 32)])
def test_long_attention_dropout(T, hd):
    """p = 0.1 past the limit: the forward against a torch reference that applies the kernel's own mask (row
    ((b heads + h) Np + q), column = the global key index, as tests/test_gpu_regularize.py builds it), and the
    backward within the gradient bar of that reference — forward and backward regenerate one mask across chunks."""
    B, heads = 2, 2
    C = heads * hd
    Np = -(-T // 32) * 32
    qkv, do = _attn_inputs(B, T, heads, hd, BF16, 24)
    with rng.pinned(9, first_site=6300):
        spec = rng.Drop(0.1).spec()
        z = K.dropout(torch.ones(B * heads * Np, Np, device=DEV), spec).view(B, heads, Np, Np)[:, :, :T, :T]
        out, _, dqkv = _raw(qkv, do, B, T, heads, hd, None, spec)
        plain = _raw(qkv, do, B, T, heads, hd, None, None)[0]
    frac = (z == 0).float().mean().item()
    assert abs(frac - 0.1) < 0.01 and not torch.equal(out, plain)
    ref, dref = _attn_ref(qkv, do, B, T, heads, hd, [T] * B, z)
    errs = [rel(out, ref)] + [rel(dqkv[:, i * C:(i + 1) * C], dref[:, i * C:(i + 1) * C]) for i in range(3)]
    print(f"long dropout T={T} hd={hd}: fwd {errs[0]:.3e} dq {errs[1]:.3e} dk {errs[2]:.3e} dv {errs[3]:.3e}")
    assert torch.isfinite(out).all() and torch.isfinite(dqkv).all()
    assert errs[0] < OP_FWD, errs
    assert max(errs[1:]) < OP_BWD, errs


# ---------------------------------------------------------------- 5. the model
def _grads(m):
    g = {n: p.grad.detach().clone() for n, p in m.named_parameters() if p.grad is not None}
    for p in m.parameters():
        p.grad = None
    return g


def test_long_padded_model_against_itself_alone():
    """13 s clips (208000 samples, T = 649 > 640) in the two-layer layer-norm model, bf16, lengths (208000, 120000):
    each clip gets the hidden states and pooled feature of its lone run at its own length, the parameter gradients
    are the sum of the lone runs', and the padded frames are exactly zero."""
    cfg = W.Wav2Vec2Config(**{**LN.CONFIG, **GC.w2v_overrides(LN.CASE["layers"])})
    args = types.SimpleNamespace(soft=0.01, classify_drop=0.0, swin_drop=0.0)
    m = Audio2D(args, W.Wav2Vec2Model(cfg), in_feat=cfg.hidden_size, num_classes=1, use_feat=True)
    named_fill_(m.wav_model, 361)
    m = set_compute_dtype(m.to(DEV).train(), BF16)
    S, lens = 208000, [208000, 120000]
    w = randn(362, (2, S)) * torch.tensor([0.5, 2.0])[:, None] + torch.tensor([0.1, -0.3])[:, None]
    for b, n in enumerate(lens):
        w[b, n:] = 0.0
    n_dev = i64(lens)
    x = normalize_wave(w.to(DEV), n_dev)
    cot = randn(363, (2, cfg.hidden_size)).to(DEV)
    flen = W.frame_lengths(lens, cfg)
    assert list(flen) == [649, 374]
    with torch.no_grad():
        h = m.wav_model(x, lengths=n_dev)["last_hidden_state"]
    assert h.shape[1] == 649 and torch.isfinite(h).all()
    feat = m((x, n_dev))
    (feat * cot).sum().backward()
    got = _grads(m)
    for b, (n, t) in enumerate(zip(lens, flen)):
        xb = x[b:b + 1, :n].contiguous()
        with torch.no_grad():
            hb = m.wav_model(xb)["last_hidden_state"]
        fb = m(xb)
        print(f"long alone clip {b} (T_b = {t}): y {rel(h[b, :t], hb[0]):.3e} feat {rel(feat[b], fb[0]):.3e}")
        assert hb.shape[1] == t and rel(h[b, :t], hb[0]) < MODEL_FWD
        assert rel(feat[b], fb[0]) < MODEL_FWD
        assert (h[b, t:] == 0).all()
        (fb * cot[b:b + 1]).sum().backward()      # the lone runs' gradients add up in .grad
    ref = _grads(m)
    assert set(got) == set(ref)
    for k in sorted(got):
        assert torch.isfinite(got[k]).all(), k
        if k.endswith("k_proj.bias"):   # analytically zero: held to the bar times its sibling's scale
            scale = ref[k.replace("k_proj", "q_proj")].abs().max()
            assert got[k].abs().max() < MODEL_BWD * scale, k
            continue
        print(f"long alone {k}: {rel(got[k], ref[k]):.3e}")
        assert rel(got[k], ref[k]) < MODEL_BWD, (k, rel(got[k], ref[k]))


# ---------------------------------------------------------------- 6. still an error
def _wattn_fwd_into(out, qkv, B, T, heads, hd, **kw):
    C = heads * hd
    dims, win, shift = (B, 1, 1, T), (1, 1, T), (0, 0, 0)
    return K.wattn_fwd(qkv, qkv[:, C:], qkv[:, 2 * C:], qkv.stride(0), dims, win, win, shift, heads, hd, hd ** -0.5,
                       out=out, **kw)


def test_paths_that_cannot_stream_stay_errors():
    """A relative position bias (bias tables, and the gather kernel without them) and fp32 at T = 700: RuntimeError,
    and the output buffer is untouched."""
    B, T, heads, hd = 2, 700, 2, 64
    C = heads * hd
    qkv, _ = _attn_inputs(B, T, heads, hd, BF16, 25)
    rpb = torch.zeros(2 * T - 1, heads, device=DEV)
    for dt, kw in ((BF16, dict(rpb=rpb)), (BF16, dict(rpb=rpb, use_table=False)), (torch.float32, {}),
                   (torch.float32, dict(klen=i32([T, 97])))):
        out = torch.full((B * T, C), 7.0, device=DEV, dtype=dt)
        with pytest.raises(RuntimeError):
            _wattn_fwd_into(out, qkv.to(dt), B, T, heads, hd, **kw)
        torch.cuda.synchronize()
        assert (out == 7.0).all(), (dt, sorted(kw))
    out = torch.full((B * T, C), 7.0, device=DEV, dtype=BF16)      # the no-bias bf16 call of the same shape runs
    _wattn_fwd_into(out, qkv, B, T, heads, hd)
    assert torch.isfinite(out).all() and not (out == 7.0).all()
