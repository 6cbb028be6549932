"""GPU: wav2vec2 padded batches (lengths= / klen=, layer-norm family).  A clip's result does not depend on what it is
batched with: the attention op with per-clip key lengths against a torch fp32 masked softmax, the small device ops
(ragged normalisation, row mask, ragged mean, SpecAugment inside the clip's frames), the two-layer model against
transformers' run with an attention mask (tests/golden/w2v_ln_padded_2layer_1s.npz) and against its own lone-clip
runs, and a captured train step whose lengths change from step to step.

Bars are those of tests/test_gpu_w2v_ln.py, fp32 / bf16: op forward 1e-4 / 2e-2, op gradients 1e-3 / 3e-2, model
forward 1e-3 / 5e-2, model gradients 2e-3 / 1e-1 (max|a-b| / max|b|); the captured step 1e-5."""
import types

import numpy as np
import pytest
import torch

import golden_cases as GC
import make_w2v_ln_fixture as LN
import make_w2v_padded_fixture as PD
from fixtures import check, keys, load
from oracle.fill import named_fill_, randn

pytestmark = pytest.mark.gpu
if torch.cuda.is_available():
    from deepfake_amd import functional as Fn
    from deepfake_amd import kernels as K
    from deepfake_amd import rng
    from deepfake_amd.ddp import GradBucketer
    from deepfake_amd.models import set_compute_dtype
    from deepfake_amd.models import wav2vec2 as W
    from deepfake_amd.models.audioTransformer import Audio2D
    from deepfake_amd.optim import FusedSGD
    from deepfake_amd.params import ParamStore
    from deepfake_amd.trainer import TrainStep, normalize_wave

DEV = "cuda"
DTYPES = [torch.float32, torch.bfloat16]
NAN = float("nan")


def rel(a, b):
    return ((a.float() - b.float()).abs().max() / b.float().abs().max().clamp_min(1e-12)).item()


def op_bars(dt):
    return (1e-4, 1e-3) if dt == torch.float32 else (2e-2, 3e-2)


def model_bars(dt):
    return (1e-3, 2e-3) if dt == torch.float32 else (5e-2, 1e-1)


def small_config(**kw):
    return W.Wav2Vec2Config(**{**LN.CONFIG, **GC.w2v_overrides(LN.CASE["layers"]), **kw})


def i32(v):
    return torch.tensor(v, dtype=torch.int32, device=DEV)


def i64(v):
    return torch.tensor(v, dtype=torch.int64, device=DEV)


# ---------------------------------------------------------------- the attention op
def _geo(B, T, heads, hd):
    return ((B, 1, 1, T), (1, 1, T), (1, 1, T), (0, 0, 0), heads, hd, hd ** -0.5)


def _attn_inputs(B, T, heads, hd, dt, seed):
    C = heads * hd
    g = torch.Generator(device=DEV).manual_seed(seed)
    qkv = (torch.randn(B * T, 3 * C, device=DEV, generator=g) * 0.5).to(dt)
    do = torch.randn(B * T, C, device=DEV, generator=g).to(dt)
    return qkv, do


def _attn_ref(qkv, do, B, T, heads, hd, klen):
    """fp32 softmax with -inf on the keys >= kn, restricted to the rows < kn (everything else zero): out, dqkv."""
    C = heads * hd
    x = qkv.float().view(B, T, 3, heads, hd).requires_grad_(True)
    out = torch.zeros(B, T, heads, hd, device=DEV)
    for b, kn in enumerate(klen):
        q, k, v = (x[b, :kn, i].transpose(0, 1) for i in range(3))        # [heads, kn, hd]
        s = torch.softmax((q * hd ** -0.5) @ k.transpose(-1, -2), dim=-1)
        out[b, :kn] = (s @ v).transpose(0, 1)
    out = out.reshape(B * T, C)
    (gx,) = torch.autograd.grad(out, x, do.float())
    return out.detach(), gx.reshape(B * T, 3 * C)


def _run_attn(qkv, do, geo, klen, drop=None):
    x = qkv.detach().clone().requires_grad_(True)
    o = Fn.window_attention(x, None, None, geo, drop=drop, klen=klen)
    o.backward(do)
    return o.detach(), x.grad


def _rows_past(t, B, T, klen):
    """The rows >= kn of every clip of a [B*T, *] tensor, concatenated."""
    t = t.view(B, T, -1)
    return torch.cat([t[b, kn:].reshape(-1) for b, kn in enumerate(klen)])


ATTN_CASES = [(199, (199, 161, 1)), (199, (160, 97, 32)), (49, (49, 33, 32))]


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("hd", [64, 32])
@pytest.mark.parametrize("T,klen", ATTN_CASES)
def test_attention_key_lengths_against_torch(T, klen, hd, dt):
    B, heads = 3, 4
    C = heads * hd
    qkv, do = _attn_inputs(B, T, heads, hd, dt, 11)
    out, dqkv = _run_attn(qkv, do, _geo(B, T, heads, hd), i32(klen))
    ref, dref = _attn_ref(qkv, do, B, T, heads, hd, klen)
    tf, tb = op_bars(dt)
    errs = [rel(out, ref)] + [rel(dqkv[:, i * C:(i + 1) * C], dref[:, i * C:(i + 1) * C]) for i in range(3)]
    print(f"klen attention T={T} klen={klen} hd={hd} {dt}: fwd {errs[0]:.3e} dq {errs[1]:.3e} dk {errs[2]:.3e} "
          f"dv {errs[3]:.3e}")
    assert errs[0] < tf
    assert max(errs[1:]) < tb, errs
    for name, t in (("out", out), ("dqkv", dqkv)):
        past = _rows_past(t, B, T, klen)
        assert past.numel() == 0 or (past == 0).all(), name


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


@pytest.mark.parametrize("dt,dropout", [(torch.float32, False), (torch.bfloat16, False), (torch.bfloat16, True)])
@pytest.mark.parametrize("hd", [64, 32])
@pytest.mark.parametrize("T", [199, 49])
def test_full_lengths_change_nothing(T, hd, dt, dropout):
    """klen = T for every clip: out, lse, dq, dk and dv are the bits of the call without klen."""
    B, heads = 3, 4
    qkv, do = _attn_inputs(B, T, heads, hd, dt, 12)
    with rng.pinned(9, first_site=6000):
        drop = rng.Drop(0.1).spec() if dropout else None
        plain = _raw(qkv, do, B, T, heads, hd, None, drop)
        full = _raw(qkv, do, B, T, heads, hd, i32([T] * B), drop)
    Np = -(-T // 32) * 32
    for name, a, b in zip(("out", "lse", "dqkv"), plain, full):
        if name == "lse":   # the columns past T are never written
            a, b = a.view(-1, Np)[:, :T], b.view(-1, Np)[:, :T]
        assert torch.isfinite(a).all() and torch.equal(a, b), name
    if dropout:   # and the mask did something
        assert not torch.equal(plain[0], _raw(qkv, do, B, T, heads, hd, None, None)[0])


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("hd", [64, 32])
@pytest.mark.parametrize("T,klen", ATTN_CASES)
def test_attention_never_reads_the_padding(T, klen, hd, dt):
    """NaN in the rows >= kn of q / k / v and of dout: the rows < kn are bit-equal to those with zeros there, and
    everything is finite."""
    B, heads = 3, 4
    qkv, do = _attn_inputs(B, T, heads, hd, dt, 13)
    keep = (torch.arange(T, device=DEV)[None, :] < i32(klen)[:, None]).reshape(B * T, 1)
    outs = []
    for fill in (0.0, NAN):
        q = torch.where(keep, qkv, torch.full_like(qkv, fill))
        d = torch.where(keep, do, torch.full_like(do, fill))
        outs.append(_run_attn(q, d, _geo(B, T, heads, hd), i32(klen)))
    for name, a, b in zip(("out", "dqkv"), outs[0], outs[1]):
        assert torch.isfinite(b).all(), name
        assert torch.equal(a, b), name


def test_klen_with_unsupported_arguments_is_an_error():
    B, T, heads, hd = 2, 64, 2, 32
    C = heads * hd
    qkv, _ = _attn_inputs(B, T, heads, hd, torch.bfloat16, 14)
    kl = i32([40, 64])
    Fn.window_attention(qkv, None, None, _geo(B, T, heads, hd), klen=kl)      # the supported form runs
    rpb = torch.zeros(2 * T - 1, heads, device=DEV)
    with pytest.raises(RuntimeError):                                            # a relative position bias
        Fn.window_attention(qkv, rpb, None, _geo(B, T, heads, hd), klen=kl)
    with pytest.raises(RuntimeError):                                            # several windows per clip
        Fn.window_attention(qkv, None, None, ((B, 1, 1, T), (1, 1, 32), (1, 1, 32), (0, 0, 0), heads, hd, 0.2), klen=kl)
    with pytest.raises(RuntimeError):                                            # ... and a shift
        Fn.window_attention(qkv, None, None, ((B, 1, 1, T), (1, 1, 32), (1, 1, 32), (0, 0, 16), heads, hd, 0.2),
                            klen=kl)
    mask = torch.zeros(1, T, T, device=DEV)
    with pytest.raises(RuntimeError):                                            # an explicit mask
        Fn.window_attention(qkv, None, None, _geo(B, T, heads, hd), mask=mask, klen=kl)
    with pytest.raises(RuntimeError):                                            # the qkv bias as pad vectors
        Fn.window_attention(qkv, None, torch.zeros(3 * C, device=DEV), _geo(B, T, heads, hd), klen=kl)
    for bad in (kl.long(), kl[:1], kl.cpu()):                                    # int32 [B] on the device
        with pytest.raises(ValueError):
            Fn.window_attention(qkv, None, None, _geo(B, T, heads, hd), klen=bad)


# ---------------------------------------------------------------- the small device ops
def test_normalize_wave_with_lengths():
    """zero_mean_unit_var_norm with an attention mask, per clip against float64, at the uniform test's 2e-5."""
    g = np.random.default_rng(2)
    S, lens = 16000, [16000, 9999, 5200, 400]
    w = np.stack([g.standard_normal(S).astype(np.float32) * s + o for s, o in ((0.3, 0.05), (1.0, 0.0), (2.0, -0.5),
                                                                              (0.7, 0.2))])
    ref = np.zeros((4, S))
    for b, n in enumerate(lens):
        r = w[b, :n].astype(np.float64)
        ref[b, :n] = (r - r.mean()) / np.sqrt(r.var() + 1e-7)
    x = torch.from_numpy(w).to(DEV)
    got = normalize_wave(x, torch.tensor(lens))                     # host lengths
    assert np.abs(got.cpu().numpy() - ref).max() < 2e-5
    assert all((got[b, n:] == 0).all() for b, n in enumerate(lens))
    dev = K.wave_normalize(x, lengths=i64(lens))                    # device-resident lengths
    assert torch.equal(dev, got)
    xn = x.clone()                                                  # the padding is never read
    for b, n in enumerate(lens):
        xn[b, n:] = NAN
    assert torch.equal(K.wave_normalize(xn, lengths=i64(lens)), got)
    clamped = K.wave_normalize(x, lengths=i64([10 ** 9, -5, 5200, 0]))    # out-of-range device values are clamped
    assert torch.equal(clamped[0], K.wave_normalize(x)[0]) and torch.equal(clamped[2], got[2])
    assert torch.isfinite(clamped).all() and (clamped[1] == 0).all() and (clamped[3] == 0).all()   # n = 1: x - mean


@pytest.mark.parametrize("dt", DTYPES)
def test_row_mask_and_ragged_mean(dt):
    B, T, C = 4, 49, 256
    flen = [1, 32, 33, T]
    g = torch.Generator(device=DEV).manual_seed(5)
    x = torch.randn(B, T, C, device=DEV, generator=g).to(dt).requires_grad_(True)
    keep = (torch.arange(T, device=DEV)[None, :] < i64(flen)[:, None])[:, :, None]
    y = Fn.RowMaskFn.apply(x, i64(flen))
    assert torch.equal(y, torch.where(keep, x, torch.zeros_like(x)))
    dy = torch.randn(B, T, C, device=DEV, generator=g).to(dt)
    y.backward(dy)
    assert torch.equal(x.grad, torch.where(keep, dy, torch.zeros_like(dy)))
    xn = torch.where(keep, x.detach(), torch.full_like(x, NAN))      # a select, not a multiply
    assert torch.equal(K.row_mask(xn, i64(flen)), y)
    x.grad = None
    m = Fn.RowMeanRaggedFn.apply(x, i64(flen))
    ref = torch.stack([x[b, :n].float().mean(0) for b, n in enumerate(flen)])
    assert m.dtype == torch.float32 and rel(m, ref) < 1e-6
    assert torch.equal(K.rowmean_ragged(xn, i64(flen)), m)
    dm = torch.randn(B, C, device=DEV, generator=g)
    m.backward(dm)
    gref = torch.where(keep, (dm / i64(flen)[:, None].float())[:, None, :].expand(B, T, C), torch.zeros(B, T, C, device=DEV))
    assert x.grad.dtype == dt and (x.grad[~keep.expand(B, T, C)] == 0).all()
    assert rel(x.grad, gref) < (1e-6 if dt == torch.float32 else 2 ** -8)   # one rounding to dt


def test_spec_augment_with_lengths():
    """mask_time_prob 0.05, length 10, min_masks 2.  A clip of Tb frames draws at most max(int(0.05 Tb / 10 + 1), 2)
    spans (epsilon < 1, and HF's clamps only lower the count), every one inside its own frames."""
    B, T, C, mlen = 64, 199, 256, 10
    g = torch.Generator(device=DEV).manual_seed(6)
    h = torch.randn(B, T, C, device=DEV, generator=g).to(torch.bfloat16)
    emb = torch.randn(C, device=DEV, generator=g).to(torch.bfloat16)
    with rng.pinned(10, first_site=6100):
        spec = rng.Drop(0.0).spec()
        flen = [199, 120, 33, 10, 9, 1, 11, 64] * 8
        out, mask = K.spec_augment_fwd(h, emb, 0.05, mlen, 2, spec, i64(flen))
        mk = mask.bool()
        for b, n in enumerate(flen):
            assert not mk[b, n:].any(), (b, n)
            assert int(mk[b].sum()) <= max(int(0.05 * n / mlen + 1), 2) * mlen
            if n < mlen:
                assert not mk[b].any()
        assert all(mk[b].any() for b, n in enumerate(flen) if n >= 33)   # min_masks spans where they fit
        assert torch.equal(out[mk], emb.expand(int(mk.sum()), C)) and torch.equal(out[~mk], h[~mk])
        _, plain = K.spec_augment_fwd(h, emb, 0.05, mlen, 2, spec)
        _, full = K.spec_augment_fwd(h, emb, 0.05, mlen, 2, spec, i64([T] * B))
        assert torch.equal(plain, full) and plain.any()


# ---------------------------------------------------------------- the model
def _padded_model(dt, seed=PD.CASE["seed"]):
    cfg = small_config()
    args = types.SimpleNamespace(soft=0.01, classify_drop=0.0, swin_drop=0.0)
    m = Audio2D(args, W.Wav2Vec2Model(cfg), in_feat=cfg.hidden_size, num_classes=1, use_feat=True)
    named_fill_(m.wav_model, seed)
    return set_compute_dtype(m.to(DEV).train(), dt), cfg


def _grads(m):
    g = {n: p.grad.detach().clone() for n, p in m.named_parameters() if p.grad is not None}
    for p in m.parameters():
        p.grad = None
    return g


@pytest.mark.parametrize("dt", DTYPES)
def test_padded_model_against_transformers(dt):
    fx = load(PD.NAME)
    m, cfg = _padded_model(dt)
    lens = list(PD.CASE["lengths"])
    w = PD.wave_input()
    x = normalize_wave(w.to(DEV), torch.tensor(lens))
    ref_x = (w.double() - torch.from_numpy(fx["mean"])[:, None]) * torch.from_numpy(fx["rstd"])[:, None]
    for b, n in enumerate(lens):
        assert (x[b, :n].cpu().double() - ref_x[b, :n]).abs().max() < 2e-5
    n_dev = i64(lens)
    flen = W.frame_lengths(n_dev, cfg)
    assert flen.tolist() == fx["flen"].tolist()
    h = m.wav_model(x, lengths=n_dev)["last_hidden_state"]
    feat = Fn.RowMeanRaggedFn.apply(h, flen)
    feat.backward(PD.feature_cotangent(cfg.hidden_size).to(DEV))
    tf, tb = model_bars(dt)
    print(f"padded golden {dt}: y {check(fx, 'y', h, 1e9):.3e} feat {check(fx, 'feat', feat, 1e9):.3e}")
    names = dict(m.wav_model.named_parameters())
    gk = keys(fx, "g:")
    assert all(any(s in k for k in gk) for s in PD.GRAD_KEYS)
    for k in gk:
        print(f"padded golden {dt} {k}: {check(fx, k, names[k[2:]].grad, 1e9):.3e}")
    check(fx, "y", h, tf)
    check(fx, "feat", feat, tf)
    for b, t in enumerate(fx["flen"].tolist()):
        assert (h[b, t:] == 0).all()
    for k in gk:
        check(fx, k, names[k[2:]].grad, tb, what=f"[{k}] ")
    # k_proj.bias: analytically zero (softmax is invariant to a per-query shift); held to the bar times the scale of
    # its sibling, the q bias gradient (as tests/test_gpu_w2v_ln.py::_module_parity)
    scale = float(np.abs(fx["g:encoder.layers.0.attention.q_proj.bias"]).max())
    assert names["encoder.layers.0.attention.k_proj.bias"].grad.abs().max().item() < tb * scale


@pytest.mark.parametrize("dt", DTYPES)
def test_padded_model_against_itself_alone(dt):
    """Each clip of the padded batch gets the hidden states, the pooled feature and (summed over the clips) the
    parameter gradients of its lone run, the one-frame clip included; padded frames are exactly zero."""
    m, cfg = _padded_model(dt, seed=341)
    lens = list(PD.CASE["lengths"])
    n_dev = i64(lens)
    x = normalize_wave(PD.wave_input().to(DEV), n_dev)
    cot = PD.feature_cotangent(cfg.hidden_size).to(DEV)
    flen = W.frame_lengths(lens, cfg)
    with torch.no_grad():
        h = m.wav_model(x, lengths=n_dev)["last_hidden_state"]
    tf, tb = model_bars(dt)
    feat = m((x, n_dev))
    assert feat.dtype == torch.float32 and rel(m(x, lengths=lens), feat) < tf   # host integers: the same call
    (feat * cot).sum().backward()
    got = _grads(m)
    for b, (n, t) in enumerate(zip(lens, flen)):
        xb = x[b:b + 1, :n].contiguous()
        with torch.no_grad():
            hb = m.wav_model(xb)["last_hidden_state"]
        fb = m(xb)
        print(f"alone {dt} clip {b} (T_b = {t}): y {rel(h[b, :t], hb[0]):.3e} feat {rel(feat[b], fb[0]):.3e}")
        assert hb.shape[1] == t and rel(h[b, :t], hb[0]) < tf
        assert rel(feat[b], fb[0]) < tf
        assert (h[b, t:] == 0).all()
        (fb * cot[b:b + 1]).sum().backward()      # the lone runs' gradients add up in .grad
    ref = _grads(m)
    assert set(got) == set(ref)
    for k in sorted(got):
        if k.endswith("k_proj.bias"):
            scale = ref[k.replace("k_proj", "q_proj")].abs().max()
            assert got[k].abs().max() < tb * scale, k
            continue
        print(f"alone {dt} {k}: {rel(got[k], ref[k]):.3e}")
    for k in sorted(got):
        if not k.endswith("k_proj.bias"):
            assert rel(got[k], ref[k]) < tb, (k, rel(got[k], ref[k]))


def test_device_lengths_are_checked_for_shape_and_dtype_only():
    m, cfg = _padded_model(torch.float32)
    x = torch.zeros(2, 16000, device=DEV)
    for bad in (i32([16000, 8000]), i64([16000]), i64([[16000, 8000]])):
        with pytest.raises(ValueError):
            m.wav_model(x, lengths=bad)


# ---------------------------------------------------------------- the captured step
def _padded_step(graph):
    cfg = small_config()
    args = types.SimpleNamespace(soft=0.01, classify_drop=0.0, swin_drop=0.0)
    m = Audio2D(args, W.Wav2Vec2Model(cfg), in_feat=cfg.hidden_size, num_classes=1)
    m = named_fill_(set_compute_dtype(m, torch.float32), 351).to(DEV).train()
    store = ParamStore(m, torch.float32)
    return store, TrainStep(m, store, FusedSGD(store, 0.01, 0.9, 0.05), GradBucketer(store), graph=graph)


STEP_LENGTHS = [(16000, 9999), (5200, 16000), (400, 10640)]


def _run_padded(graph):
    store, step = _padded_step(graph)
    losses = []
    for i, lens in enumerate(STEP_LENGTHS):
        n = i64(list(lens))
        wave = normalize_wave(randn(500 + i, (2, 16000)).to(DEV), n)
        loss, _ = step((wave, n), torch.tensor([1.0, 0.0], device=DEV))
        losses.append(float(loss))
    torch.cuda.synchronize()
    return store.flat.clone(), losses, step


def test_graph_captured_step_with_changing_lengths_matches_eager():
    """Step 1 runs eager and captures; steps 2 and 3 replay the graph with other lengths in the same buffers: the
    parameters and losses are those of three eager steps (1e-5, as test_graph_captured_step_matches_eager)."""
    ref, lref, _ = _run_padded(False)
    got, lgot, st = _run_padded(True)
    assert st.graph is not None and st.graph_mode, "the step was not captured"
    assert len(set(round(l, 6) for l in lref)) == 3
    assert max(abs(a - b) for a, b in zip(lgot, lref)) < 1e-5, (lgot, lref)
    assert float((got - ref).abs().max() / ref.abs().max()) < 1e-5
