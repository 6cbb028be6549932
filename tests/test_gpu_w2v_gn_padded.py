"""GPU: padded batches on the group-norm / post-LN wav2vec2 family (masked_group_norm).  A clip's result does not
depend on what it is batched with: conv0 + GroupNorm + GELU with per-clip frame counts against torch fp32 on each clip
alone, the two-layer model against transformers' lone-clip runs (tests/golden/w2v_gn_padded_2layer_1s.npz) and
against its own, a captured train step whose lengths change from step to step, and a regularised step.

Bars are those of tests/test_gpu_w2v.py and tests/test_gpu_w2v_padded.py, fp32 / bf16: op forward 1e-4 / 2e-2, op
gradients 1e-3 / 3e-2, model forward 1e-3 / 5e-2, model gradients 2e-3 / 1e-1 (max|a-b| / max|b|); the captured step
1e-5."""
import functools
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import golden_cases as GC
import make_w2v_gn_padded_fixture as GP
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
EPS = 1e-5


def rel(a, b):
    return ((a.float() - b.float()).abs().max() / b.float().abs().max().clamp_min(1e-12)).item()


def op_bars(dt):
    return (1e-4, 1e-3) if dt == torch.float32 else (2e-2, 3e-2)


def model_bars(dt):
    return (1e-3, 2e-3) if dt == torch.float32 else (5e-2, 1e-1)


def i64(v):
    return torch.tensor(v, dtype=torch.int64, device=DEV)


def conv0_frames(n):
    return (n - 10) // 5 + 1


# ---------------------------------------------------------------- conv0 + GroupNorm + GELU
# T0 = 799: 13 time blocks of 64.  T0_b = 799 / 65 / 64 / 63 / 1: the whole row, one frame into the second block, the
# first block exactly, one frame short of it, a single frame
S0, LENS0 = 4000, (4000, 330, 329, 324, 10)


def _conv0_params(seed=0):
    g = torch.Generator().manual_seed(seed)
    w = (torch.randn(512, 1, 10, generator=g) * 0.3).to(DEV)
    ga = (1 + 0.1 * torch.randn(512, generator=g)).to(DEV)
    be = (0.1 * torch.randn(512, generator=g)).to(DEV)
    return w, ga, be


@functools.lru_cache(maxsize=None)
def _conv0_case(dt):
    """wave [5, S0] (zero past each clip), dout [5, T0, 512] (dt, random everywhere) and the torch fp32 reference of
    every clip alone: out [5, T0, 512] with zeros past T0_b, and dw / dgamma / dbeta summed over the clips (dout's
    rows < T0_b only).  Computed once per dtype and never written to."""
    g = torch.Generator().manual_seed(3)
    B, T0 = len(LENS0), conv0_frames(S0)
    wave = torch.randn(B, S0, generator=g).to(DEV)
    for b, n in enumerate(LENS0):
        wave[b, n:] = 0.0
    dout = torch.randn(B, T0, 512, generator=g).to(DEV).to(dt)
    w, ga, be = (p.clone().requires_grad_(True) for p in _conv0_params())
    ref = torch.zeros(B, T0, 512, device=DEV)
    for b, n in enumerate(LENS0):
        t = conv0_frames(n)
        # torch.group_norm: F.group_norm's op without its refusal of one value per channel (the single-frame clip)
        y = F.gelu(torch.group_norm(F.conv1d(wave[b:b + 1, None, :n], w, stride=5), 512, ga, be, EPS)).transpose(1, 2)
        assert y.shape == (1, t, 512)
        y.backward(dout[b:b + 1, :t].float())
        ref[b, :t] = y[0].detach()
    return wave, dout, ref, (w.grad.view(512, 10), ga.grad, be.grad)


def _conv0_run(wave, dout, lengths, dt):
    """out and (dw, dgamma, dbeta) of the op; lengths None: the uniform call."""
    w, ga, be = (p.clone().requires_grad_(True) for p in _conv0_params())
    args = (wave, w, ga, be, EPS, dt) + (() if lengths is None else (lengths,))
    out = Fn.W2VConv0Fn.apply(*args)
    out.backward(dout)
    return out.detach(), (w.grad.view(512, 10), ga.grad, be.grad)


def _check_conv0(out, grads, ref, gref, dt, what):
    tf, tb = op_bars(dt)
    errs = [rel(out, ref)] + [rel(a, r) for a, r in zip(grads, gref)]
    print(f"conv0 {what} {dt}: fwd {errs[0]:.3e} dw {errs[1]:.3e} dgamma {errs[2]:.3e} dbeta {errs[3]:.3e}")
    assert all(torch.isfinite(t).all() for t in (out,) + tuple(grads))
    assert errs[0] < tf, errs
    assert max(errs[1:]) < tb, errs
    for b, n in enumerate(LENS0):
        assert (out[b, conv0_frames(n):] == 0).all(), b


@pytest.mark.parametrize("dt", DTYPES)
def test_conv0_against_torch_per_clip(dt):
    wave, dout, ref, gref = _conv0_case(dt)
    out, grads = _conv0_run(wave, dout, i64(LENS0), dt)
    assert out.dtype == dt and out.shape == ref.shape
    _check_conv0(out, grads, ref, gref, dt, "per clip")
    # a single frame: the variance is zero, z = beta
    assert rel(out[4, 0], F.gelu(_conv0_params()[2])) < op_bars(dt)[0]


@pytest.mark.parametrize("dt", DTYPES)
def test_conv0_full_lengths_change_nothing(dt):
    """Every length full: the output and the saved statistics are the bits of the uniform call; the gradients agree
    within the op bar only (conv0_bwd_stats adds with float atomics, in both calls)."""
    g = torch.Generator().manual_seed(4)
    wave = torch.randn(2, S0, generator=g).to(DEV)
    w, ga, be = _conv0_params()
    plain, st_plain = K.w2v_conv0_fwd(wave, w.view(512, 10), ga, be, EPS, dt)
    full, st_full = K.w2v_conv0_fwd(wave, w.view(512, 10), ga, be, EPS, dt, i64([S0, S0]))
    assert torch.isfinite(plain).all() and torch.equal(plain, full)
    assert torch.equal(st_plain, st_full)
    dout = torch.randn(plain.shape, generator=g).to(DEV).to(dt)
    _, gp = _conv0_run(wave, dout, None, dt)
    _, gf = _conv0_run(wave, dout, i64([S0, S0]), dt)
    errs = [rel(a, b) for a, b in zip(gf, gp)]
    print(f"conv0 full lengths {dt}: dw {errs[0]:.3e} dgamma {errs[1]:.3e} dbeta {errs[2]:.3e}")
    assert max(errs) < op_bars(dt)[1], errs


@pytest.mark.parametrize("dt", DTYPES)
def test_conv0_never_reads_the_padding(dt):
    """NaN in the samples past n_b and in dout's rows past T0_b: the forward is bit-equal to the zero-padded run, the
    gradients are finite and within the bars of the per-clip test."""
    wave, dout, ref, gref = _conv0_case(dt)
    zero_out, _ = _conv0_run(wave, dout, i64(LENS0), dt)
    wn, dn = wave.clone(), dout.clone()
    for b, n in enumerate(LENS0):
        wn[b, n:] = NAN
        dn[b, conv0_frames(n):] = NAN
    out, grads = _conv0_run(wn, dn, i64(LENS0), dt)
    assert torch.isfinite(out).all() and torch.equal(out, zero_out)
    _check_conv0(out, grads, ref, gref, dt, "NaN padding")


@pytest.mark.parametrize("dt", DTYPES)
def test_conv0_device_lengths_are_clamped(dt):
    """10**9 -> S (the uniform result), -5 and 0 -> one sample, so one live frame; nothing leaves the row."""
    g = torch.Generator().manual_seed(5)
    wave = torch.randn(3, S0, generator=g).to(DEV)
    dout = torch.randn(3, conv0_frames(S0), 512, generator=g).to(DEV).to(dt)
    out, grads = _conv0_run(wave, dout, i64([10 ** 9, -5, 0]), dt)
    plain, _ = _conv0_run(wave, dout, None, dt)
    assert all(torch.isfinite(t).all() for t in (out,) + tuple(grads))
    assert torch.equal(out[0], plain[0])
    for b in (1, 2):
        assert (out[b, 1:] == 0).all() and (out[b, 0] != 0).any()


# ---------------------------------------------------------------- the model
def masked_config(**kw):
    return W.Wav2Vec2Config.from_json_file(GC.W2V_CONFIG_JSON, masked_group_norm=True,
                                           **{**GC.w2v_overrides(GP.CASE["layers"]), **kw})


def _padded_model(dt, seed=GP.CASE["seed"], cfg=None):
    cfg = cfg or masked_config()
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
def test_padded_model_against_transformers_alone(dt):
    fx = load(GP.NAME)
    m, cfg = _padded_model(dt)
    lens = list(GP.CASE["lengths"])
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
    print(f"gn padded golden {dt}: y {check(fx, 'y', h, 1e9):.3e} feat {check(fx, 'feat', feat, 1e9):.3e}")
    names = dict(m.wav_model.named_parameters())
    gk = keys(fx, "g:")
    assert all(any(s in k for k in gk) for s in GP.GRAD_KEYS)
    for k in gk:
        print(f"gn padded golden {dt} {k}: {check(fx, k, names[k[2:]].grad, 1e9):.3e}")
    check(fx, "y", h, tf)
    check(fx, "feat", feat, tf)
    for b, t in enumerate(fx["flen"].tolist()):
        assert (h[b, t:] == 0).all()
    for k in gk:
        check(fx, k, names[k[2:]].grad, tb, what=f"[{k}] ")
    # k_proj.bias: analytically zero (softmax is invariant to a per-query shift); held to the bar times the scale of
    # its sibling, the q bias gradient (as tests/test_gpu_w2v_padded.py)
    scale = float(np.abs(fx["g:encoder.layers.0.attention.q_proj.bias"]).max())
    assert names["encoder.layers.0.attention.k_proj.bias"].grad.abs().max().item() < tb * scale


@pytest.mark.parametrize("dt", DTYPES)
def test_padded_model_against_itself_alone(dt):
    """Each clip of the padded batch gets the hidden states, the pooled feature and (summed over the clips) the
    parameter gradients of its lone run through the uniform code, the one-frame clip included; padded frames are
    exactly zero."""
    m, cfg = _padded_model(dt, seed=342)
    lens = list(GP.CASE["lengths"])
    n_dev = i64(lens)
    x = normalize_wave(PD.wave_input().to(DEV), n_dev)
    cot = PD.feature_cotangent(cfg.hidden_size).to(DEV)
    flen = W.frame_lengths(lens, cfg)
    with torch.no_grad():
        h = m.wav_model(x, lengths=n_dev)["last_hidden_state"]
    tf, tb = model_bars(dt)
    feat = m((x, n_dev))                                                          # the (wave, lengths) tuple form
    assert feat.dtype == torch.float32 and rel(m(x, lengths=lens), feat) < tf   # host integers: the same call
    (feat * cot).sum().backward()
    got = _grads(m)
    for b, (n, t) in enumerate(zip(lens, flen)):
        xb = x[b:b + 1, :n].contiguous()
        with torch.no_grad():
            hb = m.wav_model(xb)["last_hidden_state"]
        fb = m(xb)
        print(f"gn alone {dt} clip {b} (T_b = {t}): y {rel(h[b, :t], hb[0]):.3e} feat {rel(feat[b], fb[0]):.3e}")
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
        print(f"gn alone {dt} {k}: {rel(got[k], ref[k]):.3e}")
    for k in sorted(got):
        if not k.endswith("k_proj.bias"):
            assert rel(got[k], ref[k]) < tb, (k, rel(got[k], ref[k]))


# ---------------------------------------------------------------- the captured step
STEP_LENGTHS = [(16000, 9999), (5200, 16000), (400, 10640)]


def _padded_step(graph):
    cfg = masked_config()
    args = types.SimpleNamespace(soft=0.01, classify_drop=0.0, swin_drop=0.0)
    m = Audio2D(args, W.Wav2Vec2Model(cfg), in_feat=cfg.hidden_size, num_classes=1)
    m = named_fill_(set_compute_dtype(m, torch.float32), 352).to(DEV).train()
    store = ParamStore(m, torch.float32)
    return store, TrainStep(m, store, FusedSGD(store, 0.01, 0.9, 0.05), GradBucketer(store), graph=graph)


def _run_padded(graph):
    store, step = _padded_step(graph)
    losses = []
    for i, lens in enumerate(STEP_LENGTHS):
        n = i64(list(lens))
        wave = normalize_wave(randn(510 + i, (2, 16000)).to(DEV), n)
        loss, _ = step((wave, n), torch.tensor([1.0, 0.0], device=DEV))
        losses.append(float(loss))
    torch.cuda.synchronize()
    return store.flat.clone(), losses, step


def test_graph_captured_step_with_changing_lengths_matches_eager():
    """Step 1 runs eager and captures; steps 2 and 3 replay the graph with other lengths in the same buffers: the
    parameters and losses are those of three eager steps (1e-5)."""
    ref, lref, _ = _run_padded(False)
    got, lgot, st = _run_padded(True)
    assert st.graph is not None and st.graph_mode, "the step was not captured"
    assert len(set(round(l, 6) for l in lref)) == 3
    assert max(abs(a - b) for a, b in zip(lgot, lref)) < 1e-5, (lgot, lref)
    assert float((got - ref).abs().max() / ref.abs().max()) < 1e-5


# ---------------------------------------------------------------- the regularised step
def test_regularised_padded_step():
    """The checkpoint config's own dropouts, LayerDrop and SpecAugment on a padded batch (bf16: the attention-
    probability dropout lives in the bf16 kernels): the loss and every gradient are finite, the padded rows are zero,
    and the SpecAugment spans lie inside each clip's own frames."""
    dt = torch.bfloat16
    cfg = W.Wav2Vec2Config.from_json_file(GC.W2V_CONFIG_JSON, masked_group_norm=True,
                                          num_hidden_layers=GP.CASE["layers"])
    assert cfg.layerdrop > 0 and cfg.hidden_dropout > 0 and cfg.attention_dropout > 0 and cfg.mask_time_prob > 0
    with rng.pinned(11, first_site=6200):
        m, _ = _padded_model(dt, seed=343, cfg=cfg)
        lens = list(GP.CASE["lengths"])
        n_dev = i64(lens)
        flen = W.frame_lengths(lens, cfg)
        x = normalize_wave(PD.wave_input().to(DEV), n_dev)
        x = torch.where(torch.arange(x.shape[1], device=DEV)[None, :] < n_dev[:, None], x, torch.full_like(x, NAN))
        h = m.wav_model(x, lengths=n_dev)["last_hidden_state"]
        assert torch.isfinite(h).all()
        for b, t in enumerate(flen):
            assert (h[b, t:] == 0).all() and (h[b, :t] != 0).any()
        loss = F.binary_cross_entropy_with_logits(m((x, n_dev)).mean(1), torch.tensor([1.0, 0.0, 1.0, 0.0], device=DEV))
        loss.backward()
        assert torch.isfinite(loss)
        grads = _grads(m)
        assert any(k.endswith("masked_spec_embed") for k in grads)
        for k, g in grads.items():
            assert torch.isfinite(g).all(), k
        # the model's own SpecAugment site on distinct rows: a masked row is the embedding, and lies inside the clip
        B, T, C = h.shape
        h0 = randn(7, (B, T, C)).to(DEV).to(dt)
        emb = m.wav_model.masked_spec_embed.detach().to(dt)
        hit = torch.zeros(B, T, dtype=torch.bool, device=DEV)
        for _ in range(8):
            out = m.wav_model._mask_hidden_states(h0, W.frame_lengths(n_dev, cfg))
            mk = (out != h0).any(-1)
            assert torch.equal(out[mk], emb.expand(int(mk.sum()), C))
            hit |= mk
        assert hit.any()
        for b, t in enumerate(flen):
            assert not hit[b, t:].any(), (b, t)
            assert t >= cfg.mask_time_length or not hit[b].any(), (b, t)   # no room for a span: none drawn
