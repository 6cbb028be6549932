"""GPU parity of the layer-norm / pre-norm wav2vec2 family (feat_extract_norm="layer", conv_bias,
do_stable_layer_norm): the new feature-encoder kernels against torch fp32 ops, the pre-LN encoder against a plain
torch restatement, the whole model against transformers 5.15.0's Wav2Vec2Model (tests/golden/w2v_ln_2layer_1s.npz),
and the train step's HIP-graph capture.  Bars as tests/test_gpu_w2v.py, fp32 / bf16: op forward 1e-4 / 2e-2, op
gradients 1e-3 / 3e-2, model forward 1e-3 / 5e-2, model gradients 2e-3 / 1e-1 (max|a-b| / max|b|).  The encoder
layer and the encoder are compositions of eight and more ops, so they are held to the model bars; that choice was
made before any run and not because an op bar was missed (measured forward errors: layer 1.5e-7 fp32 / 3.8e-3 bf16,
two-layer encoder 3.7e-7 / 9.7e-3, all inside the op bars too)."""
import copy
import types

import pytest
import torch
import torch.nn.functional as F

import golden_cases as GC
import make_w2v_ln_fixture as LN
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
    from deepfake_amd.trainer import TrainStep

DEV = "cuda"
DTYPES = [torch.float32, torch.bfloat16]


def rel(a, b):
    return ((a.float() - b.float()).abs().max() / b.float().abs().max().clamp_min(1e-12)).item()


def op_bars(dt):
    return (1e-4, 1e-3) if dt == torch.float32 else (2e-2, 3e-2)


def model_bars(dt):
    return (1e-3, 2e-3) if dt == torch.float32 else (5e-2, 1e-1)


def small_config(**kw):
    return W.Wav2Vec2Config(**{**LN.CONFIG, **GC.w2v_overrides(LN.CASE["layers"]), **kw})


def _conv0_params(g, bias):
    w = (torch.randn(512, 1, 10, generator=g) * 0.3).to(DEV).requires_grad_(True)
    b = (0.2 * torch.randn(512, generator=g)).to(DEV).requires_grad_(True) if bias else None
    ga = (1 + 0.1 * torch.randn(512, generator=g)).to(DEV).requires_grad_(True)
    be = (0.1 * torch.randn(512, generator=g)).to(DEV).requires_grad_(True)
    return w, b, ga, be


def _conv0_check(wave, dt, bias, g):
    """W2VConv0LNFn on wave against gelu(layer_norm(conv1d + b)): output and parameter gradients."""
    w, b, ga, be = _conv0_params(g, bias)
    y = Fn.W2VConv0LNFn.apply(wave, w, b, ga, be, 1e-5, dt)
    T0 = (wave.shape[1] - 10) // 5 + 1
    assert y.shape == (wave.shape[0], T0, 512) and y.dtype == dt
    ref = F.gelu(F.layer_norm(F.conv1d(wave[:, None], w, b, stride=5).transpose(1, 2), (512,), ga, be, 1e-5))
    tf, tb = op_bars(dt)
    print(f"conv0_ln fwd S={wave.shape[1]} {dt} bias={bias}: {rel(y, ref):.3e}")
    assert rel(y, ref) < tf
    dy = torch.randn(y.shape, generator=g).to(DEV).to(dt)
    ps = [p for p in (w, b, ga, be) if p is not None]
    y.backward(dy)
    got = [p.grad.clone() for p in ps]
    for p in ps:
        p.grad = None
    ref.backward(dy.float())
    for name, a, p in zip(("dw", "db", "dgamma", "dbeta") if bias else ("dw", "dgamma", "dbeta"), got, ps):
        print(f"conv0_ln {name}: {rel(a, p.grad):.3e}")
        assert rel(a, p.grad) < tb, (name, rel(a, p.grad))
    return y


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("S", [4000, 325, 330, 14])
def test_conv0_layernorm_gelu(dt, bias, S):
    """T0 = 799 (a ragged last block of 64 frames), 64 (exactly one block), 65 (one frame more), 1."""
    g = torch.Generator().manual_seed(S)
    _conv0_check(torch.randn(2, S, generator=g).to(DEV), dt, bias, g)


@pytest.mark.parametrize("dt", DTYPES)
def test_conv0_workgroups_walk_several_time_blocks(dt):
    """B = 48 clips of 799 frames: the backward runs 512 / 48 = 10 workgroups per clip over 13 time blocks, so
    three of them restage the waveform and keep accumulating over a second block (the loop every training shape
    takes: B = 8 at 4 s is 200 blocks over 64 workgroups)."""
    g = torch.Generator().manual_seed(48)
    _conv0_check(torch.randn(48, 4000, generator=g).to(DEV), dt, True, g)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("rows", [8192 + 37, 2048 + 5])
def test_ln_gelu_rows_beyond_one_grid(dt, rows):
    """The row kernels' grid-stride loops: the forward strides above 4 x 2048 = 8192 rows, the backward above
    4 x 512 = 2048 (a ragged last stride in both).  Against torch fp32 on the same (rounded) input."""
    g = torch.Generator().manual_seed(rows)
    x = (2 * torch.randn(rows, 512, generator=g) + 0.5).to(DEV).to(dt)
    ga = (1 + 0.1 * torch.randn(512, generator=g)).to(DEV).requires_grad_(True)
    be = (0.1 * torch.randn(512, generator=g)).to(DEV).requires_grad_(True)
    y, st = K.w2v_ln_gelu_fwd(x, ga.detach(), be.detach(), 1e-5)
    xr = x.float().requires_grad_(True)
    ref = F.gelu(F.layer_norm(xr, (512,), ga, be, 1e-5))
    tf, tb = op_bars(dt)
    assert rel(y, ref) < tf, rel(y, ref)
    dy = torch.randn(rows, 512, generator=g).to(DEV).to(dt)
    sinks = [torch.zeros(512, device=DEV) for _ in range(3)]
    dx = K.w2v_ln_gelu_bwd(dy, x, ga.detach(), be.detach(), st, *sinks)
    ref.backward(dy.float())
    for name, a, r in (("dx", dx, xr.grad), ("dgamma", sinks[0], ga.grad), ("dbeta", sinks[1], be.grad),
                       ("dbias", sinks[2], xr.grad.sum(0))):
        print(f"ln_gelu rows={rows} {dt} {name}: {rel(a, r):.3e}")
        assert rel(a, r) < tb, (name, rel(a, r))


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("S", [4000, 330])
def test_conv0_reads_nothing_past_the_waveform(dt, S):
    """The waveform sits at the front of a buffer whose remainder is NaN: outputs and gradients are those of
    the plain call (no sample at or past S of the last clip reaches arithmetic)."""
    g = torch.Generator().manual_seed(S)
    wave = torch.randn(2, S, generator=g)
    buf = torch.full((2 * S + 4096,), float("nan"), device=DEV)
    buf[:2 * S] = wave.reshape(-1).to(DEV)
    view = buf[:2 * S].view(2, S)
    assert view.data_ptr() == buf.data_ptr() and view.is_contiguous()
    y = _conv0_check(view, dt, True, g)
    assert torch.isfinite(y).all()


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("k,s,Tin", [(3, 2, 99), (3, 2, 100), (2, 2, 50), (2, 2, 49)])
def test_conv_layernorm_gelu(dt, bias, k, s, Tin):
    g = torch.Generator().manual_seed(1)
    x = torch.randn(3, Tin, 512, generator=g).to(DEV).to(dt).requires_grad_(True)
    w = (torch.randn(512, 512, k, generator=g) / 40).to(DEV).requires_grad_(True)
    b = (0.1 * torch.randn(512, generator=g)).to(DEV).requires_grad_(True) if bias else None
    ga = (1 + 0.1 * torch.randn(512, generator=g)).to(DEV).requires_grad_(True)
    be = (0.1 * torch.randn(512, generator=g)).to(DEV).requires_grad_(True)
    y = Fn.ConvLNGeluFn.apply(x, w, b, ga, be, s, 1e-5)
    xr = x.detach().float().requires_grad_(True)
    ref = F.gelu(F.layer_norm(F.conv1d(xr.transpose(1, 2), w, b, stride=s).transpose(1, 2), (512,), ga, be, 1e-5))
    tf, tb = op_bars(dt)
    print(f"conv_ln fwd {dt} k={k} Tin={Tin} bias={bias}: {rel(y, ref):.3e}")
    assert y.dtype == dt and rel(y, ref) < tf
    dy = torch.randn(y.shape, generator=g).to(DEV).to(dt)
    ps = [p for p in (w, b, ga, be) if p is not None]
    y.backward(dy)
    got = [x.grad.clone()] + [p.grad.clone() for p in ps]
    for p in ps:
        p.grad = None
    ref.backward(dy.float())
    names = ("dx", "dw", "db", "dgamma", "dbeta") if bias else ("dx", "dw", "dgamma", "dbeta")
    for name, a, r in zip(names, got, [xr.grad] + [p.grad for p in ps]):
        print(f"conv_ln {name}: {rel(a, r):.3e}")
        assert rel(a, r) < tb, (name, rel(a, r))


@pytest.mark.parametrize("dt", DTYPES)
def test_backward_is_bitwise_repeatable(dt):
    """Two identical backward calls of each new kernel give bit-equal results (fixed-order partial sums, no float
    atomics).  ConvLNGeluFn's dW GEMM has split-K atomics of its own and is outside this claim: only what the
    new kernels write is compared."""
    g = torch.Generator().manual_seed(5)
    wave = torch.randn(2, 4000, generator=g).to(DEV)
    w, b, ga, be = (p.detach() for p in _conv0_params(g, True))
    w = w.reshape(512, 10).contiguous()
    y, stats = K.w2v_conv0_ln_fwd(wave, w, b, ga, be, 1e-5, dt)
    dy = torch.randn(y.shape, generator=g).to(DEV).to(dt)
    runs = []
    for _ in range(2):
        sinks = [torch.zeros_like(p) for p in (w, b, ga, be)]
        K.w2v_conv0_ln_bwd(wave, w, b, ga, be, stats, dy, *sinks)
        runs.append(sinks)
    assert all(torch.equal(a, c) for a, c in zip(*runs)) and all(s.abs().max() > 0 for s in runs[0])
    # accumulation: a second call into the same sinks adds (the contract gradient accumulation relies on)
    K.w2v_conv0_ln_bwd(wave, w, b, ga, be, stats, dy, *runs[0])
    assert all(torch.equal(a, 2 * c) for a, c in zip(runs[0], runs[1]))
    x = torch.randn(3 * 49, 512, generator=g).to(DEV).to(dt)
    o, st = K.w2v_ln_gelu_fwd(x, ga, be, 1e-5)
    do = torch.randn(o.shape, generator=g).to(DEV).to(dt)
    runs = []
    for _ in range(2):
        sinks = [torch.zeros(512, device=DEV) for _ in range(3)]
        runs.append([K.w2v_ln_gelu_bwd(do, x, ga, be, st, *sinks)] + sinks)
    assert all(torch.equal(a, c) for a, c in zip(*runs)) and all(s.float().abs().max() > 0 for s in runs[0])


# ---------------------------------------------------------------- pre-LN encoder against plain torch
def _ref_attention(a, x):
    B, T, C = x.shape
    hd = C // a.num_heads
    q, k, v = (F.linear(x, p.weight, p.bias).view(B, T, a.num_heads, hd).transpose(1, 2)
               for p in (a.q_proj, a.k_proj, a.v_proj))
    s = torch.softmax((q * a.scaling) @ k.transpose(-1, -2), dim=-1)
    return F.linear((s @ v).transpose(1, 2).reshape(B, T, C), a.out_proj.weight, a.out_proj.bias)


def _ref_ln(ln, x):
    return F.layer_norm(x, (x.shape[-1],), ln.weight, ln.bias, ln.eps)


def _ref_layer(l, x):
    """HF Wav2Vec2EncoderLayerStableLayerNorm.forward with the dropouts off."""
    x = x + _ref_attention(l.attention, _ref_ln(l.layer_norm, x))
    ff = l.feed_forward
    h = _ref_ln(l.final_layer_norm, x)
    return x + F.linear(F.gelu(F.linear(h, ff.intermediate_dense.weight, ff.intermediate_dense.bias)),
                        ff.output_dense.weight, ff.output_dense.bias)


def _ref_encoder(e, h):
    """HF Wav2Vec2EncoderStableLayerNorm.forward with no mask, dropouts and LayerDrop off."""
    pc = e.pos_conv_embed
    k = pc.conv.kernel_size[0]
    pos = F.conv1d(h.transpose(1, 2), pc.weight(), pc.conv.bias, padding=k // 2, groups=pc.groups)[:, :, :-1]
    x = h + F.gelu(pos).transpose(1, 2)
    for l in e.layers:
        x = _ref_layer(l, x)
    return _ref_ln(e.layer_norm, x)


def _module_parity(build, ref_fn, run, dt, seed):
    cfg = small_config()
    m = named_fill_(build(cfg), seed).to(DEV).train()
    r = copy.deepcopy(m)
    set_compute_dtype(m, dt)
    B, T, C = 2, 49, cfg.hidden_size
    x = randn(seed + 1, (B, T, C)).to(DEV).to(dt).requires_grad_(True)
    xr = x.detach().float().requires_grad_(True)
    y, ref = run(m, x), ref_fn(r, xr)
    tf, tb = model_bars(dt)
    print(f"{type(m).__name__} fwd {dt}: {rel(y, ref):.3e}")
    assert y.shape == ref.shape and rel(y, ref) < tf
    dy = randn(seed + 2, y.shape).to(DEV).to(dt)
    y.backward(dy)
    ref.backward(dy.float())
    assert rel(x.grad, xr.grad) < tb, ("dx", rel(x.grad, xr.grad))
    ref_grads = {n: q.grad for n, q in r.named_parameters()}
    for n, p in m.named_parameters():
        assert p.grad is not None, n
        if n.endswith("k_proj.bias"):
            # softmax is invariant to a per-query shift of the scores, so this gradient is exactly zero: hold it
            # to the bar against the scale of its sibling, the q bias gradient
            scale = ref_grads[n.replace("k_proj", "q_proj")].abs().max()
            assert p.grad.abs().max() < tb * scale, (n, p.grad.abs().max().item(), scale.item())
            continue
        assert rel(p.grad, ref_grads[n]) < tb, (n, rel(p.grad, ref_grads[n]))


@pytest.mark.parametrize("dt", DTYPES)
def test_stable_layer_norm_encoder_layer(dt):
    _module_parity(W.Wav2Vec2EncoderLayerStableLayerNorm, _ref_layer,
                   lambda m, x: m(x.reshape(-1, x.shape[-1]), x.shape[0], x.shape[1]).view(x.shape), dt, 301)


@pytest.mark.parametrize("dt", DTYPES)
def test_stable_layer_norm_encoder(dt):
    _module_parity(W.Wav2Vec2EncoderStableLayerNorm, _ref_encoder, lambda m, x: m(x), dt, 311)


# ---------------------------------------------------------------- the transformers fixture
@pytest.mark.parametrize("dt", DTYPES)
def test_w2v_ln_2layer_golden(dt):
    fx = load(LN.NAME)
    m = named_fill_(W.Wav2Vec2Model(small_config()), LN.CASE["seed"]).to(DEV).train()
    set_compute_dtype(m, dt)
    out = m(LN.wave_input().to(DEV))
    h = out["last_hidden_state"]
    h.backward(randn(LN.CASE["seed"] + 2, h.shape).to(DEV).to(dt))
    tf, tb = model_bars(dt)
    print(f"golden {dt}: y {check(fx, 'y', h, 1e9):.3e} extract {check(fx, 'extract', out['extract_features'], 1e9):.3e}")
    check(fx, "y", h, tf)
    check(fx, "extract", out["extract_features"], tf)
    names = dict(m.named_parameters())
    gk = keys(fx, "g:")
    assert all(any(s in k for k in gk) for s in LN.GRAD_KEYS)
    for k in gk:
        print(f"golden {dt} {k}: {check(fx, k, names[k[2:]].grad, 1e9):.3e}")
    for k in gk:
        check(fx, k, names[k[2:]].grad, tb, what=f"[{k}] ")


# ---------------------------------------------------------------- train step: capture, LayerDrop gates
class _WaveSlot(torch.nn.Module):
    """TrainStep hands the model a tuple of input tensors: the paudio model takes its only member."""

    def __init__(self, inner):
        super().__init__()
        self.inner = inner

    def forward(self, feature):
        return self.inner(feature[0])


def _paudio_step(cfg, dt, graph, seed=321):
    args = types.SimpleNamespace(soft=0.01, classify_drop=0.0, swin_drop=0.0)
    m = _WaveSlot(Audio2D(args, W.Wav2Vec2Model(cfg), in_feat=cfg.hidden_size, num_classes=1))
    m = named_fill_(set_compute_dtype(m, dt), seed).to(DEV).train()
    store = ParamStore(m, dt)
    return m, store, TrainStep(m, store, FusedSGD(store, 0.01, 0.9, 0.05), GradBucketer(store), graph=graph)


def _batch(i):
    wave = randn(400 + i, (2, 16000)).to(DEV)
    return (wave,), torch.tensor([1.0, 0.0], device=DEV)


def _run_paudio(steps, graph):
    m, store, step = _paudio_step(small_config(), torch.float32, graph)
    losses = []
    for i in range(steps):
        loss, _ = step(*_batch(i))
        losses.append(float(loss))
    torch.cuda.synchronize()
    return store.flat.clone(), losses, step


def test_graph_captured_step_matches_eager():
    """Step 1 runs eager and captures; steps 2-3 replay the graph on new inputs: parameters and losses equal
    three eager steps, at the bar of tests/test_gpu_trainstep.py (1e-5, fp32 parity mode as there)."""
    ref, lref, _ = _run_paudio(3, False)
    got, lgot, st = _run_paudio(3, True)
    assert st.graph is not None and st.graph_mode, "the step was not captured"
    assert max(abs(a - b) for a, b in zip(lgot, lref)) < 1e-5, (lgot, lref)
    assert float((got - ref).abs().max() / ref.abs().max()) < 1e-5


@pytest.fixture
def pinned_draws():
    """The regularisers' draws made independent of what ran before in the process (rng.pinned: fixed seeds, site
    ids from a fixed number on, both put back afterwards)."""
    with rng.pinned(7, first_site=5000):
        yield


@pytest.mark.parametrize("dt", DTYPES)
def test_regularised_steps_and_layerdrop_gates(dt, pinned_draws):
    """LayerDrop 0.5 with every dropout and SpecAugment on, captured: the losses stay finite, and over a
    two-micro-step accumulation window the parameters of a layer no micro-step kept (layer_used = 0) are unchanged
    while a kept layer's move."""
    # attention-probability dropout exists in the bf16 attention kernels only (fp32 is the parity mode: p = 0)
    cfg = small_config(num_hidden_layers=8, layerdrop=0.5, hidden_dropout=0.1,
                       attention_dropout=0.1 if dt == torch.bfloat16 else 0.0,
                       activation_dropout=0.1, feat_proj_dropout=0.1, mask_time_prob=0.05)
    m, store, step = _paudio_step(cfg, dt, True)
    for i in range(3):   # eager + capture, then replays
        loss, _ = step(*_batch(i))
        assert torch.isfinite(loss).all()
    assert step.graph is not None and step.graph_mode, "the step was not captured"
    enc = m.inner.wav_model.encoder
    # an eager accumulation window from clean gradients and gates, so the flags can be read between its micro-steps
    step.graph_mode = False
    store.zero_grad()
    before = [[p.detach().clone() for p in l.parameters()] for l in enc.layers]
    step.micro(*_batch(3), False, 2)
    used = enc.layer_used.clone()
    loss, _ = step.micro(*_batch(4), True, 2)
    used = torch.maximum(used, enc.layer_keep).cpu()   # the window's second set of coins
    assert torch.isfinite(loss).all()
    assert (used == 0).any() and (used > 0).any(), used
    for i, l in enumerate(enc.layers):
        same = all(torch.equal(p, q) for p, q in zip(l.parameters(), before[i]))
        assert same == bool(used[i] == 0), (i, used)
