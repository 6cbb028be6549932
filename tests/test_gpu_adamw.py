"""GPU: the fused AdamW step (dfk_adamw_prelude / dfk_adamw_step / dfk_adamw_step_runs, optim.FusedAdamW).

The yardstick of the kernel tests is torch.optim.AdamW on the CPU, run in float64 on the same fp32 inputs (truth
a64) and in float32 (a32): with d_ref = max|a32 - a64|, each of the kernel's p, exp_avg and exp_avg_sq must satisfy
max|a_kernel - a64| <= 2 d_ref + 2^-23 max|a64|  (the kernel's rounding sequence may differ from torch's; the ulp
term is the floor for the case where torch lands exactly).  Every test prints its figures before it asserts."""
import functools
import math

import pytest
import torch

import golden_cases as GC
from oracle.fill import named_fill_, synthetic_inputs

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from deepfake_amd import kernels as K
    from deepfake_amd import rng
    from deepfake_amd.optim import FusedAdamW
    from deepfake_amd.params import ParamStore

DEV = "cuda"
B1, B2, EPS, WD, STEPS = 0.9, 0.999, 1e-8, 0.05, 6
SIZES = [1, 3, 4, 5, 1023, 1024, 1025, 2047, 2048, 2049, 4099]


def lr_at(t):
    return 1e-3 * (1 + math.cos(math.pi * t / STEPS)) / 2


def torch_adamw(p0, grads, lrs, dtype):
    """(p, exp_avg, exp_avg_sq) of torch.optim.AdamW on the CPU in `dtype`; a None gradient skips the step."""
    p = torch.nn.Parameter(p0.to(dtype).clone())
    opt = torch.optim.AdamW([p], lr=lrs[0], betas=(B1, B2), eps=EPS, weight_decay=WD)
    for g, lr in zip(grads, lrs):
        opt.param_groups[0]["lr"] = lr
        p.grad = None if g is None else g.to(dtype).clone()
        opt.step()
    st = opt.state[p]
    return p.detach(), st["exp_avg"], st["exp_avg_sq"]


@functools.lru_cache(maxsize=None)
def case(n):
    """Inputs and both torch runs for size n, computed once: p0 = randn, g_t = 1e-2 randn with every 7th element zero
    in all steps (m = v = 0 exactly: only the decay acts) and every 5th zero in step 1."""
    gen = torch.Generator().manual_seed(1000 + n)
    p0 = torch.randn(n, generator=gen)
    grads = []
    for t in range(STEPS):
        g = 1e-2 * torch.randn(n, generator=gen)
        g[::7] = 0
        if t == 0:
            g[::5] = 0
        grads.append(g)
    lrs = [lr_at(t) for t in range(STEPS)]
    return p0, grads, lrs, torch_adamw(p0, grads, lrs, torch.float64), torch_adamw(p0, grads, lrs, torch.float32)


def check_bar(what, got, a64, a32):
    """The bar of the module docstring for (p, exp_avg, exp_avg_sq); returns the three error / d_ref ratios."""
    ratios, bad = [], []
    for name, k, t64, t32 in zip(("p", "exp_avg", "exp_avg_sq"), got, a64, a32):
        d_ref = float((t32.double() - t64).abs().max())
        d = float((k.detach().cpu().double() - t64).abs().max())
        bar = 2 * d_ref + 2.0 ** -23 * float(t64.abs().max())
        ratios.append(d / d_ref if d_ref > 0 else float("inf") if d > 0 else 0.0)
        print(f"{what} {name}: err {d:.3e} d_ref {d_ref:.3e} bar {bar:.3e} ratio {ratios[-1]:.3f}")
        if not d <= bar:
            bad.append((name, d, bar))
    assert not bad, (what, bad)
    return ratios


class Flat:
    """p / m / v / shadow / grad buffers of n elements with the device step state of `nclass` classes."""

    def __init__(self, p0, nclass=1):
        self.p = p0.to(DEV).clone()
        self.m, self.v, self.g = torch.zeros_like(self.p), torch.zeros_like(self.p), torch.zeros_like(self.p)
        self.s = torch.zeros(self.p.numel(), device=DEV, dtype=torch.bfloat16)
        self.counters = torch.zeros(nclass, device=DEV, dtype=torch.int32)
        self.corr = torch.zeros(2 * nclass, device=DEV)
        self.lr = torch.zeros(1, device=DEV)

    def step_runs(self, runs, classes, grad_scale=1.0, grad_bf16=None):
        K.adamw_prelude(self.counters, self.corr, classes, B1, B2)
        K.adamw_step_runs(self.p, self.g, self.m, self.v, self.s, runs, B1, B2, EPS, WD, self.lr, self.corr,
                          grad_scale=grad_scale, grad_bf16=grad_bf16)

    def step_each(self, runs, classes, grad_scale=1.0, grad_bf16=None):
        K.adamw_prelude(self.counters, self.corr, classes, B1, B2)
        for s, e, gate, c in runs:
            K.adamw_step(self.p[s:e], self.g[s:e], self.m[s:e], self.v[s:e], self.s[s:e], 0.0, B1, B2, EPS, WD,
                         self.corr[2 * c:2 * c + 2], lr_dev=self.lr, gate=gate, grad_scale=grad_scale,
                         grad_bf16=grad_bf16[s:e] if grad_bf16 is not None else None)

    def state(self):
        return [t.clone() for t in (self.p, self.m, self.v, self.s, self.counters)]


@pytest.mark.parametrize("entry", ["step", "runs"])
@pytest.mark.parametrize("n", SIZES)
def test_kernel_against_torch(n, entry):
    """6 steps of one run of n elements, cosine lr from 1e-3, wd 0.05, through dfk_adamw_step and through
    dfk_adamw_step_runs (the tails, the 2048-element workgroup edge, a multi-workgroup run)."""
    p0, grads, lrs, a64, a32 = case(n)
    f = Flat(p0)
    for g, lr in zip(grads, lrs):
        f.g.copy_(g)
        f.lr.fill_(lr)
        (f.step_each if entry == "step" else f.step_runs)([(0, n, None, 0)], [(0, None)])
    torch.cuda.synchronize()
    check_bar(f"n={n} {entry}", (f.p, f.m, f.v), a64, a32)
    assert torch.equal(f.s, f.p.to(torch.bfloat16)), "shadow != bf16(p)"
    assert int(f.counters[0]) == STEPS
    assert not f.m[::7].any() and not f.v[::7].any()      # zero gradients: the moments stay exactly zero


def test_gate_and_counters():
    """Two runs sharing one gated class.  Flag 0: p, m, v, shadow and the counter stay bit-identical.  Then two
    steps with flag 1 equal torch's run whose first step was skipped (grad None), and the class counter has
    advanced once per step, not once per run."""
    n = 3080
    p0, grads, lrs, _, _ = case(4099)
    p0, grads = p0[:n], [g[:n] for g in grads[:3]]
    f = Flat(p0, nclass=2)
    f.s.copy_(f.p)
    gate = torch.zeros(1, device=DEV)
    runs = [(0, 1025, gate, 1), (1028, 3077, gate, 1)]
    before = f.state()
    f.g.copy_(grads[0])
    f.lr.fill_(lrs[0])
    f.step_runs(runs, [(1, gate)])
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(f.state(), before)), "a gated-off step changed state"
    gate.fill_(1.0)
    for t in (1, 2):
        f.g.copy_(grads[t])
        f.lr.fill_(lrs[t])
        f.step_runs(runs, [(1, gate)])
    torch.cuda.synchronize()
    assert f.counters.tolist() == [0, 2]
    sched = [None, grads[1], grads[2]]
    a64, a32 = torch_adamw(p0, sched, lrs[:3], torch.float64), torch_adamw(p0, sched, lrs[:3], torch.float32)
    idx = torch.cat([torch.arange(s, e) for s, e, _, _ in runs])
    check_bar("gate", [t.cpu()[idx] for t in (f.p, f.m, f.v)], [t[idx] for t in a64], [t[idx] for t in a32])
    for s, e in ((1025, 1028), (3077, n)):               # the gap and the rest: never touched
        assert torch.equal(f.p[s:e].cpu(), p0[s:e]) and not f.m[s:e].any() and not f.v[s:e].any()


def _ragged_five(on, off):
    """(n, runs, classes, counters after two steps, untouched ranges, a range that must change, a shadow range)"""
    runs = [(0, 4, None, 0), (4, 9, on, 1), (12, 2059, off, 2), (2060, 4109, on, 1), (4112, 8211, None, 0)]
    untouched = ((9, 12), (12, 2059), (2059, 2060), (4109, 4112), (8211, 8216))
    return 8216, runs, [(0, None), (1, on), (2, off)], [2, 2, 0], untouched, (2060, 4109), (4112, 8211)


def _full_table(on, off):
    """Exactly 64 runs in 64 classes, the limit of both tables (the last slot, prefix[64], class 63): 63 runs of
    lengths cycling 1..9 at starts 12 r, then one of 2049 elements (two workgroups and a tail) in class 63 behind an
    open gate; class 33 is gated off."""
    gate = {33: off, 63: on}
    runs = [(12 * r, 12 * r + 1 + r % 9, gate.get(r), r) for r in range(63)] + [(756, 756 + 2049, on, 63)]
    untouched = tuple((runs[r][1], runs[r + 1][0]) for r in range(63)) + ((runs[33][0], runs[33][1]), (2805, 2808))
    counters = [0 if c == 33 else 2 for c in range(64)]
    return 2808, runs, [(c, gate.get(c)) for c in range(64)], counters, untouched, (756, 2805), (756, 2805)


@pytest.mark.parametrize("grad_scale,bf16_grad,table",
                         [(1.0, False, _ragged_five), (0.25, False, _ragged_five), (1.0, True, _ragged_five),
                          (0.25, True, _ragged_five), (1.0, False, _full_table), (0.25, True, _full_table)],
                         ids=["1.0-False", "0.25-False", "1.0-True", "0.25-True", "64runs-1.0-False",
                              "64runs-0.25-True"])
def test_runs_one_launch_matches_per_run(grad_scale, bf16_grad, table):
    """dfk_adamw_step_runs over 5 runs (lengths 4, 5, 2047, 2049, 4099, starts multiples of 4) against one
    dfk_adamw_step per run, bit for bit over two steps: an ungated class and two gated ones, one of them off; the
    data-parallel fold (grad_scale, bf16 bucket gradient — the fp32 gradient is then NaN and must not be read).
    Also over a full table of 64 runs in 64 classes."""
    on, off = torch.ones(1, device=DEV), torch.zeros(1, device=DEV)
    n, runs, classes, counters, untouched, changed, shadowed = table(on, off)
    gen = torch.Generator().manual_seed(5)
    p0 = torch.randn(n, generator=gen)
    a, b = Flat(p0, len(classes)), Flat(p0, len(classes))
    for t in range(2):
        g = (1e-2 * torch.randn(n, generator=gen)).to(DEV)
        gb = g.to(torch.bfloat16) if bf16_grad else None
        for f in (a, b):
            f.g.copy_(torch.full_like(g, float("nan")) if bf16_grad else g)
            f.lr.fill_(lr_at(t))
        a.step_each(runs, classes, grad_scale, gb)
        b.step_runs(runs, classes, grad_scale, gb)
    torch.cuda.synchronize()
    for x, y, name in zip(a.state(), b.state(), ("p", "exp_avg", "exp_avg_sq", "shadow", "counters")):
        assert torch.equal(x, y), name
    assert b.counters.tolist() == counters
    assert torch.isfinite(b.p).all()
    for s, e in untouched:                                                        # gaps and the gated-off run
        assert torch.equal(b.p[s:e].cpu(), p0[s:e]) and not b.m[s:e].any() and not b.v[s:e].any()
    s, e = changed
    assert not torch.equal(b.p[s:e].cpu(), p0[s:e])
    s, e = shadowed
    assert torch.equal(b.s[s:e], b.p[s:e].to(torch.bfloat16))


def _toy_store():
    torch.manual_seed(0)
    m = torch.nn.Sequential(torch.nn.Linear(33, 65), torch.nn.Linear(65, 7)).to(DEV)
    store = ParamStore(m, torch.bfloat16)
    return m, store, FusedAdamW(store, 1e-3, betas=(B1, B2), eps=EPS, weight_decay=WD)


def test_captured_step_advances_device_counters():
    """store.grad.copy_(g_static); opt.step() captured once and replayed 3 times with a new gradient and a new lr
    each time is bit-equal to three eager steps: the step counts advance on the device at every replay."""
    gen = torch.Generator().manual_seed(9)
    _, se, oe = _toy_store()
    gs = [(1e-2 * torch.randn(se.numel, generator=gen)).to(DEV) for _ in range(3)]
    for t, g in enumerate(gs):
        oe.set_lr(lr_at(t))
        se.grad.copy_(g)
        oe.step()
    _, sg, og = _toy_store()
    g_static = torch.zeros_like(gs[0])
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            sg.grad.copy_(g_static)
            og.step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert og.counters.tolist() == [0], "the capture itself must not step"
    for t, g in enumerate(gs):
        og.set_lr(lr_at(t))
        g_static.copy_(g)
        graph.replay()
    torch.cuda.synchronize()
    assert og.counters.tolist() == oe.counters.tolist() == [3]
    assert torch.equal(sg.flat, se.flat) and torch.equal(sg.shadow, se.shadow)
    assert torch.equal(og.exp_avg, oe.exp_avg) and torch.equal(og.exp_avg_sq, oe.exp_avg_sq)
    assert not torch.equal(sg.flat, _toy_store()[1].flat)


def _c1_run(graph):
    from deepfake_amd.ddp import GradBucketer
    from deepfake_amd.models.fused import build_fused
    from deepfake_amd.trainer import TrainStep
    c = GC.FUSED_C1
    m = named_fill_(build_fused("c1", compute_dtype=torch.float32), c["seed"]).to(DEV)
    m.train()
    store = ParamStore(m, torch.float32)
    opt = FusedAdamW(store, 1e-4, weight_decay=0.05)
    step = TrainStep(m, store, opt, GradBucketer(store), graph=graph)
    losses = []
    for i in range(3):
        v, mel, w, lab = synthetic_inputs(c["B"], c["T"], c["H"], c["W"], c["seconds"], seed=c["seed"] + 10 * i)
        loss, _ = step((v.to(DEV), mel.to(DEV), w.to(DEV)), lab.to(DEV))
        losses.append(float(loss))
    torch.cuda.synchronize()
    return losses, opt.exp_avg_sq.clone(), opt.counters.clone(), step


def test_whole_step_graph_matches_eager():
    """TrainStep at the C1 fixture (fp32 parity mode) with FusedAdamW(1e-4, wd 0.05), 3 steps, graph against eager.
    Parameters are not compared element-wise: Adam's first update is lr sign(g), so an element whose gradient is
    atomics-order noise may move by 2 lr between any two runs.  The losses and exp_avg_sq (quadratic in g,
    well-conditioned) are compared, at the larger of the SGD test's 1e-5 and twice the distance of two identical
    eager runs."""
    la, va, ca, _ = _c1_run(graph=False)
    lb, vb, _, _ = _c1_run(graph=False)
    lg, vg, cg, step = _c1_run(graph=True)
    assert step.graph is not None and step.graph_mode, "the step was not captured"

    def dist(l1, v1, l2, v2):
        return max(abs(x - y) for x, y in zip(l1, l2)), float((v1 - v2).abs().max() / v2.abs().max())
    ee, ge = dist(lb, vb, la, va), dist(lg, vg, la, va)
    bars = [max(1e-5, 2 * d) for d in ee]
    print(f"eager-eager: loss {ee[0]:.3e} exp_avg_sq rel {ee[1]:.3e}; graph-eager: loss {ge[0]:.3e} "
          f"exp_avg_sq rel {ge[1]:.3e}; bars {bars[0]:.3e} {bars[1]:.3e}; losses {la}")
    assert all(math.isfinite(x) for x in lg) and float(va.abs().max()) > 0
    assert ge[0] <= bars[0] and ge[1] <= bars[1], (ge, bars)
    assert torch.equal(cg, ca) and int(ca[0]) == 3


def test_layerdrop_accumulation_window():
    """The accumulation case of tests/test_gpu_regularize.py with FusedAdamW: a wav2vec2 layer kept in any
    micro-step of the window is stepped (AdamW's first step from the accumulated gradient) and its class counter
    advances once; a layer dropped in every micro-step keeps parameters, moments and counter."""
    from deepfake_amd.models import set_compute_dtype
    from deepfake_amd.models.fused import W2V_CONFIG
    from deepfake_amd.models.wav2vec2 import Wav2Vec2Config, Wav2Vec2Encoder
    torch.manual_seed(0)
    cfg = Wav2Vec2Config.from_json_file(W2V_CONFIG, num_hidden_layers=8).deterministic()
    cfg.layerdrop = 0.5
    enc = set_compute_dtype(Wav2Vec2Encoder(cfg), torch.float32).to(DEV).train()
    store = ParamStore(enc, torch.float32)
    lr = 1e-2
    opt = FusedAdamW(store, lr, weight_decay=WD)
    g = torch.Generator(device=DEV).manual_seed(3)
    h = torch.randn(2, 49, 768, device=DEV, generator=g)
    wy = torch.randn(2, 49, 768, device=DEV, generator=g)
    # the coins depend on the LayerDrop site id, i.e. on how many dropout sites earlier tests created: take the
    # first seed whose window has a layer kept in an earlier micro-step and dropped in the last one, and a layer
    # dropped in all four
    for seed in range(11, 75):
        rng.manual_seed(seed, 0)
        store.zero_grad()
        coins = []
        for _ in range(4):
            rng.advance(DEV)
            (enc(h).float() * wy).sum().backward()
            coins.append(enc.layer_keep.clone())
        c = torch.stack(coins)
        used = c.amax(0)
        if bool(((c[-1] == 0) & (used == 1)).any()) and bool((used == 0).any()):
            break
    else:
        pytest.fail("no seed in 11..74 exercises kept-then-dropped together with dropped-in-all")
    assert torch.equal(enc.layer_used, used)
    p0, g0, touched = store.flat.clone(), store.grad.clone(), list(store.touched)
    opt.step()
    torch.cuda.synchronize()

    def first_step_err(s, e):
        want = p0[s:e] * (1 - lr * WD) - lr * g0[s:e] / (g0[s:e].abs() + EPS)
        return float((store.flat[s:e] - want).abs().max() / want.abs().max().clamp_min(1e-12))
    layer_params = set()
    for i, layer in enumerate(enc.layers):
        classes = set()
        for p in layer.parameters():
            k = store.index[id(p)]
            layer_params.add(k)
            classes.add(opt.cls[k])
            s, e = store.span(k)
            if used[i] == 0:
                assert torch.equal(store.flat[s:e], p0[s:e])
                assert not opt.exp_avg[s:e].any() and not opt.exp_avg_sq[s:e].any()
            else:
                assert touched[k] and first_step_err(s, e) < 1e-5, (i, first_step_err(s, e))
        assert len(classes) == 1 and classes != {0}
        assert int(opt.counters[classes.pop()]) == int(used[i]), i
    rest = [k for k in range(len(store.params)) if k not in layer_params and touched[k]]
    assert rest and int(opt.counters[0]) == 1
    for k in rest:                                   # the ungated parameters: one class, stepped once
        assert opt.cls[k] == 0 and first_step_err(*store.span(k)) < 1e-5, store.name(k)
    store.zero_grad()
    assert torch.equal(enc.layer_used, torch.zeros_like(enc.layer_used))
