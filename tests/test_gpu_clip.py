"""GPU: global gradient-norm clipping on the device (dfk_grad_sqnorm_runs, dfk_grad_clip_coef, the dfk_*_clip update
entry points, FusedSGD / FusedAdamW(max_grad_norm=...)).

The yardstick of the norm is the float64 norm of the same fp32 (or bf16) inputs on the CPU, bar 8 * 2^-24 relative:
the double accumulation is exact to far below fp32, a thread's 8 squares summed in fp32 would add <= 8 * 2^-24 on the
sum = 4 * 2^-24 on the root, the fp32 rounding of the root 2^-24, the rest is margin.  The yardstick of the update is
torch.nn.utils.clip_grad_norm_ + torch.optim.SGD / AdamW on the CPU, in float64 on the same fp32 inputs (a64) and in
float32 (a32): with d_ref = max|a32 - a64| every state tensor must satisfy max|a_kernel - a64| <= 2 d_ref + 2^-23
max|a64| (the rule of tests/test_gpu_adamw.py).  Every test prints its figures before it asserts."""
import functools
import math

import pytest
import torch

import golden_cases as GC
from oracle.fill import named_fill_, synthetic_inputs

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from deepfake_amd import kernels as K
    from deepfake_amd.optim import FusedAdamW, FusedSGD
    from deepfake_amd.params import ParamStore

DEV = "cuda"
B1, B2, EPS, WD, MOM, STEPS = 0.9, 0.999, 1e-8, 0.05, 0.9, 6
PARTIALS = 2048                       # DFK_GNORM_PARTIALS (tests/test_clip_cpu.py holds it to the header)
LARGE = PARTIALS * 2048 + 5           # every persistent workgroup owns a block, workgroup 0 a second one (5 elements)
SIZES = [1, 3, 4, 5, 1023, 1024, 1025, 2047, 2048, 2049, 4099, LARGE]
NORM_BAR = 8 * 2.0 ** -24
SCALES = [1.0, 0.25, 2.0, 0.25, 2.0, 1.0]     # of the gradient per step: max_norm = half of step 1's norm


def lr_at(t):
    return 1e-3 * (1 + math.cos(math.pi * t / STEPS)) / 2


def slab(chunks=1):
    return torch.full((chunks * PARTIALS,), float("nan"), device=DEV, dtype=torch.float64)


def device_norm(grad, runs, max_norm, grad_scale=1.0, grad_bf16=None, partials=None):
    """{norm, coef} (device fp32 [2]) of the runs [(start, end, gate)]."""
    partials = slab(-(-len(runs) // 64)) if partials is None else partials
    out = torch.full((2,), float("nan"), device=DEV)
    n = K.grad_sqnorm_runs(grad, runs, partials, grad_scale=grad_scale, grad_bf16=grad_bf16)
    K.grad_clip_coef(partials, n, max_norm, out)
    return out


def coef_of(norm32, max_norm):
    """clip_grad_norm_'s coefficient from an fp32 norm, in fp32 as torch evaluates it."""
    c = torch.tensor(max_norm, dtype=torch.float32) / (norm32.float().cpu() + torch.tensor(1e-6, dtype=torch.float32))
    return torch.clamp(c, max=1.0)


def check_norm(what, out, ref64, max_norm):
    norm, coef = float(out[0]), float(out[1])
    rel = abs(norm - ref64) / ref64 if ref64 > 0 else abs(norm)
    want = float(coef_of(out[0], max_norm))
    print(f"{what}: norm {norm:.9e} ref {ref64:.9e} rel {rel:.3e} bar {NORM_BAR:.3e} coef {coef:.9e} want {want:.9e}")
    assert rel <= NORM_BAR, (what, rel)
    assert abs(coef - want) <= 2.0 ** -23 * want, (what, coef, want)     # correctly rounded fp32 divide: equal


@functools.lru_cache(maxsize=None)
def gradient(n):
    """Three runs: n elements, then 1021 and 2051 (n % 4 != 0 tails), starts multiples of 4 with a gap before each;
    the gaps hold NaN and must never be read.  Returns (fp32 buffer on the CPU, runs)."""
    gen = torch.Generator().manual_seed(77 + n)
    a1 = -(-n // 4) * 4 + 4
    a2 = -(-(a1 + 1021) // 4) * 4 + 8
    runs = ((0, n), (a1, a1 + 1021), (a2, a2 + 2051))
    g = torch.full((a2 + 2051 + 3,), float("nan"))
    for s, e in runs:
        g[s:e] = 1e-2 * torch.randn(e - s, generator=gen)
    return g, runs


def norm_inputs(n, nruns, bf16, mag=1.0):
    """Device buffers and the float64 reference sum of squares per run."""
    g, runs = gradient(n)
    g = g * mag
    runs = runs[:nruns]
    gb = g.to(torch.bfloat16) if bf16 else None
    src = gb if bf16 else g
    sq = [float((src[s:e].double() ** 2).sum()) for s, e in runs]
    dev_g = torch.full_like(g, float("nan")).to(DEV) if bf16 else g.to(DEV)     # bf16: the fp32 buffer is not read
    return dev_g, gb.to(DEV) if bf16 else None, runs, sq


@pytest.mark.parametrize("nruns", [1, 3])
@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("s", [1.0, 0.25])
@pytest.mark.parametrize("n", SIZES)
def test_norm_against_float64(n, s, bf16, nruns):
    g, gb, runs, sq = norm_inputs(n, nruns, bf16)
    ref = s * math.sqrt(sum(sq))
    out = device_norm(g, [(a, b, None) for a, b in runs], 0.5 * ref, grad_scale=s, grad_bf16=gb)
    check_norm(f"n={n} s={s} bf16={bf16} runs={nruns}", out, ref, 0.5 * ref)
    assert float(out[1]) < 1.0


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("mag", [1e-25, 1e18])
@pytest.mark.parametrize("n", SIZES)
def test_norm_of_gradients_whose_squares_leave_fp32(n, mag, bf16):
    """|g| ~ 1e-27 (squares underflow fp32 to zero) and ~ 1e16 (squares overflow it): the same bar holds only if
    every element is squared and accumulated in double."""
    g, gb, runs, sq = norm_inputs(n, 3, bf16, mag=mag)
    ref = math.sqrt(sum(sq))
    assert 1e-30 < ref < 1e25
    out = device_norm(g, [(a, b, None) for a, b in runs], 2 * ref, grad_bf16=gb)
    check_norm(f"n={n} mag={mag} bf16={bf16}", out, ref, 2 * ref)


def test_repeatable_and_independent_of_a_stale_slab():
    """Two calls on the same input are bit-equal; the largest size followed by n = 5 on the same slab gives n = 5's
    result (every slot is rewritten, with zero where a workgroup had no work)."""
    g, _, runs, sq = norm_inputs(LARGE, 3, False)
    table = [(a, b, None) for a, b in runs]
    part = slab()
    first = device_norm(g, table, 1.0, partials=part).clone()
    assert not torch.isnan(part).any()
    again = device_norm(g, table, 1.0, partials=part).clone()
    other = device_norm(g, table, 1.0).clone()                       # a fresh slab
    print(f"large: {first.tolist()} {again.tolist()} {other.tolist()}")
    assert torch.equal(first, again) and torch.equal(first, other)
    g5, _, runs5, sq5 = norm_inputs(5, 1, False)
    small = device_norm(g5, [(0, 5, None)], 1.0, partials=part).clone()
    fresh = device_norm(g5, [(0, 5, None)], 1.0).clone()
    print(f"n=5 after the large call: {small.tolist()} fresh: {fresh.tolist()} slab nonzero {int((part != 0).sum())}")
    assert torch.equal(small, fresh)
    assert int((part != 0).sum()) == 1 and float(part[0]) > 0
    check_norm("n=5 stale slab", small, math.sqrt(sq5[0]), 1.0)


def test_more_than_64_runs_go_in_chunks():
    """70 runs of 9 elements: two chunks, each into its own slab, summed by the coefficient kernel."""
    gen = torch.Generator().manual_seed(3)
    g = 1e-2 * torch.randn(70 * 12, generator=gen)
    runs = [(12 * i, 12 * i + 9, None) for i in range(70)]
    ref = math.sqrt(sum(float((g[s:e].double() ** 2).sum()) for s, e, _ in runs))
    part = slab(2)
    out = device_norm(g.to(DEV), runs, 1.0, partials=part)
    check_norm("70 runs", out, ref, 1.0)
    assert not torch.isnan(part).any() and float(part[PARTIALS:].sum()) > 0


# ---- the update -------------------------------------------------------------------------------------------------
class Flat:
    """State of one optimizer over n elements: p, the gradient, two state buffers (SGD: momentum and an unused one;
    AdamW: exp_avg, exp_avg_sq), the bf16 shadow and the device scalars."""

    def __init__(self, kind, p0, nclass=1):
        self.kind = kind
        self.p = p0.to(DEV).clone()
        self.a, self.b, self.g = torch.zeros_like(self.p), torch.zeros_like(self.p), torch.zeros_like(self.p)
        self.s = self.p.to(torch.bfloat16)
        self.counters = torch.zeros(nclass, device=DEV, dtype=torch.int32)
        self.corr = torch.zeros(2 * nclass, device=DEV)
        self.lr = torch.zeros(1, device=DEV)
        self.part = slab()
        self.pair = torch.zeros(2, device=DEV)

    def step(self, runs, entry, max_norm=None, grad_scale=1.0, grad_bf16=None, first=False):
        """runs [(start, end, gate, class)]; max_norm None: the plain entry points."""
        ck = {}
        if max_norm is not None:
            n = K.grad_sqnorm_runs(self.g, [r[:3] for r in runs], self.part, grad_scale=grad_scale,
                                   grad_bf16=grad_bf16)
            K.grad_clip_coef(self.part, n, max_norm, self.pair)
            ck["clip_coef"] = self.pair[1:2]
        fold = {"grad_scale": grad_scale, "grad_bf16": grad_bf16}
        if self.kind == "adamw":
            cls = {c: g for _, _, g, c in runs}
            K.adamw_prelude(self.counters, self.corr, [(c, cls[c]) for c in sorted(cls)], B1, B2)
            if entry == "runs":
                return K.adamw_step_runs(self.p, self.g, self.a, self.b, self.s, runs, B1, B2, EPS, WD, self.lr,
                                         self.corr, **fold, **ck)
            for s, e, gate, c in runs:
                K.adamw_step(self.p[s:e], self.g[s:e], self.a[s:e], self.b[s:e], self.s[s:e], 0.0, B1, B2, EPS, WD,
                             self.corr[2 * c:2 * c + 2], lr_dev=self.lr, gate=gate, grad_scale=grad_scale,
                             grad_bf16=grad_bf16[s:e] if grad_bf16 is not None else None, **ck)
            return None
        if entry == "runs":
            return K.sgd_step_runs(self.p, self.g, self.a, self.s, [(s, e, gate, first) for s, e, gate, _ in runs],
                                   MOM, WD, self.lr, **fold, **ck)
        for s, e, gate, _ in runs:
            K.sgd_step(self.p[s:e], self.g[s:e], self.a[s:e], self.s[s:e], 0.0, MOM, WD, first, lr_dev=self.lr,
                       gate=gate, grad_scale=grad_scale, grad_bf16=grad_bf16[s:e] if grad_bf16 is not None else None,
                       **ck)
        return None

    def state(self):
        return [t.clone() for t in (self.p, self.a, self.b, self.s, self.counters)]


def torch_clipped(kind, p0, grads, lrs, max_norm, dtype):
    """clip_grad_norm_ + torch.optim.SGD / AdamW on the CPU in `dtype` -> (state tensors, norms, coefficients)."""
    p = torch.nn.Parameter(p0.to(dtype).clone())
    if kind == "adamw":
        opt = torch.optim.AdamW([p], lr=lrs[0], betas=(B1, B2), eps=EPS, weight_decay=WD)
    else:
        opt = torch.optim.SGD([p], lr=lrs[0], momentum=MOM, weight_decay=WD)
    norms = []
    for g, lr in zip(grads, lrs):
        opt.param_groups[0]["lr"] = lr
        p.grad = g.to(dtype).clone()
        norms.append(float(torch.nn.utils.clip_grad_norm_([p], max_norm, norm_type=2, error_if_nonfinite=False)))
        opt.step()
    st = opt.state[p]
    state = (p.detach(), st["exp_avg"], st["exp_avg_sq"]) if kind == "adamw" else (p.detach(), st["momentum_buffer"])
    return state, norms


@functools.lru_cache(maxsize=None)
def case(kind, n):
    gen = torch.Generator().manual_seed(2000 + n)
    p0 = torch.randn(n, generator=gen)
    grads = [sc * 1e-2 * torch.randn(n, generator=gen) for sc in SCALES]
    max_norm = 0.5 * float(grads[0].double().norm())
    lrs = [lr_at(t) for t in range(STEPS)]
    a64, norms = torch_clipped(kind, p0, grads, lrs, max_norm, torch.float64)
    a32, _ = torch_clipped(kind, p0, grads, lrs, max_norm, torch.float32)
    return p0, grads, lrs, max_norm, a64, a32, norms


def check_bar(what, names, got, a64, a32):
    bad = []
    for name, k, t64, t32 in zip(names, got, a64, a32):
        d_ref = float((t32.double() - t64).abs().max())
        d = float((k.detach().cpu().double() - t64).abs().max())
        bar = 2 * d_ref + 2.0 ** -23 * float(t64.abs().max())
        print(f"{what} {name}: err {d:.3e} d_ref {d_ref:.3e} bar {bar:.3e} ratio {d / d_ref if d_ref else 0:.3f}")
        if not d <= bar:
            bad.append((name, d, bar))
    assert not bad, (what, bad)


@pytest.mark.parametrize("entry", ["step", "runs"])
@pytest.mark.parametrize("kind", ["sgd", "adamw"])
@pytest.mark.parametrize("n", SIZES)
def test_update_against_torch(n, kind, entry):
    """6 steps, cosine lr, one run of n elements; max_norm is half the float64 norm of step 1 and the later gradients
    come at 0.25x and 2x scale, so clipping acts in some steps and not in others."""
    p0, grads, lrs, max_norm, a64, a32, norms = case(kind, n)
    f = Flat(kind, p0)
    pairs = []
    for t, (g, lr) in enumerate(zip(grads, lrs)):
        f.g.copy_(g)
        f.lr.fill_(lr)
        f.step([(0, n, None, 0)], entry, max_norm=max_norm, first=(t == 0))
        pairs.append(f.pair.clone())
    torch.cuda.synchronize()
    pairs = torch.stack(pairs).cpu()
    print(f"n={n} {kind} {entry}: max_norm {max_norm:.6e} norms {pairs[:, 0].tolist()} torch64 {norms} "
          f"coef {pairs[:, 1].tolist()}")
    for t in range(STEPS):
        assert abs(float(pairs[t, 0]) - norms[t]) <= NORM_BAR * norms[t], t
    active = [t for t in range(STEPS) if float(pairs[t, 1]) < 1.0]
    assert active and len(active) < STEPS, active
    assert active == [t for t in range(STEPS) if norms[t] > max_norm]
    names = ("p", "exp_avg", "exp_avg_sq") if kind == "adamw" else ("p", "momentum")
    check_bar(f"n={n} {kind} {entry}", names, (f.p, f.a, f.b)[:len(names)], a64, a32)
    assert torch.equal(f.s, f.p.to(torch.bfloat16)), "shadow != bf16(p)"


@pytest.mark.parametrize("grad_scale", [1.0, 0.25, 1.0 / 3.0])
@pytest.mark.parametrize("entry", ["step", "runs"])
@pytest.mark.parametrize("kind", ["sgd", "adamw"])
def test_coef_one_is_bit_equal_to_the_plain_entry_points(kind, entry, grad_scale):
    """A max_norm far above the norm: coef == 1 in every step, and p, the moments and the shadow equal the plain
    entry points' bit for bit, also at a grad_scale that is no power of two (3 ranks)."""
    p0, grads, lrs, _, _, _, _ = case(kind, 4099)
    runs = [(0, 1025, None, 0), (1028, 4099, None, 0)]
    a, b = Flat(kind, p0), Flat(kind, p0)
    for t in range(3):
        for f in (a, b):
            f.g.copy_(grads[t])
            f.lr.fill_(lrs[t])
        a.step(runs, entry, max_norm=None, grad_scale=grad_scale, first=(t == 0))
        b.step(runs, entry, max_norm=1e6, grad_scale=grad_scale, first=(t == 0))
        assert float(b.pair[1]) == 1.0 and float(b.pair[0]) > 0
    torch.cuda.synchronize()
    for x, y, name in zip(a.state(), b.state(), ("p", "state a", "state b", "shadow", "counters")):
        assert torch.equal(x, y), name
    assert not torch.equal(a.p.cpu(), p0)


@pytest.mark.parametrize("kind", ["sgd", "adamw"])
def test_gates(kind):
    """Two runs, the second gated.  Flag 0: the norm is the first run's alone (the gated run's gradient is NaN and is
    not read) and the gated run's p, state and shadow stay bit-identical.  Flag 1: both runs count."""
    n = 3080
    gen = torch.Generator().manual_seed(21)
    p0 = torch.randn(n, generator=gen)
    g = 1e-2 * torch.randn(n, generator=gen)
    gate = torch.zeros(1, device=DEV)
    runs = [(0, 1025, None, 0), (1028, 3077, gate, 1)]
    sq = [float((g[s:e].double() ** 2).sum()) for s, e, _, _ in runs]
    f = Flat(kind, p0, nclass=2)
    before = f.state()
    f.g.copy_(g)
    f.g[1028:3077] = float("nan")
    f.lr.fill_(1e-3)
    max_norm = 0.5 * math.sqrt(sq[0])
    f.step(runs, "runs", max_norm=max_norm, first=True)
    torch.cuda.synchronize()
    check_norm(f"{kind} gate 0", f.pair, math.sqrt(sq[0]), max_norm)
    after = f.state()
    for x, y in zip(before[:4], after[:4]):
        assert torch.equal(x[1025:], y[1025:]), "a gated-off run changed state"
    assert not torch.equal(before[0][:1025], after[0][:1025]) and torch.isfinite(f.p).all()
    gate.fill_(1.0)
    f.g.copy_(g)
    f.step(runs, "runs", max_norm=max_norm)
    torch.cuda.synchronize()
    check_norm(f"{kind} gate 1", f.pair, math.sqrt(sq[0] + sq[1]), max_norm)
    assert not torch.equal(f.p[1028:3077].cpu(), p0[1028:3077])
    assert torch.equal(f.p[1025:1028].cpu(), p0[1025:1028]) and torch.equal(f.p[3077:].cpu(), p0[3077:])


@pytest.mark.parametrize("kind", ["sgd", "adamw"])
def test_zero_gradient(kind):
    """norm 0, coef 1, and the weight decay still acts."""
    n, lr = 1025, 1e-2
    p0 = torch.randn(n, generator=torch.Generator().manual_seed(4))
    f = Flat(kind, p0)
    f.lr.fill_(lr)
    f.step([(0, n, None, 0)], "runs", max_norm=1.0, first=True)
    torch.cuda.synchronize()
    print(f"{kind} zero gradient: {f.pair.tolist()}")
    assert f.pair.tolist() == [0.0, 1.0]
    want = p0.double() * (1 - lr * WD)
    err = float((f.p.cpu().double() - want).abs().max())
    print(f"{kind} decay err {err:.3e}")
    assert err <= 2.0 ** -22 * float(want.abs().max()) and not torch.equal(f.p.cpu(), p0)


@pytest.mark.parametrize("kind", ["sgd", "adamw"])
def test_fold_runs_launch_equals_per_run_launches(kind):
    """grad_scale 0.25 with the bf16 bucket copy (the fp32 gradient is NaN and must not be read): five runs with two
    gated classes, one off, through the runs launch and through one launch per run, bit for bit over two steps; the
    norm is that of 0.25 * the bf16 sum over the open runs."""
    n = 8216
    gen = torch.Generator().manual_seed(5)
    p0 = torch.randn(n, generator=gen)
    on, off = torch.ones(1, device=DEV), torch.zeros(1, device=DEV)
    runs = [(0, 4, None, 0), (4, 9, on, 1), (12, 2059, off, 2), (2060, 4109, on, 1), (4112, 8211, None, 0)]
    a, b = Flat(kind, p0, 3), Flat(kind, p0, 3)
    for t in range(2):
        g = 1e-2 * torch.randn(n, generator=gen)
        gb = g.to(torch.bfloat16)
        ref = 0.25 * math.sqrt(sum(float((gb[s:e].double() ** 2).sum()) for s, e, gate, _ in runs if gate is not off))
        for f in (a, b):
            f.g.fill_(float("nan"))
            f.lr.fill_(lr_at(t))
        a.step(runs, "step", max_norm=0.5 * ref, grad_scale=0.25, grad_bf16=gb.to(DEV), first=(t == 0))
        b.step(runs, "runs", max_norm=0.5 * ref, grad_scale=0.25, grad_bf16=gb.to(DEV), first=(t == 0))
        check_norm(f"{kind} fold step {t}", b.pair, ref, 0.5 * ref)
        assert torch.equal(a.pair, b.pair) and float(b.pair[1]) < 1.0
    torch.cuda.synchronize()
    for x, y, name in zip(a.state(), b.state(), ("p", "state a", "state b", "shadow", "counters")):
        assert torch.equal(x, y), name
    assert torch.isfinite(b.p).all()
    for s, e in ((9, 12), (12, 2059), (2059, 2060), (4109, 4112), (8211, n)):     # gaps and the gated-off run
        assert torch.equal(b.p[s:e].cpu(), p0[s:e]) and not b.a[s:e].any()
    assert not torch.equal(b.p[2060:4109].cpu(), p0[2060:4109])


@pytest.mark.parametrize("kind", ["sgd", "adamw"])
@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
def test_non_finite_norm_propagates_as_in_torch(bad, kind):
    """One NaN / Inf element: clip_grad_norm_ (error_if_nonfinite=False) gets norm NaN -> coef NaN and every gradient
    element NaN, or norm Inf -> coef 0 and Inf * 0 = NaN at that element, 0 elsewhere; the device does the same."""
    n = 1025
    gen = torch.Generator().manual_seed(8)
    p0, g = torch.randn(n, generator=gen), 1e-2 * torch.randn(n, generator=gen)
    g[7] = bad
    tp = torch.nn.Parameter(p0.clone())
    tp.grad = g.clone()
    tnorm = float(torch.nn.utils.clip_grad_norm_([tp], 1.0, error_if_nonfinite=False))
    f = Flat(kind, p0)
    f.g.copy_(g)
    f.lr.fill_(1e-3)
    f.step([(0, n, None, 0)], "runs", max_norm=1.0, first=True)
    torch.cuda.synchronize()
    norm, coef = f.pair.tolist()
    print(f"{kind} {bad}: device {{norm, coef}} {norm} {coef}; torch norm {tnorm} clipped grad NaNs "
          f"{int(torch.isnan(tp.grad).sum())}; device p NaNs {int(torch.isnan(f.p).sum())}")
    if math.isnan(bad):
        assert math.isnan(tnorm) and math.isnan(norm) and math.isnan(coef)
    else:
        assert math.isinf(tnorm) and math.isinf(norm) and coef == 0.0
    assert torch.equal(torch.isnan(f.p).cpu(), torch.isnan(tp.grad))     # p turns NaN exactly where torch's grad did
    assert bool(torch.isnan(f.p[7]))


# ---- the optimizer classes --------------------------------------------------------------------------------------
def _toy(kind, max_grad_norm):
    torch.manual_seed(0)
    m = torch.nn.Sequential(torch.nn.Linear(33, 65), torch.nn.Linear(65, 7)).to(DEV)
    store = ParamStore(m, torch.bfloat16)
    if kind == "adamw":
        return store, FusedAdamW(store, 1e-3, betas=(B1, B2), eps=EPS, weight_decay=WD, max_grad_norm=max_grad_norm)
    return store, FusedSGD(store, 1e-3, MOM, WD, max_grad_norm=max_grad_norm)


@pytest.mark.parametrize("kind", ["sgd", "adamw"])
def test_captured_step_takes_a_fresh_norm_at_every_replay(kind):
    """store.grad.copy_(g_static); opt.step() captured once with clipping on and replayed with three gradients (two
    clipped, one not) equals three eager steps bit for bit, opt.grad_norm included, with no host call in between."""
    gen = torch.Generator().manual_seed(9)
    se, oe = _toy(kind, 0.3)
    gs = [(sc * 1e-2 * torch.randn(se.numel, generator=gen)).to(DEV) for sc in (1.0, 0.25, 2.0)]
    want = []
    for t, g in enumerate(gs):
        oe.set_lr(lr_at(t))
        se.grad.copy_(g)
        oe.step(first=False)
        want.append(oe.grad_norm.clone())
    sg, og = _toy(kind, 0.3)
    pair_ptr = og.grad_norm.data_ptr()
    g_static = torch.zeros_like(gs[0])
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            sg.grad.copy_(g_static)
            og.step(first=False)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    got = []
    for t, g in enumerate(gs):
        og.set_lr(lr_at(t))
        g_static.copy_(g)
        graph.replay()
        got.append(og.grad_norm.clone())          # a device copy on the stream: no host call between replays
    torch.cuda.synchronize()
    print(f"{kind} captured {[x.tolist() for x in got]} eager {[x.tolist() for x in want]}")
    assert og.grad_norm.data_ptr() == pair_ptr
    for x, y in zip(got, want):
        assert torch.equal(x, y)
    coefs = [float(x[1]) for x in got]
    assert coefs[0] < 1.0 and coefs[1] == 1.0 and coefs[2] < 1.0, coefs
    assert torch.equal(sg.flat, se.flat) and torch.equal(sg.shadow, se.shadow)
    st = (og.exp_avg, oe.exp_avg) if kind == "adamw" else (og.buf, oe.buf)
    assert torch.equal(*st)
    assert not torch.equal(sg.flat, _toy(kind, None)[0].flat)


class _Striped(torch.nn.Module):
    """70 small layers whose parameters alternate between two skip flags: no two neighbours share a run."""

    def __init__(self):
        super().__init__()
        torch.manual_seed(1)
        self.layers = torch.nn.ModuleList([torch.nn.Linear(5 + i % 3, 7, bias=False) for i in range(70)])
        self.flags = [torch.ones(1, device=DEV), torch.ones(1, device=DEV)]

    def param_gates(self):
        return [([l.weight for l in self.layers[k::2]], self.flags[k]) for k in (0, 1)]


@pytest.mark.parametrize("kind", ["sgd", "adamw"])
def test_optimizer_with_more_than_64_runs(kind):
    """70 runs: the optimizer takes the norm in two chunks (two slabs) and one _clip launch per run.  Against the
    same state stepped through the entry points by hand — norm in chunks, the runs-form _clip launches in chunks of
    64 — bit for bit, and the norm against float64."""
    def make():
        m = _Striped().to(DEV)
        store = ParamStore(m, torch.bfloat16)
        opt = FusedAdamW(store, 1e-3, betas=(B1, B2), eps=EPS, weight_decay=WD, max_grad_norm=0.05) \
            if kind == "adamw" else FusedSGD(store, 1e-3, MOM, WD, max_grad_norm=0.05)
        return m, store, opt
    ma, sa, oa = make()
    mb, sb, ob = make()
    g = torch.zeros(sa.numel)
    gen = torch.Generator().manual_seed(6)
    for i in range(len(sa.params)):                  # the alignment gaps stay zero, as in training
        s, e = sa.span(i)
        g[s:e] = 1e-2 * torch.randn(e - s, generator=gen)
    ref = float(g.double().norm())
    for st in (sa, sb):
        st.grad.copy_(g.to(DEV))
    oa.step(first=False)
    gates = [x for x in sb.gate]
    if kind == "adamw":
        runs = [(s, e, ob.gates[c], c) for s, e, c in sb.touched_runs(also=ob.cls, every=True)]
    else:
        key = [id(x) for x in gates]
        byid = {id(x): x for x in gates}
        runs = [(s, e, byid[k], False) for s, e, k in sb.touched_runs(also=key, every=True)]
    assert len(runs) == 70 and oa._partials.numel() == 2 * PARTIALS
    part, pair = slab(2), torch.zeros(2, device=DEV)
    K.grad_clip_coef(part, K.grad_sqnorm_runs(sb.grad, [r[:3] for r in runs], part), 0.05, pair)
    if kind == "adamw":
        K.adamw_prelude(ob.counters, ob.corr, [(c, ob.gates[c]) for c in sorted({r[3] for r in runs})], B1, B2)
    for k in (0, 64):
        if kind == "adamw":
            K.adamw_step_runs(sb.flat, sb.grad, ob.exp_avg, ob.exp_avg_sq, sb.shadow, runs[k:k + 64], B1, B2, EPS, WD,
                              ob.lr_dev, ob.corr, clip_coef=pair[1:2])
        else:
            K.sgd_step_runs(sb.flat, sb.grad, ob.buf, sb.shadow, runs[k:k + 64], MOM, WD, ob.lr_dev,
                            clip_coef=pair[1:2])
    torch.cuda.synchronize()
    print(f"{kind} 70 runs: optimizer {oa.grad_norm.tolist()} by hand {pair.tolist()} float64 norm {ref:.9e}")
    check_norm(f"{kind} 70 runs", oa.grad_norm, ref, 0.05)
    assert torch.equal(oa.grad_norm, pair) and float(pair[1]) < 1.0
    assert torch.equal(sa.flat, sb.flat) and torch.equal(sa.shadow, sb.shadow)
    sta, stb = ((oa.exp_avg, oa.exp_avg_sq), (ob.exp_avg, ob.exp_avg_sq)) if kind == "adamw" else ((oa.buf,), (ob.buf,))
    assert all(torch.equal(x, y) for x, y in zip(sta, stb))
    assert not torch.equal(sa.flat, make()[1].flat)


@pytest.mark.parametrize("kind", ["sgd", "adamw"])
def test_per_run_launches_of_the_optimizer_equal_the_runs_launch(kind, monkeypatch):
    """optim._RUNS False: a clipped step goes through one _clip launch per run and gives the bits
    of the one-launch form."""
    from deepfake_amd import optim
    gen = torch.Generator().manual_seed(12)
    sa, oa = _toy(kind, 0.3)
    sb, ob = _toy(kind, 0.3)
    g = (1e-2 * torch.randn(sa.numel, generator=gen)).to(DEV)
    sa.grad.copy_(g)
    oa.step(first=False)
    monkeypatch.setattr(optim, "_RUNS", False)
    calls = []
    one = K.adamw_step if kind == "adamw" else K.sgd_step
    monkeypatch.setattr(K, "adamw_step" if kind == "adamw" else "sgd_step",
                        lambda *a, **k: (calls.append(k.get("clip_coef") is not None), one(*a, **k))[1])
    sb.grad.copy_(g)
    ob.step(first=False)
    torch.cuda.synchronize()
    assert calls and all(calls), calls
    assert torch.equal(oa.grad_norm, ob.grad_norm) and float(ob.grad_norm[1]) < 1.0
    assert torch.equal(sa.flat, sb.flat) and torch.equal(sa.shadow, sb.shadow)


@pytest.mark.parametrize("kind", ["sgd", "adamw"])
def test_max_grad_norm_none_issues_the_plain_launches(kind):
    """Without clipping the optimizer holds no clip state and steps to the bits of an optimizer built without the
    argument."""
    gen = torch.Generator().manual_seed(2)
    sa, oa = _toy(kind, None)
    torch.manual_seed(0)
    m = torch.nn.Sequential(torch.nn.Linear(33, 65), torch.nn.Linear(65, 7)).to(DEV)
    sb = ParamStore(m, torch.bfloat16)
    ob = FusedAdamW(sb, 1e-3, betas=(B1, B2), eps=EPS, weight_decay=WD) if kind == "adamw" else \
        FusedSGD(sb, 1e-3, MOM, WD)
    g = (1e-2 * torch.randn(sa.numel, generator=gen)).to(DEV)
    for s, o in ((sa, oa), (sb, ob)):
        s.grad.copy_(g)
        o.step()
    torch.cuda.synchronize()
    assert oa.grad_norm is None and oa._partials is None
    assert torch.equal(sa.flat, sb.flat) and torch.equal(sa.shadow, sb.shadow)


def _c1_run(kind, graph, max_grad_norm):
    from deepfake_amd.ddp import GradBucketer
    from deepfake_amd.models.fused import build_fused
    from deepfake_amd.trainer import TrainStep
    c = GC.FUSED_C1
    m = named_fill_(build_fused("c1", compute_dtype=torch.float32), c["seed"]).to(DEV)
    m.train()
    store = ParamStore(m, torch.float32)
    if kind == "adamw":
        opt = FusedAdamW(store, 1e-4, weight_decay=0.05, max_grad_norm=max_grad_norm)
    else:
        opt = FusedSGD(store, 0.01, 0.9, 0.05, max_grad_norm=max_grad_norm)
    step = TrainStep(m, store, opt, GradBucketer(store), graph=graph)
    losses, pairs = [], []
    for i in range(3):
        v, mel, w, lab = synthetic_inputs(c["B"], c["T"], c["H"], c["W"], c["seconds"], seed=c["seed"] + 10 * i)
        loss, _ = step((v.to(DEV), mel.to(DEV), w.to(DEV)), lab.to(DEV))
        losses.append(float(loss))
        pairs.append(opt.grad_norm.tolist())
    torch.cuda.synchronize()
    state = opt.exp_avg_sq.clone() if kind == "adamw" else store.flat.clone()
    return losses, state, pairs, step


C1_MAX_NORM = 1e-2


@pytest.mark.parametrize("kind", ["sgd", "adamw"])
def test_whole_step_graph_matches_eager(kind):
    """TrainStep at the C1 fixture (fp32 parity mode), 3 steps with clipping active in each, graph against eager.
    SGD: the parameters; AdamW: exp_avg_sq (Adam's first update is lr sign(g), so an element whose gradient is
    atomics-order noise may move by 2 lr between any two runs).  Bar, as tests/test_gpu_adamw.py's whole-step test: the
    larger of 1e-5 and twice the distance of two identical eager runs, on the losses, on the state (relative to its
    largest element); the norms of the two forms agree within 1e-5 relative outright."""
    la, sa, pa, _ = _c1_run(kind, False, C1_MAX_NORM)
    lb, sb, pb, _ = _c1_run(kind, False, C1_MAX_NORM)
    lg, sg, pg, step = _c1_run(kind, True, C1_MAX_NORM)
    assert step.graph is not None and step.graph_mode, "the step was not captured"

    def dist(l1, s1, p1):
        return (max(abs(x - y) for x, y in zip(l1, la)), float((s1 - sa).abs().max() / sa.abs().max()),
                max(abs(x[0] - y[0]) / y[0] for x, y in zip(p1, pa)))
    ee, ge = dist(lb, sb, pb), dist(lg, sg, pg)
    bars = [max(1e-5, 2 * d) for d in ee[:2]] + [1e-5]        # the norm: 1e-5 relative outright
    print(f"{kind}: losses {la} graph {lg}; {{norm, coef}} eager {pa} graph {pg}; (loss, state rel, norm rel) "
          f"eager-eager {ee} graph-eager {ge} bars {bars}")
    assert all(math.isfinite(x) for x in lg) and float(sa.abs().max()) > 0
    assert all(0 < p[1] < 1 for p in pa + pg), "clipping was not active in every step"
    assert all(d <= b for d, b in zip(ge, bars)), (ge, bars)


def test_trainer_passes_the_flag_and_logs_the_norm():
    """Trainer with --clip_grad_norm: the optimizer clips, and the train line of a log step ends in the device norm;
    with the default 0 the optimizer holds no clip state."""
    import types
    from deepfake_amd.models.fused import build_fused
    from deepfake_amd.trainer import Trainer
    c = GC.FUSED_C1

    class OneBatch:
        def __init__(self):
            v, mel, wave, label = synthetic_inputs(c["B"], c["T"], c["H"], c["W"], c["seconds"], seed=c["seed"] + 1)
            self.batch = ({"Video": v, "Audio": mel, "PAudio": [w.numpy() for w in wave]}, label)

        def train_dataloader(self):
            return [self.batch]

        def val_dataloader(self):
            return None

    def args(**kw):
        a = dict(epochs=0, learning_rate=0.01, batch_size=2, modality="fused", model_save=0, log_step=1, accum_step=1,
                 l2_decacy=0.05, dtype="fp32", bucket_mb=64.0, soft=0.01, classify_drop=0.0, swin_drop=0.0)
        a.update(kw)
        return types.SimpleNamespace(**a)
    for opt in ("sgd", "adamw"):
        off = Trainer(named_fill_(build_fused("c1", compute_dtype=torch.float32), c["seed"]), args(optimizer=opt),
                      torch.device(DEV), OneBatch(), compute_dtype=torch.float32)
        assert off.optimizer.max_grad_norm is None and off.optimizer.grad_norm is None
    lines = []
    tr = Trainer(named_fill_(build_fused("c1", compute_dtype=torch.float32), c["seed"]),
                 args(optimizer="adamw", clip_grad_norm=C1_MAX_NORM), torch.device(DEV), OneBatch(),
                 logger=lines.append, compute_dtype=torch.float32)
    assert tr.optimizer.max_grad_norm == C1_MAX_NORM
    tr.train()
    torch.cuda.synchronize()
    norm, coef = tr.optimizer.grad_norm.tolist()
    train_lines = [ln for ln in lines if "Train Loss Avg" in ln]
    print(train_lines, norm, coef)
    assert len(train_lines) == 1 and train_lines[0].endswith("| grad norm {:.4E}".format(norm))
    assert math.isfinite(norm) and 0 < coef < 1
