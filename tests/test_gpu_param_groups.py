"""GPU: parameter groups in the fused optimizers (dfk_sgd_step_runs_groups / dfk_adamw_step_runs_groups,
optim.ParamGroups, FusedSGD / FusedAdamW with groups=).

One flat buffer laid out as a ParamStore lays it out (every tensor on a multiple of 8 elements, zero padding behind
it) with the tensor sizes SIZES; with the run table RUNS the second run starts at the 2048-element tensor, so that
tensor ends at a workgroup edge of its run, the 1016 / 1032 pair puts a group boundary 8 elements before the
1024-element half-block of the next workgroup, the 2500 tensor spans two workgroups and the last tensor ends the run
in an n % 4 tail; the first run ends in the 3-element tensor whose group differs from both neighbours.  Tensor k is in
group k % 3 of HYPER, so no two neighbours share a group.

Bit-for-bit tests compare with the plain entry points (one group: dfk_*_step_runs; several: one dfk_*_step per
tensor with lr_dev = fp32(lr) * fp32(mult) and that group's decay).  The torch test uses the bar of
tests/test_gpu_adamw.py: max|kernel - a64| <= 2 d_ref + 2^-23 max|a64| per state tensor, d_ref = max|a32 - a64| of
torch.optim on the CPU with three param groups.  Every test prints its figures before it asserts."""
import functools
import math

import pytest
import torch

import golden_cases as GC
from oracle.fill import named_fill_, synthetic_inputs
from test_gpu_adamw import B1, B2, EPS, STEPS, WD, lr_at

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from deepfake_amd import kernels as K
    from deepfake_amd.optim import FusedAdamW, FusedSGD, ParamGroups
    from deepfake_amd.params import ParamStore

DEV = "cuda"
MOM = 0.9
SIZES = [1, 8, 96, 1000, 3, 2048, 1016, 1032, 2500, 5]
SPANS, _o = [], 0
for _n in SIZES:
    SPANS.append((_o, _o + _n))
    _o += -(-_n // 8) * 8
N = _o                                                  # 7728
RUNS = [(0, SPANS[4][1]), (SPANS[5][0], SPANS[9][1])]   # (0, 1115), (1120, 7725)
ONE_RUN = [(0, SPANS[9][1])]                            # the padding elements lie inside the run
HYPER = [(1.0, WD), (1.0, 0.0), (10.0, WD)]
GROUP_OF = [k % 3 for k in range(len(SIZES))]
MAX_NORM = 0.1                                          # the gradients' norm is about 0.9: this clips


def test_layout_is_the_one_the_docstring_describes():
    assert N == 7728 and RUNS == [(0, 1115), (1120, 7725)]
    rel = [(s - 1120, e - 1120) for s, e in SPANS[5:]]
    assert rel[0] == (0, 2048) and rel[1] == (2048, 3064) and rel[2] == (3064, 4096)
    assert rel[3] == (4096, 6596) and rel[4] == (6600, 6605) and 6605 % 4 == 1 and 1115 % 4 == 3
    assert all(GROUP_OF[k] != GROUP_OF[k + 1] for k in range(len(SIZES) - 1))


def group_map(group_of=GROUP_OF):
    m = torch.zeros(N // 8, dtype=torch.uint8)
    for (s, e), g in zip(SPANS, group_of):
        m[s // 8:-(-e // 8)] = g
    return m.to(DEV)


def hyper(pairs=HYPER):
    return torch.tensor(pairs, dtype=torch.float32, device=DEV)


@functools.lru_cache(maxsize=None)
def inputs():
    """p0 = randn and STEPS gradients 1e-2 randn on the tensors' elements, zero on the padding; never modified."""
    gen = torch.Generator().manual_seed(77)
    mask = torch.zeros(N)
    for s, e in SPANS:
        mask[s:e] = 1
    p0 = torch.randn(N, generator=gen) * mask
    return p0, [1e-2 * torch.randn(N, generator=gen) * mask for _ in range(STEPS)]


class Bufs:
    """p, gradient, first state (momentum / exp_avg), second state (exp_avg_sq), bf16 shadow"""

    def __init__(self):
        self.p = inputs()[0].to(DEV).clone()
        self.g, self.a, self.v = torch.zeros_like(self.p), torch.zeros_like(self.p), torch.zeros_like(self.p)
        self.s = self.p.to(torch.bfloat16)
        self.gb = None

    def load(self, g, bf16):
        """this step's gradient: fp32, or the bf16 copy with the fp32 buffer NaN (it must not be read)"""
        g = g.to(DEV)
        self.gb = g.to(torch.bfloat16) if bf16 else None
        self.g.copy_(torch.full_like(g, float("nan")) if bf16 else g)

    def state(self):
        return {"p": self.p, "a": self.a, "v": self.v, "shadow": self.s}


class Dev:
    """The device scalars both sides of a comparison share: lr, AdamW's counters / corrections, the clip pair"""

    def __init__(self, nclass=1):
        self.lr = torch.zeros(1, device=DEV)
        self.counters = torch.zeros(nclass, device=DEV, dtype=torch.int32)
        self.corr = torch.zeros(2 * nclass, device=DEV)
        self.part = torch.zeros(K.GNORM_PARTIALS, device=DEV, dtype=torch.float64)
        self.pair = torch.zeros(2, device=DEV)

    def clip(self, b, runs, grad_scale):
        """the global coefficient of this step's runs [(s, e, gate, x)], as the optimizers compute it"""
        n = K.grad_sqnorm_runs(b.g, [(s, e, g) for s, e, g, _ in runs], self.part, grad_scale=grad_scale,
                               grad_bf16=b.gb)
        K.grad_clip_coef(self.part, n, MAX_NORM, self.pair)
        return self.pair[1:2]


def step_groups(opt, b, d, runs, gmap, hy, grad_scale=1.0, clip=None):
    """runs [(s, e, gate, first | class)] through the groups entry point"""
    if opt == "sgd":
        K.sgd_step_runs_groups(b.p, b.g, b.a, b.s, runs, MOM, d.lr, gmap, hy, grad_scale=grad_scale, grad_bf16=b.gb,
                               clip_coef=clip)
    else:
        K.adamw_step_runs_groups(b.p, b.g, b.a, b.v, b.s, runs, B1, B2, EPS, d.lr, d.corr, gmap, hy,
                                 grad_scale=grad_scale, grad_bf16=b.gb, clip_coef=clip)


def step_plain(opt, b, d, runs, wd, grad_scale=1.0, clip=None):
    ck = {} if clip is None else {"clip_coef": clip}
    if opt == "sgd":
        K.sgd_step_runs(b.p, b.g, b.a, b.s, runs, MOM, wd, d.lr, grad_scale=grad_scale, grad_bf16=b.gb, **ck)
    else:
        K.adamw_step_runs(b.p, b.g, b.a, b.v, b.s, runs, B1, B2, EPS, wd, d.lr, d.corr, grad_scale=grad_scale,
                          grad_bf16=b.gb, **ck)


def step_per_tensor(opt, b, d, runs, grad_scale=1.0, clip=None, group_of=GROUP_OF):
    """One plain one-run launch per tensor, with its run's gate and first flag / class, its group's decay and
    lr_dev = fp32(lr) * fp32(mult)."""
    ck = {} if clip is None else {"clip_coef": clip}
    for (s, e), g in zip(SPANS, group_of):
        gate, x = next((gate, x) for rs, re, gate, x in runs if rs <= s and e <= re)
        mult, wd = HYPER[g]
        lr = d.lr * torch.tensor(mult, dtype=torch.float32, device=DEV)
        gb = b.gb[s:e] if b.gb is not None else None
        if opt == "sgd":
            K.sgd_step(b.p[s:e], b.g[s:e], b.a[s:e], b.s[s:e], 0.0, MOM, wd, bool(x), lr_dev=lr, gate=gate,
                       grad_scale=grad_scale, grad_bf16=gb, **ck)
        else:
            K.adamw_step(b.p[s:e], b.g[s:e], b.a[s:e], b.v[s:e], b.s[s:e], 0.0, B1, B2, EPS, wd,
                         d.corr[2 * x:2 * x + 2], lr_dev=lr, gate=gate, grad_scale=grad_scale, grad_bf16=gb, **ck)


def table(opt, runs, t, gates=None, classes=None):
    """[(s, e, gate, first | class)]: SGD takes its first momentum step at t == 0"""
    return [(s, e, gates[i] if gates else None, (t == 0) if opt == "sgd" else (classes[i] if classes else 0))
            for i, (s, e) in enumerate(runs)]


def assert_same(x, y, what):
    diff = {k: int((x.state()[k] != y.state()[k]).sum()) for k in x.state()}
    print(f"{what}: elements that differ {diff}")
    assert not any(diff.values()), (what, diff)
    for k in x.state():
        assert torch.equal(x.state()[k], y.state()[k]), (what, k)     # NaN-safe: != counts NaN, equal rejects it


@pytest.mark.parametrize("fold", [(1.0, False), (0.5, True)], ids=["fp32", "bf16x0.5"])
@pytest.mark.parametrize("clip", [False, True], ids=["noclip", "clip"])
@pytest.mark.parametrize("opt", ["sgd", "adamw"])
def test_one_group_equals_plain(opt, clip, fold):
    """Every tensor in group (1.0, WD): 6 steps, cosine lr, bit-equal to dfk_*_step_runs (its _clip twin)."""
    scale, bf16 = fold
    gmap, hy = group_map([0] * len(SIZES)), hyper([(1.0, WD)])
    x, y, d = Bufs(), Bufs(), Dev()
    for t, g in enumerate(inputs()[1]):
        d.lr.fill_(lr_at(t))
        runs = table(opt, RUNS, t)
        for b in (x, y):
            b.load(g, bf16)
        coef = d.clip(x, runs, scale) if clip else None
        if opt == "adamw":
            K.adamw_prelude(d.counters, d.corr, [(0, None)], B1, B2)
        step_groups(opt, x, d, runs, gmap, hy, scale, coef)
        step_plain(opt, y, d, runs, WD, scale, coef)
    torch.cuda.synchronize()
    if clip:
        print(f"norm, coef of the last step: {d.pair.tolist()}")
        assert 0 < float(d.pair[1]) < 1, "max_norm does not clip"
    assert_same(x, y, f"{opt} clip={clip} fold={fold}")
    assert torch.isfinite(x.p).all() and not torch.equal(x.p.cpu(), inputs()[0])
    assert torch.equal(x.s, x.p.to(torch.bfloat16))


@pytest.mark.parametrize("runs", [RUNS, ONE_RUN], ids=["two_runs", "one_run"])
@pytest.mark.parametrize("clip", [False, True], ids=["noclip", "clip"])
@pytest.mark.parametrize("opt", ["sgd", "adamw"])
def test_groups_equal_per_group_plain_runs(opt, clip, runs):
    """The interleaved layout, 6 steps: the whole flat state, padding included, is bit-equal to one plain one-run
    launch per tensor at fp32(lr) * fp32(mult) and its group's decay; with clipping on, one global coefficient."""
    gmap, hy = group_map(), hyper()
    x, y, d = Bufs(), Bufs(), Dev()
    for t, g in enumerate(inputs()[1]):
        d.lr.fill_(lr_at(t))
        tab = table(opt, runs, t)
        for b in (x, y):
            b.load(g, False)
        coef = d.clip(x, tab, 1.0) if clip else None
        if opt == "adamw":
            K.adamw_prelude(d.counters, d.corr, [(0, None)], B1, B2)
        step_groups(opt, x, d, tab, gmap, hy, 1.0, coef)
        step_per_tensor(opt, y, d, tab, 1.0, coef)
    torch.cuda.synchronize()
    assert_same(x, y, f"{opt} clip={clip} runs={len(runs)}")
    pad = torch.ones(N, dtype=torch.bool)
    for s, e in SPANS:
        pad[s:e] = False
    for k, v in x.state().items():
        assert not v.cpu()[pad].float().any(), f"{k}: a padding element left 0"
    # the groups act: against the same steps with every tensor in group 0, exactly the tensors of groups 1, 2 differ
    z = Bufs()
    d2 = Dev()
    for t, g in enumerate(inputs()[1]):
        d2.lr.fill_(lr_at(t))
        z.load(g, False)
        tab = table(opt, runs, t)
        coef = d2.clip(z, tab, 1.0) if clip else None
        if opt == "adamw":
            K.adamw_prelude(d2.counters, d2.corr, [(0, None)], B1, B2)
        step_groups(opt, z, d2, tab, group_map([0] * len(SIZES)), hy, 1.0, coef)
    for (s, e), g in zip(SPANS, GROUP_OF):
        assert torch.equal(z.p[s:e], x.p[s:e]) == (g == 0), (s, e, g)


@functools.lru_cache(maxsize=None)
def torch_reference(opt, dtype):
    """torch.optim.SGD / AdamW on the CPU in `dtype` with the three param groups: the states over the tensors'
    elements, concatenated, (p, momentum) or (p, exp_avg, exp_avg_sq)."""
    p0, grads = inputs()
    ps = [torch.nn.Parameter(p0[s:e].to(dtype).clone()) for s, e in SPANS]
    pgs = [{"params": [p for p, g in zip(ps, GROUP_OF) if g == k], "lr": lr_at(0) * mult, "weight_decay": wd}
           for k, (mult, wd) in enumerate(HYPER)]
    o = torch.optim.SGD(pgs, lr=lr_at(0), momentum=MOM) if opt == "sgd" else \
        torch.optim.AdamW(pgs, lr=lr_at(0), betas=(B1, B2), eps=EPS)
    for t, g in enumerate(grads):
        for pg, (mult, _) in zip(o.param_groups, HYPER):
            pg["lr"] = lr_at(t) * mult
        for p, (s, e) in zip(ps, SPANS):
            p.grad = g[s:e].to(dtype).clone()
        o.step()
    keys = ("momentum_buffer",) if opt == "sgd" else ("exp_avg", "exp_avg_sq")
    return (torch.cat([p.detach() for p in ps]),) + tuple(torch.cat([o.state[p][k] for p in ps]) for k in keys)


@pytest.mark.parametrize("opt", ["sgd", "adamw"])
def test_against_torch(opt):
    """6 steps of the interleaved layout against torch.optim with three param groups, at the bar of the module
    docstring."""
    a64, a32 = torch_reference(opt, torch.float64), torch_reference(opt, torch.float32)
    gmap, hy = group_map(), hyper()
    x, d = Bufs(), Dev()
    for t, g in enumerate(inputs()[1]):
        d.lr.fill_(lr_at(t))
        x.load(g, False)
        if opt == "adamw":
            K.adamw_prelude(d.counters, d.corr, [(0, None)], B1, B2)
        step_groups(opt, x, d, table(opt, RUNS, t), gmap, hy)
    torch.cuda.synchronize()
    got = [torch.cat([v.cpu()[s:e] for s, e in SPANS]) for v in ((x.p, x.a) if opt == "sgd" else (x.p, x.a, x.v))]
    bad = []
    for name, k, t64, t32 in zip(("p", "state1", "state2"), got, a64, a32):
        d_ref = float((t32.double() - t64).abs().max())
        err = float((k.double() - t64).abs().max())
        bar = 2 * d_ref + 2.0 ** -23 * float(t64.abs().max())
        print(f"{opt} {name}: err {err:.3e} d_ref {d_ref:.3e} bar {bar:.3e} ratio {err / d_ref if d_ref else 0:.3f}")
        if not err <= bar:
            bad.append((name, err, bar))
    assert not bad, bad
    assert torch.equal(x.s, x.p.to(torch.bfloat16))


@pytest.mark.parametrize("opt", ["sgd", "adamw"])
def test_gates_and_classes(opt):
    """An ungated run and two gated runs of one class, groups crossing all three.  Step 1 with the flag 0 leaves the
    gated runs' p, states and shadow, and the class counter, bit-identical; with the flag 1 in steps 2 and 3 the
    whole state equals the per-tensor construction."""
    runs = [RUNS[0], (SPANS[5][0], SPANS[6][1]), (SPANS[7][0], SPANS[9][1])]
    gate = torch.zeros(1, device=DEV)
    gates, classes = [None, gate, gate], [0, 1, 1]
    gmap, hy = group_map(), hyper()
    x, y, d = Bufs(), Bufs(), Dev(nclass=2)
    before = {k: v.clone() for k, v in x.state().items()}
    for t, g in enumerate(inputs()[1][:3]):
        gate.fill_(0.0 if t == 0 else 1.0)
        d.lr.fill_(lr_at(t))
        for b in (x, y):
            b.load(g, False)
        # SGD: the ungated run takes its first step at t = 0, the gated ones at their first open step
        tab = [(s, e, gt, (t == (0 if gt is None else 1)) if opt == "sgd" else c)
               for (s, e), gt, c in zip(runs, gates, classes)]
        if opt == "adamw":
            K.adamw_prelude(d.counters, d.corr, [(0, None), (1, gate)], B1, B2)
        step_groups(opt, x, d, tab, gmap, hy)
        step_per_tensor(opt, y, d, tab)
        if t == 0:
            torch.cuda.synchronize()
            s = runs[1][0]
            for k, v in x.state().items():
                assert torch.equal(v[s:], before[k][s:]), f"a gated-off step changed {k}"
            assert not torch.equal(x.p[:s], before["p"][:s])
            if opt == "adamw":
                assert d.counters.tolist() == [1, 0]
    torch.cuda.synchronize()
    if opt == "adamw":
        assert d.counters.tolist() == [3, 2]
    assert_same(x, y, f"{opt} gates")
    assert not torch.equal(x.p[runs[1][0]:], before["p"][runs[1][0]:])


GUARD = 64


def guarded(t):
    """a copy of t inside a larger buffer, GUARD sentinel elements on both sides; (view, whole buffer)"""
    big = torch.full((t.numel() + 2 * GUARD,), 7, dtype=t.dtype, device=DEV)
    view = big[GUARD:GUARD + t.numel()].view(t.shape)
    view.copy_(t)
    return view, big


@pytest.mark.parametrize("opt", ["sgd", "adamw"])
def test_map_byte_beyond_the_table_is_clamped(opt):
    """A map byte of 255 with three groups: its elements are updated as group 2 (the last row), and no buffer's
    surroundings change.  The cell belongs to the 1000-element tensor (group 0), so the clamp shows."""
    cell = SPANS[3][0] // 8 + 5
    assert GROUP_OF[3] == 0

    def run(byte):
        gm = group_map()
        gm[cell] = byte
        b, d = Bufs(), Dev()
        bigs = {}
        for name in ("p", "g", "a", "v", "s"):
            view, bigs[name] = guarded(getattr(b, name))
            setattr(b, name, view)
        gm, bigs["map"] = guarded(gm)
        hy, bigs["hyper"] = guarded(hyper())
        for t, g in enumerate(inputs()[1][:2]):
            d.lr.fill_(lr_at(t))
            b.load(g, False)
            if opt == "adamw":
                K.adamw_prelude(d.counters, d.corr, [(0, None)], B1, B2)
            step_groups(opt, b, d, table(opt, RUNS, t), gm, hy)
        torch.cuda.synchronize()
        for name, big in bigs.items():
            assert (big[:GUARD] == 7).all() and (big[-GUARD:] == 7).all(), f"{name}: a guard element changed"
        assert int(gm.view(-1)[cell]) == byte and torch.equal(hy, hyper())
        return b
    high, two, plain = run(255), run(2), run(0)
    assert_same(high, two, f"{opt} clamp")
    s = cell * 8
    differs = (high.p != plain.p).nonzero().flatten().tolist()
    print(f"{opt}: elements that differ from the unclamped map: {differs}")
    assert differs and set(differs) <= set(range(s, s + 8))


def _toy(groups_of=None):
    torch.manual_seed(0)
    m = torch.nn.Sequential(torch.nn.Linear(33, 65), torch.nn.Linear(65, 7)).to(DEV)
    store = ParamStore(m, torch.bfloat16)
    groups = ParamGroups(m, store, WD, no_decay="norm_bias", lr_scale={"1": 10.0})
    return store, groups, FusedAdamW(store, 1e-3, betas=(B1, B2), eps=EPS, weight_decay=WD, groups=groups)


def test_group_hyper_changed_between_replays_takes_effect():
    """store.grad.copy_(g_static); opt.step() with groups captured once: a replay, then group_hyper overwritten in
    place and a second replay, is bit-equal to the two eager steps with the same change between them."""
    gen = torch.Generator().manual_seed(9)
    se, ge, oe = _toy()
    assert len(ge.param_groups) == 4
    gs = [(1e-2 * torch.randn(se.numel, generator=gen)).to(DEV) for _ in range(2)]
    new = torch.tensor([0.5, 0.25], device=DEV)

    se.grad.copy_(gs[0])
    oe.step()
    ge.group_hyper[0].copy_(new)
    se.grad.copy_(gs[1])
    oe.step()

    sg, gg, og = _toy()
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
    g_static.copy_(gs[0])
    graph.replay()
    gg.group_hyper[0].copy_(new)
    g_static.copy_(gs[1])
    graph.replay()
    torch.cuda.synchronize()
    assert og.counters.tolist() == oe.counters.tolist() == [2]
    assert torch.equal(sg.flat, se.flat) and torch.equal(sg.shadow, se.shadow)
    assert torch.equal(og.exp_avg, oe.exp_avg) and torch.equal(og.exp_avg_sq, oe.exp_avg_sq)
    # and the change matters: the same two steps without it end elsewhere
    sn, _, on = _toy()
    for g in gs:
        sn.grad.copy_(g)
        on.step()
    torch.cuda.synchronize()
    assert not torch.equal(sn.flat, se.flat)


TRUNKS = {"vExtract": 0.1, "aExtract": 0.1, "paExtract": 0.1}


def _c1(seed):
    from deepfake_amd.models.fused import build_fused
    m = named_fill_(build_fused("c1", compute_dtype=torch.float32), seed).to(DEV)
    m.train()
    store = ParamStore(m, torch.float32)
    groups = ParamGroups(m, store, 0.05, no_decay="norm_bias", lr_scale=TRUNKS)
    return m, store, groups, FusedAdamW(store, 1e-4, weight_decay=0.05, groups=groups)


def test_whole_store_equals_per_parameter_plain_steps():
    """The C1 model's store (fp32) with its flat_groups() gaps: two FusedAdamW steps with groups (no decay on norm /
    bias / position parameters, the trunks at 0.1 lr) are bit-equal over flat, exp_avg and exp_avg_sq to one plain
    dfk_adamw_step per parameter at that parameter's fp32 lr product and decay."""
    _, store, groups, opt = _c1(GC.FUSED_C1["seed"])
    assert sorted(r[:2] for r in groups.summary()) == [(0.1, 0.0), (0.1, 0.05), (1.0, 0.0), (1.0, 0.05)]
    for gate in store.gate:                       # every LayerDrop layer kept: all runs do their work
        if gate is not None:
            gate.fill_(1.0)
    mask = torch.zeros(store.numel)
    for i in range(len(store.params)):
        s, e = store.span(i)
        mask[s:e] = 1
    rp, rm, rv = store.flat.clone(), torch.zeros_like(store.flat), torch.zeros_like(store.flat)
    p0 = store.flat.clone()
    gen = torch.Generator().manual_seed(21)
    b1, b2 = opt.betas
    for t in range(2):
        opt.set_lr(lr_at(t) * 0.1)
        store.grad.copy_((1e-2 * torch.randn(store.numel, generator=gen) * mask).to(DEV))
        opt.step()
        lrs = {m: opt.lr_dev * torch.tensor(m, dtype=torch.float32, device=DEV) for m in (1.0, 0.1)}
        for i in range(len(store.params)):
            s, e = store.span(i)
            mult, wd = groups.spec[store.name(i)]
            c = opt.cls[i]
            K.adamw_step(rp[s:e], store.grad[s:e], rm[s:e], rv[s:e], None, 0.0, b1, b2, opt.eps, wd,
                         opt.corr[2 * c:2 * c + 2], lr_dev=lrs[mult], gate=opt.gates[c])
    torch.cuda.synchronize()
    diff = [int((a != b).sum()) for a, b in ((store.flat, rp), (opt.exp_avg, rm), (opt.exp_avg_sq, rv))]
    print(f"C1 store: {store.numel} elements, {len(store.params)} tensors, {len(opt.gates)} classes; elements that "
          f"differ (flat, exp_avg, exp_avg_sq): {diff}")
    assert torch.equal(store.flat, rp) and torch.equal(opt.exp_avg, rm) and torch.equal(opt.exp_avg_sq, rv)
    assert not torch.equal(store.flat, p0) and all(int(c) == 2 for c in opt.counters)


def _c1_run(graph):
    from deepfake_amd.ddp import GradBucketer
    from deepfake_amd.trainer import TrainStep
    c = GC.FUSED_C1
    m, store, _, opt = _c1(c["seed"])
    step = TrainStep(m, store, opt, GradBucketer(store), graph=graph)
    losses = []
    for i in range(3):
        v, mel, w, lab = synthetic_inputs(c["B"], c["T"], c["H"], c["W"], c["seconds"], seed=c["seed"] + 10 * i)
        loss, _ = step((v.to(DEV), mel.to(DEV), w.to(DEV)), lab.to(DEV))
        losses.append(float(loss))
    torch.cuda.synchronize()
    return losses, opt.exp_avg_sq.clone(), opt.counters.clone(), step


def test_whole_step_with_groups_graph_matches_eager():
    """TrainStep at the C1 fixture (fp32) with FusedAdamW and the groups of the test above, 3 steps, graph against
    eager, at the bar of tests/test_gpu_adamw.py's whole-step test: the larger of 1e-5 and twice the distance of two
    identical eager runs, on the losses and on exp_avg_sq."""
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
