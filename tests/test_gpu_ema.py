"""GPU: the weight EMA (dfk_ema_prelude / dfk_ema_update / dfk_ema_swap, optim.ParamEMA, TrainStep(ema=...)).

The yardstick of the update is the same recurrence e <- e + w_t (p_t - e) in float64 on the same fp32 inputs, with the
device's own fp32 w_t read back.  The bar per element is 2 T 2^-23 M over T updates, M the running max of |p| and |e|
of that element: one rounded subtraction and one fma add at most 3 2^-24 M of new error per update, and the recurrence
carries the old error forward by a factor 1 - w <= 1.  Every test prints its figures before it asserts."""
import functools

import numpy as np
import pytest
import torch

import golden_cases as GC
from oracle.fill import named_fill_, synthetic_inputs

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from deepfake_amd import kernels as K
    from deepfake_amd.optim import FusedSGD, ParamEMA
    from deepfake_amd.params import ParamStore

DEV = "cuda"
T = 6
SIZES = [1, 3, 4, 5, 1023, 1027, 2047, 2048, 2049, 4099, 5123]
PAD, SENTINEL = 64, 12345.0


def ramp_weight(decay, warmup, k):
    """fp32 weight of update k (k updates done before it): double arithmetic, rounded once."""
    return np.float32(1 - (min(decay, (1 + k) / (10 + k)) if warmup else decay))


@functools.lru_cache(maxsize=None)
def inputs(n):
    """e_0 and the T fresh p_t of size n (host, fp32), drawn once per size."""
    gen = torch.Generator().manual_seed(2000 + n)
    return torch.randn(n, generator=gen), [torch.randn(n, generator=gen) for _ in range(T)]


def recurrence64(e0, ps, ws):
    """(e_T in float64, the per-element running max of |p| and |e|)"""
    e = e0.double().clone()
    big = e.abs()
    for p, w in zip(ps, ws):
        e = e + float(w) * (p.double() - e)
        big = torch.maximum(big, torch.maximum(p.double().abs(), e.abs()))
    return e, big


def check_bar(what, got, e64, big, steps):
    err = (got.detach().cpu().double() - e64).abs()
    bar = 2 * steps * 2.0 ** -23 * big
    ratio = float((err / bar.clamp_min(1e-300)).max())
    print(f"{what}: max err {float(err.max()):.3e}, max err / bar {ratio:.3f}")
    assert bool((err <= bar).all()), (what, ratio)
    return ratio


@pytest.mark.parametrize("decay,warmup", [(0.999, False), (0.9999, True), (0.5, False), (0.0, False)])
@pytest.mark.parametrize("n", SIZES)
def test_update_against_float64(n, decay, warmup):
    """T updates of n elements with a fresh p each (the n % 4 tail alone, both quad boundaries of a 2048-block, a
    multi-block tail in the second quad); decay 0 reproduces p; nothing behind n and nothing of p is written."""
    e0, ps = inputs(n)
    pbuf = torch.full((n + PAD,), SENTINEL, device=DEV)
    ebuf = torch.full((n + PAD,), SENTINEL, device=DEV)
    ebuf[:n].copy_(e0)
    num, w = torch.zeros(1, device=DEV, dtype=torch.int32), torch.zeros(1, device=DEV)
    ws = []
    for p in ps:
        pbuf[:n].copy_(p)
        K.ema_prelude(num, w, decay, warmup)
        K.ema_update(pbuf[:n], ebuf[:n], w)
        ws.append(np.float32(w.item()))
    assert int(num) == T
    assert ws == [ramp_weight(decay, warmup, k) for k in range(T)]
    e64, big = recurrence64(e0, ps, ws)
    check_bar(f"n={n} decay={decay} warmup={warmup}", ebuf[:n], e64, big, T)
    if decay == 0.0:
        assert torch.equal(ebuf[:n].cpu(), ps[-1]), "decay 0 must reproduce p"
    assert torch.equal(pbuf[:n].cpu(), ps[-1]), "p was written"
    assert bool((pbuf[n:] == SENTINEL).all()) and bool((ebuf[n:] == SENTINEL).all()), "written behind n"


@pytest.mark.parametrize("decay", [0.9999, 0.3])
def test_prelude_counts_and_weights(decay):
    """Call k = 0..5: num_updates == k + 1 and weight == float32(1 - min(decay, (1 + k) / (10 + k))) bit for bit (at
    decay 0.3 the ramp takes over the decay from k = 3 on); with warm-up off weight == float32(1 - decay)."""
    num, w = torch.zeros(1, device=DEV, dtype=torch.int32), torch.zeros(1, device=DEV)
    for k in range(6):
        K.ema_prelude(num, w, decay, True)
        got, want = np.float32(w.item()), ramp_weight(decay, True, k)
        print(f"decay {decay} k {k}: weight {got!r} want {want!r}")
        assert int(num) == k + 1 and got == want
    K.ema_prelude(num, w, decay, False)
    assert int(num) == 7 and np.float32(w.item()) == np.float32(1 - decay)


def _toy_store(dtype):
    torch.manual_seed(0)
    m = torch.nn.Sequential(torch.nn.Linear(33, 65), torch.nn.Linear(65, 7)).to(DEV)
    return m, ParamStore(m, dtype)


def _moved_ema(store, seed=4):
    """An EMA that differs from the live weights everywhere a parameter lives: one update after a perturbation."""
    ema = ParamEMA(store, 0.75)
    gen = torch.Generator().manual_seed(seed)
    for p in store.params:
        p.data.add_((0.1 * torch.randn(p.shape, generator=gen)).to(DEV))
    store.refresh_shadow()
    ema.update()
    return ema


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_swap_and_swap_back(dtype):
    """One swap: flat is the old ema, ema the old flat, shadow == bf16(flat); a second swap restores all three bit for
    bit.  With an fp32 store there is no shadow.  applied() restores the weights when its body raises."""
    _, store = _toy_store(dtype)
    ema = _moved_ema(store)
    assert (store.shadow is None) == (dtype == torch.float32)
    flat0, ema0 = store.flat.clone(), ema.ema.clone()
    shadow0 = store.shadow.clone() if store.shadow is not None else None
    assert not torch.equal(flat0, ema0)
    ema.swap()
    assert torch.equal(store.flat, ema0) and torch.equal(ema.ema, flat0)
    if shadow0 is not None:
        assert torch.equal(store.shadow, store.flat.to(torch.bfloat16)) and not torch.equal(store.shadow, shadow0)
    ema.swap()
    assert torch.equal(store.flat, flat0) and torch.equal(ema.ema, ema0)
    if shadow0 is not None:
        assert torch.equal(store.shadow, shadow0)
    with pytest.raises(KeyError):
        with ema.applied():
            assert torch.equal(store.flat, ema0)
            raise KeyError("body")
    assert torch.equal(store.flat, flat0) and torch.equal(ema.ema, ema0) and not ema.swapped
    if shadow0 is not None:
        assert torch.equal(store.shadow, shadow0)
    with ema.applied():
        with pytest.raises(RuntimeError):
            with ema.applied():
                pass
        assert torch.equal(store.flat, ema0), "a refused nested applied() un-swapped"
    assert torch.equal(store.flat, flat0)


def test_misaligned_pointers_raise_before_any_launch():
    """A pointer one element off its alignment makes each wrapper raise (the check is on the host): the buffers and
    the count are what they were."""
    n = 4096
    p, e = torch.randn(n + 4, device=DEV), torch.randn(n + 4, device=DEV)
    s = torch.zeros(n + 4, device=DEV, dtype=torch.bfloat16)
    w4 = torch.full((4,), 0.5, device=DEV)
    num = torch.zeros(1, device=DEV, dtype=torch.int32)
    p0, e0, s0 = p.clone(), e.clone(), s.clone()
    with pytest.raises(RuntimeError, match="ema_prelude"):
        K.ema_prelude(num, w4[1:2], 0.9, False)
    for pp, ee in ((p[1:n + 1], e[:n]), (p[:n], e[1:n + 1])):
        with pytest.raises(RuntimeError, match="ema_update"):
            K.ema_update(pp, ee, w4[:1])
        with pytest.raises(RuntimeError, match="ema_swap"):
            K.ema_swap(pp, ee, s[:n])
    with pytest.raises(RuntimeError, match="ema_update"):
        K.ema_update(p[:n], e[:n], w4[1:2])
    with pytest.raises(RuntimeError, match="ema_swap"):
        K.ema_swap(p[:n], e[:n], s[1:n + 1])
    torch.cuda.synchronize()
    assert int(num) == 0 and torch.equal(p, p0) and torch.equal(e, e0) and torch.equal(s, s0)
    assert bool((w4 == 0.5).all())


def test_captured_update_advances_the_device_count():
    """store.flat.copy_(p_static); ema.update() captured once and replayed 3 times with a new p each is bit-equal to
    three eager updates (decay warm-up on: every replay takes another weight); the capture itself does not count."""
    gen = torch.Generator().manual_seed(9)
    _, se = _toy_store(torch.bfloat16)
    ps = [torch.randn(se.numel, generator=gen).to(DEV) for _ in range(3)]
    ee = ParamEMA(se, 0.9999, warmup=True)
    for p in ps:
        se.flat.copy_(p)
        ee.update()
    _, sg = _toy_store(torch.bfloat16)
    eg = ParamEMA(sg, 0.9999, warmup=True)
    start = eg.ema.clone()
    p_static = torch.zeros_like(ps[0])
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            sg.flat.copy_(p_static)
            eg.update()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert eg.num_updates.tolist() == [0] and torch.equal(eg.ema, start), "the capture itself must not update"
    for p in ps:
        p_static.copy_(p)
        graph.replay()
    torch.cuda.synchronize()
    assert eg.num_updates.tolist() == ee.num_updates.tolist() == [3]
    assert torch.equal(eg.ema, ee.ema) and torch.equal(eg.weight, ee.weight)
    assert not torch.equal(eg.ema, start)


def _c1_run(graph):
    """Three steps at the C1 fixture in fp32 with TrainStep(..., ema=ParamEMA(store, 0.9, warmup=True)).  The optimizer
    is the fused SGD of tests/test_gpu_trainstep.py, whose weights that test already compares between graph and eager
    at 1e-5: the EMA is a fixed linear combination of the weights, so it inherits their conditioning.  (Under AdamW an
    element whose gradient is atomics-order noise moves by 2 lr between any two runs, which is why
    tests/test_gpu_adamw.py does not compare parameters.)"""
    from deepfake_amd.ddp import GradBucketer
    from deepfake_amd.models.fused import build_fused
    from deepfake_amd.trainer import TrainStep
    c = GC.FUSED_C1
    m = named_fill_(build_fused("c1", compute_dtype=torch.float32), c["seed"]).to(DEV)
    m.train()
    store = ParamStore(m, torch.float32)
    ema = ParamEMA(store, 0.9, warmup=True)
    step = TrainStep(m, store, FusedSGD(store, 0.01, 0.9, 0.05), GradBucketer(store), graph=graph, ema=ema)
    snaps, ws = [store.flat.cpu()], []
    for i in range(3):
        v, mel, w, lab = synthetic_inputs(c["B"], c["T"], c["H"], c["W"], c["seconds"], seed=c["seed"] + 10 * i)
        step((v.to(DEV), mel.to(DEV), w.to(DEV)), lab.to(DEV))
        snaps.append(store.flat.cpu())
        ws.append(np.float32(ema.weight.item()))
    torch.cuda.synchronize()
    return store, ema, step, snaps, ws


def test_whole_step_graph_matches_eager():
    """Graph against eager: 3 updates in both, the EMA buffers within the larger of 1e-5 relative and twice the
    distance of two identical eager runs (the whole-step rule: the fp32 atomics' order moves the weights themselves).
    Eager: the EMA equals the float64 recurrence over the three recorded store.flat snapshots within the module's bar.
    The launch is whole-store: a gap element of the average is 0, a parameter's elements follow the weights."""
    sa, ea, _, snaps, ws = _c1_run(graph=False)
    _, eb, _, _, _ = _c1_run(graph=False)
    _, eg, step, _, wg = _c1_run(graph=True)
    assert step.graph is not None and step.graph_mode, "the step was not captured"
    assert ea.num_updates.tolist() == eg.num_updates.tolist() == [3]
    assert ws == wg == [ramp_weight(0.9, True, k) for k in range(3)]

    def rel(a, b):
        return float((a - b).abs().max() / b.abs().max())
    ee, ge = rel(eb.ema, ea.ema), rel(eg.ema, ea.ema)
    bar = max(1e-5, 2 * ee)
    print(f"eager-eager {ee:.3e}; graph-eager {ge:.3e}; bar {bar:.3e}")
    assert ge <= bar, (ge, bar)
    e64, big = recurrence64(snaps[0], snaps[1:], ws)
    check_bar("C1 eager against the float64 recurrence", ea.ema, e64, big, 3)
    assert not torch.equal(ea.ema.cpu(), snaps[0]) and not torch.equal(ea.ema.cpu(), snaps[-1])
    covered = torch.zeros(sa.numel, dtype=torch.bool)
    for i in range(len(sa.params)):
        s, e = sa.span(i)
        covered[s:e] = True
    gaps = (~covered).nonzero().reshape(-1)
    assert gaps.numel() > 0, "the C1 store has alignment gaps"
    assert not ea.ema.cpu()[gaps].any() and not eg.ema.cpu()[gaps].any()


def test_trainer_validates_through_the_average_in_bf16():
    """Trainer with --ema_decay on the C1 model in bf16 compute (the GEMMs read the shadow), graph on: three steps (one
    eager, two replayed) make three updates; validation logs 'Val(EMA) Loss' and leaves flat and shadow as they were;
    inside applied() the logits are those of the model with the average copied in by torch and the shadow re-cast
    (within two bf16 ulps of the largest logit: the forward is not pinned to be bitwise repeatable), and far from
    the live model's once the average is made to differ visibly."""
    import types
    from deepfake_amd.models.fused import build_fused
    from deepfake_amd.trainer import Trainer
    c = GC.FUSED_C1
    v, mel, wave, label = synthetic_inputs(c["B"], c["T"], c["H"], c["W"], c["seconds"], seed=c["seed"] + 1)
    batch = ({"Video": v, "Audio": mel, "PAudio": [w.numpy() for w in wave]}, label)

    class Data:
        def train_dataloader(self):
            return [batch] * 3

        def val_dataloader(self):
            return [batch]

    args = types.SimpleNamespace(epochs=0, learning_rate=0.01, batch_size=2, modality="fused", model_save=0,
                                 log_step=1, accum_step=1, l2_decacy=0.05, dtype="bf16", bucket_mb=64.0, soft=0.01,
                                 classify_drop=0.0, swin_drop=0.0, ema_decay=0.9, ema_warmup=True)
    lines = []
    tr = Trainer(named_fill_(build_fused("c1", compute_dtype=torch.bfloat16), c["seed"]), args, torch.device(DEV),
                 Data(), logger=lines.append, compute_dtype=torch.bfloat16, graph=True)
    assert tr.ema is not None and tr.store.shadow is not None
    tr.train()
    torch.cuda.synchronize()
    assert tr.step_fn.graph is not None, "the step was not captured"
    assert tr.ema.num_updates.tolist() == [3] and not tr.ema.swapped
    assert any("Val(EMA) Loss" in ln for ln in lines) and not any("| Val Loss" in ln for ln in lines)
    store, ema, model = tr.store, tr.ema, tr.model
    assert torch.equal(store.shadow, store.flat.to(torch.bfloat16))
    ema.ema.mul_(0.5)                                   # an average that evaluates visibly differently
    flat0, shadow0, ema0 = store.flat.clone(), store.shadow.clone(), ema.ema.clone()
    feat, _ = tr._prep(batch)
    model.eval()

    def logits():
        with torch.no_grad():
            model(feat)
        return model.last_logits.detach().float().clone()
    live = logits()
    with ema.applied():
        inside = logits()
        assert torch.equal(store.flat, ema0) and torch.equal(store.shadow, ema0.to(torch.bfloat16))
    assert torch.equal(store.flat, flat0) and torch.equal(store.shadow, shadow0) and torch.equal(ema.ema, ema0)
    store.flat.copy_(ema0)
    store.refresh_shadow()
    want = logits()
    store.flat.copy_(flat0)
    store.refresh_shadow()
    assert torch.equal(store.shadow, shadow0)
    tol = 2.0 ** -7 * float(want.abs().max())
    d_in, d_live = float((inside - want).abs().max()), float((inside - live).abs().max())
    print(f"logits: |inside - copied| {d_in:.3e} (tol {tol:.3e}), |inside - live| {d_live:.3e}")
    assert d_in <= tol and d_live > 4 * tol


def test_evaluation_goes_through_the_average():
    """Inside applied() the model's eval output is that of the same model with the EMA values copied into its
    parameters by plain torch copies; after exit it is the pre-swap output bit for bit."""
    m, store = _toy_store(torch.bfloat16)
    ema = _moved_ema(store)
    m.eval()
    x = torch.randn(5, 33, device=DEV, generator=torch.Generator(device=DEV).manual_seed(1))
    with torch.no_grad():
        before = m(x)
        with ema.applied():
            inside = m(x)
            assert torch.equal(store.shadow, store.flat.to(torch.bfloat16))
        after = m(x)
        live = store.flat.clone()
        for name, avg in ema.named_tensors(m).items():
            m.get_parameter(name).data.copy_(avg)
        want = m(x)
        store.flat.copy_(live)
    assert torch.equal(inside, want) and torch.equal(after, before)
    assert not torch.equal(inside, before)
