"""GPU: grouped weight-gradient GEMMs (dfk_gemm_dw_group) and their deferral in the backward pass.

Native: on small-integer operands every fp32 sum is exact, so the grouped launch must equal torch and the same
problems launched singly bit for bit.  Deferral: a SwinV2 block and a wav2vec2 layer give the gradients of the
ungrouped backward, report every parameter ready exactly once and only after its flush, leave no problem queued
when backward() returns, and replay from a captured graph."""
import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from deepfake_amd import kernels as K
    from deepfake_amd.models import set_compute_dtype
    from deepfake_amd.models.swin_transformer2d import SwinTransformerBlock
    from deepfake_amd.models.wav2vec2 import Wav2Vec2Config, Wav2Vec2EncoderLayer
    from deepfake_amd.params import ParamStore

# (tokens, N of dy, K of x, with db): ragged tiles + db; 128x128 split tiles without db; the unsplit 64x64 path;
# the split 128x128 path; one tiny tile
SHAPES = [(200, 136, 72, True), (1568, 512, 512, False), (1592, 768, 3072, True), (1568, 2048, 512, True),
          (64, 8, 8, False)]


def _ints(gen, *shape, lim=2):
    return torch.randint(-lim, lim + 1, shape, device="cuda", generator=gen).to(torch.bfloat16)


@pytest.fixture(scope="module")
def operands():
    """Per shape: dy, x (integers, |v| <= 2, bf16) and the exact products in fp64."""
    gen = torch.Generator(device="cuda").manual_seed(5)
    out = []
    for M, N, Kd, has_db in SHAPES:
        dy, x = _ints(gen, M, N), _ints(gen, M, Kd)
        out.append((dy, x, dy.double().T @ x.double(), dy.double().sum(0), has_db))
    return out


def _outputs(ops, n, only=None):
    """n problems cycling through the shapes (only: all of that one shape), each with its own pre-filled dW / db
    (the += contract)."""
    probs, want = [], []
    for i in range(n):
        dy, x, w64, b64, has_db = ops[i % len(ops) if only is None else only]
        dw = torch.full(w64.shape, float(3 + i), device="cuda")
        db = torch.full(b64.shape, float(-5 - i), device="cuda") if has_db else None
        probs.append((dy, x, dw, db))
        want.append((w64 + (3 + i), b64 - (5 + i) if has_db else None))
    return probs, want


# mixed: the shapes in turn (several tile shapes, with and without db, in one call); a shape index: n problems of
# that one shape, so that one instantiation's 8-record chunk overflows (9 = 8 + a single, 10 = 8 + a group of 2)
@pytest.mark.parametrize("n,only", [(1, None), (2, None), (5, None), (9, None), (9, 0), (10, 3)])
def test_group_is_exact(operands, n, only):
    grouped, want = _outputs(operands, n, only)
    K.linear_dw_group(grouped)
    singles, _ = _outputs(operands, n, only)
    for dy, x, dw, db in singles:
        K.linear_dw(dy, x, dw, db)
    torch.cuda.synchronize()
    for i, ((_, _, dw, db), (_, _, sw, sb), (w64, b64)) in enumerate(zip(grouped, singles, want)):
        assert torch.equal(dw.double(), w64), f"problem {i}: grouped dW differs from torch"
        assert torch.equal(dw, sw), f"problem {i}: grouped dW differs from the single launch"
        if db is not None:
            assert torch.equal(db.double(), b64), f"problem {i}: grouped db differs from torch"
            assert torch.equal(db, sb), f"problem {i}: grouped db differs from the single launch"


def test_group_shared_output_is_serialised(operands):
    """Two problems of one call adding into the same dW / db (a weight used twice) never share a launch: the
    unsplit problems add without atomics."""
    dy, x, w64, b64, _ = operands[0]
    dw, db = torch.full(w64.shape, 1.0, device="cuda"), torch.full(b64.shape, 2.0, device="cuda")
    other = torch.zeros_like(dw)
    K.linear_dw_group([(dy, x, dw, db), (dy, x, other, None), (dy, x, dw, db), (dy, x, dw, db)])
    torch.cuda.synchronize()
    assert torch.equal(dw.double(), 3 * w64 + 1) and torch.equal(db.double(), 3 * b64 + 2)
    assert torch.equal(other.double(), w64)


def _swin_block():
    torch.manual_seed(0)
    m = SwinTransformerBlock(128, (7, 14), 4, window_size=7)   # 2 windows of 49 tokens
    x = torch.randn(1, 98, 128, device="cuda").to(torch.bfloat16)
    return (set_compute_dtype(m, torch.bfloat16).cuda().train(), (x,),
            ("attn.qkv.", "attn.q_bias", "attn.v_bias", "attn.proj.", "mlp.fc1.", "mlp.fc2."))


def _w2v_layer():
    torch.manual_seed(0)
    m = Wav2Vec2EncoderLayer(Wav2Vec2Config().deterministic())   # C = 768
    x = torch.randn(2 * 40, 768, device="cuda").to(torch.bfloat16)   # B = 2, T = 40
    return set_compute_dtype(m, torch.bfloat16).cuda().train(), (x, 2, 40), ("attention.", "feed_forward.")


def _run(m, st, args, gy):
    st.zero_grad()
    x = args[0].clone().requires_grad_(True)
    y = m(x, *args[1:])
    (y.float() * gy).sum().backward()
    pending = K.dw_pending()
    torch.cuda.synchronize()
    return torch.cat([st.grad.float().reshape(-1), x.grad.float().reshape(-1)]).clone(), pending


def _rel(a, b):
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


@pytest.mark.parametrize("make", [_swin_block, _w2v_layer], ids=["swinv2", "w2v"])
def test_deferral_matches_ungrouped(make):
    m, args, linear_names = make()
    st = ParamStore(m, torch.bfloat16)
    gy = torch.randn(args[0].shape, device="cuda")   # both blocks keep their input's shape
    ready = []
    st.listeners.append(ready.append)
    old = K.dw_group_policy(0)
    try:
        a, _ = _run(m, st, args, gy)
        ready_off = sorted(ready)
        b, _ = _run(m, st, args, gy)
        del ready[:]
        K.dw_group_policy(1)
        flushed = []
        flush = K.dw_flush

        def spy():
            n = len(K._dw_queues.get(torch.cuda.current_stream().cuda_stream, (None, []))[1])
            before = len(ready)
            flush()
            if n:
                flushed.append((n, before, len(ready)))
        K.dw_flush = spy
        try:
            g, pending = _run(m, st, args, gy)
        finally:
            K.dw_flush = flush
    finally:
        K.dw_group_policy(old)
    assert pending == 0, "problems left queued when backward() returned"
    assert flushed and sum(n for n, _, _ in flushed) == 4, flushed   # qkv, proj, fc1, fc2
    # every parameter reported exactly once, as without grouping; the Linears' (all queued) only inside a flush
    assert sorted(ready) == ready_off and len(set(ready)) == len(ready), (ready, ready_off)
    queued = {st.index[id(p)] for n, p in m.named_parameters() if n.startswith(linear_names)}
    in_flush = [i for _, before, after in flushed for i in ready[before:after]]
    assert sorted(in_flush) == sorted(queued), (in_flush, queued)
    dab, dga = _rel(a, b), _rel(g, a)
    print(f"off/off rel L2 {dab:.3e}, grouped/off rel L2 {dga:.3e}")
    if torch.equal(a, b):
        assert torch.equal(g, a), f"ungrouped runs are bitwise equal, the grouped run differs (rel L2 {dga:.3e})"
    else:
        assert dga <= 4 * dab, (dga, dab)


def test_deferred_ready_only_after_flush():
    """A queued problem's done() runs at the flush, not at the queueing call."""
    gen = torch.Generator(device="cuda").manual_seed(1)
    dy, x = _ints(gen, 64, 8), _ints(gen, 64, 8)
    dw, dw2 = torch.zeros(8, 8, device="cuda"), torch.zeros(8, 8, device="cuda")
    seen = []
    old = K.dw_group_policy(1)
    try:
        assert K.linear_dw(dy, x, dw, defer=True, done=lambda: seen.append(0)) is True
        assert K.linear_dw(dy, x, dw2, defer=True, done=lambda: seen.append(1)) is True
        assert seen == [] and K.dw_pending() == 2
        K.dw_flush()
        assert seen == [0, 1] and K.dw_pending() == 0
        K.dw_group_policy(0)
        assert K.linear_dw(dy, x, dw, defer=True, done=lambda: seen.append(2)) is dw and seen[-1] == 2
    finally:
        K.dw_group_policy(old)
    torch.cuda.synchronize()
    assert torch.equal(dw, 2 * dw2) and torch.equal(dw2.double(), dy.double().T @ x.double())


def test_deferral_graph_replay_matches_eager():
    m, (x,), _ = _swin_block()
    st = ParamStore(m, torch.bfloat16)
    gy = torch.randn(x.shape, device="cuda")

    def body():
        st.zero_grad()
        (m(x).float() * gy).sum().backward()

    old = K.dw_group_policy(1)
    try:
        body()
        torch.cuda.synchronize()
        eager = st.grad.clone()
        body()
        torch.cuda.synchronize()
        eager2 = st.grad.clone()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.stream(s):
            body()   # warm the allocator on the capture stream
            with torch.cuda.graph(graph, stream=s, capture_error_mode="thread_local"):
                body()
        torch.cuda.current_stream().wait_stream(s)
        assert K.dw_pending() == 0
        st.grad.fill_(7.0)
        graph.replay()
        torch.cuda.synchronize()
    finally:
        K.dw_group_policy(old)
    # the same kernels on the same inputs: at most the order of fp32 atomics differs, as between two eager runs
    if torch.equal(eager, eager2):
        assert torch.equal(st.grad, eager)
    else:
        assert _rel(st.grad, eager) <= 4 * _rel(eager2, eager)
