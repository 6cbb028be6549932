"""CPU: the host side of the weight EMA (deepfake_amd.optim.ParamEMA) — flags, ABI tables, validation, checkpoint
state, where TrainStep and Trainer call it, and the data-parallel start — with the three kernel entry points
(K.ema_prelude / ema_update / ema_swap) replaced by a torch CPU evaluation of the formulas of include/dfk.h.  The
kernels themselves are tested on the device (tests/test_gpu_ema.py)."""
import io
import math
import os
import re
import types

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = []   # the stand-ins' call record, in order


# ---- torch CPU stand-ins for the three entry points ----
def _fake_prelude(num_updates, weight, decay, warmup=False):
    CALLS.append("prelude")
    t = int(num_updates[0])
    num_updates[0] = t + 1
    weight[0] = 1.0 - (min(decay, (1 + t) / (10 + t)) if warmup else decay)   # double, rounded once by the store


def _fake_update(param, ema, weight):
    CALLS.append("update")
    ema.add_(weight[0] * (param - ema))


def _fake_swap(param, ema, shadow=None):
    CALLS.append("swap")
    old = param.clone()
    param.copy_(ema)
    ema.copy_(old)
    if shadow is not None:
        shadow.copy_(param)


def _install(K):
    K.ema_prelude, K.ema_update, K.ema_swap = _fake_prelude, _fake_update, _fake_swap


@pytest.fixture
def cpu_kernels(monkeypatch):
    from deepfake_amd import kernels as K
    monkeypatch.setattr(K, "ema_prelude", _fake_prelude)
    monkeypatch.setattr(K, "ema_update", _fake_update)
    monkeypatch.setattr(K, "ema_swap", _fake_swap)
    del CALLS[:]
    yield CALLS
    del CALLS[:]


class Net(torch.nn.Module):
    """Two layers, a BatchNorm (buffers beside the parameters) and a head that never gets a gradient."""

    def __init__(self):
        super().__init__()
        self.a = torch.nn.Linear(16, 32)
        self.b = torch.nn.Linear(32, 8)
        self.bn = torch.nn.BatchNorm1d(8)
        self.unused = torch.nn.Linear(4, 4)

    def forward(self, x):
        return torch.sigmoid(self.bn(self.b(torch.relu(self.a(x[0])))).sum(-1))


class PlainSGD:
    """CPU stand-in for the fused optimizers: flat -= lr * grad; records its calls beside the EMA stand-ins'."""

    def __init__(self, store, lr=0.1):
        self.store, self.lr = store, lr

    def step(self, first=None, **kw):
        CALLS.append("step")
        self.store.flat.add_(self.store.grad, alpha=-self.lr)


def _batch(seed, n=4):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(n, 16, generator=g),), (torch.rand(n, generator=g) < 0.5).float()


def _store(seed=0):
    from deepfake_amd.params import ParamStore
    torch.manual_seed(seed)
    m = Net().train()
    return m, ParamStore(m, torch.float32, device=torch.device("cpu"))


# ---- flags ----
def test_flags_parse_and_default_to_off():
    from config import get_opt
    a = get_opt([])
    assert (a.ema_decay, a.ema_warmup) == (0.0, False)
    b = get_opt(["--ema_decay", "0.9999", "--ema_warmup"])
    assert (b.ema_decay, b.ema_warmup) == (0.9999, True)
    with pytest.raises(SystemExit):
        get_opt(["--ema_decay", "slow"])


def test_help_lists_the_ema_flags(capsys):
    from config import get_opt
    with pytest.raises(SystemExit) as e:
        get_opt(["--help"])
    assert e.value.code == 0
    out = capsys.readouterr().out
    assert "--ema_decay" in out and "--ema_warmup" in out
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "--ema_decay" in readme and "--ema_warmup" in readme


def test_ema_arg_validates():
    from deepfake_amd.trainer import ema_arg
    assert ema_arg(types.SimpleNamespace()) is None
    assert ema_arg(types.SimpleNamespace(ema_decay=0.0)) is None
    assert ema_arg(types.SimpleNamespace(ema_decay=0.999)) == 0.999
    for bad in (-0.1, 1.0, 1.5, float("nan"), float("inf"), -float("inf")):
        with pytest.raises(ValueError, match="ema_decay"):
            ema_arg(types.SimpleNamespace(ema_decay=bad))


def test_ema_entry_points_in_header_and_binding_table():
    from deepfake_amd import _lib
    from deepfake_amd import kernels as K
    src = open(os.path.join(ROOT, "include", "dfk.h")).read()
    for name in ("dfk_ema_prelude", "dfk_ema_update", "dfk_ema_swap"):
        assert re.search(r"^int\s+" + name + r"\s*\(", src, flags=re.M), name
        assert name in _lib.SIGNATURES, name
        assert callable(getattr(K, name[4:])), name
    assert os.path.exists(os.path.join(ROOT, "deepfake_amd", "csrc", "ema.hip"))


# ---- ParamEMA ----
def test_param_ema_validates_decay():
    from deepfake_amd.optim import ParamEMA
    _, store = _store()
    for bad in (-1e-3, 1.0, 2.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            ParamEMA(store, bad)
    e = ParamEMA(store, 0.0)
    assert e.num_updates.dtype == torch.int32 and e.num_updates.tolist() == [0]
    assert e.weight.dtype == torch.float32 and e.weight.numel() == 1
    assert torch.equal(e.ema, store.flat) and e.ema.data_ptr() != store.flat.data_ptr()


def test_update_is_the_warmed_up_recurrence(cpu_kernels):
    """3 updates with warm-up at decay 0.9999: the weights are 1 - (1 + t) / (10 + t), and the average follows them."""
    from deepfake_amd.optim import ParamEMA
    _, store = _store()
    ema = ParamEMA(store, 0.9999, warmup=True)
    want = store.flat.double().clone()
    g = torch.Generator().manual_seed(5)
    for t in range(3):
        store.flat.add_(torch.randn(store.numel, generator=g) * 1e-2)
        ema.update()
        w = float(torch.tensor(1.0 - (1 + t) / (10 + t), dtype=torch.float32))
        assert float(ema.weight) == w
        want += w * (store.flat.double() - want)
    assert ema.num_updates.tolist() == [3]
    torch.testing.assert_close(ema.ema.double(), want, rtol=0, atol=1e-6)
    assert cpu_kernels == ["prelude", "update"] * 3


def test_state_dict_round_trip_is_exact(cpu_kernels):
    """2 updates, state saved and loaded into a fresh EMA over a fresh store, update 3 == the uninterrupted run."""
    from deepfake_amd.optim import ParamEMA
    g = torch.Generator().manual_seed(7)
    deltas = [torch.randn(_store()[1].numel, generator=g) * 1e-2 for _ in range(3)]
    _, sa = _store()
    ea = ParamEMA(sa, 0.99, warmup=True)
    for d in deltas:
        sa.flat.add_(d)
        ea.update()
    _, sb = _store()
    eb = ParamEMA(sb, 0.99, warmup=True)
    for d in deltas[:2]:
        sb.flat.add_(d)
        eb.update()
    sd = eb.state_dict()
    assert set(sd) == {"ema", "num_updates", "decay", "warmup"}
    buf = io.BytesIO()
    torch.save({"ema": sd}, buf)                      # as Trainer.save_ckpt stores it
    buf.seek(0)
    sd = torch.load(buf, map_location="cpu", weights_only=True)["ema"]
    _, sc = _store()
    sc.flat.copy_(sb.flat)
    ec = ParamEMA(sc, 0.5)
    ec.load_state_dict(sd)
    assert (ec.decay, ec.warmup, ec.num_updates.tolist()) == (0.99, True, [2])
    sc.flat.add_(deltas[2])
    ec.update()
    assert torch.equal(ec.ema, ea.ema) and torch.equal(ec.num_updates, ea.num_updates)
    bad = dict(sd, ema=torch.zeros(sd["ema"].numel() + 8))
    with pytest.raises(ValueError, match="another parameter store"):
        ec.load_state_dict(bad)


def test_applied_swaps_back_and_refuses_nesting(cpu_kernels):
    from deepfake_amd.optim import ParamEMA
    m, store = _store()
    ema = ParamEMA(store, 0.5)
    store.flat.add_(1.0)
    ema.update()
    live, avg = store.flat.clone(), ema.ema.clone()
    assert not torch.equal(live, avg)
    with ema.applied():
        assert torch.equal(store.flat, avg) and torch.equal(ema.ema, live)
        assert torch.equal(m.a.weight.detach().reshape(-1), avg[slice(*store.span(store.index[id(m.a.weight)]))])
        with pytest.raises(RuntimeError):
            with ema.applied():
                pass
        with pytest.raises(RuntimeError):
            ema.update()
        assert torch.equal(store.flat, avg), "the refused nested applied() must not un-swap"
    assert torch.equal(store.flat, live) and torch.equal(ema.ema, avg)
    with pytest.raises(KeyError):
        with ema.applied():
            raise KeyError("body")
    assert torch.equal(store.flat, live) and torch.equal(ema.ema, avg) and not ema.swapped


def test_swap_and_applied_refuse_a_capture(cpu_kernels, monkeypatch):
    from deepfake_amd.optim import ParamEMA
    _, store = _store()
    ema = ParamEMA(store, 0.5)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(RuntimeError, match="capture"):
        ema.swap()
    with pytest.raises(RuntimeError, match="capture"):
        with ema.applied():
            pass
    assert cpu_kernels == [] and not ema.swapped


def test_named_tensors_have_the_models_keys_and_shapes(cpu_kernels):
    from deepfake_amd.optim import ParamEMA
    m, store = _store()
    ema = ParamEMA(store, 0.5)
    named = ema.named_tensors(m)
    assert set(named) == {k for k, _ in m.named_parameters()}
    for k, p in m.named_parameters():
        assert named[k].shape == p.shape and torch.equal(named[k], p.detach())
        assert named[k].data_ptr() != p.data_ptr()


# ---- TrainStep ----
def _train_step(ema_decay):
    from deepfake_amd.ddp import GradBucketer
    from deepfake_amd.optim import ParamEMA
    from deepfake_amd.trainer import TrainStep
    m, store = _store()
    ema = ParamEMA(store, ema_decay, warmup=True) if ema_decay else None
    return store, ema, TrainStep(m, store, PlainSGD(store), GradBucketer(store), ema=ema)


def test_train_step_without_ema_never_calls_the_ema_kernels(cpu_kernels):
    store, _, step = _train_step(None)
    assert step.ema is None
    step(*_batch(1))
    for k in range(4):
        step.micro(*_batch(2 + k), last=(k == 3), accum=4)
    step._step_body(_batch(9)[0], _batch(9)[1], 1)(False, False)
    assert cpu_kernels == ["step"] * 3


def test_update_follows_the_optimizer_once_per_optimizer_step(cpu_kernels):
    """Eager step, a 4-micro-step accumulation window and the graph body (run eagerly here): each is one optimizer
    step followed by exactly one prelude + update."""
    store, ema, step = _train_step(0.9)
    one = ["step", "prelude", "update"]
    step(*_batch(1))
    assert cpu_kernels == one and ema.num_updates.tolist() == [1]
    for k in range(4):
        step.micro(*_batch(2 + k), last=(k == 3), accum=4)
        assert cpu_kernels == one * (2 if k == 3 else 1)
    for accum in (1, 4):
        step._step_body(_batch(9)[0], _batch(9)[1], accum)(False, False)
    assert cpu_kernels == one * 4 and ema.num_updates.tolist() == [4]
    assert not torch.equal(ema.ema, store.flat)
    s, e = store.span(store.index[id(step.model.unused.weight)])
    assert torch.equal(ema.ema[s:e], store.flat[s:e])     # never stepped: the average of a constant


# ---- Trainer ----
class _Data:
    def __init__(self, val=None):
        self.val = val

    def train_dataloader(self):
        return []

    def val_dataloader(self):
        return self.val


def _args(**kw):
    a = dict(epochs=1, learning_rate=0.1, batch_size=2, modality="fused", model_save=0, log_step=1, accum_step=1,
             l2_decacy=0.0, random_seed=42, bucket_mb=1.0, fused_ckpt_path=None)
    a.update(kw)
    return types.SimpleNamespace(**a)


def _trainer(seed=0, data=None, logger=None, **kw):
    from deepfake_amd.trainer import Trainer
    torch.manual_seed(seed)
    return Trainer(Net(), _args(**kw), torch.device("cpu"), data or _Data(), logger=logger,
                   compute_dtype=torch.float32)


def test_trainer_builds_no_ema_by_default_and_rejects_bad_decay(cpu_kernels):
    assert _trainer().ema is None and _trainer().step_fn.ema is None
    tr = _trainer(ema_decay=0.999, ema_warmup=True)
    assert tr.ema is tr.step_fn.ema and (tr.ema.decay, tr.ema.warmup) == (0.999, True)
    with pytest.raises(ValueError, match="ema_decay"):
        _trainer(ema_decay=1.0)


def test_save_ckpt_keys_with_ema_off_are_unchanged(cpu_kernels, tmp_path):
    tr = _trainer()
    tr.save_ckpt(str(tmp_path / "off.pth"), 3)
    ck = torch.load(str(tmp_path / "off.pth"), map_location="cpu", weights_only=True)
    assert set(ck) == {"epoch", "checkpoint", "optimizer"}
    assert cpu_kernels == []


def test_save_and_load_ckpt_with_ema(cpu_kernels, tmp_path):
    tr = _trainer(ema_decay=0.9)
    for p in tr.model.parameters():                    # the parameters only: the store's gap elements stay 0
        p.data.add_(0.25)
    tr.ema.update()
    tr.model.bn.running_mean.fill_(2.0)
    path = str(tmp_path / "on.pth")
    tr.save_ckpt(path, 3)
    ck = torch.load(path, map_location="cpu", weights_only=True)
    assert set(ck) == {"epoch", "checkpoint", "optimizer", "checkpoint_ema", "ema"}
    assert list(ck["checkpoint_ema"]) == list(ck["checkpoint"])
    params = {k for k, _ in tr.model.named_parameters()}
    for k, v in ck["checkpoint"].items():
        a = ck["checkpoint_ema"][k]
        assert a.shape == v.shape and a.dtype == v.dtype
        assert torch.equal(a, v) != (k in params), k          # averaged parameters differ, live buffers are equal
    assert torch.equal(ck["ema"]["ema"], tr.ema.ema) and ck["ema"]["num_updates"].tolist() == [1]
    Net().load_state_dict(ck["checkpoint_ema"])                  # takes "checkpoint"'s place: a strict load
    # restore: a trainer from another initialisation gets the file's weights and the file's average
    other = _trainer(seed=1, ema_decay=0.5)
    assert not torch.equal(other.store.flat, tr.store.flat)
    other.load_ckpt(_args(fused_ckpt_path=path))
    assert torch.equal(other.store.flat, tr.store.flat) and torch.equal(other.ema.ema, tr.ema.ema)
    assert other.ema.num_updates.tolist() == [1] and other.ema.decay == 0.5   # this run's flag stays
    # reset: a file without an EMA state (or with one of another size) restarts the average from the loaded weights
    for strip in (lambda c: c.pop("ema"), lambda c: c["ema"].update(ema=torch.zeros(8))):
        ck2 = torch.load(path, map_location="cpu", weights_only=True)
        strip(ck2)
        p2 = str(tmp_path / "plain.pth")
        torch.save(ck2, p2)
        fresh = _trainer(seed=2, ema_decay=0.9)
        fresh.ema.update()
        init = fresh.ema.ema.clone()
        fresh.load_ckpt(_args(fused_ckpt_path=p2))
        assert torch.equal(fresh.ema.ema, fresh.store.flat) and torch.equal(fresh.store.flat, tr.store.flat)
        assert not torch.equal(fresh.ema.ema, init) and fresh.ema.num_updates.tolist() == [0]


def test_eval_runs_on_the_average_and_says_so(cpu_kernels):
    lines = []
    val = [_batch(3), _batch(4)]
    tr = _trainer(data=_Data(val), logger=lines.append, ema_decay=0.9)
    tr._prep = lambda batch: batch                     # the batches are features already
    tr.store.flat.add_(0.25)
    tr.ema.update()
    live, avg = tr.store.flat.clone(), tr.ema.ema.clone()
    seen = []
    run = tr.run_batch
    tr.run_batch = lambda f, l: (seen.append(tr.store.flat.clone()), run(f, l))[1]
    tr.eval(val, 0, 0, 0.1)
    assert len(seen) == 2 and all(torch.equal(s, avg) for s in seen)
    assert torch.equal(tr.store.flat, live) and torch.equal(tr.ema.ema, avg)
    assert any("Val(EMA) Loss" in s for s in lines) and not any("| Val Loss" in s for s in lines)
    lines2 = []
    off = _trainer(data=_Data(val), logger=lines2.append)
    off._prep = lambda batch: batch
    off.eval(val, 0, 0, 0.1)
    assert any("| Val Loss" in s for s in lines2) and not any("EMA" in s for s in lines2)


# ---- data parallel ----
def _free_port():
    import socket
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        return sk.getsockname()[1]


def _dp_worker(rank, world, port, q):
    from deepfake_amd import kernels as K
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    _install(K)
    tr = _trainer(seed=100 + rank, ema_decay=0.9, ema_warmup=True)   # each rank its own initialisation
    start = tr.ema.ema.clone()
    tr.step_fn.opt = PlainSGD(tr.store)                              # no folds_grad: the bucketer averages
    for i in range(3):
        tr.step_fn(*_batch(10 * rank + i))                           # each rank its own clips
    q.put((rank, start.numpy().copy(), tr.ema.ema.numpy().copy(), tr.ema.num_updates.tolist()))
    dist.destroy_process_group()


def test_world2_replicas_hold_bit_equal_averages():
    """Two ranks with different initialisations and different clips: the EMA is built after the rank-0 broadcast and
    updated from all-reduced gradients, so after 3 steps both hold the same bytes with no collective of its own."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_dp_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = dict((r, (torch.from_numpy(s), torch.from_numpy(e), n)) for r, s, e, n in (q.get(timeout=120) for _ in procs))
    for p in procs:
        p.join(timeout=60)
    assert torch.equal(res[0][0], res[1][0]), "the averages did not start from rank 0's parameters"
    assert torch.equal(res[0][1], res[1][1])
    assert not torch.equal(res[0][1], res[0][0]) and bool(torch.isfinite(res[0][1]).all())
    assert res[0][2] == res[1][2] == [3]
    assert math.isfinite(float(res[0][1].abs().max()))
