"""CPU: the host side of the fused AdamW (deepfake_amd.optim.FusedAdamW) — flags, ABI tables, and the run / gate-class
construction, lr plumbing, touched-set check and checkpoint state of the optimizer class, with the three kernel
entry points (K.adamw_prelude / adamw_step / adamw_step_runs) replaced by a torch CPU evaluation of the formula of
include/dfk.h.  The kernels themselves are tested on the device (tests/test_gpu_adamw.py)."""
import copy
import io
import math
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WD, BETAS, EPS = 0.05, (0.9, 0.999), 1e-8


def test_optimizer_flag_parses_and_defaults_to_sgd():
    from config import get_opt
    a = get_opt([])
    assert (a.optimizer, a.adam_beta1, a.adam_beta2, a.adam_eps) == ("sgd", 0.9, 0.999, 1e-8)
    b = get_opt(["--optimizer", "adamw", "--adam_beta2", "0.98", "--adam_eps", "1e-6"])
    assert (b.optimizer, b.adam_beta1, b.adam_beta2, b.adam_eps) == ("adamw", 0.9, 0.98, 1e-6)
    with pytest.raises(SystemExit):
        get_opt(["--optimizer", "lamb"])


def test_help_lists_the_optimizer_flags(capsys):
    from config import get_opt
    with pytest.raises(SystemExit) as e:
        get_opt(["--help"])
    assert e.value.code == 0
    out = capsys.readouterr().out
    assert all(f in out for f in ("--optimizer", "--adam_beta1", "--adam_beta2", "--adam_eps"))


def test_adamw_entry_points_in_header_and_binding_table():
    from deepfake_amd import _lib
    src = open(os.path.join(ROOT, "include", "dfk.h")).read()
    for name in ("dfk_adamw_step", "dfk_adamw_step_runs", "dfk_adamw_prelude"):
        assert re.search(r"^int\s+" + name + r"\s*\(", src, flags=re.M), name
        assert name in _lib.SIGNATURES, name
    assert "src/trainer.py:6" in src and "src/trainer.py:78" in src


def test_fold_is_a_class_attribute():
    from deepfake_amd.optim import FusedAdamW, FusedSGD
    assert FusedSGD.folds_grad is True and FusedAdamW.folds_grad is True


# ---- torch CPU stand-ins for the three entry points (the formula of include/dfk.h, fp32 state) ----
def _fake_prelude(counters, corr, classes, b1, b2):
    assert len({c for c, _ in classes}) == len(classes)
    for c, gate in classes:
        if gate is not None and float(gate) == 0.0:
            continue
        counters[c] += 1
        t = int(counters[c])
        corr[2 * c] = 1.0 / -math.expm1(t * math.log(b1))
        corr[2 * c + 1] = 1.0 / math.sqrt(-math.expm1(t * math.log(b2)))


def _fake_step(p, grad, m, v, shadow, lr, b1, b2, eps, wd, corr, lr_dev=None, gate=None, grad_scale=1.0,
               grad_bf16=None):
    if gate is not None and float(gate) == 0.0:
        return
    lr = lr_dev[0] if lr_dev is not None else torch.tensor(lr, dtype=torch.float32)
    g = (grad_bf16.float() if grad_bf16 is not None else grad) * grad_scale
    p.mul_(1 - lr * wd)
    m.mul_(b1).add_(g, alpha=1 - b1)
    v.mul_(b2).addcmul_(g, g, value=1 - b2)
    p.sub_((lr * corr[0]) * m / (v.sqrt() * corr[1] + eps))
    if shadow is not None:
        shadow.copy_(p)


def _fake_step_runs(p, grad, m, v, shadow, runs, b1, b2, eps, wd, lr_dev, corr, grad_scale=1.0, grad_bf16=None):
    assert 0 < len(runs) <= 64 and all(s % 4 == 0 and e > s for s, e, _, _ in runs)
    for s, e, gate, c in runs:
        _fake_step(p[s:e], grad[s:e], m[s:e], v[s:e], shadow[s:e] if shadow is not None else None, 0.0, b1, b2, eps,
                   wd, corr[2 * c:2 * c + 2], lr_dev=lr_dev, gate=gate, grad_scale=grad_scale,
                   grad_bf16=grad_bf16[s:e] if grad_bf16 is not None else None)


@pytest.fixture
def cpu_kernels(monkeypatch):
    from deepfake_amd import kernels as K
    monkeypatch.setattr(K, "adamw_prelude", _fake_prelude)
    monkeypatch.setattr(K, "adamw_step", _fake_step)
    monkeypatch.setattr(K, "adamw_step_runs", _fake_step_runs)


class Toy(torch.nn.Module):
    """Three layers of odd sizes; `gated` names the layers whose parameters share one skip flag each."""

    def __init__(self, gated=()):
        super().__init__()
        torch.manual_seed(3)
        self.layers = torch.nn.ModuleList([torch.nn.Linear(7, 13), torch.nn.Linear(13, 5), torch.nn.Linear(5, 3)])
        self.flags = {i: torch.ones(1) for i in gated}

    def param_gates(self):
        return [(list(self.layers[i].parameters()), f) for i, f in self.flags.items()]


def _grads(model, steps, seed=11):
    g = torch.Generator().manual_seed(seed)
    return [[torch.randn(p.shape, generator=g) * 1e-2 for p in model.parameters()] for _ in range(steps)]


def _lr(t):
    return 1e-3 * (1 + math.cos(math.pi * t / 8)) / 2


def _torch_run(model, grads, skip):
    """torch.optim.AdamW on a copy of `model`; skip(t, i): parameter i (registration order) has grad None in step t."""
    m = copy.deepcopy(model)
    ps = list(m.parameters())
    opt = torch.optim.AdamW(ps, lr=_lr(0), betas=BETAS, eps=EPS, weight_decay=WD)
    for t, gs in enumerate(grads):
        opt.param_groups[0]["lr"] = _lr(t)
        for i, (p, g) in enumerate(zip(ps, gs)):
            p.grad = None if skip(t, i) else g.clone()
        opt.step()
    return ps, opt


def _fused_step(model, store, opt, t, gs, touched):
    ps = list(model.parameters())
    opt.set_lr(_lr(t))
    store.zero_grad()
    for i, (p, g) in enumerate(zip(ps, gs)):
        if touched(t, i):
            p.grad.copy_(g)
            store.touched[store.index[id(p)]] = True
    opt.step()


def _close(a, b):
    # the stand-in's fp32 operation order differs from torch's by a few roundings per step
    torch.testing.assert_close(a, b, rtol=2e-6, atol=1e-9)


def test_fused_adamw_matches_torch_over_a_param_store(cpu_kernels):
    """4 steps with a changing lr; parameter 1 (layers.0.bias) never receives a gradient and is never stepped."""
    from deepfake_amd.optim import FusedAdamW
    from deepfake_amd.params import ParamStore
    model = Toy()
    grads = _grads(model, 4)
    ref, ropt = _torch_run(model, grads, skip=lambda t, i: i == 1)
    before = [p.detach().clone() for p in model.parameters()]
    store = ParamStore(model, torch.float32)
    opt = FusedAdamW(store, _lr(0), betas=BETAS, eps=EPS, weight_decay=WD)
    for t, gs in enumerate(grads):
        _fused_step(model, store, opt, t, gs, touched=lambda t, i: i != 1)
    for i, (p, r) in enumerate(zip(model.parameters(), ref)):
        _close(p.detach(), r.detach())
        s, e = store.span(store.index[id(p)])
        if i == 1:
            assert torch.equal(p.detach(), before[1]) and not opt.exp_avg[s:e].any()
        else:
            _close(opt.exp_avg[s:e].view_as(p), ropt.state[r]["exp_avg"])
            _close(opt.exp_avg_sq[s:e].view_as(p), ropt.state[r]["exp_avg_sq"])
    assert opt.counters.tolist() == [4]
    assert opt.param_groups[0]["lr"] == _lr(3) and float(opt.lr_dev) == pytest.approx(_lr(3), rel=1e-7)


def test_no_bookkeeping_steps_every_parameter(cpu_kernels):
    from deepfake_amd.optim import FusedAdamW
    from deepfake_amd.params import ParamStore
    model = Toy()
    grads = _grads(model, 2)
    ref, _ = _torch_run(model, grads, skip=lambda t, i: False)
    store = ParamStore(model, torch.float32)
    opt = FusedAdamW(store, _lr(0), betas=BETAS, eps=EPS, weight_decay=WD)
    for t, gs in enumerate(grads):
        opt.set_lr(_lr(t))
        for p, g in zip(model.parameters(), gs):
            p.grad.copy_(g)          # written behind the store's back: no touched marks
        opt.step()
    for p, r in zip(model.parameters(), ref):
        _close(p.detach(), r.detach())


def test_gated_class_dropped_in_step_one_takes_t1_in_step_two(cpu_kernels):
    """Layer 1's flag is 0 in step 1 and 1 in steps 2-3: torch with grad=None in step 1 (its step count starts
    one later than the others')."""
    from deepfake_amd.optim import FusedAdamW
    from deepfake_amd.params import ParamStore
    model = Toy(gated=(1, 2))
    grads = _grads(model, 3)
    ref, ropt = _torch_run(model, grads, skip=lambda t, i: t == 0 and i in (2, 3))
    store = ParamStore(model, torch.float32)
    opt = FusedAdamW(store, _lr(0), betas=BETAS, eps=EPS, weight_decay=WD)
    assert len(opt.gates) == 3 and sorted(set(opt.cls)) == [0, 1, 2]
    for t, gs in enumerate(grads):
        model.flags[1].fill_(0.0 if t == 0 else 1.0)
        _fused_step(model, store, opt, t, gs, touched=lambda t, i: True)
    for p, r in zip(model.parameters(), ref):
        _close(p.detach(), r.detach())
    c1 = opt.cls[store.index[id(model.layers[1].weight)]]
    c2 = opt.cls[store.index[id(model.layers[2].weight)]]
    assert opt.counters[0] == 3 and opt.counters[c1] == 2 and opt.counters[c2] == 3
    assert int(ropt.state[ref[2]]["step"]) == 2


def test_change_of_touched_set_among_ungated_parameters_raises(cpu_kernels):
    from deepfake_amd.optim import FusedAdamW
    from deepfake_amd.params import ParamStore
    model = Toy()
    grads = _grads(model, 2)
    store = ParamStore(model, torch.float32)
    opt = FusedAdamW(store, 1e-3, weight_decay=WD)
    _fused_step(model, store, opt, 0, grads[0], touched=lambda t, i: True)
    flat = store.flat.clone()
    with pytest.raises(RuntimeError, match=r"layers\.1\.bias"):
        _fused_step(model, store, opt, 1, grads[1], touched=lambda t, i: i != 3)
    assert torch.equal(store.flat, flat) and opt.counters.tolist() == [1]   # raised before anything ran


def test_state_dict_round_trip_is_exact(cpu_kernels):
    """2 steps, state saved and loaded into a fresh optimizer over a fresh store, step 3 == the uninterrupted run."""
    from deepfake_amd.optim import FusedAdamW
    from deepfake_amd.params import ParamStore

    def fresh(src=None):
        model = Toy(gated=(2,))
        if src is not None:
            model.load_state_dict(src.state_dict())
        store = ParamStore(model, torch.float32)
        return model, store, FusedAdamW(store, _lr(0), betas=BETAS, eps=EPS, weight_decay=WD)
    grads = _grads(Toy(), 3)
    ma, sa, oa = fresh()
    for t in range(3):
        _fused_step(ma, sa, oa, t, grads[t], touched=lambda t, i: True)
    mb, sb, ob = fresh()
    for t in range(2):
        _fused_step(mb, sb, ob, t, grads[t], touched=lambda t, i: True)
    sd = ob.state_dict()
    assert {"exp_avg", "exp_avg_sq", "step", "lr", "betas", "eps", "weight_decay"} <= set(sd)
    buf = io.BytesIO()
    torch.save({"optimizer": sd}, buf)            # as Trainer.save_ckpt stores it
    buf.seek(0)
    sd = torch.load(buf, map_location="cpu", weights_only=True)["optimizer"]
    mc, sc, oc = fresh(mb)
    oc.load_state_dict(sd)
    assert oc.param_groups[0]["lr"] == _lr(1) and oc.counters.tolist() == [2, 2]
    _fused_step(mc, sc, oc, 2, grads[2], touched=lambda t, i: True)
    assert torch.equal(sc.flat, sa.flat) and torch.equal(oc.exp_avg, oa.exp_avg)
    assert torch.equal(oc.exp_avg_sq, oa.exp_avg_sq) and torch.equal(oc.counters, oa.counters)


def test_hyper_parameters_are_validated():
    from deepfake_amd.optim import FusedAdamW
    from deepfake_amd.params import ParamStore
    store = ParamStore(Toy(), torch.float32)
    for kw in ({"betas": (1.0, 0.999)}, {"betas": (0.9, -0.1)}, {"eps": 0.0}):
        with pytest.raises(ValueError):
            FusedAdamW(store, 1e-3, **kw)
