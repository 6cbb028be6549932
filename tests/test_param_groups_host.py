"""CPU: the host side of parameter groups (deepfake_amd.optim.ParamGroups, FusedSGD / FusedAdamW with groups=) — the
flags, the ABI tables, the no-decay rule on the real models, prefix matching, the byte map, and the optimizers'
runs, lr plumbing and checkpoint state, with the two new kernel entry points (K.sgd_step_runs_groups /
K.adamw_step_runs_groups) and K.adamw_prelude replaced by a torch CPU evaluation of the formulas of include/dfk.h.
The kernels themselves are tested on the device (tests/test_gpu_param_groups.py)."""
import copy
import io
import os
import re

import pytest
import torch

from test_adamw_host import BETAS, EPS, WD, Toy, _close, _fake_prelude, _fake_step, _fused_step, _grads, _lr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYWORDS = ("relative_position_bias_table", "absolute_pos_embed", "cpb_mlp", "logit_scale")
TRUNKS = {"vExtract": 0.1, "aExtract": 0.1, "paExtract": 0.1}


def test_flags_parse_and_default_to_one_group():
    from config import get_opt
    from deepfake_amd.trainer import groups_arg
    a = get_opt([])
    assert (a.no_decay, a.lr_scale) == ("none", []) and groups_arg(a) is None
    b = get_opt(["--no_decay", "norm_bias", "--lr_scale", "vExtract=0.1", "--lr_scale", "aExtract.encoder=0.5"])
    assert groups_arg(b) == {"no_decay": "norm_bias", "lr_scale": {"vExtract": 0.1, "aExtract.encoder": 0.5}}
    assert groups_arg(get_opt(["--lr_scale", "classify=10"])) == {"no_decay": "none", "lr_scale": {"classify": 10.0}}
    with pytest.raises(SystemExit):
        get_opt(["--no_decay", "all"])
    for bad in ("vExtract", "=0.1", "vExtract=fast"):
        with pytest.raises(ValueError, match="PREFIX=MULT"):
            groups_arg(get_opt(["--lr_scale", bad]))


def test_help_lists_the_group_flags(capsys):
    from config import get_opt
    with pytest.raises(SystemExit) as e:
        get_opt(["--help"])
    assert e.value.code == 0
    out = capsys.readouterr().out
    assert "--no_decay" in out and "--lr_scale" in out and "PREFIX=MULT" in out


def test_entry_points_in_header_and_binding_table():
    from deepfake_amd import _lib
    src = open(os.path.join(ROOT, "include", "dfk.h")).read()
    for name in ("dfk_sgd_step_runs_groups", "dfk_adamw_step_runs_groups"):
        assert re.search(r"^int\s+" + name + r"\s*\(", src, flags=re.M), name
        assert name in _lib.SIGNATURES, name
    assert len(_lib.SIGNATURES["dfk_sgd_step_runs_groups"]) == 17
    assert len(_lib.SIGNATURES["dfk_adamw_step_runs_groups"]) == 22
    assert "src/trainer.py:80-82" in src


@pytest.mark.parametrize("config,tensors,exempt,elements", [("c1", 341, 237, 221766), ("c2", 825, 581, 924384)])
def test_norm_bias_rule_on_the_real_models(config, tensors, exempt, elements):
    """The rule on the fused model: every exempt tensor is 1-D (or a scalar) or carries one of the four keywords, and
    no other tensor is exempt; the counts are those of the layouts the models have today."""
    from deepfake_amd.models.fused import build_fused
    from deepfake_amd.optim import ParamGroups
    from deepfake_amd.params import ParamStore
    model = build_fused(config, compute_dtype=torch.float32)
    store = ParamStore(model, torch.float32)
    g = ParamGroups(model, store, 0.05, no_decay="norm_bias")
    assert [(r[0], r[1]) for r in g.summary()] in ([(1.0, 0.05), (1.0, 0.0)], [(1.0, 0.0), (1.0, 0.05)])
    named = dict(model.named_parameters())
    assert len(g.spec) == len(store.params) == tensors
    got = {n for n, (_, wd) in g.spec.items() if wd == 0.0}
    want = {n for n, p in named.items() if n in g.spec and (p.ndim <= 1 or any(k in n for k in KEYWORDS))}
    assert got == want
    assert len(got) == exempt and sum(named[n].numel() for n in got) == elements
    off = next(r for r in g.summary() if r[1] == 0.0)
    assert off[2:] == (exempt, elements)
    assert any(named[n].ndim > 1 for n in got), "no keyword-only exemption in the model"
    # the map: every parameter's cells carry its group, and the trunks take their multiplier on top
    g2 = ParamGroups(model, store, 0.05, no_decay="norm_bias", lr_scale=TRUNKS)
    assert sorted((r[0], r[1]) for r in g2.summary()) == [(0.1, 0.0), (0.1, 0.05), (1.0, 0.0), (1.0, 0.05)]
    pairs = [(d["lr_scale"], d["weight_decay"]) for d in g2.param_groups]
    for i in range(len(store.params)):
        s, e = store.span(i)
        cells = g2.group_map[s // 8:-(-e // 8)]
        assert (cells == pairs.index(g2.spec[store.name(i)])).all(), store.name(i)
    for n, (mult, _) in g2.spec.items():
        assert mult == (0.1 if n.split(".")[0] in TRUNKS else 1.0), n


def test_prefix_matching_and_errors():
    from deepfake_amd.optim import ParamGroups
    from deepfake_amd.params import ParamStore
    model = Toy()
    store = ParamStore(model, torch.float32)
    g = ParamGroups(model, store, WD, lr_scale={"layers": 0.5, "layers.1": 2.0, "layers.1.bias": 4.0})
    want = {"layers.0.weight": 0.5, "layers.0.bias": 0.5, "layers.1.weight": 2.0, "layers.1.bias": 4.0,
            "layers.2.weight": 0.5, "layers.2.bias": 0.5}
    assert {n: m for n, (m, _) in g.spec.items()} == want
    assert [d["lr_scale"] for d in g.param_groups] == [0.5, 2.0, 4.0]                 # first-seen order
    assert g.param_groups[0]["params"] == ["layers.0.weight", "layers.0.bias", "layers.2.weight", "layers.2.bias"]
    assert {n: m for n, (m, _) in ParamGroups(model, store, WD).spec.items()} == {n: 1.0 for n in want}
    with pytest.raises(ValueError, match="'head'"):
        ParamGroups(model, store, WD, lr_scale={"layers.0": 0.5, "head": 2.0})
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="multiplier"):
            ParamGroups(model, store, WD, lr_scale={"layers.0": bad})
    with pytest.raises(ValueError, match="no_decay"):
        ParamGroups(model, store, WD, no_decay="bias")


def test_257_groups_raise():
    from deepfake_amd.optim import ParamGroups
    from deepfake_amd.params import ParamStore

    def wide(n):
        m = torch.nn.Module()
        m.w = torch.nn.ParameterList([torch.nn.Parameter(torch.zeros(3)) for _ in range(n)])
        return m, {f"w.{i}": 1.0 + i for i in range(n)}
    model, scale = wide(256)
    # w.1 is also a prefix of w.10 ...: the longest prefix still gives every tensor its own multiplier
    g = ParamGroups(model, ParamStore(model, torch.float32), WD, lr_scale=scale)
    assert len(g.param_groups) == 256 and int(g.group_map.max()) == 255
    model, scale = wide(257)
    with pytest.raises(ValueError, match="256"):
        ParamGroups(model, ParamStore(model, torch.float32), WD, lr_scale=scale)


class Grouped(torch.nn.Module):
    """A store with an adjacency group and a zero gap, as SwinV2's (q_bias, 0, v_bias): registration order a, q, v,
    w, so the flat order is w, (q, gap 8, v), a."""

    def __init__(self):
        super().__init__()
        self.a = torch.nn.Parameter(torch.ones(5))
        self.q = torch.nn.Parameter(torch.ones(8))
        self.v = torch.nn.Parameter(torch.ones(16))
        self.w = torch.nn.Parameter(torch.ones(3, 7))

    def flat_groups(self):
        return [[self.q, 8, self.v]]


def test_map_of_a_toy_store_equals_the_layout_by_hand():
    from deepfake_amd.optim import ParamGroups
    from deepfake_amd.params import ParamStore
    model = Grouped()
    store = ParamStore(model, torch.float32)
    # w: 21 elements at 0 (3 cells, 3 padding elements in the last); q at 24 (1 cell); gap 32..40 (1 cell);
    # v at 40 (2 cells); a: 5 elements at 56 (1 cell, 3 padding elements)
    assert [store.name(i) for i in range(4)] == ["w", "q", "v", "a"] and store.offsets == [0, 24, 40, 56]
    assert store.numel == 64
    g = ParamGroups(model, store, WD, no_decay="norm_bias", lr_scale={"v": 3.0})
    # first seen in registration order: a (1, 0) -> 0, v (3, 0) -> 1, w (1, WD) -> 2; q joins group 0
    assert [(d["lr_scale"], d["weight_decay"], d["params"]) for d in g.param_groups] == \
        [(1.0, 0.0, ["a", "q"]), (3.0, 0.0, ["v"]), (1.0, WD, ["w"])]
    assert g.group_map.dtype == torch.uint8
    assert g.group_map.tolist() == [2, 2, 2, 0, 0, 1, 1, 0]
    assert g.group_hyper.dtype == torch.float32
    assert torch.equal(g.group_hyper, torch.tensor([[1.0, 0.0], [3.0, 0.0], [1.0, WD]]))
    assert g.summary() == [(1.0, 0.0, 2, 13), (3.0, 0.0, 1, 16), (1.0, WD, 1, 21)]


# ---- torch CPU stand-ins for the two groups entry points: per map cell, the plain stand-in at the cell's pair ----
def _cells(runs, group_map, group_hyper):
    assert 0 < len(runs) <= 64 and all(s % 4 == 0 and e > s for s, e, _, _ in runs)
    assert group_map.dtype == torch.uint8 and group_hyper.dtype == torch.float32 and group_hyper.shape[1] == 2
    last = group_hyper.shape[0] - 1
    for s, e, gate, x in runs:
        assert group_map.numel() >= -(-e // 8)
        a = s
        while a < e:
            b = min(e, (a // 8 + 1) * 8)
            mult, wd = group_hyper[min(int(group_map[a // 8]), last)].tolist()
            yield a, b, gate, x, torch.tensor(mult, dtype=torch.float32), wd
            a = b


def _fake_adamw_groups(p, grad, m, v, shadow, runs, b1, b2, eps, lr_dev, corr, group_map, group_hyper, grad_scale=1.0,
                       grad_bf16=None, clip_coef=None):
    CALLS.append(("adamw", len(runs)))
    assert clip_coef is None
    for a, b, gate, c, mult, wd in _cells(runs, group_map, group_hyper):
        _fake_step(p[a:b], grad[a:b], m[a:b], v[a:b], None, 0.0, b1, b2, eps, wd, corr[2 * c:2 * c + 2],
                   lr_dev=lr_dev * mult, gate=gate, grad_scale=grad_scale)


def _fake_sgd_groups(p, grad, buf, shadow, runs, momentum, lr_dev, group_map, group_hyper, grad_scale=1.0,
                     grad_bf16=None, clip_coef=None):
    CALLS.append(("sgd", len(runs)))
    assert clip_coef is None
    for a, b, gate, first, mult, wd in _cells(runs, group_map, group_hyper):
        if gate is not None and float(gate) == 0.0:
            continue
        g = grad[a:b] * grad_scale + wd * p[a:b]
        buf[a:b] = g if first else momentum * buf[a:b] + g
        p[a:b] -= (lr_dev[0] * mult) * buf[a:b]


def _fake_sgd_runs(p, grad, buf, shadow, runs, momentum, wd, lr_dev, grad_scale=1.0, grad_bf16=None):
    CALLS.append(("sgd_plain", len(runs)))


def _fake_adamw_runs(p, grad, m, v, shadow, runs, b1, b2, eps, wd, lr_dev, corr, grad_scale=1.0, grad_bf16=None):
    CALLS.append(("adamw_plain", len(runs)))


CALLS = []


@pytest.fixture
def cpu_kernels(monkeypatch):
    from deepfake_amd import kernels as K
    del CALLS[:]
    monkeypatch.setattr(K, "adamw_prelude", _fake_prelude)
    monkeypatch.setattr(K, "adamw_step_runs_groups", _fake_adamw_groups)
    monkeypatch.setattr(K, "sgd_step_runs_groups", _fake_sgd_groups)
    monkeypatch.setattr(K, "sgd_step_runs", _fake_sgd_runs)
    monkeypatch.setattr(K, "adamw_step_runs", _fake_adamw_runs)


SCALE = {"layers.0": 0.1, "layers.2": 10.0}


def _torch_groups(model, groups, make):
    """torch's optimizer over a copy of `model` with the param groups of `groups`; returns (params, optimizer)."""
    m = copy.deepcopy(model)
    named = dict(m.named_parameters())
    opt = make([{"params": [named[n] for n in d["params"]], "lr": _lr(0) * d["lr_scale"],
                 "weight_decay": d["weight_decay"]} for d in groups.param_groups])
    return m, opt


def _torch_steps(m, opt, groups, grads):
    for t, gs in enumerate(grads):
        for pg, d in zip(opt.param_groups, groups.param_groups):
            pg["lr"] = _lr(t) * d["lr_scale"]
        for p, g in zip(m.parameters(), gs):
            p.grad = g.clone()
        opt.step()


def test_fused_adamw_with_groups_matches_torch(cpu_kernels):
    from deepfake_amd.optim import FusedAdamW, ParamGroups
    from deepfake_amd.params import ParamStore
    model = Toy()
    grads = _grads(model, 4)
    store = ParamStore(model, torch.float32)
    groups = ParamGroups(model, store, WD, no_decay="norm_bias", lr_scale=SCALE)
    assert len(groups.param_groups) == 6
    ref, ropt = _torch_groups(model, groups, lambda pg: torch.optim.AdamW(pg, lr=_lr(0), betas=BETAS, eps=EPS))
    _torch_steps(ref, ropt, groups, grads)
    opt = FusedAdamW(store, _lr(0), betas=BETAS, eps=EPS, weight_decay=WD, groups=groups)
    for t, gs in enumerate(grads):
        _fused_step(model, store, opt, t, gs, touched=lambda t, i: True)
    for p, r in zip(model.parameters(), ref.parameters()):
        _close(p.detach(), r.detach())
        s, e = store.span(store.index[id(p)])
        _close(opt.exp_avg[s:e].view_as(p), ropt.state[r]["exp_avg"])
        _close(opt.exp_avg_sq[s:e].view_as(p), ropt.state[r]["exp_avg_sq"])
    assert CALLS == [("adamw", 1)] * 4


def test_fused_sgd_with_groups_matches_torch(cpu_kernels):
    from deepfake_amd.optim import FusedSGD, ParamGroups
    from deepfake_amd.params import ParamStore
    model = Toy()
    grads = _grads(model, 4)
    store = ParamStore(model, torch.float32)
    groups = ParamGroups(model, store, WD, no_decay="norm_bias", lr_scale=SCALE)
    ref, ropt = _torch_groups(model, groups, lambda pg: torch.optim.SGD(pg, lr=_lr(0), momentum=0.9))
    _torch_steps(ref, ropt, groups, grads)
    opt = FusedSGD(store, _lr(0), momentum=0.9, weight_decay=WD, groups=groups)
    for t, gs in enumerate(grads):
        _fused_step(model, store, opt, t, gs, touched=lambda t, i: True)
    for p, r in zip(model.parameters(), ref.parameters()):
        _close(p.detach(), r.detach())
        s, e = store.span(store.index[id(p)])
        _close(opt.buf[s:e].view_as(p), ropt.state[r]["momentum_buffer"])
    assert CALLS == [("sgd", 1)] * 4


@pytest.mark.parametrize("which", ["sgd", "adamw"])
def test_groups_issue_the_runs_of_the_plain_step(cpu_kernels, which):
    """The groups split no run: a gated layer in the middle makes three runs with groups and without."""
    from deepfake_amd.optim import FusedAdamW, FusedSGD, ParamGroups
    from deepfake_amd.params import ParamStore
    counts = []
    for with_groups in (False, True):
        del CALLS[:]
        model = Toy(gated=(1,))
        store = ParamStore(model, torch.float32)
        groups = ParamGroups(model, store, WD, no_decay="norm_bias", lr_scale=SCALE) if with_groups else None
        opt = FusedSGD(store, 1e-3, weight_decay=WD, groups=groups) if which == "sgd" else \
            FusedAdamW(store, 1e-3, weight_decay=WD, groups=groups)
        _fused_step(model, store, opt, 0, _grads(model, 1)[0], touched=lambda t, i: True)
        counts.append(list(CALLS))
    assert counts == [[(which + "_plain", 3)], [(which, 3)]]


def test_set_lr_scales_every_group(cpu_kernels):
    from deepfake_amd.optim import CosineAnnealingLR, FusedSGD, ParamGroups
    from deepfake_amd.params import ParamStore
    model = Toy()
    store = ParamStore(model, torch.float32)
    groups = ParamGroups(model, store, WD, lr_scale=SCALE)
    assert all(d["lr"] is None for d in groups.param_groups)
    opt = FusedSGD(store, 1e-2, weight_decay=WD, groups=groups)
    assert opt.param_groups is groups.param_groups
    assert [(d["lr"], d["initial_lr"], d["lr_scale"]) for d in opt.param_groups] == \
        [(1e-2 * 0.1, 1e-2 * 0.1, 0.1), (1e-2, 1e-2, 1.0), (1e-2 * 10.0, 1e-2 * 10.0, 10.0)]
    sched = CosineAnnealingLR(opt, T_max=4)
    sched.step()
    lr = sched.get_lr()
    assert lr < 1e-2 and float(opt.lr_dev) == pytest.approx(lr, rel=1e-7)
    assert [d["lr"] for d in opt.param_groups] == [lr * 0.1, lr, lr * 10.0]
    assert [d["initial_lr"] for d in opt.param_groups] == [1e-2 * 0.1, 1e-2, 1e-2 * 10.0]
    with pytest.raises(ValueError, match="another parameter store"):
        FusedSGD(ParamStore(Toy(), torch.float32), 1e-2, groups=groups)


def test_state_round_trips_and_another_layout_raises(cpu_kernels):
    from deepfake_amd.optim import FusedAdamW, FusedSGD, ParamGroups
    from deepfake_amd.params import ParamStore

    def fresh(src=None, scale=SCALE, no_decay="norm_bias"):
        model = Toy(gated=(2,))
        if src is not None:
            model.load_state_dict(src.state_dict())
        store = ParamStore(model, torch.float32)
        groups = ParamGroups(model, store, WD, no_decay=no_decay, lr_scale=scale) if scale is not None else None
        return model, store, FusedAdamW(store, _lr(0), betas=BETAS, eps=EPS, weight_decay=WD, groups=groups)
    grads = _grads(Toy(), 3)
    ma, sa, oa = fresh()
    for t in range(3):
        _fused_step(ma, sa, oa, t, grads[t], touched=lambda t, i: True)
    mb, sb, ob = fresh()
    for t in range(2):
        _fused_step(mb, sb, ob, t, grads[t], touched=lambda t, i: True)
    sd = ob.state_dict()
    assert sd["groups"]["layers.2.bias"] == (10.0, 0.0) and sd["groups"]["layers.1.weight"] == (1.0, WD)
    assert sd["lr"] == _lr(1)
    buf = io.BytesIO()
    torch.save({"optimizer": sd}, buf)            # as Trainer.save_ckpt stores it
    buf.seek(0)
    sd = torch.load(buf, map_location="cpu", weights_only=True)["optimizer"]
    mc, sc, oc = fresh(mb)
    oc.load_state_dict(sd)
    assert [d["lr"] for d in oc.param_groups] == [_lr(1) * d["lr_scale"] for d in oc.param_groups]
    _fused_step(mc, sc, oc, 2, grads[2], touched=lambda t, i: True)
    assert torch.equal(sc.flat, sa.flat) and torch.equal(oc.exp_avg, oa.exp_avg)
    assert torch.equal(oc.exp_avg_sq, oa.exp_avg_sq) and torch.equal(oc.counters, oa.counters)
    for kw in ({"scale": {"layers.0": 0.2, "layers.2": 10.0}}, {"no_decay": "none"}, {"scale": None}):
        with pytest.raises(ValueError, match="groups"):
            fresh(mb, **kw)[2].load_state_dict(sd)
    with pytest.raises(ValueError, match="groups"):       # a state without groups into an optimizer with them
        fresh(mb)[2].load_state_dict({k: v for k, v in sd.items() if k != "groups"})
    m, st, _ = fresh()
    sgd = FusedSGD(st, 1e-3, groups=ParamGroups(m, st, WD, lr_scale=SCALE))
    assert sgd.state_dict()["groups"]["layers.0.weight"] == (0.1, WD)
