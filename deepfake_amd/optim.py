"""Fused SGD / AdamW + CosineAnnealingLR over a ParamStore (src/trainer.py:80-85,295-297; AdamW: :6,78).

FusedSGD: torch.optim.SGD(lr, momentum=0.9, weight_decay=wd) semantics (dampening 0,
no nesterov; first step buf = g) in one HBM-bound kernel over the flat fp32
buffer, which also rewrites the bf16 compute shadow.  The learning rate lives
in device memory so a captured graph replays with the scheduler's current lr.
FusedAdamW: torch.optim.AdamW(betas, eps, weight_decay) in the same form, its
step counts in device memory too (one per LayerDrop gate class), so a replayed
graph takes the right bias corrections.
max_grad_norm (both): torch.nn.utils.clip_grad_norm_(params, max_grad_norm) on the mean gradient right before the
step, on the device: one reduction pass over the step's runs, a one-workgroup coefficient kernel, and update
kernels that multiply the gradient by the coefficient they read from device memory.
ParamEMA: an exponential moving average of the whole flat store, updated by one kernel right after the optimizer step
(its update count and decay warm-up in device memory, so it replays inside the captured step) and exchanged with the
live weights for evaluation, so the model itself evaluates through the average ("Weight EMA").
ParamGroups (both optimizers, groups=): a learning-rate multiplier and a weight decay per group of parameters, as
torch.optim's param groups (no decay on norm / bias / position parameters, another lr for the new head), looked up
per quad by the dfk_*_step_runs_groups kernels through a byte map of the store, so the groups split no run
("Parameter groups").
"""
import contextlib
import math

import torch

from . import kernels as K


# every run in one dfk_sgd_step_runs launch (profiles/step/r6j_sgd_one_launch.txt); False (tests set it): one
# dfk_sgd_step launch per run
_RUNS = True


NO_DECAY_KEYWORDS = ("relative_position_bias_table", "absolute_pos_embed", "cpb_mlp", "logit_scale")


class ParamGroups:
    """Which (lr multiplier, weight decay) every parameter of a ParamStore takes.

    no_decay: "none" — every parameter decays by `weight_decay` (torch's single group); "norm_bias" — weight decay 0
      for a parameter with ndim <= 1 (LayerNorm / BatchNorm gains and biases, every bias) or whose name contains one
      of NO_DECAY_KEYWORDS: the no_weight_decay() / no_weight_decay_keywords() sets of the Swin and SwinV2 recipes.
    lr_scale: {name prefix: multiplier}; a parameter takes the multiplier of the longest prefix its name starts with,
      1.0 without one.  A prefix that matches no parameter, and a multiplier that is not finite or <= 0, raise.
    The groups are the distinct (multiplier, decay) pairs in the order model.named_parameters() first shows them, at
    most 256.  Built once: group_map (device uint8, one byte per 8 elements of the store: the group index of the
    parameter that owns the cell, 0 in flat_groups() gaps) and group_hyper (device fp32 [groups][2] = (multiplier,
    decay), read by the kernels at every launch, so an entry overwritten in place acts from the next step on, also in
    a replayed graph).  param_groups is torch's list: {"lr", "initial_lr", "weight_decay", "lr_scale", "params":
    [names]}; the two rates are None until an optimizer is built over the groups and fills them in."""

    def __init__(self, model, store, weight_decay, no_decay="none", lr_scale=None):
        if no_decay not in ("none", "norm_bias"):
            raise ValueError(f"ParamGroups: no_decay is 'none' or 'norm_bias', got {no_decay!r}")
        scale = {str(k): float(v) for k, v in (lr_scale or {}).items()}
        for k, v in scale.items():
            if not (math.isfinite(v) and v > 0.0):
                raise ValueError(f"ParamGroups: lr_scale[{k!r}] must be a positive finite multiplier, got {v}")
        self.store, self.weight_decay, self.no_decay, self.lr_scale = store, float(weight_decay), no_decay, scale
        used, keys, self.spec, members = set(), {}, {}, []
        cell = K.GROUP_CELL
        if any(o % cell for o in store.offsets):
            raise ValueError(f"ParamGroups: the store places a parameter off a multiple of {cell} elements")
        gmap = torch.zeros(-(-store.numel // cell), dtype=torch.uint8)
        for name, p in model.named_parameters():
            i = store.index.get(id(p))
            if i is None or name in self.spec:
                continue
            hit = max((k for k in scale if name.startswith(k)), key=len, default=None)
            used.add(hit)
            exempt = no_decay == "norm_bias" and (p.ndim <= 1 or any(w in name for w in NO_DECAY_KEYWORDS))
            pair = (scale[hit] if hit is not None else 1.0, 0.0 if exempt else self.weight_decay)
            if pair not in keys:
                if len(keys) == K.GROUPS_MAX:
                    raise ValueError(f"ParamGroups: more than {K.GROUPS_MAX} distinct (lr_scale, weight_decay) pairs")
                keys[pair] = len(keys)
                members.append([])
            members[keys[pair]].append(name)
            self.spec[name] = pair
            s, e = store.span(i)
            gmap[s // cell:-(-e // cell)] = keys[pair]
        unused = sorted(k for k in scale if k not in used)
        if unused:
            raise ValueError(f"ParamGroups: lr_scale prefix {unused[0]!r} matches no parameter")
        dev = store.flat.device
        self.group_map = gmap.to(dev)
        self.group_hyper = torch.tensor(list(keys), dtype=torch.float32).reshape(-1, 2).to(dev)
        self.param_groups = [{"lr": None, "initial_lr": None, "weight_decay": wd, "lr_scale": mult, "params": names}
                             for (mult, wd), names in zip(keys, members)]

    def bind(self, lr):
        """The param_groups at base rate `lr` (an optimizer's constructor calls this)."""
        for g in self.param_groups:
            g["lr"] = g["initial_lr"] = float(lr) * g["lr_scale"]
        return self.param_groups

    def summary(self):
        """[(lr_scale, weight_decay, tensors, elements)] per group, for the log."""
        numel = {self.store.name(i): p.numel() for i, p in enumerate(self.store.params)}
        return [(g["lr_scale"], g["weight_decay"], len(g["params"]), sum(numel[n] for n in g["params"]))
                for g in self.param_groups]

    def check_spec(self, spec, who):
        """Raise unless `spec` (a state_dict's "groups") names this layout: the same parameters with the same pairs."""
        got = None if spec is None else {k: (float(v[0]), float(v[1])) for k, v in spec.items()}
        if got != self.spec:
            raise ValueError(f"{who}.load_state_dict: the state's parameter groups were built for another layout")


class _Fused:
    """What FusedSGD and FusedAdamW share: the store, the learning rate in device memory (a captured graph replays
    with the scheduler's current lr), and the device state of global-norm clipping, allocated once: the fp64 partial
    slabs (one per chunk of 64 runs the store can produce) and the fp32 pair grad_norm = {norm, coef} of the last
    step."""
    folds_grad = True   # step() takes the all-reduced sum and 1 / world itself (TrainStep._fold)

    def __init__(self, store, lr, max_grad_norm, groups=None):
        self.store = store
        self.base_lr = self.lr = float(lr)     # lr: the one device rate, before any group's multiplier
        dev = store.flat.device
        self.lr_dev = torch.full((1,), self.base_lr, device=dev, dtype=torch.float32)
        if groups is not None and groups.store is not store:
            raise ValueError(f"{type(self).__name__}: groups were built over another parameter store")
        self.groups = groups
        self.param_groups = [{"lr": self.base_lr, "initial_lr": self.base_lr}] if groups is None else \
            groups.bind(self.base_lr)
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.grad_norm = self._partials = None
        if self.max_grad_norm is None:
            return
        if not (self.max_grad_norm > 0.0 and math.isfinite(self.max_grad_norm)):
            raise ValueError(f"{type(self).__name__}: max_grad_norm must be a positive float or None, "
                             f"got {max_grad_norm}")
        chunks = max(1, -(-len(store.params) // K.SGD_MAX_RUNS))       # at most one run per parameter
        self._partials = torch.zeros(chunks * K.GNORM_PARTIALS, device=dev, dtype=torch.float64)
        self.grad_norm = torch.zeros(2, device=dev, dtype=torch.float32)

    def set_lr(self, lr):
        """One device rate for every group (the kernels multiply by the group's lr_scale); each group's "lr" is the
        rate it steps at."""
        for g in self.param_groups:
            g["lr"] = float(lr) * g.get("lr_scale", 1.0)
        self.lr = float(lr)
        self.lr_dev.fill_(float(lr))

    def _group_state(self):
        return {} if self.groups is None else {"groups": dict(self.groups.spec)}

    def _check_groups(self, sd):
        if self.groups is not None:
            self.groups.check_spec(sd.get("groups"), type(self).__name__)
        elif sd.get("groups") is not None:
            raise ValueError(f"{type(self).__name__}.load_state_dict: the state carries parameter groups, this "
                             f"optimizer has none")

    def zero_grad(self):
        self.store.zero_grad()

    def _clip(self, runs, grad_scale, grad_bf16):
        """norm and coefficient of this step's runs [(start, end, gate)] -> the device coefficient, or None when
        clipping is off.  Two launches per 64 runs + one; nothing is allocated and nothing read on the host."""
        if self.max_grad_norm is None:
            return None
        n = K.grad_sqnorm_runs(self.store.grad, runs, self._partials, grad_scale=grad_scale, grad_bf16=grad_bf16)
        K.grad_clip_coef(self._partials, n, self.max_grad_norm, self.grad_norm)
        return self.grad_norm[1:2]

    @staticmethod
    def _cut(x, s, e):
        """x[s:e] of an optional flat buffer (the shadow, the bf16 bucket gradient)"""
        return x[s:e] if x is not None else None


class FusedSGD(_Fused):
    def __init__(self, store, lr, momentum=0.9, weight_decay=0.0, max_grad_norm=None, groups=None):
        super().__init__(store, lr, max_grad_norm, groups)
        self.momentum, self.weight_decay = float(momentum), float(weight_decay)
        self.buf = torch.zeros_like(store.flat)
        self.first = True
        self.has_buf = [False] * len(store.params)   # torch: momentum buffer created at a param's first grad

    def step(self, first=None, grad_scale=1.0, grad_bf16=None):
        """One SGD step over the parameters that received a gradient (torch skips grad=None:
        no weight decay and no momentum for them): every contiguous run in one dfk_sgd_step_runs launch (one
        dfk_sgd_step per run beyond 64 runs, or with _RUNS off).
        grad_scale / grad_bf16: the data-parallel fold of GradBucketer.finish(fold=True) — the gradient is the
        all-reduced sum (in the fp32 buffer, or in the bf16 bucket copy) times 1 / world.
        With groups (ParamGroups): the same runs through dfk_sgd_step_runs_groups, 64 per launch, each quad taking
        its group's lr multiplier and weight decay (the constructor's weight_decay is not read); the norm of a
        clipped step is over all groups; _RUNS is ignored (the groups kernels have no one-run form)."""
        st = self.store
        gates = {id(g): g for g in st.gate if g is not None}
        gkey = [id(g) if g is not None else None for g in st.gate]
        if not any(st.touched):          # no bookkeeping (e.g. a captured replay): every parameter
            f0 = self.first if first is None else first
            runs = st.touched_runs(also=[(f0, k) for k in gkey], every=True)
        else:
            runs = st.touched_runs(also=[(not h, k) for h, k in zip(self.has_buf, gkey)])
            for i, t in enumerate(st.touched):
                if t:
                    self.has_buf[i] = True
        # a LayerDrop-gated run is skipped on the device when its layer was dropped this step
        ck = {}
        if self.max_grad_norm is not None and runs:   # the norm of the same runs, gates and fold, then the _clip twins
            ck["clip_coef"] = self._clip([(s, e, gates.get(k)) for s, e, (f, k) in runs], grad_scale, grad_bf16)
        if self.groups is not None:
            tab = [(s, e, gates.get(k), f) for s, e, (f, k) in runs]
            for c in range(0, len(tab), K.SGD_MAX_RUNS):
                K.sgd_step_runs_groups(st.flat, st.grad, self.buf, st.shadow, tab[c:c + K.SGD_MAX_RUNS],
                                       self.momentum, self.lr_dev, self.groups.group_map, self.groups.group_hyper,
                                       grad_scale=grad_scale, grad_bf16=grad_bf16, **ck)
            self.first = False
            return
        if _RUNS and 0 < len(runs) <= K.SGD_MAX_RUNS:
            K.sgd_step_runs(st.flat, st.grad, self.buf, st.shadow, [(s, e, gates.get(k), f) for s, e, (f, k) in runs],
                            self.momentum, self.weight_decay, self.lr_dev, grad_scale=grad_scale,
                            grad_bf16=grad_bf16, **ck)
            self.first = False
            return
        for s, e, (f, k) in runs:
            K.sgd_step(st.flat[s:e], st.grad[s:e], self.buf[s:e], self._cut(st.shadow, s, e), 0.0, self.momentum,
                       self.weight_decay, bool(f), lr_dev=self.lr_dev, gate=gates.get(k), grad_scale=grad_scale,
                       grad_bf16=self._cut(grad_bf16, s, e), **ck)
        self.first = False

    def state_dict(self):
        """With groups also "groups": {parameter name: (lr_scale, weight_decay)}, the layout the state belongs to."""
        return {"momentum_buffer": self.buf, "lr": self.lr, "first": self.first, **self._group_state()}


class FusedAdamW(_Fused):
    """torch.optim.AdamW(lr, betas, eps, weight_decay; amsgrad / maximize off) with FusedSGD's surface.

    Step counts are int32 device memory, one per gate class: class 0 holds the ungated parameters, every distinct
    LayerDrop flag of ParamStore.gate its own class.  Each step first runs the prelude kernel, which advances the
    counter of every class whose gate is open and writes its bias corrections, then the update over the runs
    (dfk_adamw_step_runs; one dfk_adamw_step per run beyond 64 runs).  A gated-off class keeps parameters, moments,
    shadow and counter, as torch leaves a grad=None parameter, so a layer dropped in step 1 takes t = 1 in step 2."""

    def __init__(self, store, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, max_grad_norm=None, groups=None):
        b1, b2 = float(betas[0]), float(betas[1])
        if not (0.0 <= b1 < 1.0 and 0.0 <= b2 < 1.0) or not float(eps) > 0.0:
            raise ValueError(f"FusedAdamW: betas must lie in [0, 1) and eps be positive, got {betas}, {eps}")
        super().__init__(store, lr, max_grad_norm, groups)
        self.betas, self.eps, self.weight_decay = (b1, b2), float(eps), float(weight_decay)
        dev = store.flat.device
        self.exp_avg = torch.zeros_like(store.flat)
        self.exp_avg_sq = torch.zeros_like(store.flat)
        self.gates, self.cls, seen = [None], [], {}
        for g in store.gate:
            if g is not None and id(g) not in seen:
                seen[id(g)] = len(self.gates)
                self.gates.append(g)
            self.cls.append(0 if g is None else seen[id(g)])
        if len(self.gates) > K.ADAMW_MAX_CLASSES:
            raise ValueError(f"FusedAdamW: {len(self.gates)} gate classes, at most {K.ADAMW_MAX_CLASSES}")
        self.counters = torch.zeros(len(self.gates), device=dev, dtype=torch.int32)
        self.corr = torch.zeros(2 * len(self.gates), device=dev, dtype=torch.float32)
        self.active = None   # per parameter: stepped by the eager steps so far (fixed at the first step)

    def step(self, first=None, grad_scale=1.0, grad_bf16=None):
        """One AdamW step over the parameters that received a gradient (all of them without bookkeeping, e.g. under
        a capture that ran no backward).  `first` is FusedSGD's and ignored: zero moments and the device counters
        need no first-step flag.  grad_scale / grad_bf16: the data-parallel fold, as FusedSGD.step.
        The ungated parameters share one counter, so each must be stepped in every step or in none: one whose
        gradient appears or disappears between steps would need its own count (torch keeps one per parameter).
        With groups (ParamGroups): the same runs through dfk_adamw_step_runs_groups, 64 per launch, as
        FusedSGD.step."""
        st = self.store
        every = not any(st.touched)
        touched = [True] * len(st.params) if every else list(st.touched)
        if self.active is None:
            self.active = touched
        for i, (t, a) in enumerate(zip(touched, self.active)):
            if st.gate[i] is None and t != a:
                raise RuntimeError(f"FusedAdamW: parameter {st.name(i)} {'received a gradient' if t else 'got none'} "
                                   f"in this step but {'none' if t else 'one'} before; the ungated parameters "
                                   f"share one device step count, so its bias correction would be wrong")
        runs = st.touched_runs(also=self.cls, every=every)
        if not runs:
            return
        b1, b2 = self.betas
        ck = {}
        if self.max_grad_norm is not None:    # norm and coefficient first, then the prelude and the _clip twins
            ck["clip_coef"] = self._clip([(s, e, self.gates[c]) for s, e, c in runs], grad_scale, grad_bf16)
        K.adamw_prelude(self.counters, self.corr, [(c, self.gates[c]) for c in sorted({c for _, _, c in runs})], b1, b2)
        if self.groups is not None:
            tab = [(s, e, self.gates[c], c) for s, e, c in runs]
            for k in range(0, len(tab), K.SGD_MAX_RUNS):
                K.adamw_step_runs_groups(st.flat, st.grad, self.exp_avg, self.exp_avg_sq, st.shadow,
                                         tab[k:k + K.SGD_MAX_RUNS], b1, b2, self.eps, self.lr_dev, self.corr,
                                         self.groups.group_map, self.groups.group_hyper, grad_scale=grad_scale,
                                         grad_bf16=grad_bf16, **ck)
            return
        # _RUNS off selects the per-run launches only for a clipped step (the tests of the _clip twins): without
        # clipping FusedAdamW has never read it, and its launches stay what they were
        if (_RUNS or not ck) and len(runs) <= K.SGD_MAX_RUNS:
            K.adamw_step_runs(st.flat, st.grad, self.exp_avg, self.exp_avg_sq, st.shadow,
                              [(s, e, self.gates[c], c) for s, e, c in runs], b1, b2, self.eps, self.weight_decay,
                              self.lr_dev, self.corr, grad_scale=grad_scale, grad_bf16=grad_bf16, **ck)
            return
        for s, e, c in runs:
            K.adamw_step(st.flat[s:e], st.grad[s:e], self.exp_avg[s:e], self.exp_avg_sq[s:e],
                         self._cut(st.shadow, s, e), 0.0, b1, b2, self.eps, self.weight_decay,
                         self.corr[2 * c:2 * c + 2], lr_dev=self.lr_dev, gate=self.gates[c], grad_scale=grad_scale,
                         grad_bf16=self._cut(grad_bf16, s, e), **ck)

    def state_dict(self):
        """The live state (as torch's): moments over the flat store, the per-class device step counts, lr (the one
        device rate, before any group's multiplier) and the hyper-parameters; with groups also "groups": {parameter
        name: (lr_scale, weight_decay)}."""
        return {"exp_avg": self.exp_avg, "exp_avg_sq": self.exp_avg_sq, "step": self.counters,
                "lr": self.lr, "base_lr": self.base_lr, "betas": self.betas, "eps": self.eps,
                "weight_decay": self.weight_decay, "active": self.active, **self._group_state()}

    def load_state_dict(self, sd):
        if sd["exp_avg"].numel() != self.exp_avg.numel() or sd["step"].numel() != self.counters.numel():
            raise ValueError("FusedAdamW.load_state_dict: state of another parameter store")
        self._check_groups(sd)
        self.exp_avg.copy_(sd["exp_avg"])
        self.exp_avg_sq.copy_(sd["exp_avg_sq"])
        self.counters.copy_(sd["step"])
        self.betas, self.eps = (float(sd["betas"][0]), float(sd["betas"][1])), float(sd["eps"])
        self.weight_decay, self.base_lr = float(sd["weight_decay"]), float(sd["base_lr"])
        self.active = list(sd["active"]) if sd["active"] is not None else None
        for g in self.param_groups:
            g["initial_lr"] = self.base_lr * g.get("lr_scale", 1.0)
        self.set_lr(sd["lr"])


class ParamEMA:
    """Exponential moving average of every parameter of a ParamStore: e <- e + w (p - e), w = 1 - decay, over the
    whole flat fp32 buffer (timm.ModelEmaV2 / swa_utils.AveragedModel semantics: every parameter every step, also one
    the optimizer skipped — a LayerDrop-dropped layer, a grad=None head; alignment and group gaps hold 0 and stay 0).

    update() is two launches, both capturable: the prelude advances the device count num_updates (int32 [1]) and
    writes this step's w into `weight` (fp32 [1]); with warmup the decay is min(decay, (1 + t) / (10 + t)) after t
    updates, so a short fine-tune at decay 0.9999 leaves its initial copy.  Then one pass over the store.
    swap() exchanges the average with the live weights in place (flat, and the bf16 shadow rewritten from the new
    flat), so the existing model evaluates through the average with no second module; applied() is the context
    manager around an evaluation and restores the live weights bit for bit, also when its body raises.
    Buffers (BatchNorm running statistics, ...) are not parameters and are not averaged: evaluation under applied()
    uses the live ones.
    Data parallel: built after the rank-0 parameter broadcast, every rank applies the same deterministic update to
    identical bytes, so the replicas' averages stay bit-equal with no collective."""

    def __init__(self, store, decay, warmup=False):
        decay = float(decay)
        if not (math.isfinite(decay) and 0.0 <= decay < 1.0):
            raise ValueError(f"ParamEMA: decay must lie in [0, 1), got {decay}")
        self.store, self.decay, self.warmup = store, decay, bool(warmup)
        dev = store.flat.device
        self.ema = store.flat.clone()
        self.num_updates = torch.zeros(1, device=dev, dtype=torch.int32)
        self.weight = torch.zeros(1, device=dev, dtype=torch.float32)
        self.swapped = False   # True while the store holds the average (between the two swaps of applied())

    def _live(self, what):
        if self.swapped:
            raise RuntimeError(f"ParamEMA.{what}: the store holds the averaged weights (inside applied() / after an "
                               f"odd number of swap() calls)")

    def reset(self):
        """Restart the average from the store's current weights (e.g. after a checkpoint was loaded into them)."""
        self._live("reset")
        self.ema.copy_(self.store.flat)
        self.num_updates.zero_()

    def update(self):
        """One EMA update from the store's current weights; call right after optimizer.step()."""
        self._live("update")
        K.ema_prelude(self.num_updates, self.weight, self.decay, self.warmup)
        K.ema_update(self.store.flat, self.ema, self.weight)

    def swap(self):
        """Exchange the average and the live weights (and rewrite the bf16 shadow); a second call undoes it."""
        if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("ParamEMA.swap: not during a graph capture (a replay would swap again)")
        K.ema_swap(self.store.flat, self.ema, self.store.shadow)
        self.swapped = not self.swapped

    @contextlib.contextmanager
    def applied(self):
        """Inside, the model's parameters (and store.shadow) are the averaged weights; on exit the live weights are
        back bit for bit.  Not re-entrant: a nested applied() raises instead of silently un-swapping."""
        self._live("applied")
        self.swap()
        try:
            yield self
        finally:
            self.swap()

    def named_tensors(self, model):
        """{parameter name: view of the average} with the model's own state_dict keys and shapes (the parameters the
        store holds; frozen ones are not averaged and are absent)."""
        self._live("named_tensors")
        st, out = self.store, {}
        for name, p in model.named_parameters():
            i = st.index.get(id(p))
            if i is not None:
                s, e = st.span(i)
                out[name] = self.ema[s:e].view(p.shape)
        return out

    def state_dict(self):
        self._live("state_dict")
        return {"ema": self.ema, "num_updates": self.num_updates, "decay": self.decay, "warmup": self.warmup}

    def load_state_dict(self, sd):
        self._live("load_state_dict")
        if sd["ema"].numel() != self.ema.numel() or sd["num_updates"].numel() != 1:
            raise ValueError("ParamEMA.load_state_dict: state of another parameter store")
        decay = float(sd["decay"])
        if not (math.isfinite(decay) and 0.0 <= decay < 1.0):
            raise ValueError(f"ParamEMA.load_state_dict: decay must lie in [0, 1), got {decay}")
        self.ema.copy_(sd["ema"])
        self.num_updates.copy_(sd["num_updates"])
        self.decay, self.warmup = decay, bool(sd["warmup"])


class CosineAnnealingLR:
    """torch.optim.lr_scheduler.CosineAnnealingLR (eta_min 0) closed form, stepped per optimizer step."""

    def __init__(self, optimizer, T_max, eta_min=0.0):
        self.opt, self.T_max, self.eta_min = optimizer, max(int(T_max), 1), eta_min
        self.t = 0

    def get_lr(self):
        base = self.opt.base_lr
        return self.eta_min + (base - self.eta_min) * (1 + math.cos(math.pi * self.t / self.T_max)) / 2

    def step(self):
        self.t += 1
        self.opt.set_lr(self.get_lr())
