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
"""
import contextlib
import math
import os

import torch

from . import kernels as K


# DFK_SGD_RUNS=0: one dfk_sgd_step launch per run (A/B); default: every run in one dfk_sgd_step_runs launch
_RUNS = os.environ.get("DFK_SGD_RUNS", "1") != "0"


class _Fused:
    """What FusedSGD and FusedAdamW share: the store, the learning rate in device memory (a captured graph replays
    with the scheduler's current lr), and the device state of global-norm clipping, allocated once: the fp64 partial
    slabs (one per chunk of 64 runs the store can produce) and the fp32 pair grad_norm = {norm, coef} of the last
    step."""
    folds_grad = True   # step() takes the all-reduced sum and 1 / world itself (TrainStep._fold)

    def __init__(self, store, lr, max_grad_norm):
        self.store = store
        self.base_lr = float(lr)
        dev = store.flat.device
        self.lr_dev = torch.full((1,), self.base_lr, device=dev, dtype=torch.float32)
        self.param_groups = [{"lr": self.base_lr, "initial_lr": self.base_lr}]
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
        self.param_groups[0]["lr"] = float(lr)
        self.lr_dev.fill_(float(lr))

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
    def __init__(self, store, lr, momentum=0.9, weight_decay=0.0, max_grad_norm=None):
        super().__init__(store, lr, max_grad_norm)
        self.momentum, self.weight_decay = float(momentum), float(weight_decay)
        self.buf = torch.zeros_like(store.flat)
        self.first = True
        self.has_buf = [False] * len(store.params)   # torch: momentum buffer created at a param's first grad

    def step(self, first=None, grad_scale=1.0, grad_bf16=None):
        """One SGD step over the parameters that received a gradient (torch skips grad=None:
        no weight decay and no momentum for them): every contiguous run in one dfk_sgd_step_runs launch (one
        dfk_sgd_step per run beyond 64 runs, or with DFK_SGD_RUNS=0).
        grad_scale / grad_bf16: the data-parallel fold of GradBucketer.finish(fold=True) — the gradient is the
        all-reduced sum (in the fp32 buffer, or in the bf16 bucket copy) times 1 / world."""
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
        return {"momentum_buffer": self.buf, "lr": self.param_groups[0]["lr"], "first": self.first}


class FusedAdamW(_Fused):
    """torch.optim.AdamW(lr, betas, eps, weight_decay; amsgrad / maximize off) with FusedSGD's surface.

    Step counts are int32 device memory, one per gate class: class 0 holds the ungated parameters, every distinct
    LayerDrop flag of ParamStore.gate its own class.  Each step first runs the prelude kernel, which advances the
    counter of every class whose gate is open and writes its bias corrections, then the update over the runs
    (dfk_adamw_step_runs; one dfk_adamw_step per run beyond 64 runs).  A gated-off class keeps parameters, moments,
    shadow and counter, as torch leaves a grad=None parameter, so a layer dropped in step 1 takes t = 1 in step 2."""

    def __init__(self, store, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, max_grad_norm=None):
        b1, b2 = float(betas[0]), float(betas[1])
        if not (0.0 <= b1 < 1.0 and 0.0 <= b2 < 1.0) or not float(eps) > 0.0:
            raise ValueError(f"FusedAdamW: betas must lie in [0, 1) and eps be positive, got {betas}, {eps}")
        super().__init__(store, lr, max_grad_norm)
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
        gradient appears or disappears between steps would need its own count (torch keeps one per parameter)."""
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
        # DFK_SGD_RUNS=0 selects the per-run launches only for a clipped step (A/B of the _clip twins): without
        # clipping FusedAdamW has never read the variable, and its launches stay what they were
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
        """The live state (as torch's): moments over the flat store, the per-class device step counts, lr and the
        hyper-parameters."""
        return {"exp_avg": self.exp_avg, "exp_avg_sq": self.exp_avg_sq, "step": self.counters,
                "lr": self.param_groups[0]["lr"], "base_lr": self.base_lr, "betas": self.betas, "eps": self.eps,
                "weight_decay": self.weight_decay, "active": self.active}

    def load_state_dict(self, sd):
        if sd["exp_avg"].numel() != self.exp_avg.numel() or sd["step"].numel() != self.counters.numel():
            raise ValueError("FusedAdamW.load_state_dict: state of another parameter store")
        self.exp_avg.copy_(sd["exp_avg"])
        self.exp_avg_sq.copy_(sd["exp_avg_sq"])
        self.counters.copy_(sd["step"])
        self.betas, self.eps = (float(sd["betas"][0]), float(sd["betas"][1])), float(sd["eps"])
        self.weight_decay, self.base_lr = float(sd["weight_decay"]), float(sd["base_lr"])
        self.active = list(sd["active"]) if sd["active"] is not None else None
        self.param_groups[0]["initial_lr"] = self.base_lr
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
