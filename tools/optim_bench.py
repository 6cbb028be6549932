"""Device time of the fused AdamW step against the fused SGD step over the C2 model's parameter store
(build_fused("c2"), bf16 compute: fp32 master + bf16 shadow): dfk_adamw_step_runs against dfk_sgd_step_runs (the
yardstick, timed in the same process) over the store's own run table with every LayerDrop gate open, and
FusedAdamW.step (the counter / correction prelude included).  The bytes model is 30 B per element for AdamW
(p, exp_avg, exp_avg_sq read and written, the gradient read, the shadow written) against SGD's 22 B.
HIP events on the op's stream around `inner` back-to-back calls, median over `reps` repeats, after a warm-up; the
cases are timed interleaved in each repeat.  Gradient clipping: the norm pass (dfk_grad_sqnorm_runs +
dfk_grad_clip_coef, 4 B per element, so 4/22 of the yardstick by the bytes model) alone, and FusedSGD.step /
FusedAdamW.step with max_grad_norm on and off.  With --step also the C2 step level (graph-replayed TrainStep, B = 8,
SGD and AdamW, each with clipping off and on, and SGD with the weight EMA on), for orientation.  Weight EMA:
ema_update (dfk_ema_prelude + dfk_ema_update over the whole store: p read, e read and written, 12 B per element, 12/22
of the yardstick by the bytes model) and ema_swap (dfk_ema_swap: p and e read and written, the shadow written, 18 B
per element).  Parameter groups: dfk_sgd_step_runs_groups / dfk_adamw_step_runs_groups over the same run tables with the
four groups of --no_decay norm_bias and --lr_scale {v,a,pa}Extract=0.1 (one map byte per 8 elements on top of the 22 /
30 B streams: +0.6 % / +0.4 % by the bytes model), interleaved with their plain twins.  With --bits the line also carries a sha256 of every
state buffer after the timed calls: the sequence of calls is fixed by reps / inner, the inputs are seeded and no
kernel uses atomics, so two builds that compute the same thing print the same hashes.  Prints one JSON line.
Usage: python tools/optim_bench.py [reps] [inner] [--step] [--bits]"""
import hashlib
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from deepfake_amd import kernels as K  # noqa: E402
from deepfake_amd.models.fused import CONFIGS, build_fused  # noqa: E402
from deepfake_amd.optim import FusedAdamW, FusedSGD, ParamEMA, ParamGroups  # noqa: E402
from deepfake_amd.params import ParamStore  # noqa: E402

HBM_PEAK = 8e12   # bytes / s


def timed(fn, inner):
    """Milliseconds per call: events recorded on the current stream around `inner` calls."""
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(inner):
        fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) / inner


def interleaved(cases, reps, inner, warm=5):
    for fn in cases.values():
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in cases}
    for _ in range(reps):
        for k, fn in cases.items():
            ms[k].append(timed(fn, inner))
    return ms


def sha256(t):
    return hashlib.sha256(t.detach().contiguous().view(torch.uint8).cpu().numpy().tobytes()).hexdigest()


def step_pair(reps, inner):
    """ms per graph-replayed C2 training step (B = 8, synthetic batch) with each optimizer."""
    from deepfake_amd import rng
    from deepfake_amd.ddp import GradBucketer
    from deepfake_amd.trainer import TrainStep
    cfg, dev = CONFIGS["c2"], torch.device("cuda")
    steps = {}
    for name in ("sgd", "sgd+clip", "adamw", "adamw+clip", "sgd+ema"):
        clip = 1.0 if name.endswith("+clip") else None
        torch.manual_seed(1234)
        rng.manual_seed(1234, 0)
        model = build_fused(cfg, compute_dtype=torch.bfloat16).to(dev).train()
        store = ParamStore(model, torch.bfloat16)
        opt = FusedSGD(store, 1e-4, 0.9, 1e-3, max_grad_norm=clip) if name.startswith("sgd") else \
            FusedAdamW(store, 1e-4, weight_decay=1e-3, max_grad_norm=clip)
        g = torch.Generator(device=dev).manual_seed(1234)
        feat = (torch.randn(8, cfg["T"], 3, cfg["H"], cfg["W"], device=dev, generator=g),
                torch.randn(8, 3, 224, 224, device=dev, generator=g),
                torch.randn(8, int(16000 * cfg["seconds"]), device=dev, generator=g))
        label = (torch.rand(8, device=dev, generator=g) < 0.5).float()
        ema = ParamEMA(store, 0.9999, warmup=True) if name.endswith("+ema") else None
        ts = TrainStep(model, store, opt, GradBucketer(store), graph=True, ema=ema)
        ts(feat, label)
        if ts.graph is None:
            raise SystemExit(f"optim_bench: the {name} step was not captured")
        steps[name] = (lambda ts=ts, feat=feat, label=label: ts(feat, label))
    ms = interleaved(steps, reps, inner, warm=3)
    return {k: {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}
            for k, v in ms.items()}


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    reps = int(args[0]) if len(args) > 0 else 30
    inner = int(args[1]) if len(args) > 1 else 20
    if not torch.cuda.is_available():
        raise SystemExit("optim_bench: needs the GPU (no CPU timing)")
    torch.manual_seed(0)
    model = build_fused("c2", compute_dtype=torch.bfloat16).cuda()
    store = ParamStore(model, torch.bfloat16)
    for gate in store.gate:                      # every LayerDrop layer kept: all runs do their work
        if gate is not None:
            gate.fill_(1.0)
    store.grad.normal_(0.0, 1e-3)
    sgd, adam = FusedSGD(store, 1e-4, 0.9, 1e-3), FusedAdamW(store, 1e-4, weight_decay=1e-3)
    sgd_c = FusedSGD(store, 1e-4, 0.9, 1e-3, max_grad_norm=1.0)
    adam_c = FusedAdamW(store, 1e-4, weight_decay=1e-3, max_grad_norm=1.0)
    runs = store.touched_runs(also=adam.cls, every=True)         # the table FusedAdamW.step launches
    if len(runs) > K.SGD_MAX_RUNS:
        raise SystemExit(f"optim_bench: {len(runs)} runs, the one-launch kernels take {K.SGD_MAX_RUNS}")
    n = sum(e - s for s, e, _ in runs)
    sgd_tab = [(s, e, adam.gates[c], False) for s, e, c in runs]
    adam_tab = [(s, e, adam.gates[c], c) for s, e, c in runs]
    b1, b2 = adam.betas
    norm_tab = [(s, e, adam.gates[c]) for s, e, c in runs]
    part = torch.zeros(K.GNORM_PARTIALS, device="cuda", dtype=torch.float64)
    pair = torch.zeros(2, device="cuda")

    def grad_norm():
        K.grad_clip_coef(part, K.grad_sqnorm_runs(store.grad, norm_tab, part), 1.0, pair)
    ema = ParamEMA(store, 0.9999, warmup=True)

    def ema_update():
        K.ema_prelude(ema.num_updates, ema.weight, ema.decay, ema.warmup)
        K.ema_update(store.flat, ema.ema, ema.weight)
    groups = ParamGroups(model, store, 1e-3, no_decay="norm_bias",
                         lr_scale={"vExtract": 0.1, "aExtract": 0.1, "paExtract": 0.1})
    K.adamw_prelude(adam.counters, adam.corr, [(c, g) for c, g in enumerate(adam.gates)], b1, b2)
    cases = {
        "sgd_step_runs": lambda: K.sgd_step_runs(store.flat, store.grad, sgd.buf, store.shadow, sgd_tab, 0.9, 1e-3,
                                                 sgd.lr_dev),
        "adamw_step_runs": lambda: K.adamw_step_runs(store.flat, store.grad, adam.exp_avg, adam.exp_avg_sq,
                                                     store.shadow, adam_tab, b1, b2, adam.eps, 1e-3, adam.lr_dev,
                                                     adam.corr),
        "sgd_step_runs_groups": lambda: K.sgd_step_runs_groups(store.flat, store.grad, sgd.buf, store.shadow, sgd_tab,
                                                               0.9, sgd.lr_dev, groups.group_map, groups.group_hyper),
        "adamw_step_runs_groups": lambda: K.adamw_step_runs_groups(store.flat, store.grad, adam.exp_avg,
                                                                   adam.exp_avg_sq, store.shadow, adam_tab, b1, b2,
                                                                   adam.eps, adam.lr_dev, adam.corr, groups.group_map,
                                                                   groups.group_hyper),
        "FusedAdamW.step": adam.step,
        "grad_norm": grad_norm,
        "FusedSGD.step": sgd.step,
        "FusedSGD.step+clip": sgd_c.step,
        "FusedAdamW.step+clip": adam_c.step,
        "ema_update": ema_update,
        "ema_swap": lambda: K.ema_swap(store.flat, ema.ema, store.shadow),
    }
    ms = interleaved(cases, reps, inner)
    med = {k: statistics.median(v) for k, v in ms.items()}
    bytes_per = {"sgd_step_runs": 22, "adamw_step_runs": 30, "FusedAdamW.step": 30, "grad_norm": 4,
                 "FusedSGD.step": 22, "FusedSGD.step+clip": 26, "FusedAdamW.step+clip": 34, "ema_update": 12,
                 "ema_swap": 18, "sgd_step_runs_groups": 22.125, "adamw_step_runs_groups": 30.125}
    ratio = {k: [g / p for g, p in zip(ms[k + "_step_runs_groups"], ms[k + "_step_runs"])] for k in ("sgd", "adamw")}
    elems = {k: store.numel if k.startswith("ema_") else n for k in med}   # the EMA kernels cover the gaps too
    out = {"config": "c2", "elements": n, "store_elements": store.numel, "runs": len(runs),
           "classes": len(adam.gates), "reps": reps, "inner": inner,
           "ms_median": {k: round(v, 4) for k, v in med.items()},
           "ms_min": {k: round(min(v), 4) for k, v in ms.items()},
           "ms_max": {k: round(max(v), 4) for k, v in ms.items()},
           "TB_per_s": {k: round(bytes_per[k] * elems[k] / (med[k] * 1e-3) / 1e12, 3) for k in med},
           "fraction_of_8TBps": {k: round(bytes_per[k] * elems[k] / (med[k] * 1e-3) / HBM_PEAK, 3) for k in med},
           "adamw_over_sgd": round(med["adamw_step_runs"] / med["sgd_step_runs"], 4), "bytes_ratio": round(30 / 22, 4),
           "prelude_ms": round(med["FusedAdamW.step"] - med["adamw_step_runs"], 4),
           "grad_norm_over_sgd": round(med["grad_norm"] / med["sgd_step_runs"], 4), "grad_norm_bytes_ratio": round(4 / 22, 4),
           "grad_norm_over_bytes_model": round(med["grad_norm"] / (med["sgd_step_runs"] * 4 / 22), 3),
           "clip_cost_ms": {"sgd": round(med["FusedSGD.step+clip"] - med["FusedSGD.step"], 4),
                            "adamw": round(med["FusedAdamW.step+clip"] - med["FusedAdamW.step"], 4)},
           "ema_update_over_sgd": round(med["ema_update"] / med["sgd_step_runs"], 4),
           "ema_update_over_bytes_model": round(med["ema_update"] / (med["sgd_step_runs"] * 12 / 22), 3),
           "ema_swap_over_sgd": round(med["ema_swap"] / med["sgd_step_runs"], 4),
           "ema_swap_over_bytes_model": round(med["ema_swap"] / (med["sgd_step_runs"] * 18 / 22), 3),
           "groups": [{"lr_scale": m, "weight_decay": w, "tensors": t, "elements": e}
                      for m, w, t, e in groups.summary()],
           # groups kernel / plain twin: of the medians, and median / min / max of the per-repeat ratios (the spread)
           "groups_over_plain": {k: {"of_medians": round(med[k + "_step_runs_groups"] / med[k + "_step_runs"], 4),
                                     "median": round(statistics.median(v), 4), "min": round(min(v), 4),
                                     "max": round(max(v), 4)} for k, v in ratio.items()},
           "groups_bytes_ratio": {"sgd": round(22.125 / 22, 4), "adamw": round(30.125 / 30, 4)},
           "ema_num_updates": int(ema.num_updates),
           "grad_norm_value": [round(v, 6) for v in adam_c.grad_norm.tolist()],
           "device": torch.cuda.get_device_name(0)}
    if "--bits" in sys.argv:
        torch.cuda.synchronize()
        out["sha256"] = {k: sha256(t) for k, t in {
            "store.flat": store.flat, "store.shadow": store.shadow, "sgd.buf": sgd.buf, "adam.exp_avg": adam.exp_avg,
            "adam.exp_avg_sq": adam.exp_avg_sq, "adam.counters": adam.counters, "adam.corr": adam.corr,
            "sgd+clip.grad_norm": sgd_c.grad_norm, "adam+clip.grad_norm": adam_c.grad_norm, "ema.ema": ema.ema,
            "ema.num_updates": ema.num_updates}.items()}
    if "--step" in sys.argv:
        del model, store, sgd, adam, sgd_c, adam_c, ema, cases
        torch.cuda.empty_cache()
        out["c2_step_ms"] = step_pair(max(reps // 3, 3), max(inner // 2, 5))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
