"""CPU: the host side of global gradient-norm clipping — the --clip_grad_norm flag, the max_grad_norm argument of
both fused optimizers, and the six entry points in include/dfk.h, deepfake_amd/_lib.py and deepfake_amd/kernels.py.
The kernels themselves are tested on the device (tests/test_gpu_clip.py)."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("dfk_grad_sqnorm_runs", "dfk_grad_clip_coef", "dfk_sgd_step_clip", "dfk_sgd_step_runs_clip",
                "dfk_adamw_step_clip", "dfk_adamw_step_runs_clip")


def _toy_store():
    from deepfake_amd.params import ParamStore
    torch.manual_seed(0)
    return ParamStore(torch.nn.Sequential(torch.nn.Linear(7, 13), torch.nn.Linear(13, 3)), torch.float32)


def test_flag_parses_and_defaults_to_off():
    from config import get_opt
    assert get_opt([]).clip_grad_norm == 0
    assert get_opt(["--clip_grad_norm", "1.5"]).clip_grad_norm == 1.5
    with pytest.raises(SystemExit):
        get_opt(["--clip_grad_norm", "tight"])


def test_help_lists_the_flag(capsys):
    from config import get_opt
    with pytest.raises(SystemExit) as e:
        get_opt(["--help"])
    assert e.value.code == 0
    assert "--clip_grad_norm" in capsys.readouterr().out


@pytest.mark.parametrize("name", ["FusedSGD", "FusedAdamW"])
def test_constructors_take_max_grad_norm(name):
    from deepfake_amd import kernels as K
    from deepfake_amd import optim
    cls = getattr(optim, name)
    store = _toy_store()
    off = cls(store, 1e-3)
    assert off.max_grad_norm is None and off.grad_norm is None
    assert cls(store, 1e-3, max_grad_norm=None).max_grad_norm is None
    on = cls(store, 1e-3, max_grad_norm=2)
    assert on.max_grad_norm == 2.0
    assert on.grad_norm.dtype == torch.float32 and on.grad_norm.shape == (2,)
    assert on._partials.dtype == torch.float64 and on._partials.numel() % K.GNORM_PARTIALS == 0
    assert on._partials.numel() >= -(-len(store.params) // K.SGD_MAX_RUNS) * K.GNORM_PARTIALS
    for bad in (0, 0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            cls(store, 1e-3, max_grad_norm=bad)


def test_entry_points_in_header_binding_table_and_wrappers():
    from deepfake_amd import _lib
    from deepfake_amd import kernels as K
    src = open(os.path.join(ROOT, "include", "dfk.h")).read()
    for name in ENTRY_POINTS:
        assert re.search(r"^int\s+" + name + r"\s*\(", src, flags=re.M), name
        assert name in _lib.SIGNATURES, name
        assert callable(getattr(K, name[len("dfk_"):])), name
    assert "clip_grad_norm_" in src


def test_clip_twins_take_their_twins_arguments_plus_one_pointer():
    from deepfake_amd import _lib
    for twin in ("dfk_sgd_step", "dfk_sgd_step_runs", "dfk_adamw_step", "dfk_adamw_step_runs"):
        a, b = _lib.SIGNATURES[twin], _lib.SIGNATURES[twin + "_clip"]
        assert b == a[:-1] + [_lib._VP, a[-1]], twin       # ..., clip_coef, stream


def test_partials_constant_agrees_between_header_and_wrappers():
    from deepfake_amd import kernels as K
    src = open(os.path.join(ROOT, "include", "dfk.h")).read()
    m = re.search(r"^#define\s+DFK_GNORM_PARTIALS\s+(\d+)", src, flags=re.M)
    assert m and int(m.group(1)) == K.GNORM_PARTIALS
    assert 0 < K.GNORM_PARTIALS <= 4096


def test_existing_prototypes_keep_their_parameter_counts():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dfk.h")).read(), flags=re.S)
    protos = dict(re.findall(r"^int\s+(dfk_\w+)\s*\(([^;]*)\)\s*;", src, flags=re.M | re.S))
    assert protos["dfk_sgd_step"].count(",") + 1 == 14 and protos["dfk_sgd_step_runs"].count(",") + 1 == 13
    assert protos["dfk_adamw_step"].count(",") + 1 == 17 and protos["dfk_adamw_step_runs"].count(",") + 1 == 18


def test_a_non_finite_norm_raises_at_the_log_step():
    from deepfake_amd.trainer import check_grad_norm
    assert check_grad_norm(1.5, 3) == 1.5
    for bad in (float("nan"), float("inf")):
        with pytest.raises(FloatingPointError, match="step 3"):
            check_grad_norm(bad, 3)


def test_trainer_maps_the_flag_and_rejects_bad_values():
    import types
    from deepfake_amd.trainer import clip_arg
    assert clip_arg(types.SimpleNamespace()) is None
    assert clip_arg(types.SimpleNamespace(clip_grad_norm=0.0)) is None
    assert clip_arg(types.SimpleNamespace(clip_grad_norm=1.5)) == 1.5
    for bad in (-1.0, float("nan"), float("inf"), float("-inf")):
        with pytest.raises(ValueError):
            clip_arg(types.SimpleNamespace(clip_grad_norm=bad))
