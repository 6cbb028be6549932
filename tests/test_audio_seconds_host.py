"""CPU: --audio_seconds, the clip length override of the waveform and mel slots — clip_seconds (train.py / test.py)
and trainer.wave_samples (the padded width under --paudio_lengths) follow it, --audio_seconds_min is validated
against it, and without it both return the configuration's own length."""
import pathlib

import pytest

from config import clip_seconds, get_opt
from deepfake_amd.models.fused import CONFIGS
from deepfake_amd.trainer import wave_samples


def test_audio_seconds_overrides_the_configuration():
    args = get_opt(["--audio_seconds", "13", "--paudio_lengths", "--config", "c2"])
    assert args.audio_seconds == 13.0
    assert clip_seconds(args, CONFIGS["c2"]) == 13
    assert wave_samples(args) == 208000
    assert int(16000 * clip_seconds(args, CONFIGS["c2"])) == 208000   # DeepFake's sample count agrees
    frac = get_opt(["--audio_seconds", "12.5", "--paudio_lengths"])
    assert clip_seconds(frac, CONFIGS["c2"]) == 12.5 and wave_samples(frac) == 200000


def test_absent_flag_keeps_the_configuration():
    for name in ("c2", "c5"):
        args = get_opt(["--config", name, "--paudio_lengths"])
        assert args.audio_seconds is None
        assert clip_seconds(args, CONFIGS[name]) == CONFIGS[name]["seconds"]
        assert wave_samples(args) == 16000 * CONFIGS[name]["seconds"]
    assert wave_samples(get_opt(["--audio_seconds", "13"])) is None   # --paudio_lengths off: no padded width


def test_audio_seconds_min_is_validated_against_the_override():
    cfg = CONFIGS["c2"]   # 4 s of its own
    assert clip_seconds(get_opt(["--audio_seconds", "13", "--audio_seconds_min", "5"]), cfg) == (5.0, 13)
    assert clip_seconds(get_opt(["--audio_seconds", "13", "--audio_seconds_min", "13"]), cfg) == (13.0, 13)
    with pytest.raises(ValueError):
        clip_seconds(get_opt(["--audio_seconds", "13", "--audio_seconds_min", "13.5"]), cfg)
    with pytest.raises(ValueError):   # below the configuration's 4 s, above the override
        clip_seconds(get_opt(["--audio_seconds", "2", "--audio_seconds_min", "3"]), cfg)
    for bad in ("0", "-1"):
        with pytest.raises(ValueError):
            clip_seconds(get_opt(["--audio_seconds", bad]), cfg)
        with pytest.raises(ValueError):
            wave_samples(get_opt(["--audio_seconds", bad, "--paudio_lengths"]))


def test_flag_is_documented():
    import config
    readme = (pathlib.Path(config.__file__).parent / "README.md").read_text()
    assert "--audio_seconds FLOAT" in config.__doc__ and "--audio_seconds 30" in readme
