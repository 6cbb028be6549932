"""CPU: the resampler's filter as a design (deepfake_amd.media.resample_taps) — ratio and shape, per-phase DC gain,
frequency response of the fp32-rounded table in float64, and pure tones through the float64 reference sum
(tests/resample_ref.py) against the analytic tone at the output rate.  The bars come from what the mel image can
show (one grey level of its 80 dB range is 0.31 dB; top_db = 80 is its floor), not from the measured figures,
which are quoted beside them."""
import math

import numpy as np
import pytest

from deepfake_amd import media
from resample_ref import out_len, resample_ref

SR_IN, SR_OUT = 16000, 22050


def test_ratio_shape_and_lengths():
    H, L, M = media.resample_taps(SR_IN, SR_OUT)
    assert (L, M) == (441, 320)
    assert H.dtype == np.float32 and H.shape == (441, 64)
    assert media.resample_len(64000, L, M) == 88200 == out_len(64000, L, M)
    assert media.resample_len(1000, L, M) == 1379 == out_len(1000, L, M)
    H2, L2, M2 = media.resample_taps(16000, 24000)
    assert (L2, M2) == (3, 2) and H2.shape == (3, 64)
    with pytest.raises(ValueError):
        media.resample_taps(22050, 16000)


def test_table_is_the_stated_filter():
    """H[p][j + Z - 1] = h(p / L - j) with h the Kaiser-windowed sinc (Z = 32, beta = 10), evaluated here entry by
    entry with math / np.i0 scalars."""
    H, L, M = media.resample_taps(SR_IN, SR_OUT)
    Z, beta = 32, 10.0
    for p, j in ((0, 0), (0, 32), (0, -31), (1, 0), (220, 1), (440, -31), (440, 32), (137, -5)):
        t = p / L - j
        w = float(np.i0(beta * math.sqrt(max(0.0, 1.0 - (t / Z) ** 2))) / np.i0(beta)) if abs(t) <= Z else 0.0
        s = 1.0 if t == 0 else math.sin(math.pi * t) / (math.pi * t)
        assert abs(float(H[p, j + Z - 1]) - s * w) <= 1e-7, (p, j)
    # phase 0 copies the input sample (np.sinc at the other integers leaves float64 rounding residue, below 1e-16)
    assert H[0, Z - 1] == 1.0 and np.abs(np.delete(H[0], Z - 1)).max() <= 1e-16


def test_phase_rows_sum_to_one():
    H, _, _ = media.resample_taps(SR_IN, SR_OUT)
    err = np.abs(H.astype(np.float64).sum(axis=1) - 1.0).max()
    print(f"per-phase row sum: max |sum - 1| = {err:.2e}")      # measured 3.0e-6
    assert err <= 1e-5


def test_frequency_response():
    """The table read as one prototype filter g[p - j L] = H[p][j] at the rate L * sr_in."""
    H, L, _ = media.resample_taps(SR_IN, SR_OUT)
    g = H.astype(np.float64)[:, ::-1].T.reshape(-1)
    nfft = 1 << 21
    f = np.fft.rfftfreq(nfft, d=1.0 / (L * SR_IN))
    db = 20.0 * np.log10(np.maximum(np.abs(np.fft.rfft(g, nfft)) / abs(g.sum()), 1e-300))
    pb = db[f <= 7200.0]
    ripple, dev = pb.max() - pb.min(), np.abs(pb).max()
    sb = db[(f >= 8800.0) & (f <= L * 8000.0)].max()
    print(f"passband 0-7.2 kHz: ripple {ripple:.2e} dB peak to peak, {dev:.2e} dB from the DC gain; "
          f"stopband 8.8 kHz up: {sb:.1f} dB")                  # measured 1.8e-4 dB, 1.1e-4 dB, -99.6 dB
    assert ripple <= 0.01 and dev <= 0.01
    assert sb <= -96.0


@pytest.mark.parametrize("freq", [1000.0, 5000.0, 7000.0])
def test_tone_matches_analytic(freq):
    H, L, M = media.resample_taps(SR_IN, SR_OUT)
    amp, S = 0.5, 4000
    x = amp * np.sin(2.0 * np.pi * freq * np.arange(S) / SR_IN)
    y = resample_ref(x, H, L, M)
    assert y.shape == (out_len(S, L, M),)
    want = amp * np.sin(2.0 * np.pi * freq * np.arange(len(y)) / SR_OUT)
    edge = math.ceil((32 + 1) * L / M)
    assert edge == 46
    err = np.abs(y - want)[edge:-edge].max()
    print(f"{freq:.0f} Hz tone: max error {err / amp:.2e} of the amplitude")   # measured <= 5.3e-6
    assert err <= 1e-4 * amp
