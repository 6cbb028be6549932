"""Test helper (not a test): float64 numpy evaluation of the resampler's defining sum from a given tap table,
independent of deepfake_amd.media's device path.

With x zero outside [0, S_in), table H [L, 2Z] (H[p][j + Z - 1] = h(p / L - j), j = -Z+1..Z) and
n M = i_n L + p_n (0 <= p_n < L):

    y[n] = sum_{j = -Z+1..Z} x[i_n + j] H[p_n][j + Z - 1],    n = 0 .. ceil(S_in L / M) - 1.
"""
import numpy as np


def out_len(S_in, L, M):
    """ceil(S_in L / M) (librosa.resample's length)."""
    return -((-int(S_in) * int(L)) // int(M))


def resample_ref(x, table, L, M, start=0, stop=None, with_abs=False):
    """y[start:stop] in float64 for one waveform x [S_in]; with_abs: also sum_j |x[i_n + j] H[p_n][j]| per sample
    (the scale of the dot product's rounding-error bound)."""
    x = np.asarray(x, dtype=np.float64)
    H = np.asarray(table, dtype=np.float64)
    S_in, ntaps = x.shape[0], H.shape[1]
    assert H.shape[0] == L and ntaps % 2 == 0
    Z = ntaps // 2
    stop = out_len(S_in, L, M) if stop is None else stop
    y = np.empty(stop - start)
    a = np.empty(stop - start)
    j = np.arange(-Z + 1, Z + 1, dtype=np.int64)[None, :]
    for c0 in range(start, stop, 1 << 15):
        n = np.arange(c0, min(c0 + (1 << 15), stop), dtype=np.int64)
        i, p = np.divmod(n * M, L)
        idx = i[:, None] + j
        ok = (idx >= 0) & (idx < S_in)
        prod = np.where(ok, x[np.clip(idx, 0, S_in - 1)], 0.0) * H[p]
        y[c0 - start:c0 - start + len(n)] = prod.sum(axis=1)
        a[c0 - start:c0 - start + len(n)] = np.abs(prod).sum(axis=1)
    return (y, a) if with_abs else y
