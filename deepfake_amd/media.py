"""Media front end on the device: the mel-spectrogram image of
generate_mel_spectrogram (src/utils.py:63-87) and the train-time frame transform of
data/data_process.py:62-69, as HIP kernels (csrc/media.hip) behind plain functions.

The constants the kernels read — the window-folded DFT basis of librosa's STFT and librosa's
Slaney mel filterbank — are built here once per (sr, n_fft, n_mels) in float64 and cast to
float32, as librosa does; they are parameters of the transform, not data.

Parity: the frame / mel-image transform follows PIL 12.2 (importable here), as the reference applies
torchvision's transforms to PIL images: pinned bit for bit to PIL fixtures (tests/golden/pil_frames.npz, written
by tests/golden/make_pil_fixtures.py).  librosa and cv2 are absent, so the mel-spectrogram image stays pinned to
the restatement in oracle/media.py (librosa 0.10 / OpenCV 4 semantics from their published algorithms) — parity
unpinned against those libraries.  The resampling librosa.load applies first (16 kHz -> 22.05 kHz,
src/utils.py:70) runs here with a filter of this build's own (resample_taps: a stated Kaiser-windowed sinc, held to
ideal band-limited interpolation); soxr is absent, so parity with soxr_hq is unpinned too.

Ragged batches: the reference builds each clip's image from its own track at its own length
(data/data_process.py:82-93).  resample and mel_image take a padded [B, S] batch with per-clip `lengths` and give
every clip, bit for bit, what the same call gives that clip alone; the padding is never read."""
import ctypes
import functools
import math

import numpy as np
import torch

from . import _lib as L

IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)


def _hz_to_mel(f):
    """Slaney mel scale (librosa.hz_to_mel, htk=False)."""
    f = np.asanyarray(f, dtype=np.float64)
    f_sp, min_log_hz = 200.0 / 3, 1000.0
    min_log_mel, logstep = min_log_hz / f_sp, math.log(6.4) / 27.0
    return np.where(f >= min_log_hz, min_log_mel + np.log(np.maximum(f, 1e-300) / min_log_hz) / logstep, f / f_sp)


def _mel_to_hz(m):
    m = np.asanyarray(m, dtype=np.float64)
    f_sp, min_log_hz = 200.0 / 3, 1000.0
    min_log_mel, logstep = min_log_hz / f_sp, math.log(6.4) / 27.0
    return np.where(m >= min_log_mel, min_log_hz * np.exp(logstep * (m - min_log_mel)), f_sp * m)


@functools.lru_cache(maxsize=8)
def mel_filterbank(sr=22050, n_fft=2048, n_mels=128, fmin=0.0, fmax=None):
    """librosa.filters.mel(sr, n_fft, n_mels, fmin, fmax, htk=False, norm='slaney') -> float32 [n_mels, 1+n_fft/2]."""
    fmax = sr / 2.0 if fmax is None else fmax
    fftfreqs = np.linspace(0, sr / 2.0, 1 + n_fft // 2)
    mel_f = _mel_to_hz(np.linspace(_hz_to_mel(fmin), _hz_to_mel(fmax), n_mels + 2))
    fdiff = np.diff(mel_f)
    ramps = mel_f[:, None] - fftfreqs[None, :]
    lower = -ramps[:-2] / fdiff[:-1, None]
    upper = ramps[2:] / fdiff[1:, None]
    w = np.maximum(0.0, np.minimum(lower, upper))
    w *= (2.0 / (mel_f[2:n_mels + 2] - mel_f[:n_mels]))[:, None]
    return w.astype(np.float32)


@functools.lru_cache(maxsize=8)
def stft_basis(n_fft=2048):
    """Window-folded real DFT basis [n_fft, ld] (ld = 2 (n_fft/2+1) rounded up to 4): column f = w[n] cos(2 pi f n / N),
    column nbin + f = -w[n] sin(...), w = periodic Hann (librosa's get_window('hann', fftbins=True)), so that
    frames @ basis gives Re | Im of np.fft.rfft(w * frame)."""
    nbin = n_fft // 2 + 1
    ld = (2 * nbin + 3) // 4 * 4
    n = np.arange(n_fft)
    w = 0.5 - 0.5 * np.cos(2.0 * np.pi * n / n_fft)
    k = np.outer(n, np.arange(nbin)) % n_fft          # exact phase index before the float conversion
    ang = 2.0 * np.pi * k / n_fft
    b = np.zeros((n_fft, ld))
    b[:, :nbin] = w[:, None] * np.cos(ang)
    b[:, nbin:2 * nbin] = -w[:, None] * np.sin(ang)
    return b.astype(np.float32)


_DEV_CONST = {}


def _const(key, make, device):
    k = (key, str(device))
    t = _DEV_CONST.get(k)
    if t is None:
        t = torch.from_numpy(make()).to(device)
        _DEV_CONST[k] = t
    return t


RESAMPLE_Z, RESAMPLE_BETA = 32, 10.0


@functools.lru_cache(maxsize=8)
def resample_taps(sr_in=16000, sr_out=22050):
    """The resampler's filter (librosa.load's 16 kHz -> 22.05 kHz step, src/utils.py:70, as this build defines it):
    (H float32 [L, 2Z], L, M) with L / M = sr_out / sr_in in lowest terms.  A Kaiser-windowed sinc with its cutoff
    at the input Nyquist, t in input samples,
        h(t) = sinc(t) I0(beta sqrt(1 - (t / Z)^2)) / I0(beta)  for |t| <= Z, else 0      (Z = 32, beta = 10)
        H[p][j + Z - 1] = h(p / L - j),  p = 0..L-1,  j = -Z+1..Z,
    built in float64 and cast to float32.  With x zero outside [0, S_in) and n M = i_n L + p_n (0 <= p_n < L) the
    resampled signal is y[n] = sum_j x[i_n + j] H[p_n][j + Z - 1], n < ceil(S_in L / M).  Only sr_out >= sr_in."""
    sr_in, sr_out = int(sr_in), int(sr_out)
    if sr_in <= 0 or sr_out <= 0:
        raise ValueError("resample_taps: sample rates must be positive")
    if sr_out < sr_in:
        raise ValueError("resample_taps: downsampling (sr_out < sr_in) is not built")
    g = math.gcd(sr_in, sr_out)
    up, down = sr_out // g, sr_in // g
    Z = RESAMPLE_Z
    t = np.arange(up, dtype=np.float64)[:, None] / up - np.arange(-Z + 1, Z + 1, dtype=np.float64)[None, :]
    win = np.i0(RESAMPLE_BETA * np.sqrt(np.maximum(0.0, 1.0 - (t / Z) ** 2))) / np.i0(RESAMPLE_BETA)
    h = np.where(np.abs(t) <= Z, np.sinc(t) * win, 0.0)
    return h.astype(np.float32), up, down


def resample_len(S_in, up, down):
    """ceil(S_in up / down): the length librosa.resample gives."""
    return -((-int(S_in) * up) // down)


def _resample_dev(sr_in, sr_out, device):
    """(device table, L, M, ntaps); the device copy is [ntaps][L] in period order (output r of a period reads
    column r: phase (r M) mod L), so consecutive outputs read consecutive entries."""
    H, up, down = resample_taps(sr_in, sr_out)
    perm = (np.arange(up) * down) % up
    taps = _const(("resample", sr_in, sr_out), lambda: np.ascontiguousarray(H[perm].T), device)
    return taps, up, down, H.shape[1]


def resample_lengths(lengths, sr_in=16000, sr_out=22050):
    """Per-clip output lengths of resample(..., lengths=): ceil(n sr_out / sr_in) in exact integers.  A tensor gives
    an int64 tensor on its own device (no sync, no copy to the host); a sequence of ints gives a list of ints."""
    g = math.gcd(int(sr_in), int(sr_out))
    up, down = int(sr_out) // g, int(sr_in) // g
    if torch.is_tensor(lengths):
        return torch.div(lengths.to(torch.int64) * up + (down - 1), down, rounding_mode="floor")
    return [resample_len(n, up, down) for n in lengths]


def _clip_lengths(lengths, B, S, what):
    """lengths of a ragged [B, S] batch as an int64 [B] tensor.  Values on the host (a sequence of ints or a CPU
    int tensor) are validated here — shape [B], 1 <= n <= S, else ValueError; a device tensor is passed through
    without reading it (no sync: the kernels clamp every value into [1, S])."""
    t = lengths if torch.is_tensor(lengths) else torch.as_tensor(list(lengths))
    if t.dtype.is_floating_point or t.dtype.is_complex or t.dtype == torch.bool:
        raise ValueError(f"{what}: lengths must be integers, got {t.dtype}")
    if tuple(t.shape) != (B,):
        raise ValueError(f"{what}: lengths must have shape [{B}] (one per clip), got {list(t.shape)}")
    if not t.is_cuda and (int(t.min()) < 1 or int(t.max()) > S):
        raise ValueError(f"{what}: lengths must lie in [1, {S}], got {t.tolist()}")
    return t.to(torch.int64)


def resample(wave, sr_in=16000, sr_out=22050, lengths=None):
    """wave fp32 [B, S_in] (device, at sr_in) -> fp32 [B, ceil(S_in sr_out / sr_in)] at sr_out: the band-limited
    resampling librosa.load applies before the mel spectrogram (src/utils.py:70), with the filter of
    resample_taps (parity with soxr_hq unpinned).  lengths (ragged batches, as mel_image's): clip b holds lengths[b]
    samples of its row; out[b, :m_b] equals resample(wave[b:b+1, :lengths[b]])[0] bit for bit, m_b =
    resample_lengths(lengths)[b], and out[b, m_b:] is 0.0; the rest of the input row is never read."""
    n = None if lengths is None else _clip_lengths(lengths, wave.shape[0], wave.shape[-1], "resample")
    if not wave.is_cuda:
        raise RuntimeError("resample: device tensors only (no CPU fallback)")
    x = wave.float().contiguous()
    B, S = x.shape
    taps, up, down, ntaps = _resample_dev(int(sr_in), int(sr_out), x.device)
    S_out = resample_len(S, up, down)
    y = torch.empty(B, S_out, dtype=torch.float32, device=x.device)
    if n is not None:
        n = n.to(x.device).contiguous()
        L.check(L.lib().dfk_resample_ragged(L.ptr(x), B, S, L.ptr(n), L.ptr(taps), up, down, ntaps, L.ptr(y), S_out,
                                            L.stream()), "resample_ragged")
        return y
    L.check(L.lib().dfk_resample(L.ptr(x), B, S, L.ptr(taps), up, down, ntaps, L.ptr(y), S_out, L.stream()),
            "resample")
    return y


def mel_image(wave, sr=22050, n_fft=2048, hop=512, n_mels=128, size=(224, 224), sr_in=None, lengths=None):
    """wave fp32 [B, S] (device, at `sr`) -> uint8 [B, size[1], size[0]] mel-spectrogram images
    (generate_mel_spectrogram, src/utils.py:63-87; the reference's fmax argument is unused there).  sr_in: the
    rate of `wave` where it differs from `sr` (the clip's own 16 kHz track): resampled to `sr` inside the
    pipeline (resample's kernel writes the STFT's padded buffer), bit-equal to mel_image(resample(wave)).

    lengths: a ragged batch — the reference builds every clip's image from its own track at its own length
    (data/data_process.py:82-93).  Clip b holds lengths[b] samples (1 <= n <= S) of its row, the rest of the row is
    padding of any content that is never read, and
        mel_image(wave, lengths=n, ...)[b] == mel_image(wave[b:b+1, :n[b]].contiguous(), ...)[0]   bit for bit:
    the dB reference, the min-max stretch and the resized time axis (1 + n_b / hop frames at `sr`) are the clip's
    own.  A sequence of ints or a CPU int tensor is validated (ValueError); a device int tensor is passed through
    without a sync and clamped into [1, S] by the kernels.  None: every row is S samples long."""
    n = None if lengths is None else _clip_lengths(lengths, wave.shape[0], wave.shape[-1], "mel_image")
    if not wave.is_cuda:
        raise RuntimeError("mel_image: device tensors only (no CPU fallback)")
    x = wave.float().contiguous()
    B, S = x.shape
    basis = _const(("basis", n_fft), lambda: stft_basis(n_fft), x.device)
    fb = _const(("fb", sr, n_fft, n_mels), lambda: mel_filterbank(sr, n_fft, n_mels), x.device)
    ow, oh = size
    out = torch.empty(B, oh, ow, dtype=torch.uint8, device=x.device)
    if n is not None:
        n = n.to(x.device).contiguous()
        if sr_in is not None and int(sr_in) != int(sr):
            taps, up, down, ntaps = _resample_dev(int(sr_in), int(sr), x.device)
            nbytes = L.lib().dfk_mel_resampled_workspace(B, S, up, down, n_fft, hop, n_mels)
        else:
            taps, up, down, ntaps = None, 1, 1, 0
            nbytes = L.lib().dfk_mel_workspace(B, S, n_fft, hop, n_mels)
        if nbytes < 0:
            raise RuntimeError("dfk_mel_workspace: invalid arguments")
        ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
        L.check(L.lib().dfk_mel_image_ragged(L.ptr(x), B, S, L.ptr(n), L.ptr(taps), up, down, ntaps, L.ptr(basis),
                                             L.ptr(fb), n_fft, hop, n_mels, oh, ow, L.ptr(ws), nbytes, L.ptr(out),
                                             L.stream()), "mel_image_ragged")
        return out
    if sr_in is not None and int(sr_in) != int(sr):
        taps, up, down, ntaps = _resample_dev(int(sr_in), int(sr), x.device)
        S_out = resample_len(S, up, down)
        nbytes = L.lib().dfk_mel_resampled_workspace(B, S, up, down, n_fft, hop, n_mels)
        if nbytes < 0:
            raise RuntimeError("dfk_mel_resampled_workspace: invalid arguments")
        ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
        L.check(L.lib().dfk_mel_image_resampled(L.ptr(x), B, S, L.ptr(taps), up, down, ntaps, S_out, L.ptr(basis),
                                                L.ptr(fb), n_fft, hop, n_mels, oh, ow, L.ptr(ws), nbytes, L.ptr(out),
                                                L.stream()), "mel_image_resampled")
        return out
    nbytes = L.lib().dfk_mel_workspace(B, S, n_fft, hop, n_mels)
    if nbytes < 0:
        raise RuntimeError("dfk_mel_workspace: invalid arguments")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
    L.check(L.lib().dfk_mel_image(L.ptr(x), B, S, L.ptr(basis), L.ptr(fb), n_fft, hop, n_mels, oh, ow, L.ptr(ws),
                                  nbytes, L.ptr(out), L.stream()), "mel_image")
    return out


def _f3(v):
    return (ctypes.c_float * 3)(*v)


def gray_normalize(img_u8, mean=IMAGENET_MEAN, std=IMAGENET_STD):
    """uint8 [..., H, W] gray images -> fp32 [..., 3, H, W] (convert('RGB') + ToTensor + Normalize)."""
    *lead, H, W = img_u8.shape
    x = img_u8.contiguous()
    out = torch.empty(*lead, 3, H, W, device=x.device, dtype=torch.float32)
    L.check(L.lib().dfk_gray_normalize(L.ptr(x), L.ptr(out), x.numel() // (H * W), H, W, _f3(mean), _f3(std),
                                       L.stream()), "gray_normalize")
    return out


def pil_bilinear_coeffs(in_size, out_size):
    """PIL's Image.resize(BILINEAR) coefficients along one axis (libImaging/Resample.c precompute_coeffs with the
    triangle filter, support 1 scaled by max(1, in/out), then normalize_coeffs_8bpc's 22-bit fixed point):
    (bounds int32 [out, 2] = (first source index, tap count), coeffs int32 [out, ksize], ksize)."""
    scale = float(in_size) / out_size
    filterscale = max(scale, 1.0)
    support = 1.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    bounds = np.zeros((out_size, 2), dtype=np.int32)
    kk = np.zeros((out_size, ksize), dtype=np.int32)
    ss = 1.0 / filterscale
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)          # C (int): truncation toward zero
        xmax = min(int(center + support + 0.5), in_size) - xmin
        w = []
        ww = 0.0
        for x in range(xmax):
            t = abs((x + xmin - center + 0.5) * ss)
            v = 1.0 - t if t < 1.0 else 0.0
            w.append(v)
            ww += v
        for x in range(xmax):
            k = w[x] / ww if ww != 0.0 else w[x]
            kk[xx, x] = int(-0.5 + k * (1 << 22)) if k < 0 else int(0.5 + k * (1 << 22))
        bounds[xx] = (xmin, xmax)
    return bounds, kk, ksize


def pil_rotate_fixed(angle, w, h):
    """Image.rotate(angle, NEAREST, expand=False) of a w x h image as PIL 12 runs it: the inverse affine matrix
    built in Image.rotate (angle % 360, cos / sin rounded to 15 decimals, rotation about (w/2, h/2)), then
    libImaging affine_fixed's 16.16 fixed point with the pixel-centre offset folded into the translation.
    Returns 8 int32 {on, a0, a1, a2, a3, a4, a5, 0}; on = 0 for the copy fast path (angle % 360 == 0).  The 180 /
    90 / 270 transpose fast paths give the same map as this affine (exact rounded cos / sin)."""
    angle = angle % 360.0
    if angle == 0:
        return [0] * 8
    cx, cy = w / 2, h / 2
    a = -math.radians(angle)
    m = [round(math.cos(a), 15), round(math.sin(a), 15), 0.0, round(-math.sin(a), 15), round(math.cos(a), 15), 0.0]
    m[2] = m[0] * -cx + m[1] * -cy + m[2] + cx
    m[5] = m[3] * -cx + m[4] * -cy + m[5] + cy

    def fix(v):
        return math.floor(v * 65536.0 + 0.5)
    return [1, fix(m[0]), fix(m[1]), fix(m[2] + m[1] * 0.5 + m[0] * 0.5), fix(m[3]), fix(m[4]),
            fix(m[5] + m[4] * 0.5 + m[3] * 0.5), 0]


@functools.lru_cache(maxsize=16)
def _pil_axis(in_size, out_size):
    b, k, ks = pil_bilinear_coeffs(in_size, out_size)
    return b, k, ks


def eval_size(H, W, short=224):
    """torchvision T.Resize(int) output size (h, w): the shorter side to `short`, the longer scaled and truncated."""
    if W <= H:
        return int(short * H / W), short
    return short, int(short * W / H)


def draw_augment(frames, generator=None, degrees=90.0):
    """Per-frame parameters of T.RandomHorizontalFlip, T.RandomVerticalFlip (p = 0.5) and T.RandomRotation(90),
    drawn on the CPU in the order the reference's Compose draws them for each frame (torch.rand(1) < 0.5,
    torch.rand(1) < 0.5, torch.empty(1).uniform_(-90, 90)): (flips int32 [frames] (bit 0 horizontal, bit 1
    vertical), angles: list of Python floats).  One batched draw of [frames, 3] uniforms: the CPU generator
    hands them out in the same sequence as the per-frame scalar calls, and uniform_(a, b) on one float is
    float32(double(u) * (b - a) + a) of the same 24-bit draw, so flips, angles and the generator's state afterwards
    are identical to the scalar loop (tests/test_media_oracle.py pins this)."""
    u = torch.rand(frames, 3, generator=generator)
    flips = ((u[:, 0] < 0.5).int() | ((u[:, 1] < 0.5).int() << 1)).to(torch.int32)
    angles = (u[:, 2].double() * (2.0 * degrees) - degrees).float()
    return flips, angles.tolist()


def frame_augment(frames_u8, size=(224, 224), flips=None, angles=None, mean=IMAGENET_MEAN, std=IMAGENET_STD,
                  grey=False):
    """uint8 [..., H, W, 3] decoded RGB frames (or, with grey=True, [..., H, W] grey images) on the device -> fp32
    [..., 3, size[1], size[0]]: PIL Resize, flips, rotation, ToTensor, Normalize (data_process.py:55-69 on PIL
    images).  flips: int tensor [frames] (None: none); angles: per-frame rotation angles in degrees (host floats,
    None: none)."""
    x = frames_u8
    if x.dtype != torch.uint8:
        raise ValueError("frame_augment expects uint8 frames")
    if grey and x.dim() < 2:
        raise ValueError("grey frame_augment expects [..., H, W]")
    if not grey and (x.dim() < 3 or x.shape[-1] != 3):
        raise ValueError("frame_augment expects RGB frames [..., H, W, 3] (grey=True for [..., H, W])")
    *lead, H, W = (x.shape if grey else x.shape[:-1])
    cin = 1 if grey else 3
    x = x.contiguous()
    n = x.numel() // (H * W * cin)
    ow, oh = size
    dev = x.device
    xb, xk, kx = _pil_axis(W, ow)
    yb, yk, ky = _pil_axis(H, oh)
    cxb, cxk = _const(("pilx", W, ow, "b"), lambda: xb, dev), _const(("pilx", W, ow, "k"), lambda: xk, dev)
    cyb, cyk = _const(("pily", H, oh, "b"), lambda: yb, dev), _const(("pily", H, oh, "k"), lambda: yk, dev)
    r = L.PilResize()
    r.H, r.W, r.cin, r.out_h, r.out_w = H, W, cin, oh, ow
    r.xb, r.xk, r.kx = cxb.data_ptr(), cxk.data_ptr(), kx
    r.yb, r.yk, r.ky = cyb.data_ptr(), cyk.data_ptr(), ky
    fl = flips.to(device=dev, dtype=torch.int32).contiguous() if flips is not None else None
    aff = None
    if angles is not None:
        if len(angles) != n:
            raise ValueError("one angle per frame")
        aff = torch.tensor([pil_rotate_fixed(float(a), ow, oh) for a in angles], dtype=torch.int32).to(dev)
    if fl is not None and fl.numel() != n:
        raise ValueError("one flip entry per frame")
    tmp = torch.empty(n * H * ow * cin, dtype=torch.uint8, device=dev)
    out = torch.empty(*lead, 3, oh, ow, device=dev, dtype=torch.float32)
    L.check(L.lib().dfk_frame_augment(L.ptr(x), n, r, L.ptr(fl) if fl is not None else None,
                                      L.ptr(aff) if aff is not None else None, _f3(mean), _f3(std), L.ptr(tmp),
                                      L.ptr(out), L.stream()), "frame_augment")
    return out
