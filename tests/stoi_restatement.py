"""Float64 numpy restatement of STOI / extended STOI as pystoi 0.3.3 computes them (pystoi.stoi(x, y, fs,
extended)): Taal et al. 2011 and Jensen & Taal 2016.  It is the contract dsn_stoi is tested against; parity with the
pystoi package itself is unpinned (the package is not a dependency of this project).

One intended deviation: pystoi adds EPS * randn noise before each ESTOI row / column normalisation (so that a
constant row does not divide by zero).  That noise is omitted here and in the device code; a row or column whose
centred norm is exactly zero is normalised to zero and contributes nothing (pystoi returns a random value there)."""
from __future__ import annotations

import math

import numpy as np

FS = 10000
N_FRAME = 256
NFFT = 512
HOP = 128
NUMBAND = 15
MINFREQ = 150
N = 30
BETA = -15.0
DYN_RANGE = 40.0
EPS = float(np.finfo(np.float64).eps)
WINDOW = np.hanning(N_FRAME + 2)[1:-1]


def resample_window(p: int, q: int) -> np.ndarray:
    """Octave-style Kaiser-windowed sinc of pystoi.utils._resample_window_oct (un-normalised)."""
    g = math.gcd(p, q)
    p, q = p // g, q // g
    cutoff = 1.0 / (2 * max(p, q))
    L = math.ceil((60.0 - 8.0) / (28.714 * (cutoff / 10.0)))
    t = np.arange(-L, L + 1, dtype=np.float64)
    ideal = 2 * p * cutoff * np.sinc(2 * cutoff * t)
    return np.kaiser(2 * L + 1, 0.1102 * (60.0 - 8.7)) * ideal


def resample(x: np.ndarray, fs: int) -> np.ndarray:
    """scipy.signal.resample_poly(x, 10000, fs, window=h / sum(h)) written out as its polyphase sum:
    y[i] = sum_m x[m] * up * hn[(i + n_pre_remove) * down - n_pre_pad - m * up]."""
    x = np.asarray(x, dtype=np.float64)
    g = math.gcd(FS, fs)
    up, down = FS // g, fs // g
    if up == down == 1:
        return x.copy()
    h = resample_window(FS, fs)
    h = h / h.sum() * up
    half_len = (h.size - 1) // 2
    n_in = x.size
    n_out = -(-n_in * up // down)
    n_pre_pad = down - half_len % down
    n_pre_remove = (half_len + n_pre_pad) // down
    c = (np.arange(n_out, dtype=np.int64) + n_pre_remove) * down - n_pre_pad
    y = np.zeros(n_out)
    # outputs with c = r (mod up) use the taps h[r::up]: y = (x * h[r::up])[(c - r) / up], a full convolution
    for r in range(up):
        sel = np.flatnonzero(c % up == r)
        if sel.size == 0 or r >= h.size:
            continue
        conv = np.convolve(x, h[r::up])
        idx = (c[sel] - r) // up
        ok = (idx >= 0) & (idx < conv.size)
        y[sel[ok]] = conv[idx[ok]]
    return y


def frame_energies(x: np.ndarray) -> np.ndarray:
    """20 log10(|w * frame| + EPS) of every frame that fits, last one included (start + 256 <= len)."""
    starts = range(0, len(x) - N_FRAME + 1, HOP)
    return np.array([20 * np.log10(np.linalg.norm(WINDOW * x[s:s + N_FRAME]) + EPS) for s in starts])


def remove_silent_frames(x: np.ndarray, y: np.ndarray):
    """-> (x_sil, y_sil, mask): frames of x more than 40 dB below its loudest dropped from both signals, the kept
    windowed frames overlap-added at hop 128 (length (K-1)*128 + 256)."""
    en = frame_energies(x)
    mask = (en.max() - DYN_RANGE - en) < 0
    kept = np.flatnonzero(mask)
    K = kept.size
    out = []
    for s in (x, y):
        sil = np.zeros((K - 1) * HOP + N_FRAME)
        for k, f in enumerate(kept):
            sil[k * HOP:k * HOP + N_FRAME] += WINDOW * s[f * HOP:f * HOP + N_FRAME]
        out.append(sil)
    return out[0], out[1], mask


def stft(x: np.ndarray) -> np.ndarray:
    """[frames, 257] rfft of the windowed frames.  Frames start while start < len - 256 (strict): the last frame that
    fits is EXCLUDED, so a silence-removed signal of K kept frames gives K - 1 STFT frames (pystoi.utils.stft)."""
    return np.array([np.fft.rfft(WINDOW * x[s:s + N_FRAME], n=NFFT) for s in range(0, len(x) - N_FRAME, HOP)])


def band_edges():
    """[(lo, hi)] bins of the 15 one-third-octave bands (pystoi.utils.thirdoct): each edge snapped to the nearest
    bin, first index on ties; a band covers [lo, hi)."""
    f = np.linspace(0, FS, NFFT + 1)[:NFFT // 2 + 1]
    k = np.arange(NUMBAND, dtype=np.float64)
    lo = MINFREQ * np.power(2.0, (2 * k - 1) / 6)
    hi = MINFREQ * np.power(2.0, (2 * k + 1) / 6)
    return [(int(np.argmin(np.square(f - lo[i]))), int(np.argmin(np.square(f - hi[i])))) for i in range(NUMBAND)]


def third_octave(spec: np.ndarray) -> np.ndarray:
    """[frames, 257] complex -> [15, frames] band envelopes sqrt(sum |X|^2)."""
    p = np.abs(spec) ** 2
    return np.array([np.sqrt(p[:, lo:hi].sum(axis=1)) for lo, hi in band_edges()])


def _norm0(v: np.ndarray, axis: int) -> np.ndarray:
    """v / |v| along axis, zero where |v| == 0 (the documented deviation from pystoi's noise)."""
    n = np.sqrt(np.sum(v * v, axis=axis, keepdims=True))
    return np.divide(v, n, out=np.zeros_like(v), where=n > 0)


def row_col_normalize(seg: np.ndarray) -> np.ndarray:
    """[J, 15, 30]: mean-centre and normalise each row over the frames, then each column over the bands."""
    x = seg - seg.mean(axis=-1, keepdims=True)
    x = _norm0(x, -1)
    x = x - x.mean(axis=1, keepdims=True)
    return _norm0(x, 1)


def stoi_details(x, y, fs: int, extended: bool = False):
    """-> (score, stft frames after silent-frame removal, kept-frame count K)."""
    x = np.asarray(x, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    if x.shape != y.shape:
        raise ValueError("x and y must have the same shape")
    if fs != FS:
        x, y = resample(x, fs), resample(y, fs)
    x, y, mask = remove_silent_frames(x, y)
    K = int(mask.sum())
    xs, ys = stft(x), stft(y)
    frames = xs.shape[0]
    if frames < N:
        return 1e-5, frames, K
    xt, yt = third_octave(xs), third_octave(ys)
    xseg = np.array([xt[:, m - N:m] for m in range(N, frames + 1)])
    yseg = np.array([yt[:, m - N:m] for m in range(N, frames + 1)])
    J = xseg.shape[0]
    if extended:
        xn, yn = row_col_normalize(xseg), row_col_normalize(yseg)
        return float(np.sum(xn * yn / N) / J), frames, K
    alpha = np.linalg.norm(xseg, axis=2, keepdims=True) / (np.linalg.norm(yseg, axis=2, keepdims=True) + EPS)
    yp = np.minimum(yseg * alpha, xseg * (1 + 10 ** (-BETA / 20)))
    yp = yp - yp.mean(axis=2, keepdims=True)
    xc = xseg - xseg.mean(axis=2, keepdims=True)
    yp = yp / (np.linalg.norm(yp, axis=2, keepdims=True) + EPS)
    xc = xc / (np.linalg.norm(xc, axis=2, keepdims=True) + EPS)
    return float(np.sum(yp * xc) / (J * NUMBAND)), frames, K


def stoi(x, y, fs: int, extended: bool = False) -> float:
    return stoi_details(x, y, fs, extended)[0]


def silence_margin_db(x, fs: int) -> float:
    """Smallest |max - 40 dB - energy| over the frames of the (resampled) clean signal: how close the silent-frame
    decision of this input comes to its threshold."""
    x = np.asarray(x, dtype=np.float64)
    if fs != FS:
        x = resample(x, fs)
    en = frame_energies(x)
    return float(np.min(np.abs(en.max() - DYN_RANGE - en)))
