"""The A-weighting FIR of the reference's perceptually weighted STFT loss
(stable_audio_tools/training/losses/auraloss.py::FIRFilter("aw", fs)), designed in numpy float64 without scipy:

  1. the IEC analogue A-weighting prototype  H(s) = k s^4 / ((s + w4)^2 (s + w1)^2 (s + w3) (s + w2)),
     w_i = 2 pi f_i, k = w4^2 10^(A1000 / 20);
  2. its bilinear transform at the signal rate (s = 2 fs (z - 1) / (z + 1));
  3. the magnitude of the digital filter at 512 frequencies from 0 up to (not including) fs / 2;
  4. the 101-tap linear-phase FIR that fits that magnitude in the least-squares sense, the 512 frequencies taken in
     consecutive pairs as 256 bands with the desired magnitude linear inside each band and nothing asked between
     bands (what scipy.signal.firls(101, w, |h|, fs=fs) solves).

The reference stores the taps as float32; `taps(fs)` returns them in that precision."""
from __future__ import annotations

import functools

import numpy as np

F1, F2, F3, F4, A1000 = 20.598997, 107.65265, 737.86223, 12194.217, 1.9997
NTAPS, NFREQ = 101, 512


def analog_prototype():
    """(num, den) of H(s), highest power first."""
    w1, w2, w3, w4 = (2.0 * np.pi * f for f in (F1, F2, F3, F4))
    num = np.array([w4 ** 2 * 10.0 ** (A1000 / 20.0), 0.0, 0.0, 0.0, 0.0])
    den = np.array([1.0])
    for factor in ([1.0, 2.0 * w4, w4 ** 2], [1.0, 2.0 * w1, w1 ** 2], [1.0, w3], [1.0, w2]):
        den = np.convolve(den, factor)
    return num, den


def bilinear(num, den, fs: float):
    """Substitute s = 2 fs (z - 1) / (z + 1) and clear the (z + 1)^M denominators, M = the larger degree; both results
    are polynomials in z, highest power first, scaled so that the denominator is monic."""
    M = max(len(num), len(den)) - 1

    def transform(p):
        out = np.zeros(M + 1)
        deg = len(p) - 1
        for idx, coef in enumerate(p):
            i = deg - idx                                    # coef * s^i -> coef (2 fs)^i (z - 1)^i (z + 1)^(M - i)
            term = np.array([1.0])
            for _ in range(i):
                term = np.convolve(term, [1.0, -1.0])
            for _ in range(M - i):
                term = np.convolve(term, [1.0, 1.0])
            out += coef * (2.0 * fs) ** i * term
        return out

    b, a = transform(num), transform(den)
    return b / a[0], a / a[0]


def magnitude_response(b, a, fs: float, n: int = NFREQ):
    """(frequencies in Hz, |H(e^{jw})|) at w = pi k / n, k = 0 .. n-1.  b, a: polynomials in z^-1, constant first --
    which a polynomial in z of equal degree, highest power first, already is."""
    w = np.pi * np.arange(n) / n
    zinv = np.exp(-1j * w)
    h = np.polyval(b[::-1], zinv) / np.polyval(a[::-1], zinv)
    return w * fs / (2.0 * np.pi), np.abs(h)


def least_squares_fir(ntaps: int, freqs, desired, fs: float):
    """Type-I linear-phase FIR h minimising the integral over the bands (freqs[2k], freqs[2k+1]) of
    (A(f) - D(f))^2, A the zero-phase response a_0 + 2 sum_m a_m cos(pi m f) (f in units of fs / 2) and D linear
    between desired[2k] and desired[2k+1].  The normal equations are Q a = b with
    Q[m][l] = q[|m - l|] + q[m + l], q[m] = the integral of cos(pi m f) over the bands, and the taps are
    (a_M .. a_1, 2 a_0, a_1 .. a_M)."""
    if ntaps % 2 == 0:
        raise ValueError(f"ntaps must be odd (ntaps={ntaps}).")
    M = (ntaps - 1) // 2
    f = np.asarray(freqs, dtype=np.float64).reshape(-1, 2) / (fs / 2.0)          # [bands, 2]
    d = np.asarray(desired, dtype=np.float64).reshape(-1, 2)
    f0, f1 = f[:, 0], f[:, 1]
    # q[m] = sum over bands of [f sinc(m f)] from f0 to f1  (= integral of cos(pi m f) df), m = 0 .. 2 M
    m_all = np.arange(ntaps)[:, None]
    q = (f1 * np.sinc(m_all * f1) - f0 * np.sinc(m_all * f0)).sum(axis=1)
    idx = np.arange(M + 1)
    Q = q[np.abs(idx[:, None] - idx[None, :])] + q[idx[:, None] + idx[None, :]]
    # b[m] = integral of D(f) cos(pi m f) df, D(f) = slope f + icpt in each band
    slope = (d[:, 1] - d[:, 0]) / (f1 - f0)
    icpt = d[:, 0] - f0 * slope
    m = idx[:, None].astype(np.float64)

    def antiderivative(x):
        val = x * (slope * x + icpt) * np.sinc(m * x)
        val[0] -= slope * x * x / 2.0
        val[1:] += slope * np.cos(m[1:] * np.pi * x) / (np.pi * m[1:]) ** 2
        return val

    rhs = (antiderivative(f1) - antiderivative(f0)).sum(axis=1)
    a = np.linalg.solve(Q, rhs)
    return np.concatenate((a[:0:-1], [2.0 * a[0]], a[1:]))


def design(fs: float, ntaps: int = NTAPS) -> np.ndarray:
    """The float64 taps of FIRFilter("aw", fs)."""
    b, a = bilinear(*analog_prototype(), fs)
    freqs, mag = magnitude_response(b, a, fs)
    return least_squares_fir(ntaps, freqs, mag, fs)


@functools.lru_cache(maxsize=None)
def _taps32(fs: float) -> np.ndarray:
    t = design(fs).astype(np.float32)
    t.setflags(write=False)
    return t


def taps(fs) -> np.ndarray:
    """float32 [101] (read-only, cached per fs): the weight the reference's FIRFilter("aw", fs) stores."""
    return _taps32(float(fs))
