"""Float64 numpy restatement of the objective measures behind the composite scores CSIG / CBAK / COVL, the contract
dsn_composite is tested against.  Written from the published definitions, all frames of a signal at once:

  Y. Hu and P. C. Loizou, "Evaluation of objective quality measures for speech enhancement", IEEE TASLP 16(1), 2008:
      the composite regressions, the 95 % trimmed means of LLR and WSS, the [-10, 35] dB clamp of the segmental SNR.
  D. H. Klatt, "Prediction of perceived phonetic distance from critical-band spectra", ICASSP 1982: the weighted
      spectral slope distance and its weights (Kmax = 20, Klocmax = 1; p. 1280).
  S. R. Quackenbush, T. P. Barnwell and M. A. Clements, "Objective Measures of Speech Quality", 1988: the
      log-likelihood ratio of LPC models and the segmental SNR (eq. 2.12).

Framing follows the reference's evaluate_covl.py, which tests/golden/composite.npz pins this file to: 30 ms frames a
quarter frame apart under 0.5 (1 - cos(2 pi k / (W + 1))), k = 1 .. W; int(L / hop - W / hop) frames; LPC order 16 at
fs >= 10 kHz, else 10; a zero-padded FFT of 2^ceil(log2(2 W)) points.  CENT_FREQ / BANDWIDTH are the 25 critical-band
centre frequencies and bandwidths (Hz) of the WSS measure as Hu & Loizou's composite implementation tabulates them
(Loizou, "Speech Enhancement: Theory and Practice", 2nd ed., ch. 11 companion code): constants of the measure.

The reference rounds its LPC output to float32 and conditions the segmental SNR in float32; this restatement is float64
throughout, so the two differ by that rounding (bounds in tests/test_composite_host.py)."""
from __future__ import annotations

import functools
import math

import numpy as np

NUM_CRIT = 25
CENT_FREQ = np.array([50.0, 120.0, 190.0, 260.0, 330.0, 400.0, 470.0, 540.0, 617.372, 703.378, 798.717, 904.128,
                      1020.38, 1148.30, 1288.72, 1442.54, 1610.70, 1794.16, 1993.93, 2211.08, 2446.71, 2701.97,
                      2978.04, 3276.17, 3597.63])
BANDWIDTH = np.array([70.0, 70.0, 70.0, 70.0, 70.0, 70.0, 70.0, 77.3724, 86.0056, 95.3398, 105.411, 116.256, 127.914,
                      140.423, 153.823, 168.154, 183.457, 199.776, 217.153, 235.631, 255.255, 276.072, 298.126,
                      321.465, 346.136])
KMAX, KLOCMAX = 20.0, 1.0
ALPHA = 0.95
MIN_SNR, MAX_SNR = -10.0, 35.0


def geometry(fs: int):
    """(window length, hop, FFT size, LPC order)"""
    win = round(30 * fs / 1000.0)
    return win, win // 4, 1 << math.ceil(math.log2(2 * win)), (10 if fs < 10000 else 16)


def num_frames(L: int, fs: int) -> int:
    win, hop, _, _ = geometry(fs)
    return max(int(L / hop - win / hop), 0)


def trimmed_count(F: int) -> int:
    """how many of the F per-frame values the LLR / WSS means keep: Python's round (half to even) of 0.95 F"""
    return int(round(F * ALPHA))


def window(win: int) -> np.ndarray:
    return 0.5 * (1.0 - np.cos(2.0 * np.pi * (np.arange(1, win + 1, dtype=np.float64) / (win + 1))))


def frames(x: np.ndarray, fs: int) -> np.ndarray:
    """[F, W] windowed frames of x"""
    win, hop, _, _ = geometry(fs)
    F = num_frames(x.size, fs)
    idx = hop * np.arange(F)[:, None] + np.arange(win)[None, :]
    return np.asarray(x, dtype=np.float64)[idx] * window(win)[None, :]


@functools.lru_cache(maxsize=None)
def band_table(fs: int):
    """[(first bin, weights)] per critical band: Gaussian filters over the bins below nfft / 2 whose weights sum alike
    (factor bw_min / bw_i), the entries at or below the -30 dB factor dropped"""
    _, _, nfft, _ = geometry(fs)
    n2, max_freq = nfft // 2, fs / 2.0
    min_factor = math.exp(-30.0 / (2 * 2.303))
    j = np.arange(n2, dtype=np.float64)
    out = []
    for fc, bw_hz in zip(CENT_FREQ, BANDWIDTH):
        f0 = math.floor(fc / max_freq * n2)
        bw = bw_hz / max_freq * n2
        g = np.exp(-11.0 * ((j - f0) / bw) ** 2 + (math.log(BANDWIDTH[0]) - math.log(bw_hz)))
        keep = np.nonzero(g > min_factor)[0]
        assert keep.size and np.array_equal(keep, np.arange(keep[0], keep[-1] + 1))
        out.append((int(keep[0]), g[keep[0]:keep[-1] + 1].copy()))
    return out


def band_matrix(fs: int) -> np.ndarray:
    _, _, nfft, _ = geometry(fs)
    M = np.zeros((NUM_CRIT, nfft // 2))
    for b, (s, w) in enumerate(band_table(fs)):
        M[b, s:s + w.size] = w
    return M


# ------------------------------------------------------------------------------------------------ LLR
def autocorr(fr: np.ndarray, P: int) -> np.ndarray:
    """[F, P + 1] lags 0 .. P of every frame"""
    W = fr.shape[1]
    return np.stack([(fr[:, :W - k] * fr[:, k:]).sum(axis=1) for k in range(P + 1)], axis=1)


def levinson(R: np.ndarray) -> np.ndarray:
    """[F, P + 1] prediction polynomials (1, -a_1, .., -a_P) of the lags R [F, P + 1]"""
    F, P = R.shape[0], R.shape[1] - 1
    a = np.zeros((F, P))
    E = R[:, 0].copy()
    for i in range(P):
        s = (a[:, :i] * R[:, i:0:-1]).sum(axis=1) if i else 0.0
        rc = (R[:, i + 1] - s) / np.maximum(1e-15, E)
        if i:
            a[:, :i] = a[:, :i] - rc[:, None] * a[:, i - 1::-1]
        a[:, i] = rc
        E = (1.0 - rc * rc) * E
    return np.concatenate([np.ones((F, 1)), -a], axis=1)


def toeplitz_form(c: np.ndarray, R: np.ndarray) -> np.ndarray:
    """c T(R) c^T per frame, T(R)[i, j] = R[|i - j|]"""
    n = c.shape[1]
    lag = np.abs(np.arange(n)[:, None] - np.arange(n)[None, :])
    return np.einsum("fi,fij,fj->f", c, R[:, lag], c)


def llr_frames(x: np.ndarray, y: np.ndarray, fs: int) -> np.ndarray:
    P = geometry(fs)[3]
    Rx = autocorr(frames(x, fs), P)
    Ry = autocorr(frames(y, fs), P)
    ax, ay = levinson(Rx), levinson(Ry)
    num = np.maximum(1e-10, toeplitz_form(ay, Rx))
    den = np.maximum(1e-10, toeplitz_form(ax, Rx))
    with np.errstate(all="ignore"):
        return np.nan_to_num(np.log(num / den))


# ------------------------------------------------------------------------------------------------ WSS
def band_energies_db(x: np.ndarray, fs: int) -> np.ndarray:
    """[F, 25] critical-band energies of every frame, in dB with a floor of 1e-10"""
    nfft = geometry(fs)[2]
    spec = np.abs(np.fft.fft(frames(x, fs), nfft, axis=1)[:, :nfft // 2]) ** 2
    return 10.0 * np.log10(np.maximum(spec @ band_matrix(fs).T, 1e-10))


def nearest_peaks(E: np.ndarray) -> np.ndarray:
    """[F, 24]: for band i, the band energy its slope points to.  A rising slope is followed to the right through
    the run of rising slopes up to n, the first band whose slope does not rise (or 24), and E[n - 1] is taken, as
    the reference indexes it; any other slope is followed to the left through the run of non-rising slopes down to
    n, the first band whose slope rises (or -1), and E[n + 1] is taken."""
    slope = E[:, 1:] - E[:, :-1]
    up = slope > 0
    F, nb = up.shape
    right = np.empty((F, nb), dtype=np.int64)      # first n >= i with slope[n] <= 0, or nb
    nxt = np.full(F, nb)
    for i in range(nb - 1, -1, -1):
        nxt = np.where(up[:, i], nxt, i)
        right[:, i] = nxt
    left = np.empty((F, nb), dtype=np.int64)       # last n <= i with slope[n] > 0, or -1
    prv = np.full(F, -1)
    for i in range(nb):
        prv = np.where(up[:, i], i, prv)
        left[:, i] = prv
    pick = np.where(up, right - 1, left + 1)
    return np.take_along_axis(E, pick, axis=1)


def wss_frames(x: np.ndarray, y: np.ndarray, fs: int) -> np.ndarray:
    Ex, Ey = band_energies_db(x, fs), band_energies_db(y, fs)
    sx, sy = Ex[:, 1:] - Ex[:, :-1], Ey[:, 1:] - Ey[:, :-1]

    def weight(E):
        wmax = KMAX / (KMAX + E.max(axis=1, keepdims=True) - E[:, :-1])
        wloc = KLOCMAX / (KLOCMAX + nearest_peaks(E) - E[:, :-1])
        return wmax * wloc

    W = (weight(Ex) + weight(Ey)) / 2.0
    return (W * (sx - sy) ** 2).sum(axis=1) / W.sum(axis=1)


def wss_slope_margin_db(x: np.ndarray, y: np.ndarray, fs: int) -> float:
    """smallest non-zero |slope| (dB) over all frames, bands and both signals: the slope's sign steers the peak
    search, the one hard decision the device takes on its own arithmetic (an exact 0, as between two bands on the
    floor, is exact on the device too)"""
    m = np.inf
    for s in (x, y):
        E = band_energies_db(s, fs)
        d = np.abs(E[:, 1:] - E[:, :-1])
        d = d[d > 0]
        if d.size:
            m = min(m, float(d.min()))
    return m


# ------------------------------------------------------------------------------------------------ segmental SNR
def condition(x: np.ndarray, y: np.ndarray):
    """the signals the segmental SNR (and, in the reference, PESQ after it) sees: means removed, the estimate rescaled
    to the reference's peak"""
    x = np.asarray(x, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    x = x - x.mean()
    y = y - y.mean()
    with np.errstate(all="ignore"):
        y = y * (np.abs(x).max() / np.abs(y).max())
    return x, y


def ssnr_frames(x: np.ndarray, y: np.ndarray, fs: int):
    """(overall SNR in dB, [F] segmental SNR per frame clamped to [-10, 35]); NaN passes through the clamp"""
    x, y = condition(x, y)
    with np.errstate(all="ignore"):
        snr = 10.0 * np.log10((x ** 2).sum() / (((x - y) ** 2).sum() + 1e-19))
        fx, fy = frames(x, fs), frames(y, fs)
        seg = 10.0 * np.log10((fx ** 2).sum(axis=1) / (((fx - fy) ** 2).sum(axis=1) + 1e-10) + 1e-10)
    seg = np.where(seg < MIN_SNR, MIN_SNR, seg)
    seg = np.where(seg > MAX_SNR, MAX_SNR, seg)
    return float(snr), seg


# ------------------------------------------------------------------------------------------------ aggregates
def trimmed_mean(v: np.ndarray) -> float:
    return float(np.sort(v)[:trimmed_count(v.size)].mean())


def clip_mos(v: float) -> float:
    return v if math.isnan(v) else min(max(v, 1.0), 5.0)


def composites(llr: float, wss: float, segsnr: float, pesq: float):
    """(csig, cbak, covl): Hu & Loizou's regressions, each clipped to [1, 5]"""
    return (clip_mos(3.093 - 1.029 * llr + 0.603 * pesq - 0.009 * wss),
            clip_mos(1.634 + 0.478 * pesq - 0.007 * wss + 0.063 * segsnr),
            clip_mos(1.594 + 0.805 * pesq - 0.512 * llr - 0.007 * wss))


def measures(x: np.ndarray, y: np.ndarray, fs: int) -> dict:
    """per-frame arrays and aggregates of one (reference x, estimate y) pair"""
    lf, wf = llr_frames(x, y, fs), wss_frames(x, y, fs)
    snr, sf = ssnr_frames(x, y, fs)
    return {"llr_frames": lf, "wss_frames": wf, "ssnr_frames": sf, "frames": lf.size,
            "llr": trimmed_mean(lf), "wss": trimmed_mean(wf), "segsnr": float(sf.mean()), "snr": snr}


# ------------------------------------------------------------------------------------------------ test inputs
SNRS_DB = (-5.0, 0.0, 5.0, 10.0, 15.0, 20.0, 2.5, 12.5)
# name -> (fs, n, L, rows) for make_items.  The rows, (source seed, noise seed) pairs, were searched so that every
# non-zero band slope of every item stays 1e-3 dB away from zero (tests/test_gpu_composite.py asserts it): with 24
# slopes per frame and signal, about one random row in a hundred of the 263-frame cases passes.  fs16k and fs8k (two
# seconds plus 61 samples, no multiple of the hop) are the inputs of tests/golden/composite.npz.
CASES = {
    "fs16k": (16000, 2, 2 * 16000 + 61, ((101000, 12), (102091, 1), (103063, 7))),
    "fs8k": (8000, 2, 2 * 8000 + 61, ((201154, 14), (202091, 16), (203028, 3))),
    "long": (16000, 1, 10 * 16000, ((301476, 131),)),
    "short": (16000, 2, 14 * 120 + 7, ((401000, 1),)),       # 10 frames: round(9.5) = 10, half to even
    "silence": (16000, 2, 8000 + 61, ((501007, 3),)),         # with_silence(*SILENCE) applied
}
SILENCE = (3000, 2500)        # exact zeros in ref and est: 13 frames lie wholly inside


@functools.lru_cache(maxsize=None)
def make_items(n: int, L: int, fs: int, rows: tuple):
    """(ref, est) float32 [B, n, L], one batch row per (source seed, noise seed) pair of `rows`: ref =
    synthetic_sources; est_i = ref_i + leakage of the row's other source + white noise at SNRs from -5 to +20 dB (the
    recipe of tests/test_gpu_stoi.py).  Rows carry their own seeds so that inputs whose every band slope clears
    wss_slope_margin_db can be found row by row.  Shared by the golden capture and the tests: read-only."""
    import torch

    from ditsep_amd import synthetic

    B = len(rows)
    ref = torch.empty((B, n, L), dtype=torch.float64)
    est = torch.empty_like(ref)
    for b, (seed, noise_seed) in enumerate(rows):
        ref[b] = synthetic.synthetic_sources(1, n, L, fs=fs, seed=seed)[0].double()
        noise = torch.randn((n, L), generator=torch.Generator().manual_seed(noise_seed), dtype=torch.float64)
        for i in range(n):
            s = ref[b, i]
            snr = SNRS_DB[(b * n + i) % len(SNRS_DB)]
            d = 0.5 * ref[b, (i + 1) % n] + 0.3 * s.abs().max() * noise[i]
            est[b, i] = s + d * (s.norm() / d.norm()) * 10 ** (-snr / 20)
    return ref.float(), est.float()


def with_silence(ref, est, start: int, length: int):
    """copies of (ref, est) with the same stretch of exact zeros in every item of both"""
    ref, est = ref.clone(), est.clone()
    ref[..., start:start + length] = 0.0
    est[..., start:start + length] = 0.0
    return ref, est
