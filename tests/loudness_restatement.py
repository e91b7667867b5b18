"""float64 restatement of the loudness measurement (include/ditsep_hip.h, dsn_loudness; csrc/loudness.hip).  Imports
nothing from ditsep_amd.

ITU-R BS.1770-4 / EBU R 128 integrated loudness with the K-weighting computed from the rate (the libebur128 /
pyloudnorm formulation), every channel with weight 1:
  shelf      f0 = 1681.974450955533, G = 3.999843853973347 dB, Q = 0.7071752369554196, K = tan(pi f0 / fs),
             Vh = 10^(G / 20), Vb = Vh^0.4996667741545416, a0 = 1 + K / Q + K^2,
             b = [Vh + Vb K / Q + K^2, 2 (K^2 - Vh), Vh - Vb K / Q + K^2] / a0, a = [1, 2 (K^2 - 1) / a0, (1 - K / Q + K^2) / a0]
  high-pass  f0 = 38.13547087602444, Q = 0.5003270373238773, the same K, a0 and a, b = [1, -2, 1]
  blocks     h = (fs + 5) // 10; block j = samples [j h, j h + 4 h) of the filtered signal (zero state at sample 0),
             complete blocks only; z_j = sum_c mean(y_c^2), l_j = -0.691 + 10 log10(z_j)
  gates      l_j > -70; Gamma = -0.691 + 10 log10(mean z over those) - 10; I = -0.691 + 10 log10(mean z over the
             blocks with l_j > -70 and l_j > Gamma), -inf when none passes
  true peak  max |.| of every channel resampled 1 -> 4 by tests/resample_restatement.py (the project's resampler)

`measure` runs in float64 (scipy.signal.lfilter, numpy framing); `measure(..., dtype=numpy.float32)` is the same
restatement with the recursion (lfilter computes in the dtype of its arguments: direct form II transposed), the
squares and every sum in float32 -- the yardstick for what single precision would give."""
import math

import numpy as np
from scipy.signal import lfilter

from tests import resample_restatement as rr

SHELF = (1681.974450955533, 3.999843853973347, 0.7071752369554196)
HIGHPASS = (38.13547087602444, 0.5003270373238773)
VB_EXP = 0.4996667741545416
# ITU-R BS.1770-4, tables 1 and 2 (48 kHz)
TABLE_48K = {"shelf_b": (1.53512485958697, -2.69169618940638, 1.19839281085285),
             "shelf_a": (-1.69065929318241, 0.73248077421585),
             "highpass_a": (-1.99004745483398, 0.99007225036621)}


def coeffs(fs):
    """-> float64 [10]: shelf b0 b1 b2 a1 a2, high-pass b0 b1 b2 a1 a2"""
    f0, G, Q = SHELF
    K = math.tan(math.pi * f0 / fs)
    Vh = 10.0 ** (G / 20.0)
    Vb = Vh ** VB_EXP
    a0 = 1.0 + K / Q + K * K
    shelf = [(Vh + Vb * K / Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0,
             2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0]
    f0, Q = HIGHPASS
    K = math.tan(math.pi * f0 / fs)
    a0 = 1.0 + K / Q + K * K
    return np.array(shelf + [1.0, -2.0, 1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0], dtype=np.float64)


def block_step(fs):
    return (int(fs) + 5) // 10


def kweight(x, fs, dtype=np.float64):
    """x [C, L] -> the filtered signal [C, L] in `dtype`"""
    c = coeffs(fs).astype(dtype)
    one = np.ones(1, dtype=dtype)
    x = np.asarray(x, dtype=dtype)
    y = lfilter(c[0:3], np.concatenate([one, c[3:5]]), x, axis=-1)
    y = lfilter(c[5:8], np.concatenate([one, c[8:10]]), y.astype(dtype), axis=-1)
    return y.astype(dtype)


def lufs(z):
    with np.errstate(divide="ignore"):
        return -0.691 + 10.0 * np.log10(z)


def measure(x, fs, dtype=np.float64, true_peak=True, taps=None):
    """x [C, L] (or [L]) -> dict: "loudness", "blocks", "gated_blocks", "z" [J], "l" [J], "gamma" (NaN when no block
    passes the absolute gate), "sample_peak", and with true_peak "true_peak" and "true_peak_scale" (sum |h| |x| at the
    interpolated sample where that is largest: the scale of the float32 rounding bound).  taps: the dense float32
    table [4, K] of the 1 -> 4 plan (default: resample_restatement.dense_taps)"""
    x = np.atleast_2d(np.asarray(x))
    Cn, L = x.shape
    y = kweight(x, fs, dtype)
    h = block_step(fs)
    J = (L - 4 * h) // h + 1 if L >= 4 * h else 0
    z = np.zeros(J, dtype=dtype)
    if J:
        sq = (y * y).astype(dtype)
        for c in range(Cn):
            frames = np.lib.stride_tricks.sliding_window_view(sq[c], 4 * h)[::h][:J]
            z = (z + frames.sum(axis=1, dtype=dtype) / dtype(4 * h)).astype(dtype)
    l = lufs(z.astype(np.float64)) if dtype == np.float64 else lufs(z).astype(dtype)
    out = {"blocks": J, "z": z, "l": l, "gamma": float("nan"), "loudness": -math.inf, "gated_blocks": 0,
           "sample_peak": float(np.abs(x.astype(np.float64)).max())}
    absg = l > -70.0
    if absg.any():
        gamma = lufs(z[absg].sum(dtype=dtype) / dtype(int(absg.sum()))) - dtype(10.0)
        both = absg & (l > gamma)
        out["gamma"] = float(gamma)
        out["gated_blocks"] = int(both.sum())
        if both.any():
            out["loudness"] = float(lufs(z[both].sum(dtype=dtype) / dtype(int(both.sum()))))
    if true_peak:
        tp, scale = 0.0, 0.0
        for c in range(Cn):
            v, A = rr.resample_a(x[c].astype(np.float64), 1, 4, taps)
            tp = max(tp, float(np.abs(v).max()))
            scale = max(scale, float(A.max()))
        out["true_peak"], out["true_peak_scale"] = tp, scale
    return out


def gate_margin(m):
    """how far (LU) the nearest block of a measurement lies from either gate: inf without blocks"""
    l = np.asarray(m["l"], dtype=np.float64)
    l = l[np.isfinite(l)]
    if l.size == 0:
        return math.inf
    d = np.abs(l + 70.0).min()
    if not math.isnan(m["gamma"]):
        d = min(d, np.abs(l - m["gamma"]).min())
    return float(d)


def gain_db(I_src, true_peak, target, peak):
    """the gain rule for one group: target - I_src, at most peak - 20 log10(true_peak); 0 dB for I_src = -inf"""
    if I_src == -math.inf:
        return 0.0
    g = target - I_src
    if peak is not None and true_peak > 0.0:
        g = min(g, peak - 20.0 * math.log10(true_peak))
    return g


def sine(freq, dbfs, seconds, fs, channels=1):
    t = np.arange(int(round(seconds * fs)), dtype=np.float64) / fs
    return np.tile(10.0 ** (dbfs / 20.0) * np.sin(2.0 * np.pi * freq * t), (channels, 1))
