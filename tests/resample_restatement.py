"""float64 numpy restatement of the sinc resampler (include/ditsep_hip.h, dsn_resample; csrc/resample_plan.h).  Imports
nothing from ditsep_amd.

The definition is the default of torchaudio.transforms.Resample (sinc_interp_hann, lowpass_filter_width 6, rolloff
0.99): g = gcd(fs_in, fs_out), o = fs_in / g, n = fs_out / g, base = min(o, n) 0.99, width = ceil(6 o / base),
K = 2 width + o;  t = clamp((-p / n + (k - width) / o) base, -6, 6),
h[p][k] = float32(sinc(pi t) cos^2(pi t / 12) base / o);  out[m n + p] = sum_k h[p][k] xz[m o + k - width] for
m n + p < ceil(n L / o), xz being x extended by zeros.

Two routes to the same numbers:
  resample_a   the definition, literally: the dense table, padding by (width, width + o), frames of K samples with
               stride o, the crop
  resample_b   no phases and no frames: out[j] = sum_i x[i] G(i n - j o), G(u) the float32-rounded prototype at
               t = u base / (o n)
Both take float32 taps widened to float64 and sum in float64; both also return A[j] = sum |tap| |x|, the scale of the
rounding bounds the tests derive."""
import math

import numpy as np

RATES_MODEL = (8000, 16000)
RATES_ALL = (8000, 11025, 16000, 22050, 24000, 32000, 44100, 48000)
# every pair with the model's rate on one side, both directions: 28 (the two equal pairs included)
PAIRS = sorted({(a, b) for a in RATES_MODEL for b in RATES_ALL} | {(b, a) for a in RATES_MODEL for b in RATES_ALL})


def params(fs_in, fs_out):
    """-> (o, n, base, width, K)"""
    g = math.gcd(int(fs_in), int(fs_out))
    o, n = int(fs_in) // g, int(fs_out) // g
    base = min(o, n) * 0.99
    width = int(math.ceil(6 * o / base))
    return o, n, base, width, 2 * width + o


def prototype(t, scale):
    """float32(sinc(pi t) cos^2(pi t / 12) scale) of float64 t, clamped to [-6, 6]"""
    t = np.clip(np.asarray(t, dtype=np.float64), -6.0, 6.0)
    w = np.cos(t * np.pi / 6.0 / 2.0)
    a = t * np.pi
    s = np.where(a == 0.0, 1.0, np.sin(a) / np.where(a == 0.0, 1.0, a))
    return (s * (w * w) * scale).astype(np.float32)


def dense_taps(fs_in, fs_out):
    """h float32 [n, K]"""
    o, n, base, width, K = params(fs_in, fs_out)
    p = np.arange(n, dtype=np.float64)[:, None]
    k = np.arange(K, dtype=np.float64)[None, :]
    return prototype((-p / n + (k - width) / o) * base, base / o)


def compact(h):
    """the run of non-zero taps per phase -> (k0 int [n], S, c float32 [n, S]); also checks nothing else is dropped"""
    n, K = h.shape
    k0 = np.zeros(n, dtype=np.int64)
    last = np.zeros(n, dtype=np.int64)
    for p in range(n):
        nz = np.flatnonzero(h[p] != 0.0)
        k0[p], last[p] = (nz[0], nz[-1]) if nz.size else (0, -1)
    S = max(int((last - k0 + 1).max()), 1)
    c = np.zeros((n, S), dtype=np.float32)
    for p in range(n):
        run = h[p, k0[p]:last[p] + 1]
        c[p, :run.size] = run
        assert np.all(h[p, :k0[p]] == 0.0) and np.all(h[p, last[p] + 1:] == 0.0)
    return k0, S, c


def dense_from_compact(k0, c, K):
    """the dense table [n, K] a compact one stands for (float32)"""
    n, S = c.shape
    h = np.zeros((n, K), dtype=np.float32)
    for p in range(n):
        m = min(S, K - int(k0[p]))
        h[p, k0[p]:k0[p] + m] = c[p, :m]
        assert np.all(c[p, m:] == 0.0)
    return h


def length(o, n, L):
    return -(-n * int(L) // o)


def resample_a(x, fs_in, fs_out, h=None):
    """x float [L] -> (out float64 [Lout], A float64 [Lout]).  h: float32 [n, K] (default: dense_taps)."""
    o, n, _, width, K = params(fs_in, fs_out)
    h = (dense_taps(fs_in, fs_out) if h is None else h).astype(np.float64)
    assert h.shape == (n, K)
    x = np.asarray(x, dtype=np.float64)
    L = x.shape[0]
    xp = np.concatenate([np.zeros(width), x, np.zeros(width + o)])
    M = (xp.shape[0] - K) // o + 1
    frames = np.lib.stride_tricks.sliding_window_view(xp, K)[::o][:M]         # [M, K]
    out = (frames @ h.T).reshape(-1)                                           # [M n], index m n + p
    A = (np.abs(frames) @ np.abs(h).T).reshape(-1)
    Lout = length(o, n, L)
    assert out.shape[0] >= Lout
    return out[:Lout], A[:Lout]


def resample_b(x, fs_in, fs_out):
    """the same numbers without phases or frames -> (out, A)"""
    o, n, base, _, _ = params(fs_in, fs_out)
    x = np.asarray(x, dtype=np.float64)
    L = x.shape[0]
    Lout = length(o, n, L)
    u = np.arange(L, dtype=np.int64)[None, :] * n - np.arange(Lout, dtype=np.int64)[:, None] * o      # [Lout, L]
    G = prototype(u.astype(np.float64) * base / (o * n), base / o).astype(np.float64)
    return G @ x, np.abs(G) @ np.abs(x)


def resample(x, fs_in, fs_out, h=None):
    """the public call's rule: equal rates are a copy"""
    if int(fs_in) == int(fs_out):
        x = np.asarray(x, dtype=np.float64)
        return x.copy(), np.abs(x)
    return resample_a(x, fs_in, fs_out, h)
