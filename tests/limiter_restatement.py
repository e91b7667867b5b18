"""float64 restatement of the true-peak look-ahead limiter (include/ditsep_hip.h, dsn_limiter_curve / dsn_apply_curve;
csrc/limiter.hip) and of the `limit` keyword's gain rule (native.limiter_drive).  Imports nothing from ditsep_amd.

For a group of rows (the rows that share one curve) with the pre-gain G, the ceiling c (linear) and the half-window
W = max(1, floor(lookahead_ms fs / 1000 + 1/2)):
  1 pre-gain   y = float32(G x): the one step taken in float32, because the definition names its bits
  2 envelope   p[t] = max over rows and channels of max(|y[t]|, |u[4 t]|, .., |u[4 t + 3]|), u the row interpolated
               1 -> 4 by tests/resample_restatement.py
  3 required   r[t] = min(1, c / p[t]), 1 where p = 0
  4 hold       m[t] = min over |s - t| <= W of r[s], r = 1 outside [0, L) -- for every t, also outside the item
  5 smoothing  g[t] = max(0, min(r[t], 1 - a[t])), a[t] = sum_{k=-W..W} w[k] (1 - m[t + k]),
               w[k] = float32((1/2 + 1/2 cos(pi k / (W + 1))) / (W + 1))
  6 output     out = y g
The device lowers r by one float where the float32 product r p would round above c; the restatement does not, and the
tests' bound has room for that ulp.  The hold is written twice (scipy.ndimage.minimum_filter1d and an explicit loop)
and the two must agree exactly."""
import math

import numpy as np
from scipy.ndimage import minimum_filter1d

from tests import loudness_restatement as lr
from tests import resample_restatement as rr

DEFAULTS = dict(ceiling=None, lookahead_ms=5.0, drive_db=6.0, iterations=4, tol=0.1)


def half_window(lookahead_ms, fs):
    return max(1, int(math.floor(lookahead_ms * fs / 1000.0 + 0.5)))


def window(W):
    """float32 [2 W + 1], w[-W .. W]"""
    k = np.arange(-W, W + 1, dtype=np.float64)
    return ((0.5 + 0.5 * np.cos(np.pi * k / (W + 1))) / (W + 1)).astype(np.float32)


def pregain(x, G):
    """step 1: float32(G x) widened to float64; x [..., L]"""
    return (np.float32(G) * np.asarray(x, dtype=np.float32)).astype(np.float64)


def envelope(y, taps=None):
    """y float64 [rows, L] (every channel of every row of the group) -> (p [L], A [L]: the largest sum |h| |y| behind
    an interpolated value at t -- the scale of the float32 rounding bound)"""
    y = np.atleast_2d(np.asarray(y, dtype=np.float64))
    L = y.shape[-1]
    p, A = np.zeros(L), np.zeros(L)
    for row in y:
        u, a = rr.resample_a(row, 1, 4, taps)
        p = np.maximum(p, np.maximum(np.abs(row), np.abs(u).reshape(L, 4).max(axis=1)))
        A = np.maximum(A, a.reshape(L, 4).max(axis=1))
    return p, A


def required(p, c):
    with np.errstate(divide="ignore"):
        return np.where(p > 0.0, np.minimum(1.0, c / np.where(p > 0.0, p, 1.0)), 1.0)


def hold(r, W):
    """m over [-W, L + W) (index i stands for t = i - W): the two ways, which must agree exactly"""
    ext = np.concatenate([np.ones(2 * W), r, np.ones(2 * W)])                       # t = -2 W .. L + 2 W - 1
    a = minimum_filter1d(ext, size=2 * W + 1, mode="constant", cval=1.0)[W:-W]
    b = np.array([ext[i:i + 2 * W + 1].min() for i in range(ext.shape[0] - 2 * W)])[:a.shape[0]]
    assert a.shape == b.shape == (r.shape[0] + 2 * W,) and np.array_equal(a, b)
    return a


def curve_from_required(r, W):
    """steps 4 and 5 -> g [L]"""
    m = hold(r, W)
    w = window(W).astype(np.float64)
    a = np.convolve(1.0 - m, w, mode="valid")                                       # (w is symmetric)
    assert a.shape == r.shape
    return np.maximum(0.0, np.minimum(r, 1.0 - a))


def curve(x, G, c, W, taps=None):
    """x [rows, L] float32 (all rows and channels of one group) -> dict: y [rows, L], p, A, r, g [L]"""
    y = pregain(np.atleast_2d(x), G)
    p, A = envelope(y, taps)
    r = required(p, float(c))
    return {"y": y, "p": p, "A": A, "r": r, "g": curve_from_required(r, W)}


def curve_bound(p, A, c, W, S=13):
    """|g - g64| <= max_{|s - t| <= 2 W} (c dp[s] / p[s]^2) + (2 W + 4) 2^-24, dp = (S + 1) 2^-24 A the resampler's bound:
    min and max are 1-Lipschitz and the smoothing is a convex combination.  Where p <= c both sides have r = 1."""
    u = 2.0 ** -24
    dp = (S + 1) * u * A
    with np.errstate(divide="ignore", invalid="ignore"):
        dr = np.where(p > 0.0, float(c) * dp / (p * p), 0.0)
    dr = np.where(p + dp <= float(c), 0.0, np.minimum(dr, 1.0))
    ext = np.concatenate([np.zeros(2 * W), dr, np.zeros(2 * W)])
    return -minimum_filter1d(-ext, size=4 * W + 1, mode="constant", cval=0.0)[2 * W:-2 * W] + (2 * W + 4) * u


def drive(g_lo, i_src, target, history, drive_db=6.0, iterations=4, tol=0.1):
    """the keyword's pre-gain rule, restated: -> the next G in dB or None (stop)"""
    lo, hi = g_lo, g_lo + drive_db
    if len(history) == 0:
        return float(np.clip(target - i_src, lo, hi))
    G, I = history[-1]
    if not np.isfinite(I) or abs(target - I) <= tol or len(history) >= iterations:
        return None
    if len(history) == 1:
        nxt = G + (target - I)
    else:
        Gp, Ip = history[-2]
        s = (I - Ip) / (G - Gp) if G != Gp and np.isfinite(Ip) else 1.0
        nxt = G + (target - I) / float(np.clip(s, 0.25, 1.0))
    nxt = float(np.clip(nxt, lo, hi))
    return None if nxt in [h[0] for h in history] else nxt


def best(history, target):
    d = [abs(target - I) if np.isfinite(I) else np.inf for _, I in history]
    return int(np.argmin(d))


def normalize(stems, mixture, fs, target, peak, link="mixture", limit=None, taps=None):
    """One item through the `loudness` + `limit` keywords in float64: stems [n, C, L] float32, mixture [C', L] (link
    "mixture": the gain source and the programme that is measured).  -> dict: "limited" (the single-gain rule was held
    back by the ceiling), "single" (what that rule alone reaches: gain_db, loudness_out), and with limit the history
    of (G dB, I) pairs, the kept evaluation, "out" [n, C, L] float64 after the trim, "loudness_out", "true_peak",
    "min_gain".  With link "stem" every stem is a group: the entries are lists of n."""
    opts = dict(DEFAULTS, **(limit or {}))
    stems = np.asarray(stems, dtype=np.float32)
    n, Cn, L = stems.shape
    c_db = opts["ceiling"] if opts["ceiling"] is not None else (peak if peak is not None else -1.0)
    c = float(np.float32(10.0 ** (c_db / 20.0)))
    W = half_window(opts["lookahead_ms"], fs)
    groups = [list(range(n))] if link == "mixture" else [[i] for i in range(n)]
    res = []
    for rows in groups:
        prog = np.asarray(mixture, dtype=np.float32) if link == "mixture" else stems[rows[0]]
        prog = np.atleast_2d(prog)
        i_src = lr.measure(prog.astype(np.float64), fs, true_peak=False)["loudness"]
        tp = max(lr.measure(stems[i].astype(np.float64), fs, taps=taps)["true_peak"] for i in rows)
        g_lo = lr.gain_db(i_src, tp, target, peak)
        out = {"limited": g_lo < target - i_src, "single": {"gain_db": g_lo, "loudness_out": i_src + g_lo}}
        res.append(out)
        if limit is None or not out["limited"]:
            continue
        flat = stems[rows].reshape(-1, L)
        hist, G = [], drive(g_lo, i_src, target, [], opts["drive_db"], opts["iterations"], opts["tol"])
        while G is not None:
            lin = float(np.float32(10.0 ** (G / 20.0)))
            cv = curve(flat, lin, c, W, taps)
            limited_prog = pregain(prog, lin) * cv["g"]
            hist.append((G, lr.measure(limited_prog, fs, true_peak=False)["loudness"]))
            G = drive(g_lo, i_src, target, hist, opts["drive_db"], opts["iterations"], opts["tol"])
        k = best(hist, target)
        lin = float(np.float32(10.0 ** (hist[k][0] / 20.0)))
        cv = curve(flat, lin, c, W, taps)
        y = (cv["y"] * cv["g"]).reshape(len(rows), Cn, L)
        top = max(lr.measure(v, fs, taps=taps)["true_peak"] for v in y)
        trim = float(np.float32(c / top)) if top > c else 1.0
        out.update(history=hist, kept=k, out=y * trim, trim=trim, overshoot=top - c, min_gain=float(cv["g"].min()),
                   loudness_out=hist[k][1] + 20.0 * math.log10(trim), true_peak=top * trim)
    return res[0] if link == "mixture" else res


def burst_sources(fs=16000, seconds=4.0, n=2, peak=0.3, seed=0):
    """the keyword tests' input: white noise times (0.5 (1 - cos(2 pi (3 + 2 k) t + k)))^6 for source k, each scaled to
    `peak` -> float32 [n, L]"""
    g = np.random.default_rng(seed)
    L = int(round(seconds * fs))
    t = np.arange(L, dtype=np.float64) / fs
    out = np.zeros((n, L))
    for k in range(n):
        v = g.standard_normal(L) * (0.5 * (1.0 - np.cos(2.0 * np.pi * (3 + 2 * k) * t + k))) ** 6
        out[k] = peak * v / np.abs(v).max()
    return out.astype(np.float32)
