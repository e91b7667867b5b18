"""Restatement of dsn_activity and dsn_activity_gate (include/ditsep_hip.h) in numpy.

Per item: estimates s [n, L], STFT n_fft / hop on mask_refine_restatement's framing (periodic Hann rounded once to
float32, centred, reflected at the item's own padded end, F = 1 + ceil(L / hop) frames).
  E_i(t)   = sum over the band's bins j_lo .. j_hi of |S_i(j, t)|^2, in float64 from the spectrum of the working dtype
  lev_i(t) = the mean of E_i over the frames max(0, t - h) .. min(F - 1, t + h), added in increasing order
  P = max lev, top(t) = max_i lev_i(t), NaN passed over; P = 0: inactive throughout
  on  = lev >= P c_r  and lev >= top c_d;  stay the same with the primed factors
  a(t) = on(t) or (a(t - 1) and stay(t)); then the run rules: short gaps between runs filled, short runs cleared, runs
  padded and merged.
`energies` takes the working dtype (float64: the reference; float32, through torch.stft in float32 as
mask_refine_restatement.refine_torch: the yardstick of the device's rounding error).
`decide` is written twice -- `decide_loops`, the sequential loops of the definition, and `decide_scans`, vectorised with
cumulative maxima and minima -- and the two must agree exactly.  `segments`, `gate` and `rttm_lines` restate the frame
and sample map, the gate and the RTTM text."""
import math

import numpy as np

from tests import mask_refine_restatement as mrr


def band_bins(band, fs, n_fft):
    j_lo = int(math.ceil(float(band[0]) * n_fft / fs))
    j_hi = min(n_fft // 2, int(math.floor(float(band[1]) * n_fft / fs)))
    assert j_lo <= j_hi
    return j_lo, j_hi


def constants(range_db=40.0, dominance_db=6.0, hysteresis_db=3.0):
    r, d, h = float(range_db), float(dominance_db), float(hysteresis_db)
    return 10.0 ** (-r / 10.0), 10.0 ** (-d / 10.0), 10.0 ** (-(r + h) / 10.0), 10.0 ** (-(d + h) / 10.0)


def spectra(est, n_fft=512, hop=128, dtype=np.float64):
    """est [n, L] -> S [n, F, n_fft / 2 + 1] complex, formed in `dtype`.  float64: mask_refine_restatement's explicit
    framing and numpy.fft.rfft.  float32: torch.stft in float32, the route of mask_refine_restatement.refine_torch
    that the device tests take as their yardstick.  numpy.fft.rfft is not used for it: on float32 frames numpy 2.2
    returns, bit for bit, the float64 transform rounded once, which is no float32 run of the transform and whose band
    energies are 10 to 20 times closer to float64 than any float32 FFT's."""
    est = np.asarray(est, dtype=dtype)
    n, L = est.shape
    Lp = mrr.padded_length(L, hop)
    w = mrr.window(n_fft, dtype)
    x = np.zeros((n, Lp), dtype=dtype)
    x[:, :L] = est
    if dtype == np.float64:
        return np.stack([np.fft.rfft(mrr.frames_of(r, n_fft, hop, w), axis=-1) for r in x])
    import torch

    Z = torch.stft(torch.from_numpy(x), n_fft, hop_length=hop, win_length=n_fft, window=torch.from_numpy(w), center=True,
                   pad_mode="reflect", return_complex=True)                          # [n, bins, F]
    assert Z.dtype == torch.complex64 and Z.shape[-1] == 1 + Lp // hop
    return Z.numpy().transpose(0, 2, 1)


def energies(est, n_fft=512, hop=128, bins=None, dtype=np.float64):
    """est [n, L] -> E [n, F] float64: the band energy of every frame, from spectra formed in `dtype`"""
    Z = spectra(est, n_fft, hop, dtype)
    j_lo, j_hi = (0, n_fft // 2) if bins is None else bins
    re, im = Z.real.astype(np.float64), Z.imag.astype(np.float64)
    return (re * re + im * im)[:, :, j_lo:j_hi + 1].sum(axis=2)


def levels(E, half_width):
    """E [n, F] float64 -> lev [n, F]: the box mean, added in increasing frame order, one division"""
    n, F = E.shape
    lev = np.zeros((n, F))
    for t in range(F):
        ua, ub = max(0, t - half_width), min(F - 1, t + half_width)
        s = np.zeros(n)
        for u in range(ua, ub + 1):
            s = s + E[:, u]
        lev[:, t] = s / float(ub - ua + 1)
    return lev


def thresholds(lev, consts):
    """-> (on, stay) [n, F] bool, and the ratios lev / threshold of every comparison that has a positive threshold"""
    c_r, c_d, c_rs, c_ds = consts
    ok = ~np.isnan(lev)
    P = float(np.max(np.where(ok, lev, 0.0), initial=0.0))
    top = np.max(np.where(ok, lev, 0.0), axis=0, initial=0.0)
    with np.errstate(invalid="ignore"):
        on = (P > 0.0) & (lev >= P * c_r) & (lev >= top * c_d)
        stay = (P > 0.0) & (lev >= P * c_rs) & (lev >= top * c_ds)
    thr = [np.full_like(lev, P * c_r), np.broadcast_to(top * c_d, lev.shape), np.full_like(lev, P * c_rs),
           np.broadcast_to(top * c_ds, lev.shape)]
    with np.errstate(invalid="ignore", divide="ignore"):
        ratios = np.concatenate([(lev / t)[(t > 0.0) & ok] for t in thr])
    return on, stay, ratios


def runs_of(a):
    """bool [F] -> [(s, e), ..], the runs of True"""
    edges = np.flatnonzero(np.diff(np.concatenate([[0], np.asarray(a, np.int8), [0]])))
    return list(zip(edges[0::2].tolist(), edges[1::2].tolist()))


def rules_loops(a, min_on, min_off, pad):
    """the run rules on one row, as the definition states them"""
    a = np.array(a, dtype=bool)
    F = len(a)
    rs = runs_of(a)
    for (s0, e0), (s1, e1) in zip(rs[:-1], rs[1:]):                                  # gaps between two on-runs
        if s1 - e0 < min_off:
            a[e0:s1] = True
    for s, e in runs_of(a):
        if e - s < min_on:
            a[s:e] = False
    out = np.zeros(F, dtype=bool)
    for s, e in runs_of(a):
        out[max(0, s - pad):min(F, e + pad)] = True
    return out


def hysteresis_loops(on, stay):
    a = np.zeros(len(on), dtype=bool)
    prev = False
    for t in range(len(on)):
        prev = bool(on[t]) or (prev and bool(stay[t]))
        a[t] = prev
    return a


def _nearest(v):
    """bool [F] -> (the index of the last True at or before t, -1 without one; of the first at or after t, F)"""
    F = len(v)
    idx = np.arange(F)
    before = np.maximum.accumulate(np.where(v, idx, -1))
    after = np.minimum.accumulate(np.where(v, idx, F)[::-1])[::-1]
    return before, after


def hysteresis_scans(on, stay):
    """a(t) is set iff the last frame at or before t that decides -- on, or not stay -- is an on frame"""
    on, stay = np.asarray(on, bool), np.asarray(stay, bool)
    last_on, _ = _nearest(on)
    last_drop, _ = _nearest(~stay & ~on)
    return last_on > last_drop


def rules_scans(a, min_on, min_off, pad):
    a = np.asarray(a, bool)
    F = len(a)
    t = np.arange(F)
    before, after = _nearest(a)
    a = a | ((before >= 0) & (after < F) & (after - before - 1 < min_off))
    before, after = _nearest(~a)
    a = a & ~(after - before - 1 < min_on)
    before, after = _nearest(a)
    return a | ((before >= 0) & (t - before <= pad)) | ((after < F) & (after - t <= pad))


def decide(E, half_width=2, consts=None, min_on=13, min_off=13, pad=0, form="loops"):
    """E [n, F] float64 -> (act [n, F] uint8, lev [n, F], the comparison ratios)"""
    consts = constants() if consts is None else consts
    lev = levels(np.asarray(E, np.float64), half_width)
    on, stay, ratios = thresholds(lev, consts)
    hyst, rules = (hysteresis_loops, rules_loops) if form == "loops" else (hysteresis_scans, rules_scans)
    act = np.stack([rules(hyst(on[i], stay[i]), min_on, min_off, pad) for i in range(len(lev))])
    return act.astype(np.uint8), lev, ratios


def decide_both(E, **kw):
    """`decide` in both forms, which must agree exactly -> (act, lev, ratios)"""
    a, lev, ratios = decide(E, form="loops", **kw)
    b, lev2, _ = decide(E, form="scans", **kw)
    assert np.array_equal(a, b) and np.array_equal(lev, lev2, equal_nan=True), "the two forms of decide disagree"
    return a, lev, ratios


def segments(act_row, F, hop, L):
    """the runs of a row as sample segments: frame t owns [t hop - hop / 2, (t + 1) hop - hop / 2) of [0, L)"""
    out = []
    for s, e in runs_of(np.asarray(act_row)[:F] != 0):
        lo, hi = max(0, s * hop - hop // 2), min(L, e * hop - hop // 2)
        if hi > lo:
            out.append((lo, hi))
    return out


def ramp(fade):
    d = np.arange(1, fade + 1, dtype=np.float64)
    return (0.5 + 0.5 * np.cos(np.pi * d / (fade + 1))).astype(np.float32)


def gate(x, act_row, hop, fade):
    """x [L] float32, one row of act -> the gated row, by brute force over the samples"""
    x = np.asarray(x, np.float32)
    L = len(x)
    m = np.arange(L)
    fr = (m + hop // 2) // hop
    a = np.asarray(act_row)
    inside = a[np.minimum(fr, len(a) - 1)] != 0
    idx = np.flatnonzero(inside)
    out = np.zeros(L, dtype=np.float32)
    out[inside] = x[inside]
    if len(idx) == 0 or fade == 0:
        return out
    pos = np.searchsorted(idx, m)
    left = np.where(pos > 0, m - idx[np.maximum(pos - 1, 0)], np.iinfo(np.int64).max)
    right = np.where(pos < len(idx), idx[np.minimum(pos, len(idx) - 1)] - m, np.iinfo(np.int64).max)
    d = np.minimum(left, right)
    fading = ~inside & (d <= fade)
    r = ramp(fade)
    with np.errstate(invalid="ignore"):
        out[fading] = r[d[fading] - 1] * x[fading]
    return out


def rttm_lines(stem, segs_per_source, fs):
    """segments in samples per source -> the RTTM lines, sorted by onset then source"""
    rows = sorted((s, i, e) for i, row in enumerate(segs_per_source) for s, e in row)
    return [f"SPEAKER {stem} 1 {s / fs:.3f} {(e - s) / fs:.3f} <NA> <NA> s{i} <NA> <NA>" for s, i, e in rows]


def burst_case(seed, n, L, hop, leak=0.1):
    """n white-noise sources switched on and off in stretches of 1 to 40 hops at levels spread over 20 dB, each
    estimate with `leak` of the others added -> est [n, L] float32: runs and gaps on both sides of every minimum
    duration the tests use"""
    g = np.random.default_rng(seed)
    src = g.standard_normal((n, L)) * 0.1
    for i in range(n):
        p, on = 0, bool(g.integers(2))
        while p < L:
            q = p + int(g.integers(1, 41)) * hop + int(g.integers(hop))
            src[i, p:q] *= (10.0 ** (-g.uniform(0.0, 1.0))) if on else 0.0
            p, on = q, not on
    est = src + leak * (src.sum(axis=0)[None] - src)
    return est.astype(np.float32)


def truth_frames(on_samples, hop):
    """on_samples [n, L] bool -> [n, F]: the source is on at sample min(L - 1, t hop)"""
    n, L = on_samples.shape
    F = 1 + -(-L // hop)
    return on_samples[:, np.minimum(L - 1, np.arange(F) * hop)]
