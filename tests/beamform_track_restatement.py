"""Restatement of dsn_beamform_track (include/ditsep_hip.h): mask-based MVDR beamforming with block-adaptive weights.

Everything up to the statistics is tests/beamform_restatement.py's (the frames, the spectra X, the masks M, F = 1 +
ceil(L / hop), the widening to float64), and so are the statistics of a range of frames (`statistics`) and the solve
(`weights`), which are called, not copied.  With Tb = block_frames, per item, source i and bin f:
  blocks         block k holds the frames [k Tb, min(F, (k + 1) Tb)), K = ceil(F / Tb)
  partials       P_i^(k) = sum_{t in block k} M_i X X^H
  context        N_i^(k) = sum_{j = max(0, k - context)}^{min(K - 1, k + context)} P_i^(j), added in increasing j
  weights        w_i^(k) = beamform_restatement.weights(N^(k))
  frame weights  num = 2 t + 1 - Tb in integers; num <= 0: k0 = 0, alpha = 0; otherwise k0 = num // (2 Tb), alpha =
                 float(num % (2 Tb)) / float(2 Tb); k0 >= K - 1: k0 = K - 1, alpha = 0.  interpolate = False: k0 = t //
                 Tb, alpha = 0.  w(t) = w^(k0) + alpha (w^(k0+1) - w^(k0)) per real and imaginary part; where alpha = 0,
                 w(t) = w^(k0)
  apply          Y_i(f, t) = sum_c conj(w_i,c(t)) X_c in channel order, rounded once to the working precision; postfilter
                 "mask": Y_i <- M_i Y_i; y_i is the inverse transform of Y_i, cropped to L.
dtype = float64 is the reference, dtype = float32 the yardstick of the device's rounding error, as in
beamform_restatement."""
import numpy as np
import torch

from tests import beamform_restatement as br
from tests import stems_restatement as sr

DEFAULTS = dict(block_frames=100, context=1, interpolate=True)


def frame_plan(F, Tb, interpolate=True):
    """-> (k0 [F] int, alpha [F] float64), one frame at a time in Python integers"""
    K = -(-F // Tb)
    k0, alpha = np.zeros(F, dtype=np.int64), np.zeros(F, dtype=np.float64)
    for t in range(F):
        if not interpolate:
            k0[t] = t // Tb
            continue
        num = 2 * t + 1 - Tb
        if num <= 0:
            continue
        k = num // (2 * Tb)
        if k >= K - 1:
            k0[t] = K - 1
            continue
        k0[t], alpha[t] = k, float(num % (2 * Tb)) / float(2 * Tb)
    return k0, alpha


def block_weights(X, M, ref, eps, reg, Tb, context, solver="cholesky"):
    """X [C, bins, F] complex128, M [n, bins, F] float64 -> w [K, n, bins, C] complex128"""
    F = X.shape[-1]
    K = -(-F // Tb)
    P = [br.statistics(X[:, :, k * Tb:min(F, (k + 1) * Tb)], M[:, :, k * Tb:min(F, (k + 1) * Tb)]) for k in range(K)]
    w = []
    for k in range(K):
        N = np.zeros_like(P[0])
        for j in range(max(0, k - context), min(K - 1, k + context) + 1):
            N = N + P[j]
        w.append(br.weights(N, ref, eps, reg, solver))
    return np.stack(w)


def beamform_track(mix, est, ref=0, n_fft=512, hop=128, power=2, eps=1e-10, reg=1e-3, postfilter=None, block_frames=100,
                   context=1, interpolate=True, dtype=np.float64, solver="cholesky", return_info=False):
    """mix [C, L], est [n, L] -> out [n, L] in `dtype` (and {"w": [K, n, bins, C], "power": [K, bins], the mixture's
    power per bin summed over the channels and the frames of block k's context window})"""
    mix, est = np.atleast_2d(np.asarray(mix, dtype=dtype)), np.asarray(est, dtype=dtype)
    (C, L), n = mix.shape, est.shape[0]
    assert 0 <= ref < C and postfilter in (None, "none", "mask")
    tdt = torch.float64 if dtype == np.float64 else torch.float32
    Z, win, Lp = sr._stft(np.concatenate([mix, est]), n_fft, hop, dtype)
    X, M = Z[:C], sr._masks(Z[C:], n, power, eps, tdt)
    e32, r32 = float(np.float32(eps)), float(np.float32(reg))
    X64, M64 = X.numpy().astype(np.complex128), M.numpy().astype(np.float64)
    F, Tb = X64.shape[-1], int(block_frames)
    K = -(-F // Tb)
    wt = block_weights(X64, M64, ref, e32, r32, Tb, int(context), solver)
    k0, alpha = frame_plan(F, Tb, interpolate)
    w0 = wt[k0]                                                        # [F, n, bins, C]
    w1 = wt[np.minimum(k0 + 1, K - 1)]
    a = alpha[:, None, None, None]
    wf = np.where(a == 0.0, w0, (w0.real + a * (w1.real - w0.real)) + 1j * (w0.imag + a * (w1.imag - w0.imag)))
    Y64 = np.zeros((n,) + X64.shape[1:], dtype=np.complex128)
    for c in range(C):                                                 # conj(w_c(t)) X_c, in channel order, in reals
        wr, wi = wf[..., c].real.transpose(1, 2, 0), wf[..., c].imag.transpose(1, 2, 0)
        xr, xi = X64[c].real[None], X64[c].imag[None]
        p = (wr * xr + wi * xi) + 1j * (wr * xi - wi * xr)
        Y64 = p if c == 0 else Y64 + p
    Y = torch.from_numpy(Y64).to(Z.dtype)                              # rounded once
    if postfilter == "mask":
        Y = M * Y
    y = torch.istft(Y, n_fft, hop_length=hop, win_length=n_fft, window=win, center=True, length=Lp)
    out = y[:, :L].numpy()
    if not return_info:
        return out
    p = (np.abs(X64) ** 2).sum(axis=0)                                 # [bins, F]
    blocks = np.stack([p[:, k * Tb:min(F, (k + 1) * Tb)].sum(axis=-1) for k in range(K)])
    pw = np.stack([blocks[max(0, k - context):min(K - 1, k + context) + 1].sum(axis=0) for k in range(K)])
    return out, {"w": wt, "power": pw}


def moving_case(seed=0, C=3, n=2, L=128000, taps=24, leak=0.3, burst=2000, pos=4):
    """beamform_restatement.sanity_case with a source that moves: source 0's samples are cut into `pos` equal segments,
    each segment goes through its own random `taps`-tap mixing filters (the first through sanity_case's own) and the
    segments' images are summed; the other sources keep one filter each.  -> (mix [C, L], est [n, L], img0 [n, L], the
    images at channel 0) float32"""
    g = np.random.default_rng(seed)
    src = g.standard_normal((n, L)) * 0.1
    for i in range(n):
        on = (np.arange(L) // burst + i) % (n + 1) != 0
        src[i] *= on
    h = g.standard_normal((n, C, taps)) / np.sqrt(taps)
    moved = g.standard_normal((pos - 1, C, taps)) / np.sqrt(taps)
    img = np.stack([[np.convolve(src[i], h[i, c])[:L] for c in range(C)] for i in range(n)])
    seg = -(-L // pos)
    img[0] = 0.0
    for p in range(pos):
        part = np.zeros(L)
        part[p * seg:(p + 1) * seg] = src[0, p * seg:(p + 1) * seg]
        hp = h[0] if p == 0 else moved[p - 1]
        img[0] += np.stack([np.convolve(part, hp[c])[:L] for c in range(C)])
    mix = img.sum(axis=0) + 1e-3 * g.standard_normal((C, L))
    img0 = img[:, 0]
    est = img0 + leak * (img0.sum(axis=0)[None] - img0)
    return mix.astype(np.float32), est.astype(np.float32), img0.astype(np.float32)
