"""Restatement of dsn_beamform (include/ditsep_hip.h): mask-based MVDR beamforming.

Per item: mixture x [C, L], mono estimates s [n, L], reference channel ref, parameters n_fft, hop, power, eps, reg,
postfilter.  Padding, analysis, window and masks M_i are those of tests/mask_refine_restatement.py (torch.stft /
torch.istft, center = True, pad_mode = "reflect", the periodic Hann window rounded once to float32).  Per bin f:
  N_i = sum_t M_i X X^H                       (C x C Hermitian)
  Q_i = sum_{j != i} N_j                      (increasing j; zero for n = 1)
  lambda_i = reg tr(Q_i) / C + eps,  A = Q_i + lambda I
  Z = A^-1 N_i,  tau = sum_c Re Z_cc
  w_i = Z[:, ref] / tau where tau is finite and > 0, otherwise e_ref
  Y_i(f, t) = sum_c conj(w_i,c) X_c, rounded once to the working precision; postfilter "mask": Y_i <- M_i Y_i
and y_i is the inverse transform of Y_i, cropped to L.

The per-bin solve is written twice: numpy.linalg.solve (`solver="solve"`) and the explicit Cholesky factorisation with
two triangular solves per column that the device runs (`solver="cholesky"`).  On the cases of tests/test_beamform_host.py
the two sets of weights are at most 1e-9 apart relative to the largest weight (the systems are regularised to a condition
number of about 1 / reg = 1e3; measured: at most 3e-12).

dtype = float64 is the reference.  dtype = float32 is the yardstick of the device's rounding error: transforms and masks
in float32 (pocketfft's), statistics and solve in float64 on the widened values, Y rounded once to float32 -- the
device's own split of precisions.  eps and reg are the float32 values the device call takes, widened."""
import numpy as np
import torch

from tests import mask_refine_restatement as mr
from tests import stems_restatement as sr

DEFAULTS = dict(ref=0, n_fft=512, hop=128, power=2, eps=1e-10, reg=1e-3, postfilter=None)
KINDS = ("generic", "dual", "hard", "silent_ch", "silent_est")


def statistics(X, M):
    """X [C, bins, F] complex128, M [n, bins, F] float64 -> N [n, bins, C, C]: the products X_c conj X_d first (real on
    the diagonal), then the masks; the upper triangle is formed and mirrored"""
    C, n = X.shape[0], M.shape[0]
    N = np.zeros((n, X.shape[1], C, C), dtype=np.complex128)
    for c in range(C):
        for d in range(c, C):
            P = X[c] * X[d].conj() if d > c else (X[c].real ** 2 + X[c].imag ** 2).astype(np.complex128)
            N[:, :, c, d] = (M * P[None]).sum(axis=-1)
            if d > c:
                N[:, :, d, c] = N[:, :, c, d].conj()
    return N


def cholesky_solve(A, Bm):
    """A [..., C, C] Hermitian positive definite, Bm [..., C, K] -> A^-1 Bm by A = L L^H, L y = b, L^H z = y, written
    out column by column (NaN where A is not positive definite)"""
    C = A.shape[-1]
    Lm = np.zeros_like(A)
    with np.errstate(invalid="ignore", divide="ignore"):
        for c in range(C):
            d = A[..., c, c].real - np.sum(np.abs(Lm[..., c, :c]) ** 2, axis=-1)
            l = np.sqrt(d)
            Lm[..., c, c] = l
            for r in range(c + 1, C):
                s = A[..., r, c] - np.sum(Lm[..., r, :c] * Lm[..., c, :c].conj(), axis=-1)
                Lm[..., r, c] = s / l
        Y = np.zeros_like(Bm)
        for r in range(C):
            s = Bm[..., r, :] - np.einsum("...k,...kj->...j", Lm[..., r, :r], Y[..., :r, :])
            Y[..., r, :] = s / Lm[..., r, r][..., None]
        Z = np.zeros_like(Bm)
        for r in range(C - 1, -1, -1):
            s = Y[..., r, :] - np.einsum("...k,...kj->...j", Lm[..., r + 1:, r].conj(), Z[..., r + 1:, :])
            Z[..., r, :] = s / Lm[..., r, r][..., None]
    return Z


def weights(N, ref, eps, reg, solver="cholesky"):
    """N [n, bins, C, C] -> w [n, bins, C] complex128"""
    n, bins, C, _ = N.shape
    w = np.zeros((n, bins, C), dtype=np.complex128)
    for i in range(n):
        Q = np.zeros_like(N[0])
        for j in range(n):
            if j != i:
                Q = Q + N[j]
        lam = reg * np.einsum("fcc->f", Q).real / C + eps
        A = Q + lam[:, None, None] * np.eye(C)
        Z = np.linalg.solve(A, N[i]) if solver == "solve" else cholesky_solve(A, N[i])
        tau = np.einsum("fcc->f", Z).real
        ok = np.isfinite(tau) & (tau > 0)
        w[i, :, ref] = 1.0
        with np.errstate(invalid="ignore", divide="ignore"):
            col = Z[ok][:, :, ref]                                    # (a complex over a real: two real divisions)
            w[i, ok] = col.real / tau[ok, None] + 1j * (col.imag / tau[ok, None])
    return w


def beamform(mix, est, ref=0, n_fft=512, hop=128, power=2, eps=1e-10, reg=1e-3, postfilter=None, dtype=np.float64,
             solver="cholesky", return_info=False):
    """mix [C, L], est [n, L] -> out [n, L] in `dtype` (and {"w": [n, bins, C], "power": [bins], the mixture's power
    per bin summed over channels and frames})"""
    mix, est = np.atleast_2d(np.asarray(mix, dtype=dtype)), np.asarray(est, dtype=dtype)
    (C, L), n = mix.shape, est.shape[0]
    assert 0 <= ref < C and postfilter in (None, "none", "mask")
    tdt = torch.float64 if dtype == np.float64 else torch.float32
    Z, w, Lp = sr._stft(np.concatenate([mix, est]), n_fft, hop, dtype)
    X, M = Z[:C], sr._masks(Z[C:], n, power, eps, tdt)
    e32, r32 = float(np.float32(eps)), float(np.float32(reg))
    X64, M64 = X.numpy().astype(np.complex128), M.numpy().astype(np.float64)
    wt = weights(statistics(X64, M64), ref, e32, r32, solver)
    Y = torch.from_numpy(np.einsum("ifc,cft->ift", wt.conj(), X64)).to(Z.dtype)   # rounded once
    if postfilter == "mask":
        Y = M * Y
    y = torch.istft(Y, n_fft, hop_length=hop, win_length=n_fft, window=w, center=True, length=Lp)
    out = y[:, :L].numpy()
    if not return_info:
        return out
    return out, {"w": wt, "power": (np.abs(X64) ** 2).sum(axis=(0, 2))}


def images(seed, n, C, L, taps):
    """seeded white Gaussian sources through random mixing filters of `taps` taps -> (src [n, L], img [n, C, L]), img
    the source's image at every channel; the direct path (tap 0) of every filter is 1"""
    g = np.random.default_rng(seed)
    src = g.standard_normal((n, L)) * 0.1
    h = g.standard_normal((n, C, taps)) * (0.5 / np.sqrt(np.arange(1, taps + 1)))
    h[:, :, 0] = 1.0
    img = np.stack([[np.convolve(src[i], h[i, c])[:L] for c in range(C)] for i in range(n)])
    return src, img


def make_case(seed, kind, n, C, L, noise=0.3, taps=8):
    """-> (mix [C, L], est [n, L]) float32.  Every source is white, so every bin carries signal.  kind: "generic"
    (random short mixing filters plus sensor noise; the estimates are the noisy images at channel 0), "dual" (all
    channels equal), "hard" (every source in one channel only: source 1 in the last, source i in channel i mod C
    otherwise), "silent_ch" (generic with a silent channel C // 2), "silent_est" (generic with zero estimates)"""
    assert kind in KINDS
    g = np.random.default_rng(seed + 1)
    src, img = images(seed, n, C, L, taps)
    if kind == "dual":
        mix = np.repeat(src.sum(axis=0)[None], C, axis=0)
        clean = src
    elif kind == "hard":
        mix = np.zeros((C, L))
        for i in range(n):
            mix[C - 1 if i == 1 else i % C] += src[i]
        clean = src
    else:
        mix = img.sum(axis=0) + 0.01 * g.standard_normal((C, L))
        clean = img[:, 0]
        if kind == "silent_ch" and C > 1:
            mix[C // 2] = 0.0
    est = clean + noise * 0.1 * g.standard_normal((n, L))
    if kind == "silent_est":
        est = np.zeros_like(est)
    return mix.astype(np.float32), est.astype(np.float32)


def sanity_case(seed=0, C=4, n=2, L=32000, taps=24, leak=0.3, burst=2000):
    """n burst-noise sources (white noise switched on and off every `burst` samples, source i on in the bursts with
    (b + i) mod (n + 1) != 0 -- they overlap most of the time and each is alone for a while) through random `taps`-tap
    mixing filters into C channels, plus sensor noise 40 dB down; the estimates are the images at channel 0 with `leak`
    of every other image added.  -> (mix [C, L], est [n, L], img0 [n, L], the images at channel 0) float32"""
    g = np.random.default_rng(seed)
    src = g.standard_normal((n, L)) * 0.1
    for i in range(n):
        on = (np.arange(L) // burst + i) % (n + 1) != 0
        src[i] *= on
    h = g.standard_normal((n, C, taps)) / np.sqrt(taps)
    img = np.stack([[np.convolve(src[i], h[i, c])[:L] for c in range(C)] for i in range(n)])
    mix = img.sum(axis=0) + 1e-3 * g.standard_normal((C, L))
    img0 = img[:, 0]
    est = img0 + leak * (img0.sum(axis=0)[None] - img0)
    return mix.astype(np.float32), est.astype(np.float32), img0.astype(np.float32)


def rel_err(a, b, mix):
    return float(np.max(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))) / np.max(np.abs(mix)))


def si_sdr(est, ref):
    """scale-invariant signal-to-distortion ratio in dB"""
    est, ref = np.asarray(est, np.float64), np.asarray(ref, np.float64)
    t = (est @ ref) / (ref @ ref) * ref
    return float(10.0 * np.log10((t @ t) / ((est - t) @ (est - t))))
