"""Restatement of dsn_dereverb (include/ditsep_hip.h): weighted prediction error (WPE) dereverberation, the offline
recipe (Nakatani et al. 2010; Yoshioka & Nakatani 2012).

Per item: mixture y [C, L], parameters taps K, delay D, iterations I, n_fft, hop, reg, eps.  Padding, analysis and window
are those of tests/mask_refine_restatement.py (torch.stft / torch.istft, center = True, pad_mode = "reflect", the
periodic Hann window rounded once to float32).  Per bin f, with Y(t) in C^C the frame's channels:
  y~(t) in C^(C K), entry k C + c = Y_c(t - D - k), zero where t - D - k < 0
  X = Y;  I times:
    lambda(t) = mean_c |X_c(t)|^2,  m = max_t lambda,  lambda <- max(lambda, 1e-10 m);  m == 0: the bin passes (G = 0)
    R = sum_t y~ y~^H / lambda(t),  P = sum_t y~ Y(t)^H / lambda(t)
    delta = reg tr(R) / (C K) + eps,  A = R + delta I,  G = A^-1 P
    a pivot of A's Cholesky factorisation that is not finite and positive: G = 0 from here on, the bin is counted
    X_c(t) = Y_c(t) - sum_j conj(G[j][c]) y~_j(t)
and x is the inverse transform of X, rounded once to the working precision, cropped to L.

The per-bin solve is written twice: numpy.linalg.solve (`solver="solve"`) and the explicit Cholesky factorisation with
the two triangular solves that the device runs (`solver="cholesky"`, the default; it is the one that sees the pivots).
tests/test_dereverb_host.py records how closely the two agree (the filters of its cases: at most 1e-7 of the largest
entry apart at cond(A) <= 1e7).

dtype = float64 is the reference.  dtype = float32 is the yardstick of the device's rounding error: transforms in
float32 (pocketfft's), the whole solve in float64 on the widened spectra, X rounded once to float32 -- the device's own
split of precisions.  reg and eps are the float32 values the device call takes, widened."""
import numpy as np
import torch

from tests import stems_restatement as sr

DEFAULTS = dict(taps=10, delay=3, iterations=3, n_fft=512, hop=128, reg=1e-4, eps=1e-10)


def stack(Y, taps, delay):
    """Y [bins, C, F] -> y~ [bins, C taps, F], entry k C + c = Y_c(t - delay - k), zero before the first frame"""
    bins, C, F = Y.shape
    out = np.zeros((bins, C * taps, F), dtype=Y.dtype)
    for k in range(taps):
        s = delay + k
        if s < F:
            out[:, k * C:(k + 1) * C, s:] = Y[:, :, :F - s]
    return out


def cholesky_solve(A, Bm):
    """A [bins, N, N] Hermitian, Bm [bins, N, C] -> (A^-1 Bm by A = L L^H, L y = b, L^H z = y, column by column; ok
    [bins], False where a pivot was not finite and positive -- the solution is zero there)"""
    N = A.shape[-1]
    Lm = np.zeros_like(A)
    ok = np.ones(A.shape[0], dtype=bool)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for c in range(N):
            d = A[:, c, c].real - np.sum(np.abs(Lm[:, c, :c]) ** 2, axis=-1)
            ok &= np.isfinite(d) & (d > 0)
            l = np.sqrt(np.where(ok, d, 1.0))
            Lm[:, c, c] = l
            s = A[:, c + 1:, c] - np.einsum("frk,fk->fr", Lm[:, c + 1:, :c], Lm[:, c, :c].conj())
            Lm[:, c + 1:, c] = s / l[:, None]
        Yv = np.zeros_like(Bm)
        for r in range(N):
            s = Bm[:, r, :] - np.einsum("fk,fkj->fj", Lm[:, r, :r], Yv[:, :r, :])
            Yv[:, r, :] = s / Lm[:, r, r][:, None]
        Z = np.zeros_like(Bm)
        for r in range(N - 1, -1, -1):
            s = Yv[:, r, :] - np.einsum("fk,fkj->fj", Lm[:, r + 1:, r].conj(), Z[:, r + 1:, :])
            Z[:, r, :] = s / Lm[:, r, r][:, None]
    Z[~ok] = 0.0
    return Z, ok


def wpe(Y, taps, delay, iterations, reg, eps, solver="cholesky", return_cond=False):
    """Y [bins, C, F] complex128 -> (X [bins, C, F], G [bins, C taps, C] of the last iteration, fail [bins] bool,
    cond [bins]: cond(A) of the last iteration, or None)"""
    bins, C, F = Y.shape
    N = C * taps
    Yt = stack(Y, taps, delay)
    X = Y.copy()
    G = np.zeros((bins, N, C), dtype=np.complex128)
    fail = np.zeros(bins, dtype=bool)
    cond = None
    for _ in range(iterations):
        lam = (X.real ** 2 + X.imag ** 2).sum(axis=1) / C
        m = lam.max(axis=-1)
        live = (m != 0) & ~fail
        lam = np.maximum(lam, 1e-10 * m[:, None])
        lam[~live] = 1.0
        with np.errstate(invalid="ignore"):                                  # (a NaN sample: the pivots catch it)
            Yw = Yt / lam[:, None, :]
            R = np.einsum("fit,fjt->fij", Yw, Yt.conj())
            P = np.einsum("fit,fct->fic", Yw, Y.conj())
        delta = reg * np.einsum("fii->f", R).real / N + eps
        A = R + delta[:, None, None] * np.eye(N)
        if solver == "solve":
            Gn = np.linalg.solve(A, P)
            ok = np.isfinite(Gn).all(axis=(1, 2))
            Gn[~ok] = 0.0
        else:
            Gn, ok = cholesky_solve(A, P)
        fail |= live & ~ok
        live &= ok
        G = np.where(live[:, None, None], Gn, 0.0)
        X = Y - np.einsum("fjc,fjt->fct", G.conj(), Yt)
        if return_cond:
            cond = np.where(live, np.linalg.cond(A), 1.0)
    return X, G, fail, cond


def dereverb(mix, taps=10, delay=3, iterations=3, n_fft=512, hop=128, reg=1e-4, eps=1e-10, dtype=np.float64,
             solver="cholesky", return_info=False, return_cond=False):
    """mix [C, L] -> out [C, L] in `dtype` (and {"G": [bins, C taps, C], "fail": the count of bins a failed pivot
    passed through, "cond": the worst bin's cond(A) in the last iteration (with return_cond)})"""
    mix = np.atleast_2d(np.asarray(mix, dtype=dtype))
    C, L = mix.shape
    Z, w, Lp = sr._stft(mix, n_fft, hop, dtype)
    Y = np.ascontiguousarray(Z.numpy().astype(np.complex128).transpose(1, 0, 2))
    r32, e32 = float(np.float32(reg)), float(np.float32(eps))
    X, G, fail, cond = wpe(Y, taps, delay, iterations, r32, e32, solver, return_cond)
    Xt = torch.from_numpy(np.ascontiguousarray(X.transpose(1, 0, 2))).to(Z.dtype)   # rounded once
    y = torch.istft(Xt, n_fft, hop_length=hop, win_length=n_fft, window=w, center=True, length=Lp)
    out = y[:, :L].numpy()
    if not return_info:
        return out
    return out, {"G": G, "fail": int(fail.sum()), "cond": None if cond is None else float(cond.max())}


def round_trip(mix, n_fft=512, hop=128, dtype=np.float64):
    """analysis and synthesis alone: what an item with F <= delay, or a silent one, comes back as"""
    mix = np.atleast_2d(np.asarray(mix, dtype=dtype))
    Z, w, Lp = sr._stft(mix, n_fft, hop, dtype)
    return torch.istft(Z, n_fft, hop_length=hop, win_length=n_fft, window=w, center=True, length=Lp)[:, :mix.shape[1]].numpy()


def reverb_case(seed, C, L, fs=16000, rt=0.3, early=0.02, noise=1e-3, burst=2000):
    """Burst noise (white noise switched on and off every `burst` samples) through C exponentially decaying random
    impulse responses of `rt` seconds (60 dB down at their end), plus sensor noise.
    -> (mix [C, L] float32, the source convolved with the first `early` seconds of channel 0's response [L])"""
    g = np.random.default_rng(seed)
    src = g.standard_normal(L) * ((np.arange(L) // burst) % 2 == 0)
    T = int(rt * fs)
    h = g.standard_normal((C, T)) * np.exp(-6.9 * np.arange(T) / T)
    n = 1 << int(np.ceil(np.log2(L + T)))
    S = np.fft.rfft(src, n)
    wet = np.stack([np.fft.irfft(S * np.fft.rfft(h[c], n), n)[:L] for c in range(C)])
    scale = 0.5 / np.max(np.abs(wet))
    mix = scale * wet + noise * g.standard_normal((C, L))
    h0 = h[0].copy()
    h0[int(early * fs):] = 0.0
    target = scale * np.fft.irfft(S * np.fft.rfft(h0, n), n)[:L]
    return mix.astype(np.float32), target.astype(np.float32)


def rel_err(a, b, mix):
    return float(np.max(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))) / np.max(np.abs(mix)))


def si_sdr(est, ref):
    """scale-invariant signal-to-distortion ratio in dB"""
    est, ref = np.asarray(est, np.float64), np.asarray(ref, np.float64)
    t = (est @ ref) / (ref @ ref) * ref
    return float(10.0 * np.log10((t @ t) / ((est - t) @ (est - t))))
