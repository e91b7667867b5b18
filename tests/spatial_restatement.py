"""Restatement of dsn_beamform_spatial (include/ditsep_hip.h): the masks that steer dsn_beamform refined by a complex
angular central Gaussian mixture model (cACGMM; Ito, Araki, Nakatani 2016) with the estimates' masks as time-frequency
priors (Nakatani et al. 2017; Drude & Haeb-Umbach 2017), then dsn_beamform's weights and apply.

Per item: mixture x [C, L], mono estimates s [n, L], reference channel ref, the parameters of tests/beamform_restatement.py
(n_fft, hop, power, eps, reg) and iterations, noise nu, floor phi, mask_reg, mask_eps.  Padding, analysis, window, spectra
X_c(f,t) and masks M_k are those of tests/mask_refine_restatement.py.  Per bin f:
  p(t) = sum_c |X_c|^2 (channel order);  a frame is live where p > 0;  z(t) = X(t) / sqrt(p(t))
  K = n + 1 classes if nu > 0, otherwise n;  priors a_k = (1 - nu) ((1 - phi) M_k + phi / n) for k < n,  a_n = nu
  B_k = I;  `iterations` times:
    E-step  B_k = L L^H,  q_k(t) = z^H B_k^-1 z = sum |y|^2 with L y = z,  l_k = 2 sum_c log L_cc,
            log gamma_k(t) = log a_k - l_k - C log q_k, normalised over the classes with the maximum subtracted
    M-step  over the live frames in increasing t:  B_k = C sum_t (gamma_k / q_k) z z^H / sum_t gamma_k, the identity
            where sum_t gamma_k is zero;  then B_k += (mask_reg tr(B_k) / C + mask_eps) I
            a Cholesky pivot of any B_k that is not finite and positive: every B_k of the bin is the identity from here
            on (gamma is then the normalised prior) and the bin is counted in `failed`
  one more E-step gives gamma; dead frames take gamma = a; an item with one channel skips the EM and takes gamma = a,
  and so does a call with iterations = 0 (every B_k is the identity: the posterior is the prior)
  N_k = sum_t gamma_k X X^H for all K classes (the unnormalised spectra, as in dsn_beamform)
  the weights of dsn_beamform with Q_i = sum_{j != i, j < K} N_j: the noise class enters every Q_i and gets no filter
  Y_i = sum_c conj(w_i,c) X_c rounded once to the working precision, no post-filter; y_i its inverse transform.

The quadratic form q and the log-determinant l are written twice: numpy.linalg (`solver="solve"`: numpy.linalg.solve and
numpy.linalg.slogdet) and the explicit Cholesky factorisation with one forward substitution that the device runs
(`solver="cholesky"`, the default).  The pivots are those of the explicit factorisation under either solver.
tests/test_spatial_host.py measures how closely the two agree.

dtype = float64 is the reference.  dtype = float32 is the yardstick of the device's rounding error: transforms and masks
in float32 (pocketfft's), the mixture model, statistics and solve in float64 on the widened values, Y rounded once to
float32 -- the device's own split of precisions.  eps, reg, noise, floor, mask_reg and mask_eps are the float32 values
the device call takes, widened."""
import numpy as np
import torch

from tests import beamform_restatement as br
from tests import stems_restatement as sr

DEFAULTS = dict(iterations=1, noise=0.1, floor=0.1, reg=1e-3, eps=1e-10)


def priors(M, noise, floor):
    """M [n, bins, F] float64 -> a [K, bins, F]"""
    n = M.shape[0]
    a = (1.0 - noise) * ((1.0 - floor) * M + floor / n)
    if noise > 0:
        a = np.concatenate([a, np.full_like(M[:1], noise)])
    return a


def cholesky(B):
    """B [bins, K, C, C] Hermitian -> (L [bins, K, C, C] lower triangular with B = L L^H, ok [bins]: False where a
    pivot of any class was not finite and positive), column by column as the device does"""
    C = B.shape[-1]
    Lm = np.zeros_like(B)
    ok = np.ones(B.shape[0], dtype=bool)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for c in range(C):
            d = B[..., c, c].real - np.sum(Lm[..., c, :c].real ** 2 + Lm[..., c, :c].imag ** 2, axis=-1)
            ok &= (np.isfinite(d) & (d > 0)).all(axis=-1)
            l = np.sqrt(d)
            Lm[..., c, c] = l
            for r in range(c + 1, C):
                s = B[..., r, c] - np.sum(Lm[..., r, :c] * Lm[..., c, :c].conj(), axis=-1)
                Lm[..., r, c] = s / l
    return Lm, ok


def quadratic(B, Lm, z, solver):
    """B, Lm [bins, K, C, C], z [bins, F, C] -> (q [bins, K, F] = z^H B^-1 z, l [bins, K] = log det B)"""
    C = B.shape[-1]
    if solver == "solve":
        zt = np.swapaxes(z, 1, 2)[:, None]                                          # [bins, 1, C, F]
        u = np.linalg.solve(B, np.broadcast_to(zt, B.shape[:2] + zt.shape[2:]))
        q = np.einsum("fct,fkct->fkt", z.conj().swapaxes(1, 2), u).real
        return q, np.linalg.slogdet(B)[1]
    y = np.zeros(B.shape[:2] + (z.shape[1], C), dtype=np.complex128)               # [bins, K, F, C]
    for r in range(C):
        s = z[:, None, :, r] - np.einsum("fkc,fktc->fkt", Lm[:, :, r, :r], y[..., :r])
        y[..., r] = s / Lm[:, :, r, r].real[..., None]
    q = np.sum(y.real ** 2 + y.imag ** 2, axis=-1)
    return q, 2.0 * np.sum(np.log(np.einsum("fkcc->fkc", Lm).real), axis=-1)


def e_step(B, Lm, z, a, live, solver):
    """-> (gamma [K, bins, F], q [K, bins, F], the log-likelihood summed over the live frames and all bins)"""
    C = B.shape[-1]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        q, l = quadratic(B, Lm, z, solver)
        q, l = np.moveaxis(q, 1, 0), np.moveaxis(l, 1, 0)
        lg = np.log(a) - l[..., None] - C * np.log(q)
        mx = lg.max(axis=0)
        e = np.exp(lg - mx)
        s = e.sum(axis=0)
        gamma = e / s
        ll = float(np.sum((mx + np.log(s))[live]))
    return np.where(live[None], gamma, a), q, ll


def m_step(gamma, q, z, live, reg, eps):
    """-> B [bins, K, C, C]"""
    K, bins, F = gamma.shape
    C = z.shape[-1]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        wgt = np.where(live[None], gamma / q, 0.0)
        den = np.where(live[None], gamma, 0.0).sum(axis=-1)                          # [K, bins]
        zz = np.where(live[..., None], z, 0.0)
        S = np.einsum("kft,ftc,ftd->fkcd", wgt, zz, zz.conj())
        B = C * S / den.T[..., None, None]
    B[den.T == 0] = np.eye(C)
    tr = np.einsum("fkcc->fk", B).real
    return B + (reg * tr / C + eps)[..., None, None] * np.eye(C)


def mixture_model(X, M, iterations, noise, floor, reg, eps, solver="cholesky"):
    """X [C, bins, F] complex128, M [n, bins, F] float64 -> (gamma [K, bins, F], failed [bins] bool, the
    log-likelihood before every M-step and after the last: iterations + 1 values)"""
    C, bins, F = X.shape
    a = priors(M, noise, floor)
    K = a.shape[0]
    if C == 1 or iterations == 0:
        return a, np.zeros(bins, dtype=bool), []
    p = np.zeros((bins, F))
    for c in range(C):
        p = p + (X[c].real ** 2 + X[c].imag ** 2)
    live = p > 0
    with np.errstate(invalid="ignore", divide="ignore"):
        z = np.moveaxis(X, 0, -1) / np.sqrt(p)[..., None]                            # [bins, F, C]
    z = np.where(live[..., None], z, 0.0)
    eye = np.broadcast_to(np.eye(C, dtype=np.complex128), (bins, K, C, C)).copy()
    B, Lm = eye.copy(), eye.copy()
    failed = np.zeros(bins, dtype=bool)
    lls = []
    for _ in range(iterations):
        gamma, q, ll = e_step(B, Lm, z, a, live, solver)
        lls.append(ll)
        Bn = m_step(gamma, q, z, live, reg, eps)
        Ln, ok = cholesky(Bn)
        failed |= ~ok
        B = np.where(failed[:, None, None, None], eye, Bn)
        Lm = np.where(failed[:, None, None, None], eye, Ln)
    gamma, _, ll = e_step(B, Lm, z, a, live, solver)
    lls.append(ll)
    return gamma, failed, lls


def weights(N, n, ref, eps, reg, solver="cholesky"):
    """N [K, bins, C, C], K >= n classes -> w [n, bins, C]: tests/beamform_restatement.py's weights with the
    interference summed over all K classes"""
    K, bins, C, _ = N.shape
    w = np.zeros((n, bins, C), dtype=np.complex128)
    for i in range(n):
        Q = np.zeros_like(N[0])
        for j in range(K):
            if j != i:
                Q = Q + N[j]
        lam = reg * np.einsum("fcc->f", Q).real / C + eps
        A = Q + lam[:, None, None] * np.eye(C)
        with np.errstate(invalid="ignore", divide="ignore"):
            Z = np.linalg.solve(A, N[i]) if solver == "solve" and np.all(np.isfinite(A)) \
                else br.cholesky_solve(A, N[i])
            tau = np.einsum("fcc->f", Z).real
            ok = np.isfinite(tau) & (tau > 0)
            w[i, :, ref] = 1.0
            col = Z[ok][:, :, ref]
            w[i, ok] = col.real / tau[ok, None] + 1j * (col.imag / tau[ok, None])
    return w


def beamform_spatial(mix, est, ref=0, n_fft=512, hop=128, power=2, eps=1e-10, reg=1e-3, iterations=1, noise=0.1,
                     floor=0.1, mask_reg=1e-3, mask_eps=1e-10, dtype=np.float64, solver="cholesky",
                     return_info=False):
    """mix [C, L], est [n, L] -> out [n, L] in `dtype` (and {"w": [n, bins, C], "gamma": [K, bins, F] float64,
    "failed": the count of failed bins, "ll": the log-likelihoods, "power": the mixture's power per bin})"""
    mix, est = np.atleast_2d(np.asarray(mix, dtype=dtype)), np.asarray(est, dtype=dtype)
    (C, L), n = mix.shape, est.shape[0]
    assert 0 <= ref < C
    tdt = torch.float64 if dtype == np.float64 else torch.float32
    Z, w, Lp = sr._stft(np.concatenate([mix, est]), n_fft, hop, dtype)
    X, M = Z[:C], sr._masks(Z[C:], n, power, eps, tdt)
    f32 = lambda v: float(np.float32(v))
    X64, M64 = X.numpy().astype(np.complex128), M.numpy().astype(np.float64)
    gamma, failed, lls = mixture_model(X64, M64, int(iterations), f32(noise), f32(floor), f32(mask_reg), f32(mask_eps),
                                       solver)
    with np.errstate(invalid="ignore", over="ignore"):
        wt = weights(br.statistics(X64, gamma), n, ref, f32(eps), f32(reg), solver)
        Y = torch.from_numpy(np.einsum("ifc,cft->ift", wt.conj(), X64)).to(Z.dtype)   # rounded once
    y = torch.istft(Y, n_fft, hop_length=hop, win_length=n_fft, window=w, center=True, length=Lp)
    out = y[:, :L].numpy()
    if not return_info:
        return out
    return out, {"w": wt, "gamma": gamma, "failed": int(failed.sum()), "ll": lls,
                 "power": (np.abs(X64) ** 2).sum(axis=(0, 2))}
