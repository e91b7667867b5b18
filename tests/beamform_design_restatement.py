"""Restatement of the beamforming designs (include/ditsep_hip.h: DSN_BEAMFORM_DESIGN_*, dsn_beamform_design,
dsn_beamform_spatial_design, dsn_beamform_track_design, dsn_beamform_solve): rank-one MVDR and GEV weights.

Everything up to A = Q_i + lambda I is tests/beamform_restatement.py's (and tests/spatial_restatement.py's noise class:
all K >= n classes enter Q_i, the first n get a filter).  Per source i and bin, with A = L L^H:
  G = L^-1 N_i L^-H (Hermitian, positive semidefinite; the diagonal taken as real)
  (mu, u) the principal eigenpair of G, v = L^-H u, h = L u = A v (the steering estimate), v^H A v = 1
  "rank1":  w = v conj(h_ref)                                   = A^-1 h / (h^H A^-1 h) conj(h_ref)
  "gev":    w = v (conj(h_ref) / |h_ref|) |h| / sqrt(C)         (phase factor 1 where |h_ref| = 0)
  "souden": the weights of tests/beamform_restatement.py, untouched
  w = e_ref where a Cholesky pivot or mu is not finite and positive; C = 1: w = 1.0 exactly.

The per-bin design is written twice.  form = "eigh": scipy.linalg.eigh(N_i, A), the generalised problem solved directly
(its eigenvectors come normalised to v^H A v = 1).  form = "jacobi": the explicit Cholesky whitening by two forward solves
per column and the cyclic-by-row two-sided complex Jacobi iteration the device runs: `sweeps` sweeps over (p, q), p < q;
a pair with G_pq = 0 exactly is skipped; theta = (G_qq - G_pp) / (2 |G_pq|), t = sign(theta) / (|theta| + sqrt(1 +
theta^2)) (sign(0) = 1; 1 / (2 theta) where |theta| > 1e150), c = 1 / sqrt(1 + t^2), s = t c, e = G_pq / |G_pq|,
J = [[c, s e], [-s conj(e), c]]; G <- G J, V <- V J, G <- J^H G; mu is the largest diagonal entry after the last sweep
(ties: the lowest index).  tests/test_beamform_design_host.py holds the two forms to 1e-11 of the largest weight.

dtype = float64 is the reference.  dtype = float32 is the yardstick of the device's rounding error, with the split of
tests/beamform_restatement.py: transforms and masks in float32, statistics and design in float64.

beamform / beamform_spatial / beamform_track are the three restatements with these weights substituted for theirs."""
import contextlib

import numpy as np
import scipy.linalg

from tests import beamform_restatement as br
from tests import beamform_track_restatement as tr
from tests import spatial_restatement as sp

DESIGNS = {"souden": 0, "rank1": 1, "gev": 2}
SWEEPS = 10
_souden, _souden_spatial = br.weights, sp.weights


def loaded(N, i, eps, reg):
    """N [K, bins, C, C] -> A [bins, C, C] = Q_i + lambda I, Q_i over all classes j != i in increasing j"""
    C = N.shape[-1]
    Q = np.zeros_like(N[0])
    for j in range(N.shape[0]):
        if j != i:
            Q = Q + N[j]
    lam = reg * np.einsum("fcc->f", Q).real / C + eps
    return Q + lam[:, None, None] * np.eye(C)


def cholesky(A):
    """A [bins, C, C] -> L, column after column as tests/beamform_restatement.py's cholesky_solve (NaN where a pivot
    fails)"""
    C = A.shape[-1]
    Lm = np.zeros_like(A)
    with np.errstate(invalid="ignore", divide="ignore"):
        for c in range(C):
            d = A[..., c, c].real - np.sum(np.abs(Lm[..., c, :c]) ** 2, axis=-1)
            l = np.sqrt(d)
            Lm[..., c, c] = l
            for r in range(c + 1, C):
                Lm[..., r, c] = (A[..., r, c] - np.sum(Lm[..., r, :c] * Lm[..., c, :c].conj(), axis=-1)) / l
    return Lm


def forward(Lm, Bm):
    """L Y = Bm, row after row"""
    Y = np.zeros_like(Bm)
    for r in range(Lm.shape[-1]):
        s = Bm[..., r, :] - np.einsum("...k,...kj->...j", Lm[..., r, :r], Y[..., :r, :])
        Y[..., r, :] = s / Lm[..., r, r][..., None]
    return Y


def backward(Lm, Bm):
    """L^H Z = Bm, from the last row up"""
    Z = np.zeros_like(Bm)
    for r in range(Lm.shape[-1] - 1, -1, -1):
        s = Bm[..., r, :] - np.einsum("...k,...kj->...j", Lm[..., r + 1:, r].conj(), Z[..., r + 1:, :])
        Z[..., r, :] = s / Lm[..., r, r][..., None]
    return Z


def whiten(Lm, Ni):
    """G = L^-1 N_i L^-H by two forward solves: Y = L^-1 N_i, G = L^-1 Y^H; the diagonal taken as real"""
    Y = forward(Lm, Ni)
    G = forward(Lm, np.swapaxes(Y, -1, -2).conj())
    idx = np.arange(G.shape[-1])
    G[..., idx, idx] = G[..., idx, idx].real
    return G


def jacobi(G, sweeps=SWEEPS):
    """G [bins, C, C] Hermitian -> (mu [bins], u [bins, C], off: the off-diagonal Frobenius norm left over ||G||)"""
    G = G.copy()
    bins, C, _ = G.shape
    V = np.broadcast_to(np.eye(C, dtype=np.complex128), G.shape).copy()
    norm = np.sqrt((np.abs(G) ** 2).sum(axis=(1, 2)))
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for _ in range(int(sweeps)):
            for p in range(C - 1):
                for q in range(p + 1, C):
                    g = G[:, p, q].copy()
                    rot = ~((g.real == 0.0) & (g.imag == 0.0))
                    m = np.hypot(g.real, g.imag)
                    th = (G[:, q, q].real - G[:, p, p].real) / (2.0 * m)
                    ab = np.abs(th)
                    t = np.where(ab > 1e150, 1.0 / (2.0 * th), np.where(th < 0.0, -1.0, 1.0) / (ab + np.sqrt(1.0 + th * th)))
                    c = 1.0 / np.sqrt(1.0 + t * t)
                    s, e = t * c, g.real / m + 1j * (g.imag / m)             # (two real divisions)
                    c, s, e = np.where(rot, c, 1.0), np.where(rot, s, 0.0), np.where(rot, e, 1.0)
                    for Mx in (G, V):                                   # columns p, q: M J
                        x, y = Mx[:, :, p].copy(), Mx[:, :, q].copy()
                        Mx[:, :, p] = np.where(rot[:, None], c[:, None] * x - (s * e.conj())[:, None] * y, x)
                        Mx[:, :, q] = np.where(rot[:, None], c[:, None] * y + (s * e)[:, None] * x, y)
                    x, y = G[:, p, :].copy(), G[:, q, :].copy()         # rows p, q: J^H G
                    G[:, p, :] = np.where(rot[:, None], c[:, None] * x - (s * e)[:, None] * y, x)
                    G[:, q, :] = np.where(rot[:, None], c[:, None] * y + (s * e.conj())[:, None] * x, y)
        d = np.einsum("fcc->fc", G).real
        m = np.zeros(bins, dtype=np.int64)
        mu = d[:, 0].copy()
        for c in range(1, C):
            up = d[:, c] > mu
            mu, m = np.where(up, d[:, c], mu), np.where(up, c, m)
        off = np.sqrt((np.abs(G * (1.0 - np.eye(C))) ** 2).sum(axis=(1, 2))) / norm
    return mu, V[np.arange(bins), :, m], off


def principal(A, Ni, form="jacobi", sweeps=SWEEPS):
    """A, N_i [bins, C, C] -> (ok [bins], v [bins, C], h [bins, C], mu [bins]): the principal generalised eigenvector
    normalised to v^H A v = 1 and h = A v; ok where the pivots and mu are finite and positive"""
    bins, C, _ = A.shape
    Lm = cholesky(A)
    piv = np.einsum("fcc->fc", Lm).real
    with np.errstate(invalid="ignore"):
        ok = np.all(np.isfinite(piv) & (piv > 0), axis=1)
    v, h, mu = (np.zeros((bins, C), dtype=np.complex128), np.zeros((bins, C), dtype=np.complex128), np.zeros(bins))
    if form == "eigh":
        for f in np.nonzero(ok & np.all(np.isfinite(Ni), axis=(1, 2)))[0]:
            vals, vecs = scipy.linalg.eigh(Ni[f], A[f])
            mu[f], v[f] = vals[-1], vecs[:, -1]
            h[f] = A[f] @ v[f]
        ok = ok & np.all(np.isfinite(Ni), axis=(1, 2))
    else:
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            mu, u, _ = jacobi(whiten(Lm, Ni), sweeps)
            v = backward(Lm, u[..., None])[..., 0]
            h = np.einsum("fck,fk->fc", Lm, u)
    with np.errstate(invalid="ignore"):
        ok = ok & np.isfinite(mu) & (mu > 0)
    return ok, v, h, mu


def design_weights(N, n, ref, eps, reg, kind="rank1", sweeps=SWEEPS, form="jacobi", phase=None):
    """N [K, bins, C, C], K >= n -> w [n, bins, C] complex128.  phase [bins] (optional): u is multiplied with
    exp(i phase) first, which the weights must not see"""
    K, bins, C, _ = N.shape
    if kind in (None, "souden"):
        return _souden(N, ref, eps, reg) if K == n else _souden_spatial(N, n, ref, eps, reg)
    assert kind in DESIGNS
    w = np.zeros((n, bins, C), dtype=np.complex128)
    w[:, :, ref] = 1.0
    if C == 1:
        return w
    for i in range(n):
        ok, v, h, _ = principal(loaded(N, i, eps, reg), N[i], form, sweeps)
        if phase is not None:
            v, h = v * np.exp(1j * phase)[:, None], h * np.exp(1j * phase)[:, None]
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            if kind == "rank1":
                wi = v * h[:, ref].conj()[:, None]
            else:
                ma = np.abs(h[:, ref])
                ph = np.where(ma > 0, h[:, ref].conj() / np.where(ma > 0, ma, 1.0), 1.0)
                wi = v * ph[:, None] * (np.sqrt((np.abs(h) ** 2).sum(axis=1)) / np.sqrt(float(C)))[:, None]
        w[i, ok] = wi[ok]
    return w


def gaps(N, n, eps, reg):
    """the relative eigenvalue gap (mu_1 - mu_2) / mu_1 of every (source, bin) -> [n, bins] (numpy.linalg.eigvalsh on
    the whitened matrix)"""
    out = np.zeros((n, N.shape[1]))
    for i in range(n):
        vals = np.linalg.eigvalsh(whiten(cholesky(loaded(N, i, eps, reg)), N[i]))
        out[i] = (vals[:, -1] - vals[:, -2]) / vals[:, -1]
    return out


@contextlib.contextmanager
def substituted(kind, sweeps=SWEEPS, form="jacobi", record=None):
    """the three restatements compute these weights in place of Souden's; `record` (a list) receives the smallest
    relative eigenvalue gap of every set of statistics they are asked for"""
    def weights(N, n, ref, eps, reg):
        if record is not None:
            with np.errstate(invalid="ignore", divide="ignore"):
                record.append(float(gaps(N, n, eps, reg).min()))
        return design_weights(N, n, ref, eps, reg, kind, sweeps, form)

    br.weights = lambda N, ref, eps, reg, solver="cholesky": weights(N, N.shape[0], ref, eps, reg)
    sp.weights = lambda N, n, ref, eps, reg, solver="cholesky": weights(N, n, ref, eps, reg)
    try:
        yield
    finally:
        br.weights, sp.weights = _souden, _souden_spatial


def beamform(mix, est, design="rank1", sweeps=SWEEPS, form="jacobi", record=None, **kw):
    """tests/beamform_restatement.py's beamform with the design's weights"""
    with substituted(design, sweeps, form, record):
        return br.beamform(mix, est, **kw)


def beamform_spatial(mix, est, design="rank1", sweeps=SWEEPS, form="jacobi", record=None, **kw):
    """tests/spatial_restatement.py's beamform_spatial with the design's weights on the refined statistics"""
    with substituted(design, sweeps, form, record):
        return sp.beamform_spatial(mix, est, **kw)


def beamform_track(mix, est, design="rank1", sweeps=SWEEPS, form="jacobi", record=None, **kw):
    """tests/beamform_track_restatement.py's beamform_track with the design's weights in every block"""
    with substituted(design, sweeps, form, record):
        return tr.beamform_track(mix, est, **kw)


def item_statistics(mix, est, n_fft=512, hop=128, power=2, eps=1e-10, dtype=np.float64):
    """mix [C, L], est [n, L] -> N [n, bins, C, C] complex128, the statistics tests/beamform_restatement.py forms"""
    import torch

    from tests import stems_restatement as sr

    mix, est = np.atleast_2d(np.asarray(mix, dtype=dtype)), np.asarray(est, dtype=dtype)
    C, n = mix.shape[0], est.shape[0]
    Z, _, _ = sr._stft(np.concatenate([mix, est]), n_fft, hop, dtype)
    M = sr._masks(Z[C:], n, power, eps, torch.float64 if dtype == np.float64 else torch.float32)
    return br.statistics(Z[:C].numpy().astype(np.complex128), M.numpy().astype(np.float64))


def pack(N, C):
    """N [K, bins, Cb, Cb] complex128 -> [K, C (C + 1), bins] float64, the layout dsn_beamform_solve reads for an item
    of Cb <= C channels: the upper triangle of C x C row after row, per entry the real then the imaginary plane;
    entries of channels >= Cb are NaN (they must not be read)"""
    K, bins, Cb, _ = N.shape
    out = np.full((K, C * (C + 1), bins), np.nan)
    u = 0
    for c1 in range(C):
        for c2 in range(c1, C):
            if c2 < Cb:
                out[:, 2 * u], out[:, 2 * u + 1] = N[:, :, c1, c2].real, N[:, :, c1, c2].imag
            u += 1
    return out
