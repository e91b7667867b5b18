"""Restatement of dsn_stems and dsn_pcm_encode_frames (include/ditsep_hip.h).

Per item: mixture x [C, L], mono estimates s [n, L], parameters mode, n_fft, hop, power, eps, reg.  Padding, analysis,
window, masks M_i and synthesis are those of tests/mask_refine_restatement.py (`refine_torch`: torch.stft / torch.istft,
center = True, pad_mode = "reflect", the periodic Hann window rounded once to float32).
  mask     Y_i,c = M_i X_c
  wiener   v_i = M_i^2 (1/C) sum_c |X_c|^2;  N_i(f) = sum_t M_i^2 X X^H,  d_i(f) = sum_t v_i;  R_i = N_i / d_i (the
           identity where d_i = 0);  Sigma = sum_j v_j R_j;  lambda = reg tr(Sigma) / C + eps;
           z = (Sigma + lambda I)^-1 X;  Y_i = v_i R_i z + (lambda / n) z
The per-bin filter is written twice: numpy.linalg.solve (`solver="solve"`) and the closed form the device uses, a
division for C = 1 and the 2 x 2 adjugate for C = 2 (`solver="adjugate"`).

dtype = float64 is the reference.  dtype = float32 is the yardstick of the device's rounding error: transforms and masks
in float32 (pocketfft's), statistics and solve in float64 on the widened values, Y rounded once to float32 -- the
device's own split of precisions.  eps and reg are the float32 values the device call takes, widened.

`encode_frames` restates the interleaved encoder on top of tests/pcm_restatement.quantise."""
import numpy as np
import torch

from tests import mask_refine_restatement as mr
from tests import pcm_restatement as pr

DEFAULTS = dict(mode="wiener", n_fft=512, hop=128, power=2, eps=1e-10, reg=1e-3)


def _stft(x, n_fft, hop, dtype):
    """x [rows, L] -> (Z [rows, bins, F] torch complex, the window, Lp)"""
    L = x.shape[-1]
    Lp = mr.padded_length(L, hop)
    tdt = torch.float64 if dtype == np.float64 else torch.float32
    xp = torch.zeros((x.shape[0], Lp), dtype=tdt)
    xp[:, :L] = torch.from_numpy(np.asarray(x, dtype=dtype))
    w = torch.from_numpy(mr.window(n_fft, dtype))
    Z = torch.stft(xp, n_fft, hop_length=hop, win_length=n_fft, window=w, center=True, pad_mode="reflect",
                   return_complex=True)
    assert Z.shape[-1] == 1 + Lp // hop
    return Z, w, Lp


def _masks(S, n, power, eps, tdt):
    a = S.abs() if power == 1 else S.real ** 2 + S.imag ** 2
    e = torch.tensor(eps, dtype=tdt)
    return (a + e) / (a.sum(dim=0) + torch.tensor(float(n), dtype=tdt) * e)


def statistics(X, M):
    """X [C, bins, F] complex128, M [n, bins, F] float64 -> (v [n, bins, F], R [n, bins, C, C], d [n, bins])"""
    C = X.shape[0]
    p = (X.real ** 2 + X.imag ** 2).sum(axis=0) / C
    m2 = M * M
    v = m2 * p
    N = np.einsum("ift,cft,dft->ifcd", m2, X, X.conj())
    d = v.sum(axis=-1)
    R = np.broadcast_to(np.eye(C, dtype=np.complex128), N.shape).copy()
    nz = d != 0
    R[nz] = N[nz] / d[nz][:, None, None]
    return v, R, d


def wiener_filter(X, v, R, eps, reg, solver="adjugate"):
    """X [C, bins, F], v [n, bins, F], R [n, bins, C, C] -> Y [n, C, bins, F] complex128"""
    C, n = X.shape[0], v.shape[0]
    Sig = np.einsum("jft,jfcd->ftcd", v, R)                                           # [bins, F, C, C]
    lam = reg * np.einsum("ftcc->ft", Sig).real / C + eps
    Xt = np.moveaxis(X, 0, -1)                                                        # [bins, F, C]
    if solver == "solve":
        A = Sig + lam[..., None, None] * np.eye(C)
        z = np.linalg.solve(A, Xt[..., None])[..., 0]
    elif C == 1:
        z = Xt / (Sig[..., 0, 0].real + lam)[..., None]
    else:
        assert C == 2, "the closed form is the 2 x 2 adjugate"
        a00, a11, s01 = Sig[..., 0, 0].real + lam, Sig[..., 1, 1].real + lam, Sig[..., 0, 1]
        det = a00 * a11 - (s01.real ** 2 + s01.imag ** 2)
        z = np.stack([(a11 * Xt[..., 0] - s01 * Xt[..., 1]) / det,
                      (a00 * Xt[..., 1] - s01.conj() * Xt[..., 0]) / det], axis=-1)
    Y = v[..., None] * np.einsum("ifcd,ftd->iftc", R, z) + (lam / n)[None, ..., None] * z[None]
    return np.moveaxis(Y, -1, 1)                                                      # [n, C, bins, F]


def stems(mix, est, mode="wiener", n_fft=512, hop=128, power=2, eps=1e-10, reg=1e-3, dtype=np.float64,
          solver="adjugate", return_info=False):
    """mix [C, L], est [n, L] -> out [n, C, L] in `dtype` (and {"R": [n, bins, C, C], "den": [n, bins]})"""
    mix, est = np.atleast_2d(np.asarray(mix, dtype=dtype)), np.asarray(est, dtype=dtype)
    (C, L), n = mix.shape, est.shape[0]
    tdt = torch.float64 if dtype == np.float64 else torch.float32
    Z, w, Lp = _stft(np.concatenate([mix, est]), n_fft, hop, dtype)
    X, M = Z[:C], _masks(Z[C:], n, power, eps, tdt)
    info = None
    if mode == "mask":
        Y = M[:, None] * X[None]
    else:
        assert mode == "wiener"
        e32, r32 = float(np.float32(eps)), float(np.float32(reg))
        X64, M64 = X.numpy().astype(np.complex128), M.numpy().astype(np.float64)
        v, R, d = statistics(X64, M64)
        Y = torch.from_numpy(wiener_filter(X64, v, R, e32, r32, solver)).to(Z.dtype)  # rounded once
        info = {"R": R, "den": d}
    y = torch.istft(Y.reshape(n * C, *Y.shape[2:]), n_fft, hop_length=hop, win_length=n_fft, window=w, center=True,
                    length=Lp)
    out = y[:, :L].numpy().reshape(n, C, L)
    return (out, info) if return_info else out


def make_case(seed, kind, n, C, L, noise=0.3):
    """seeded Gaussian sources, panned into C channels, with noisy mono estimates -> (mix [C, L], est [n, L]) float32.
    kind: "generic" (random pans), "dual" (identical channels), "hard" (every source in one channel only), "silent_ch"
    (the last channel is zero), "silent_est" (the estimates are zero)"""
    g = np.random.default_rng(seed)
    src = g.standard_normal((n, L)) * 0.1
    if kind == "dual":
        pan = np.ones((n, C))
    elif kind == "hard":
        pan = np.zeros((n, C))
        pan[np.arange(n), np.arange(n) % C] = 1.0
    else:
        pan = 0.2 + 0.8 * g.random((n, C))
        if kind == "silent_ch" and C > 1:
            pan[:, -1] = 0.0
    mix = np.einsum("ic,il->cl", pan, src)
    est = pan.mean(axis=1)[:, None] * src + noise * 0.1 * g.standard_normal((n, L))
    if kind == "silent_est":
        est = np.zeros_like(est)
    return mix.astype(np.float32), est.astype(np.float32)


def rel_err(a, b, mix):
    return float(np.max(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))) / np.max(np.abs(mix)))


def encode_frames(x, frames, channels, encoding):
    """x [C, Lmax] float32 -> (the payload of `frames` frames of the first `channels` channels, interleaved sample by
    sample; the clipped count over those channels)"""
    x = np.asarray(x, dtype=np.float32)
    inter = np.ascontiguousarray(x[:channels, :frames].T).reshape(-1)
    return pr.quantise(inter, encoding)
