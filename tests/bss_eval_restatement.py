"""Float64 restatement of dsn_bss_eval (include/ditsep_hip.h): bss_eval SDR / SIR / SAR with F-tap distortion filters
(Vincent et al. 2006), written twice.

(a) `normal`: the contract's own route -- lag tables of the unit-norm references, the block-Toeplitz Gram matrix,
    scipy.linalg.cho_factor, the quadratic forms pt_ij = d_ij^T G_ii^-1 d_ij and pall_j = d_j^T G^-1 d_j.
(b) `lstsq`: the least-squares problem those are the normal equations of -- the explicit [L + F - 1, M] matrix of the
    F shifts of every zero-extended reference, numpy.linalg.lstsq, and the energies of the projections themselves.

Both return {"sdr_pairs", "sir_pairs": [n, n] ([i, j]: est j against ref i), "sar_j": [n]}; (a) also "cond", the
2-norm condition number of the Gram matrix.  `choose` solves the permutation as the device does."""
import itertools

import numpy as np
import scipy.linalg as sl

TINY = 1e-300


def db(num, den, clamp_db=0.0):
    with np.errstate(divide="ignore"):
        v = 10.0 * np.log10(np.maximum(num, TINY) / np.maximum(den, TINY))
    return np.clip(v, -clamp_db, clamp_db) if clamp_db > 0 else v


def scales(ref):
    e = np.einsum("it,it->i", ref, ref)
    return np.where(e > 0, 1.0 / np.sqrt(np.where(e > 0, e, 1.0)), 0.0)


def corr(x, y, F):
    """c[k] = sum_t x[t] y[t + k] for 0 <= k < F, both zero-extended"""
    L = len(x)
    return np.array([x[:L - k] @ y[k:] if k < L else 0.0 for k in range(F)])


def gram(ref, F, load_diag=0.0):
    n = len(ref)
    s = scales(ref)
    G = np.zeros((n * F, n * F))
    for i in range(n):
        for j in range(n):
            pos, neg = corr(ref[i], ref[j], F), corr(ref[j], ref[i], F)       # c_ij[k], c_ij[-k]
            G[i * F:(i + 1) * F, j * F:(j + 1) * F] = s[i] * s[j] * sl.toeplitz(pos, neg)   # [p, q] = c_ij[p - q]
    return G + load_diag * np.eye(n * F)


def rhs(ref, est, F):
    n = len(ref)
    s = scales(ref)
    return np.concatenate([np.stack([s[i] * corr(ref[i], est[j], F) for j in range(n)], axis=1) for i in range(n)])


def ratios(ee, pt, pall, clamp_db=0.0):
    return {"sdr_pairs": db(pt, ee[None] - pt, clamp_db), "sir_pairs": db(pt, pall[None] - pt, clamp_db),
            "sar_j": db(pall, ee - pall, clamp_db)}


def normal(ref, est, F, load_diag=0.0, clamp_db=0.0):
    """ref, est [n, L] float64"""
    n = len(ref)
    G, D = gram(ref, F, load_diag), rhs(ref, est, F)
    ee = np.einsum("jt,jt->j", est, est)
    pall = np.einsum("kj,kj->j", D, sl.cho_solve(sl.cho_factor(G, lower=True), D))
    pt = np.zeros((n, n))
    for i in range(n):
        blk = slice(i * F, (i + 1) * F)
        pt[i] = np.einsum("kj,kj->j", D[blk], sl.cho_solve(sl.cho_factor(G[blk, blk], lower=True), D[blk]))
    out = ratios(ee, pt, pall, clamp_db)
    out["cond"] = float(np.linalg.cond(G))
    return out


def lstsq(ref, est, F, clamp_db=0.0):
    """ref, est [n, L] float64; no load_diag (it has no least-squares form here)"""
    n, L = ref.shape

    def shifts(x):
        A = np.zeros((L + F - 1, F))
        for p in range(F):
            A[p:p + L, p] = x
        return A

    As = [shifts(r) for r in ref]
    A = np.concatenate(As, axis=1)
    E = np.zeros((L + F - 1, n))
    E[:L] = est.T
    Pall = A @ np.linalg.lstsq(A, E, rcond=None)[0]
    sdr, sir = np.zeros((n, n)), np.zeros((n, n))
    for i in range(n):
        Pt = As[i] @ np.linalg.lstsq(As[i], E, rcond=None)[0]
        num = (Pt ** 2).sum(0)
        sdr[i] = db(num, ((E - Pt) ** 2).sum(0), clamp_db)
        sir[i] = db(num, ((Pall - Pt) ** 2).sum(0), clamp_db)
    return {"sdr_pairs": sdr, "sir_pairs": sir, "sar_j": db((Pall ** 2).sum(0), ((E - Pall) ** 2).sum(0), clamp_db)}


def choose(tables, perm_by="sir", perm=None):
    """-> (sdr, sir, sar [n], perm [n]): all n! candidates in lexicographic order, a later one wins only when its key
    (the sum over i of key[i, perm[i]], added in that order) is strictly greater"""
    n = len(tables["sar_j"])
    key = tables["sir_pairs"] if perm_by == "sir" else tables["sdr_pairs"]
    if perm is None:
        best = None
        for p in itertools.permutations(range(n)):
            s = 0.0
            for i in range(n):
                s += key[i, p[i]]
            if best is None or s > best[0]:
                best = (s, p)
        perm = best[1]
    perm = [int(v) for v in perm]
    idx = np.arange(n)
    return tables["sdr_pairs"][idx, perm], tables["sir_pairs"][idx, perm], tables["sar_j"][perm], np.array(perm)


def mixtures(B, n, L, seed=0, noise=0.05):
    """[B, n, L] float32 pair (ref, est): synthetic_sources and a diagonally dominant n x n mixing of them plus white
    noise (the off-diagonal leak grows with the column, so the estimates differ), rounded to fp32"""
    import torch

    from ditsep_amd.synthetic import synthetic_sources

    ref = synthetic_sources(B, n, L, seed=1234 + 17 * seed).double().numpy()
    rng = np.random.default_rng(seed)
    mix = np.eye(n) + (0.1 + 0.05 * np.arange(n))[None, :] * (1 - np.eye(n))
    est = np.einsum("ij,bjt->bit", mix, ref) + noise * 0.1 * rng.standard_normal(ref.shape)
    return torch.from_numpy(ref.astype(np.float32)), torch.from_numpy(est.astype(np.float32))


def bound(v, cond, L, F):
    """the allowed |device - restatement| of a dB value v: the fp64 summation and solve error cond (L + F) 2^-52 of
    an energy, amplified by the cancellation in ee - pt (a relative error e of pt moves 10 log10(pt / (ee - pt)) by
    (10 / ln 10) (1 + pt / (ee - pt)) e)"""
    with np.errstate(over="ignore"):
        return (10.0 / np.log(10.0)) * (1.0 + 10.0 ** (np.abs(v) / 10.0)) * cond * (L + F) * 2.0 ** -52
