"""The ensemble combine (dsn_ensemble_combine, ditsep_amd/csrc/ensemble.hip; include/ditsep_hip.h states the
definition) restated in numpy: the Gram exactly rounded (math.fsum over the exact float64 products), the alignment
written twice -- an exhaustive search over the Gram and scipy.optimize.linear_sum_assignment --, the info figures in
float64 and the combine in float32 with the device's expressions.  Besides the values every case carries

  bound    [R, R]: L 2^-53 sum_t |x_p[t]| |x_q[t]|, what a float64 sum of L exact products in any order may be off by
  margins  the distance between the best and the second-best value of every discrete choice (each permutation, the
           anchor, `best`), and the error `bound` allows the compared values, so that a test can require the choice to
           be out of rounding's reach
  resid_db / agree_db intervals: the figures recomputed at the ends of G +- bound
"""
import itertools
import math

import numpy as np

U = 2.0 ** -53
MODES = ("mean", "median", "best", "medoid")


def gram(rows, exact=True):
    """rows [R, L] float32 -> (G [R, R] float64, bound [R, R]).  exact: every entry is math.fsum of the exact products
    (rounded once); otherwise a float64 dot."""
    x = np.asarray(rows, dtype=np.float32).astype(np.float64)
    R, L = x.shape
    G = np.zeros((R, R))
    if exact:
        for p in range(R):
            for q in range(p, R):
                G[p, q] = G[q, p] = math.fsum(x[p] * x[q])
    else:
        G = x @ x.T
    return G, L * U * (np.abs(x) @ np.abs(x).T)


def block(G, n, a, k):
    return G[a * n:(a + 1) * n, k * n:(k + 1) * n]


def assign_exhaustive(C):
    """C [n, n] -> (the lexicographically first permutation maximising sum_i C[i, pi(i)], its score, the margin to the
    best score of any other permutation -- inf for n = 1)"""
    n = C.shape[0]
    best, score, second = None, None, -math.inf
    for pi in itertools.permutations(range(n)):
        s = 0.0
        for i in range(n):
            s += C[i, pi[i]]
        if best is None:
            best, score = pi, s
        elif s > score:
            best, score, second = pi, s, score
        else:
            second = max(second, s)
    return list(best), score, score - second


def assign_lsa(C):
    from scipy.optimize import linear_sum_assignment

    r, c = linear_sum_assignment(C, maximize=True)
    assert list(r) == list(range(C.shape[0]))
    return [int(v) for v in c]


def align(G, K, n, assign="exhaustive"):
    """-> (perm [K, n], anchor, S [K, K]).  assign: "exhaustive" or "lsa" (the scores are then summed the same way)"""
    S = np.zeros((K, K))
    P = [[None] * K for _ in range(K)]
    for a in range(K):
        for k in range(K):
            C = block(G, n, a, k)
            pi = assign_exhaustive(C)[0] if assign == "exhaustive" else assign_lsa(C)
            s = 0.0
            for i in range(n):
                s += C[i, pi[i]]
            P[a][k], S[a, k] = pi, s
    totals = []
    for a in range(K):
        s = 0.0
        for k in range(K):
            if k != a:
                s += S[min(a, k), max(a, k)]           # S is symmetric: the one formed for a < k serves both
        totals.append(s)
    anchor = int(np.argmax(totals)) if K > 1 else 0        # argmax: the first of equal values
    perm = [list(range(n)) if k == anchor else P[anchor][k] for k in range(K)]
    return np.array(perm, dtype=np.int64), anchor, S, totals


def _db(x):
    if math.isnan(x):
        return math.nan
    return math.inf if x == math.inf else (-math.inf if x <= 0 else 10.0 * math.log10(x))


def residuals(G, bound, K, n):
    """-> (E [K], its error bound [K]): E_k = (G_mm - 2 sum_i G_m,(k,i)) + sum_ij G_(k,i),(k,j)"""
    m = K * n
    E, err = np.zeros(K), np.zeros(K)
    for k in range(K):
        cross = self = 0.0
        for i in range(n):
            cross += G[m, k * n + i]
        for i in range(n):
            for j in range(n):
                self += G[k * n + i, k * n + j]
        E[k] = (G[m, m] - 2.0 * cross) + self
        sl = slice(k * n, (k + 1) * n)
        mag = abs(G[m, m]) + 2.0 * np.abs(G[m, sl]).sum() + np.abs(G[sl, sl]).sum()
        err[k] = bound[m, m] + 2.0 * bound[m, sl].sum() + bound[sl, sl].sum() + (n * n + n + 4) * U * mag
    return E, err


def agreement(gaa, gcc, g, baa=0.0, bcc=0.0, bg=0.0):
    """SI-SDR in dB of a row against the anchor's from the three Gram entries -> (value, low, high) with the entries
    anywhere within their bounds"""
    if gaa == 0.0 or gcc == 0.0:
        return math.nan, math.nan, math.nan
    g2 = g * g
    den = gaa * gcc - g2
    val = _db(g2 / den) if den > 0 else math.inf
    g_lo, g_hi = max(abs(g) - bg, 0.0), abs(g) + bg
    p_lo, p_hi = max(gaa - baa, 0.0) * max(gcc - bcc, 0.0), (gaa + baa) * (gcc + bcc)
    r = 4.0 * U * (p_hi + g_hi * g_hi)
    den_lo, den_hi = p_lo - g_hi * g_hi - r, p_hi - g_lo * g_lo + r
    hi = _db(g_hi * g_hi / den_lo) if den_lo > 0 else math.inf
    lo = _db(g_lo * g_lo / den_hi) if den_hi > 0 else math.inf
    return val, lo, hi


def combine_rows(c, mode, pick=None):
    """c [K, n, L] float32 aligned rows -> [n, L] float32, the device's expressions"""
    K = c.shape[0]
    if mode == "mean":
        # candidate order, every addition's rounding error (Knuth's two-sum, exact) collected and given back at the end
        acc, err = c[0].copy(), np.zeros_like(c[0])
        for k in range(1, K):
            t = acc + c[k]
            xv = t - acc
            av = t - xv
            err = err + ((acc - av) + (c[k] - xv))
            acc = t
        # (nothing rounded off: the sum itself, so that -0 + -0 stays -0)
        return np.where(err != 0, acc + err, acc) / np.float32(K) if K > 1 else acc
    if mode == "median":
        s = np.sort(c, axis=0, kind="stable")
        if K % 2:
            return s[K // 2].copy()
        return (s[(K - 1) // 2] + s[K // 2]) * np.float32(0.5)
    return c[pick].copy()


def restate_item(cands, mix=None, exact=True):
    """cands [K, n, L] float32, mix [L] float32 or None -> dict: gram, bound, perm, perm_lsa, anchor, best, E, E_err,
    resid_db (+ _lo, _hi), agree_db (+ _lo, _hi), out {mode: [n, L]}, margins"""
    cands = np.ascontiguousarray(cands, dtype=np.float32)
    K, n, L = cands.shape
    rows = cands.reshape(K * n, L)
    if mix is not None:
        rows = np.concatenate([rows, np.asarray(mix, dtype=np.float32).reshape(1, L)])
    G, bound = gram(rows, exact)
    perm, anchor, S, totals = align(G, K, n)
    perm_lsa, anchor_lsa, _, _ = align(G, K, n, "lsa")
    res = {"gram": G, "bound": bound, "perm": perm, "perm_lsa": perm_lsa, "anchor": anchor, "anchor_lsa": anchor_lsa,
           "best": -1}
    # the margins of the discrete choices and the error the bound allows the compared values
    blk_err = lambda a, k: float(block(bound, n, a, k).sum()) + n * U * float(np.abs(block(G, n, a, k)).sum())
    margins = {"perm": [], "perm_err": [], "anchor": math.inf, "anchor_err": 0.0, "best": math.inf, "best_err": 0.0}
    for k in range(K):
        margins["perm"].append(math.inf if k == anchor else assign_exhaustive(block(G, n, anchor, k))[2])
        margins["perm_err"].append(2.0 * blk_err(anchor, k))       # two scores, each off by at most the block's bound
    if K > 2:                                                      # (K = 2: the two totals are one number)
        order = np.argsort(-np.array(totals), kind="stable")
        tot_err = [sum(blk_err(a, k) for k in range(K) if k != a) + K * U * abs(totals[a]) for a in range(K)]
        margins["anchor"] = totals[order[0]] - totals[order[1]]
        margins["anchor_err"] = 2.0 * max(tot_err)
    if mix is not None:
        E, E_err = residuals(G, bound, K, n)
        m = K * n
        res["best"] = int(np.argmin(E))
        res["E"], res["E_err"] = E, E_err
        if K > 1:
            s = np.sort(E)
            margins["best"], margins["best_err"] = s[1] - s[0], 2.0 * float(E_err.max())
        gm, bm = G[m, m], bound[m, m]
        res["resid_db"] = np.array([_db(max(e, 0.0) / gm) if gm > 0 else math.nan for e in E])
        res["resid_db_lo"] = np.array([_db(max(e - d, 0.0) / (gm + bm)) if gm > 0 else math.nan
                                       for e, d in zip(E, E_err)])
        res["resid_db_hi"] = np.array([_db(max(e + d, 0.0) / (gm - bm)) if gm - bm > 0 else math.nan
                                       for e, d in zip(E, E_err)])
    else:
        res["resid_db"] = res["resid_db_lo"] = res["resid_db_hi"] = np.full(K, math.nan)
    ag = np.zeros((3, K, n))
    for k in range(K):
        for i in range(n):
            a, c = anchor * n + i, k * n + perm[k][i]
            v = agreement(G[a, a], G[c, c], G[a, c], bound[a, a], bound[c, c], bound[a, c])
            if k == anchor and not math.isnan(v[0]):
                v = (math.inf, math.inf, math.inf)
            ag[:, k, i] = v
    res["agree_db"], res["agree_db_lo"], res["agree_db_hi"] = ag
    res["margins"] = margins
    aligned = np.stack([cands[k][perm[k]] for k in range(K)])
    res["out"] = {mode: combine_rows(aligned, mode, res["best"] if mode == "best" else anchor)
                  for mode in MODES if not (mode == "best" and mix is None)}
    return res


def margins_clear(res, factor=2.0):
    """every discrete choice of the case is further from its runner-up than `factor` x what the Gram bound allows"""
    m = res["margins"]
    ok = all(d > factor * e for d, e in zip(m["perm"], m["perm_err"]))
    return ok and m["anchor"] > factor * m["anchor_err"] and m["best"] > factor * m["best_err"]


def make_case(seed, K, n, L, levels=None):
    """Known sources under known permutations: -> (cands [K, n, L], mix [L], perms [K, n], levels [K]).  Candidate k's
    slot j holds source perms[k][j] plus independent noise `levels[k]` dB below it (default -10 dB for every k); the
    mixture is the sum of the sources.  For L < 257 the sources are axis vectors of distinct amplitudes (n <= L)."""
    g = np.random.default_rng(seed)
    if L >= 257:
        src = g.standard_normal((n, L))
    else:
        assert n <= L
        src = np.zeros((n, L))
        for i in range(n):
            src[i, i] = 1.0 + 0.25 * i
    src = (0.3 * src).astype(np.float32)
    levels = [-10.0] * K if levels is None else list(levels)
    perms = np.stack([g.permutation(n) for _ in range(K)])
    cands = np.zeros((K, n, L), dtype=np.float32)
    for k in range(K):
        for j in range(n):
            s = src[perms[k][j]]
            rms = math.sqrt(float((s.astype(np.float64) ** 2).mean()))
            noise = g.standard_normal(L) * rms * 10.0 ** (levels[k] / 20.0)
            cands[k, j] = (s + noise).astype(np.float32)
    return cands, src.sum(axis=0, dtype=np.float32), perms, levels
