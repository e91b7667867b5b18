"""Float64 restatement of the window stitch (dsn_window_stitch, ditsep_amd/csrc/stitch.hip; Engine.window_stitch):
the window plan, the fade tables, the overlap Gram, the permutation rule with its tie order, the cumulative table and
the cross-fade, in plain numpy / Python.  Shared by tests/test_stitch_host.py (the restatement against itself and
against ditsep_amd.native's host helpers) and the GPU tests (the device against it).

Conventions.  chunks [W, n, Lw] float32; window w covers samples [w hop, w hop + Lw), hop = Lw - O.  Slot i of the
output is slot P_w(i) of window w: P_0 = id, P_{w+1}(i) = sigma_w(P_w(i)), where sigma_w maximises
sum_i G[w][i][sigma(i)] and G[w][i][j] = sum_k chunks[w][i][hop + k] chunks[w + 1][j][k]."""
import math
from itertools import permutations

import numpy as np


def plan(L, window, overlap):
    """(W, hop): the fewest windows of hop = window - overlap that cover [0, L)"""
    hop = window - overlap
    W = 1
    while (W - 1) * hop + window < L:
        W += 1
    return W, hop


def fade(overlap, kind="hann"):
    """(fall32, rise32, rise64): rise in float64, both weights rounded once to float32"""
    O = overlap
    if kind == "linear":
        rise = np.array([(k + 0.5) / float(O) for k in range(O)], dtype=np.float64)
    else:
        sn = [math.sin(math.pi * (k + 0.5) / (2.0 * float(O))) for k in range(O)]
        rise = np.array([s * s for s in sn], dtype=np.float64)
    return (1.0 - rise).astype(np.float32), rise.astype(np.float32), rise


def cut(x, window, overlap):
    """x [n, L] -> chunks [W, n, window] float32, the last window zero-extended"""
    x = np.asarray(x, dtype=np.float32)
    n, L = x.shape
    W, hop = plan(L, window, overlap)
    pad = np.zeros((n, (W - 1) * hop + window), dtype=np.float32)
    pad[:, :L] = x
    return np.stack([pad[:, w * hop:w * hop + window] for w in range(W)])


def gram(chunks, overlap):
    """(G, A) [W-1, n, n] float64: G the overlap inner products -- float32 x float32 products are exact in float64
    and math.fsum adds them without rounding until the end -- and A = sum_k |a_k b_k|, the scale of a summation-order
    difference"""
    c = np.asarray(chunks, dtype=np.float64)
    W, n, Lw = c.shape
    hop = Lw - overlap
    G = np.zeros((max(W - 1, 0), n, n))
    A = np.zeros_like(G)
    for w in range(W - 1):
        for i in range(n):
            a = c[w, i, hop:hop + overlap]
            for j in range(n):
                p = a * c[w + 1, j, :overlap]
                G[w, i, j] = math.fsum(p.tolist())
                A[w, i, j] = math.fsum(np.abs(p).tolist())
    return G, A


def scores(G):
    """[(sigma, score)] of one boundary's n x n table in the rule's order: lexicographic in (sigma(0) .. sigma(n-1)),
    the score summed over i = 0 .. n-1 in that order, in float64, as the device does"""
    n = G.shape[0]
    out = []
    for sg in permutations(range(n)):           # itertools.permutations of a sorted input is lexicographic
        s = 0.0
        for i in range(n):
            s += float(G[i, sg[i]])
        out.append((sg, s))
    return out


def best_perm(G):
    """the first candidate no later one exceeds strictly (ties go to the identity, the first candidate)"""
    best, best_s = None, None
    for sg, s in scores(G):
        if best is None or s > best_s:
            best, best_s = sg, s
    return best


def margins(Gs):
    """per boundary (best score, runner-up score); (best, None) with a single candidate (n = 1)"""
    out = []
    for G in Gs:
        s = sorted((v for _, v in scores(G)), reverse=True)
        out.append((s[0], s[1] if len(s) > 1 else None))
    return out


def perms_from_gram(Gs, W, n):
    """the cumulative table [W, n] the rule gives from the tables Gs [W-1, n, n] (the GPU tests feed it the device's
    own gram: the device's decisions must then be reproduced exactly, whatever the margins)"""
    P = np.zeros((W, n), dtype=np.int64)
    P[0] = np.arange(n)
    for w in range(W - 1):
        sg = best_perm(np.asarray(Gs[w]))
        P[w + 1] = [sg[P[w, i]] for i in range(n)]
    return P


def crossfade(chunks, P, L, overlap, fall32, rise32):
    """(out, bound, copied): out [n, L] float64 -- fall a + rise b in float64 from the float32 tables inside an
    overlap, the chunk's own sample elsewhere (copied True) -- and bound = 2^-22 (|fall a| + |rise b|), what a float32
    evaluation may differ by (see tests/test_gpu_stitch.py)"""
    c = np.asarray(chunks, dtype=np.float64)
    W, n, Lw = c.shape
    hop = Lw - overlap
    f, r = np.asarray(fall32, dtype=np.float64), np.asarray(rise32, dtype=np.float64)
    t = np.arange(L)
    w = np.minimum(t // hop, W - 1)
    k = t - w * hop
    inside = (w >= 1) & (k < overlap)
    out = np.zeros((n, L))
    bound = np.zeros((n, L))
    for i in range(n):
        b = c[w, P[w, i], k]
        out[i] = b
        ti = t[inside]
        wi, ki = w[inside], k[inside]
        a = c[wi - 1, P[wi - 1, i], hop + ki]
        fa, rb = f[ki] * a, r[ki] * b[inside]
        out[i, ti] = fa + rb
        bound[i, ti] = 2.0 ** -22 * (np.abs(fa) + np.abs(rb))
    return out, bound, ~inside


def stitch(chunks, L, overlap, kind="hann", align=True):
    """-> (out, bound, copied, P, G, A)"""
    W, n, _ = np.asarray(chunks).shape
    G, A = gram(chunks, overlap)
    P = perms_from_gram(G if align else np.zeros_like(G), W, n)
    f, r, _ = fade(overlap, kind)
    return (*crossfade(chunks, P, L, overlap, f, r), P, G, A)


def decisive_case(seed, n, L, window, overlap, permute=True, noise=0.1):
    """Independent white Gaussian sources [n, L] cut into windows, 0.1 x independent noise added per window, the slots
    of every window shuffled (window w's slot s holds source q[w][s]).  -> (chunks float32 [W, n, window], sources,
    q [W, n], expected table P [W, n]): in window 0's order, P_w(i) = the slot of window w that holds source q[0][i].
    The diagonal of an overlap table is about O sigma^2, the off-diagonals about sqrt(O) sigma^2."""
    rng = np.random.default_rng(seed)
    src = rng.standard_normal((n, L)).astype(np.float32)
    chunks = cut(src, window, overlap)
    W = chunks.shape[0]
    chunks = (chunks + noise * rng.standard_normal(chunks.shape)).astype(np.float32)
    q = np.stack([rng.permutation(n) if permute else np.arange(n) for _ in range(W)])
    shuffled = np.stack([chunks[w][q[w]] for w in range(W)])
    P = np.stack([[int(np.nonzero(q[w] == q[0][i])[0][0]) for i in range(n)] for w in range(W)])
    return shuffled, src, q, P
