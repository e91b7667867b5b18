"""Host side of the window stitch, no GPU: native.window_plan and native.fade_table, and the float64 restatement
(tests/stitch_restatement.py) against itself -- the GPU tests then hold the device against that restatement."""
import os
import re

import numpy as np
import pytest

from ditsep_amd import native
from tests import stitch_restatement as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PLAN_SWEEP = [(L, window, overlap)
              for window, overlaps in ((1, (0,)), (2, (0, 1)), (7, (0, 1, 3)), (64, (0, 16, 32)), (1537, (0, 517, 768)))
              for overlap in overlaps
              for L in sorted({1, window - 1, window, window + 1, 2 * window - overlap, 2 * window - overlap + 1,
                               3 * window + 5, 10 * window + 3} - {0, -1})]


@pytest.mark.parametrize("L,window,overlap", PLAN_SWEEP)
def test_window_plan(L, window, overlap):
    W, hop = native.window_plan(L, window, overlap)
    assert hop == window - overlap and (W, hop) == sr.plan(L, window, overlap)
    assert W == (1 if L <= window else 1 + -((window - L) // hop))               # 1 + ceil((L - window) / hop)
    # the windows cover [0, L), each sample by one or two of them, and no window starts at or past L
    cover = np.zeros(L, dtype=int)
    for w in range(W):
        cover[w * hop:w * hop + window] += 1
    assert cover.min() >= 1 and cover.max() <= 2
    assert (W - 1) * hop < L <= (W - 1) * hop + window
    # the last overlap holds real samples only: the invariant dsn_window_stitch refuses a violation of
    if W > 1:
        assert (W - 1) * hop + overlap < L


def test_window_plan_edges():
    assert native.window_plan(5, 8, 2) == (1, 6)                 # L <= window
    assert native.window_plan(8, 8, 2) == (1, 6)
    assert native.window_plan(9, 8, 2) == (2, 6)                 # L = window + 1
    assert native.window_plan(17, 8, 0) == (3, 8)                # overlap = 0
    assert native.window_plan(13, 8, 4) == (3, 4)                # 2 overlap = window
    assert native.window_plan(9000, 4096, 2048) == (4, 2048) and native.window_plan(5000, 4096, 2048) == (2, 2048)


@pytest.mark.parametrize("args,msg", [((10, 0, 0), "window = 0 < 1"), ((10, 8, -1), "overlap = -1 < 0"),
                                      ((0, 8, 2), "L = 0 < 1"),
                                      ((10, 8, 5), "2 * overlap = 10 > window = 8: a sample may lie in at most two")])
def test_window_plan_refusals(args, msg, monkeypatch):
    monkeypatch.setattr(native, "load_library", lambda: pytest.fail("a refused plan touched the library"))
    with pytest.raises(ValueError, match=re.escape(msg)):
        native.window_plan(*args)


@pytest.mark.parametrize("kind", ["hann", "linear"])
@pytest.mark.parametrize("O", [1, 2, 16, 517, 1024])
def test_fade_table(O, kind):
    fall, rise = native.fade_table(O, kind)
    assert fall.dtype == rise.dtype == np.float32 and fall.shape == rise.shape == (O,)
    f, r, r64 = sr.fade(O, kind)
    assert np.array_equal(fall, f) and np.array_equal(rise, r)                   # the restatement's own tables
    assert np.array_equal(native.fade_rise64(O, kind), r64)
    # fall + rise = 1 to one float32 ulp (each is within half an ulp, 2^-25, of its float64 value, and those add to 1)
    assert np.abs(fall.astype(np.float64) + rise.astype(np.float64) - 1.0).max() <= 2.0 ** -23
    assert np.all(np.diff(rise) >= 0) and np.all(np.diff(r64) > 0) and 0 < r64[0] and r64[-1] < 1
    # rise[k] + rise[O-1-k] = 1 before rounding: sin^2 x + sin^2 (pi/2 - x).  In float64 the argument carries a few
    # 2^-53 relative (the product with pi, the division, pi itself), at most about 2^-50 absolute for x <= pi/2, which
    # sin^2 (slope <= 1) passes on; sin and the square add about 3 * 2^-53 relative.  Two such terms: below 2^-48.
    assert np.abs(r64 + r64[::-1] - 1.0).max() <= 2.0 ** -48
    if kind == "linear":
        assert np.abs(r64 - (np.arange(O) + 0.5) / O).max() == 0
    else:
        assert np.abs(r64 - np.sin(np.pi * (np.arange(O) + 0.5) / (2 * O)) ** 2).max() < 1e-15


def test_fade_table_refusals():
    with pytest.raises(ValueError, match="fade must be one of"):
        native.fade_table(8, "triangle")
    with pytest.raises(ValueError, match="overlap = -1 < 0"):
        native.fade_table(-1)
    assert native.fade_table(0)[0].shape == (0,)


def test_entry_point_is_declared():
    hdr = open(os.path.join(ROOT, "include", "ditsep_hip.h")).read()
    assert "int dsn_window_stitch(dsn_ctx* ctx, const float* chunks" in hdr and "dsn_window_stitch" in native.EXPORTS
    assert hasattr(native.load_library(), "dsn_window_stitch")
    assert native.FADES == {"hann": int(re.search(r"DSN_FADE_HANN = (\d)", hdr).group(1)),
                            "linear": int(re.search(r"DSN_FADE_LINEAR = (\d)", hdr).group(1))}


# ------------------------------------------------------------------ the restatement against itself
SHAPES = [(1537, 517, 3910), (2048, 1024, 3000), (64, 16, 14400), (1537, 517, 1000), (96, 0, 250)]


@pytest.mark.parametrize("kind", ["hann", "linear"])
@pytest.mark.parametrize("Lw,O,L", SHAPES)
def test_restatement_stitches_a_cut_signal_back(Lw, O, L, kind):
    """no permutation: the windows of a known signal give the signal back -- exactly where a sample is copied, within
    2^-23 |x| inside an overlap, where fall32 + rise32 is 1 to one float32 ulp"""
    x = np.random.default_rng(5).standard_normal((3, L)).astype(np.float32)
    chunks = sr.cut(x, Lw, O)
    out, _, copied, P, _, _ = sr.stitch(chunks, L, O, kind)
    assert np.array_equal(P, np.tile(np.arange(3), (chunks.shape[0], 1)))
    assert np.array_equal(out[:, copied], x.astype(np.float64)[:, copied])
    assert np.all(np.abs(out - x) <= 2.0 ** -23 * np.abs(x))
    assert copied.sum() == L - (chunks.shape[0] - 1) * O


# (n, Lw, O, L, seed).  The margin asked of every boundary: the best score exceeds the runner-up by more than half
# the best.  The runner-up of well separated sources is a transposition, which keeps n - 2 of the n diagonal terms:
# about 0, 1/3 and 1/2 of the best for n = 2, 3, 4.  So for n = 4 the margin is about half the best and cannot
# exceed it reliably whatever the overlap; there the bound is a quarter of the best (half of what a transposition
# loses), with the overlap long enough that the off-diagonal terms, about sqrt(O) against O, stay well inside it.
DECISIVE = [(2, 1537, 517, 3910, 11), (3, 1537, 517, 3910, 12), (2, 2048, 1024, 3000, 13), (4, 1537, 517, 3910, 14),
            (1, 1537, 517, 3910, 15)]


def margin_fraction(n):
    return 0.25 if n == 4 else 0.5


@pytest.mark.parametrize("n,Lw,O,L,seed", DECISIVE)
def test_restatement_recovers_permutations(n, Lw, O, L, seed):
    chunks, src, q, expect = sr.decisive_case(seed, n, L, Lw, O)
    out, _, _, P, G, _ = sr.stitch(chunks, L, O)
    for w, (best, second) in enumerate(sr.margins(G)):
        assert best > 0.5 * O * n                                   # about O sigma^2 per source
        if second is not None:
            assert best - second > margin_fraction(n) * best, (w, best, second)
    assert np.array_equal(P, expect)
    # the signal in window 0's order, up to the 0.1 x noise of the windows (a convex combination of two noises)
    want = src[q[0]].astype(np.float64)
    err = out - want
    assert np.sqrt((err ** 2).mean()) < 0.11 and np.abs(err).max() < 0.6
    # and exactly the sources with noise-free windows
    clean, _, q2, expect2 = sr.decisive_case(seed, n, L, Lw, O, noise=0.0)
    out2, _, copied, P2, _, _ = sr.stitch(clean, L, O)
    assert np.array_equal(P2, expect2)
    want2 = src[q2[0]].astype(np.float64)
    assert np.array_equal(out2[:, copied], want2[:, copied]) and np.all(np.abs(out2 - want2) <= 2.0 ** -23 * np.abs(want2))


def test_restatement_tie_rule():
    ident = lambda W, n: np.tile(np.arange(n), (W, 1))
    rng = np.random.default_rng(7)
    Lw, O, hop = 64, 16, 48
    chunks = rng.standard_normal((3, 3, Lw)).astype(np.float32)
    zero = chunks.copy()
    zero[1:, :, :O] = 0                                              # an all-zero overlap (the later window's side)
    assert np.array_equal(sr.stitch(zero, 150, O)[3], ident(3, 3))
    zero = chunks.copy()
    zero[:-1, :, hop:] = 0                                           # (the earlier window's side)
    assert np.array_equal(sr.stitch(zero, 150, O)[3], ident(3, 3))
    same = chunks.copy()
    same[1:, 1] = same[1:, 0]                                        # two identical sources in the later window ...
    same[1:, 2] = same[1:, 0]                                        # ... and three: every candidate scores alike
    G = sr.gram(same, O)[0]
    assert all(len({s for _, s in sr.scores(g)}) == 1 for g in G)
    assert np.array_equal(sr.stitch(same, 150, O)[3], ident(3, 3))
    two = rng.standard_normal((2, 2, Lw)).astype(np.float32)
    two[1, 1] = two[1, 0]
    assert np.array_equal(sr.stitch(two, 100, O)[3], ident(2, 2))
    assert np.array_equal(sr.stitch(chunks, 3 * Lw, 0)[3], ident(3, 3))      # overlap = 0: empty sums
    # a strictly greater later candidate does replace the identity
    assert sr.best_perm(np.array([[0.0, 1.0], [1.0, 0.0]])) == (1, 0)
    assert sr.best_perm(np.array([[1.0, 1.0], [1.0, 1.0]])) == (0, 1)
    # lexicographic order of the candidates
    assert [sg for sg, _ in sr.scores(np.zeros((3, 3)))] == [(0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1),
                                                              (2, 1, 0)]


def test_restatement_cumulative_table():
    """P_{w+1}(i) = sigma_w(P_w(i)) from hand-made tables"""
    swap = np.array([[0.0, 1.0], [1.0, 0.0]])
    keep = np.eye(2)
    assert sr.perms_from_gram([swap, keep, swap, swap], 5, 2).tolist() == [[0, 1], [1, 0], [1, 0], [0, 1], [1, 0]]
    rot = np.array([[0.0, 1.0, 0.0], [0.0, 0.0, 1.0], [1.0, 0.0, 0.0]])       # sigma = (1, 2, 0)
    assert sr.perms_from_gram([rot, rot, rot], 4, 3).tolist() == [[0, 1, 2], [1, 2, 0], [2, 0, 1], [0, 1, 2]]
