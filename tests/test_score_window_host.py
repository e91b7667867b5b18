"""The plan of the window-blended score call on the host (no GPU): ditsep_amd.native.score_window_plan, its C++ mirror
(dsn_score_window_plan, csrc/score_window.h) and the independent restatement tests/score_window_restatement.py agree,
exhaustively for T in 1 .. 4 Tw + 1 with (Tw, To) in {(8, 0), (8, 2), (8, 4), (5, 1)}; the refusals; the C-ABI."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from ditsep_amd import native
from tests import score_window_restatement as swr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(8, 0), (8, 2), (8, 4), (5, 1)]


def c_plan(frames, T, Tw, To, fade="hann"):
    lib = native.load_library()
    R = len(frames)
    fr = (C.c_int32 * R)(*frames)
    Wtot, Twin = C.c_int(), C.c_int()
    rc = lib.dsn_score_window_plan(fr, R, T, Tw, To, native.FADES[fade], None, None, None, C.byref(Wtot), C.byref(Twin))
    if rc:
        return rc
    wtab = np.zeros((Wtot.value, 3), dtype=np.int32)
    ftab = np.zeros((R * T, 4), dtype=np.int32)
    fw = np.zeros((R * T, 2), dtype=np.float32)
    i32p, fp = C.POINTER(C.c_int32), C.POINTER(C.c_float)
    assert lib.dsn_score_window_plan(fr, R, T, Tw, To, native.FADES[fade], wtab.ctypes.data_as(i32p),
                                     ftab.ctypes.data_as(i32p), fw.ctypes.data_as(fp), None, None) == 0
    return {"Wtot": Wtot.value, "Twin": Twin.value, "windows": wtab, "table": ftab, "weights": fw}


@pytest.mark.parametrize("Tw,To", SHAPES)
def test_plan_properties(Tw, To):
    hop = Tw - To
    for T in range(1, 4 * Tw + 2):
        p = native.score_window_plan([T], Tw, To)
        win, tab, wts = p["windows"], p["table"], p["weights"]
        W = p["Wtot"]
        assert p["W"] == [W] and W == native.window_plan(T, Tw, To)[0], (T, W)
        if T <= Tw:
            assert win.tolist() == [[0, 0, T]] and p["Twin"] == T
        else:
            assert p["Twin"] == Tw
        for r, s, l in win.tolist():
            assert r == 0 and 0 <= s and s + l <= T and (l == Tw or T <= Tw), (T, s, l)
        assert sorted(win[:, 1].tolist()) == win[:, 1].tolist()
        # seams: To frames each, disjoint, the last To frames of window j, covered by window j + 1
        seams = [range((j + 1) * hop, (j + 1) * hop + To) for j in range(W - 1)]
        flat = [f for s in seams for f in s]
        assert len(flat) == len(set(flat)) and all(0 <= f < T for f in flat)
        for j, s in enumerate(seams):
            for f in s:
                assert win[j, 1] + Tw - To <= f < win[j, 1] + Tw and win[j + 1, 1] <= f < win[j + 1, 1] + Tw
        # every frame: one or two windows that hold it, weights summing to 1
        for f in range(T):
            w0, o0, w1, o1 = tab[f].tolist()
            fall, rise = wts[f].tolist()
            assert 0 <= w0 < W and win[w0, 1] + o0 == f and 0 <= o0 < win[w0, 2]
            if f in flat:
                assert w1 == w0 + 1 and win[w1, 1] + o1 == f and 0 <= o1 < win[w1, 2]
                assert abs(fall + rise - 1.0) <= 2.0 ** -24 and 0.0 < rise < 1.0
            else:
                assert w1 == -1 and (fall, rise) == (1.0, 0.0)
                assert w0 == sum(1 for s in seams if len(s) and f > s[-1]) or To == 0
        used = {int(w) for w in tab[:T, 0]} | {int(w) for w in tab[:T, 2] if w >= 0}
        assert used == set(range(W)), "a window serves no frame"
        # the restatement, written from the seams outwards, names the same windows, offsets and weights
        rwin, serve = swr.plan([T], Tw, To)
        assert [list(w) for w in rwin] == win.tolist()
        for f, e in enumerate(serve[0]):
            if len(e) == 1:
                assert (e[0][0], e[0][1], -1) == tuple(tab[f, :3])
            else:
                assert (e[0][0], e[0][1], e[1][0], e[1][1]) == tuple(tab[f]) and (e[0][2], e[1][2]) == tuple(wts[f])


def test_plan_pool_and_padding():
    """several recordings: windows in order, pool-wide indices, frames past a recording's end marked (-1)"""
    frames, Tw, To, T = [21, 5, 8, 9], 8, 2, 23
    p = native.score_window_plan(frames, Tw, To, T=T)
    assert p["W"] == [4, 1, 1, 2] and p["Wtot"] == 8 and p["Twin"] == 8 and p["short"] and p["T"] == T
    assert p["windows"][:, 0].tolist() == [0, 0, 0, 0, 1, 2, 3, 3]
    assert p["windows"][4].tolist() == [1, 0, 5] and p["windows"][7].tolist() == [3, 1, 8]     # shifted back by 5
    tab = p["table"].reshape(4, T, 4)
    for r, F in enumerate(frames):
        assert (tab[r, F:, 0] == -1).all() and (tab[r, F:, 2] == -1).all() and (tab[r, :F, 0] >= 0).all()
        assert set(p["windows"][tab[r, :F, 0], 0].tolist()) == {r}
    assert not native.score_window_plan([8, 8], 8, 2)["short"]
    assert native.score_window_plan([5, 5], 8, 2)["Twin"] == 5 and not native.score_window_plan([5, 5], 8, 2)["short"]
    assert native.score_window_plan([5, 4], 8, 2)["short"]


@pytest.mark.parametrize("fade", ["hann", "linear"])
def test_c_plan_mirrors_python(fade):
    for Tw, To in SHAPES:
        for T in range(1, 4 * Tw + 2):
            frames = [T, max(1, T // 2), min(T, Tw)]
            py, c = native.score_window_plan(frames, Tw, To, fade, T=T + 1), c_plan(frames, T + 1, Tw, To, fade)
            assert (py["Wtot"], py["Twin"]) == (c["Wtot"], c["Twin"])
            for k in ("windows", "table", "weights"):
                assert np.array_equal(py[k], c[k]), (Tw, To, T, k)


def test_refusals_by_name():
    with pytest.raises(ValueError, match="2 \\* overlap = 10 > window = 8: a sample may lie in at most two windows"):
        native.score_window_plan([20], 8, 5)
    with pytest.raises(ValueError, match="window = 0 < 1"):
        native.score_window_plan([20], 0, 0)
    with pytest.raises(ValueError, match="overlap = -1 < 0"):
        native.score_window_plan([20], 8, -1)
    with pytest.raises(ValueError, match="frames\\[1\\] = 0 outside \\[1, T = 20\\]"):
        native.score_window_plan([20, 0], 8, 2)
    with pytest.raises(ValueError, match="frames\\[0\\] = 20 outside \\[1, T = 19\\]"):
        native.score_window_plan([20], 8, 2, T=19)
    assert c_plan([20], 20, 8, 5) == -1 and c_plan([21], 20, 8, 2) == -1 and c_plan([20], 20, 0, 0) == -1
    # the engine-side checks, before the library is touched
    with pytest.raises(ValueError, match="need the DiT score network"):
        native.check_windowed(native.SCORE_NCSNPP, [20], 1, 20, (8, 2))
    with pytest.raises(ValueError, match="langevin corrector has no form for recordings of different lengths"):
        native.check_windowed(native.SCORE_DIT, [20, 19], 2, 20, (8, 2), "langevin")
    assert native.check_windowed(native.SCORE_DIT, [20, 20], 2, 20, (8, 2), "langevin") == ([20, 20], 8, 2)
    with pytest.raises(ValueError, match="needs frames="):
        native.check_windowed(native.SCORE_DIT, None, 1, 20, (8, 2))


def test_abi():
    hdr = open(os.path.join(ROOT, "include", "ditsep_hip.h")).read()
    lib = native.load_library()
    for name in ("dsn_score_windowed", "dsn_pc_sample_windowed", "dsn_separate_windowed", "dsn_score_window_plan"):
        assert re.search(r"\bint %s\(" % name, hdr) and name in native.EXPORTS and hasattr(lib, name)
    for kind in ("win_pack_tokens", "win_blend_tokens"):
        assert kind in native.TEST_KERNEL_KINDS
    from ditsep_amd import LatentDiffSep

    for cls in (native.Engine, LatentDiffSep):
        assert inspect.signature(cls.separate_long).parameters["mode"].default == "stitch"
    for fn in (native.Engine.score, native.Engine.pc_sample):
        assert inspect.signature(fn).parameters["window"].default is None


def test_restatement_blend_is_a_convex_combination():
    """blend64 of constant window scores is that constant on every valid frame; of window-indexed scores it is monotone
    across a seam"""
    frames, Tw, To = [21, 5], 8, 4
    windows, serve = swr.plan(frames, Tw, To)
    ws = np.ones((len(windows), 1, 1, Tw))
    out = swr.blend64(ws, serve, 21)
    assert np.allclose(out[0, 0, 0], 1.0, atol=1e-7) and np.allclose(out[1, 0, 0, :5], 1.0) and (out[1, 0, 0, 5:] == 0).all()
    ws = np.arange(len(windows), dtype=np.float64)[:, None, None, None] * np.ones((1, 1, 1, Tw))
    row = swr.blend64(ws, serve, 21)[0, 0, 0]
    assert (np.diff(row) >= 0).all() and row[0] == 0 and row[-1] == 4
