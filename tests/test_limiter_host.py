"""The host side of the true-peak look-ahead limiter (no GPU): the options of the `limit` keyword, the refusals of the
two calls, the smoothing window, the pre-gain rule native.limiter_drive against its restatement
(tests/limiter_restatement.py), the restatement's own two ways to the hold, and the command line."""
import math

import numpy as np
import pytest

from ditsep_amd import native
from tests import limiter_restatement as lim


# ---------------------------------------------------------------------------------------------- options
def test_limit_options():
    assert native.limit_options(None) is None
    assert native.limit_options(True) == native.LIMIT_DEFAULTS == dict(ceiling=None, lookahead_ms=5.0, drive_db=6.0,
                                                                       iterations=4, tol=0.1)
    assert native.limit_options(True) is not native.LIMIT_DEFAULTS
    assert native.limit_options({}) == native.LIMIT_DEFAULTS
    got = native.limit_options({"ceiling": -2, "lookahead_ms": 1, "iterations": 2})
    assert got == dict(ceiling=-2.0, lookahead_ms=1.0, drive_db=6.0, iterations=2, tol=0.1)
    assert lim.DEFAULTS == native.LIMIT_DEFAULTS
    # the loudness keyword keeps its three keys
    assert native.LOUDNESS_DEFAULTS == dict(target=-23.0, peak=-1.0, link="mixture")


def test_level_options_merge_the_two_keywords():
    assert native.level_options(None, None) is None
    assert native.level_options(-16, None) == dict(target=-16.0, peak=-1.0, link="mixture")      # as before: three keys
    assert native.level_options(-16, True) == dict(target=-16.0, peak=-1.0, link="mixture", limit=native.LIMIT_DEFAULTS)
    assert native.level_options(None, {"ceiling": -3}) == dict(target=None, peak=None, link="mixture",
                                                               limit=dict(native.LIMIT_DEFAULTS, ceiling=-3.0))
    with pytest.raises(ValueError, match="limit must be"):
        native.level_options(-16, False)


@pytest.mark.parametrize("spec,msg", [
    (False, "limit must be None, True"), ("on", "limit must be None, True"), (5.0, "limit must be None, True"),
    ({"lookahead": 5.0}, "unknown keys"), ({"target": -14.0}, "unknown keys"),
    ({"ceiling": math.nan}, "ceiling = nan"), ({"ceiling": True}, "ceiling = True"),
    ({"lookahead_ms": 0.0}, "lookahead_ms = 0.0 is not positive"), ({"lookahead_ms": math.inf}, "lookahead_ms = inf"),
    ({"lookahead_ms": None}, "lookahead_ms = None"), ({"drive_db": -1.0}, "drive_db = -1.0 is negative"),
    ({"tol": 0.0}, "tol = 0.0 is not positive"), ({"tol": "0.1"}, "tol = '0.1'"),
    ({"iterations": 0}, "iterations = 0"), ({"iterations": 17}, "iterations = 17"), ({"iterations": 2.0}, "iterations = 2.0"),
    ({"iterations": True}, "iterations = True"),
])
def test_limit_options_refusals(spec, msg):
    with pytest.raises(ValueError, match=msg):
        native.limit_options(spec)


# ---------------------------------------------------------------------------------------------- the two calls
def test_check_limiter():
    got = native.check_limiter((4, 2, 9), [8000, 8000, 16000, 16000], [0, 0, 1, 2], [1.0, 2, 0.5], 0.89, 5.0,
                               [9, 9, 4, 4], [1, 2, 2, 1])
    assert got == ((4, 2, 9), [8000, 8000, 16000, 16000], [9, 9, 4, 4], [1, 2, 2, 1], [0, 0, 1, 2], [1.0, 2.0, 0.5])
    # apply_curve: any order, a group without a row
    got = native.check_limiter((2, 1, 9), 8000, [2, 0], [1.0, 1.0, 1.0])
    assert got[4] == [2, 0]
    assert native.limiter_half_window(5.0, 16000) == 80 and native.limiter_half_window(5.0, 44100) == 221
    assert native.limiter_half_window(0.01, 8000) == 1 and native.limiter_half_window(5.0, 192000) == 960
    for ms, fs in [(5.0, 8000), (0.0625, 8000), (0.3125, 8000), (2.5, 44100), (5.33, 192000)]:
        assert native.limiter_half_window(ms, fs) == lim.half_window(ms, fs)


@pytest.mark.parametrize("args,msg", [
    (((1, 3, 5), 8000, [0], [1.0], 0.9, 5.0), "C = 3 outside"),
    (((1, 1, 5), 7999, [0], [1.0], 0.9, 5.0), "rates\\[0\\] = 7999"),
    (((2, 1, 5), 8000, [0], [1.0], 0.9, 5.0), "one integer label per row"),
    (((2, 1, 5), 8000, [0, 0.5], [1.0], 0.9, 5.0), "one integer label per row"),
    (((2, 1, 5), 8000, [0, 1], [], 0.9, 5.0), "at least one"),
    (((2, 1, 5), 8000, [0, 1], [1.0, math.inf], 0.9, 5.0), "pregain\\[1\\] = inf"),
    (((2, 1, 5), 8000, [0, 1], [1.0, math.nan], 0.9, 5.0), "pregain\\[1\\] = nan"),
    (((2, 1, 5), 8000, [1, 0], [1.0, 1.0], 0.9, 5.0), "non-decreasing order"),
    (((2, 1, 5), 8000, [0, 2], [1.0, 1.0, 1.0], 0.9, 5.0), "non-decreasing order"),
    (((2, 1, 5), 8000, [0, 0], [1.0, 1.0], 0.9, 5.0), "non-decreasing order"),
    (((2, 1, 5), 8000, [1, 1], [1.0, 1.0], 0.9, 5.0), "non-decreasing order"),
    (((2, 1, 5), 8000, [0, 0], [1.0], 0.0, 5.0), "ceiling 0.0"),
    (((2, 1, 5), 8000, [0, 0], [1.0], -0.5, 5.0), "ceiling -0.5"),
    (((2, 1, 5), 8000, [0, 0], [1.0], math.inf, 5.0), "ceiling inf"),
    (((2, 1, 5), 8000, [0, 0], [1.0], math.nan, 5.0), "ceiling nan"),
    (((2, 1, 5), 8000, [0, 0], [1.0], 0.9, math.nan), "lookahead_ms = nan"),
    (((2, 1, 5), 8000, [0, 0], [1.0], 0.9, -1.0), "lookahead_ms = -1.0"),
    (((2, 1, 5), 8000, [0, 0], [1.0], 0.9, 128.125), "W = 1025 outside"),
    (((2, 1, 5), 192000, [0, 0], [1.0], 0.9, 5.5), "W = 1056 outside"),
    (((2, 1, 5), 8000, [0, 0], [1.0], 0.9, 5.0, [5, 4]), "disagree on length or rate"),
    (((2, 1, 5), [8000, 16000], [0, 0], [1.0], 0.9, 5.0), "disagree on length or rate"),
    (((2, 1, 5), 8000, [0, 1], [1.0], None), "group\\[1\\] = 1 outside"),
    (((2, 1, 5), 8000, [-1, 0], [1.0], None), "group\\[0\\] = -1 outside"),
])
def test_check_limiter_refusals(args, msg):
    with pytest.raises(ValueError, match=msg):
        native.check_limiter(*args)


def test_rows_of_different_groups_may_differ():
    native.check_limiter((2, 1, 5), [8000, 16000], [0, 1], [1.0, 1.0], 0.9, 5.0, [5, 4])
    native.check_limiter((1, 1, 5), 8000, [0], [1.0], 0.9, 128.0)                        # W = 1024 exactly


# ---------------------------------------------------------------------------------------------- the window
@pytest.mark.parametrize("W", [1, 2, 80, 1024])
def test_window_sums_to_one(W):
    w = native.limiter_window(W)
    assert w.dtype == np.float32 and w.shape == (2 * W + 1,)
    assert abs(float(w.astype(np.float64).sum()) - 1.0) <= 1e-7
    assert np.array_equal(w, w[::-1]) and float(w.min()) > 0.0 and int(w.argmax()) == W
    assert np.array_equal(w, lim.window(W))
    k = np.arange(-W, W + 1, dtype=np.float64)
    exact = (0.5 + 0.5 * np.cos(np.pi * k / (W + 1))) / (W + 1)
    assert abs(exact.sum() - 1.0) <= 1e-12 and np.array_equal(w, exact.astype(np.float32))


def test_window_refusals():
    for W in (0, 1025):
        with pytest.raises(ValueError, match="half-window"):
            native.limiter_window(W)


# ---------------------------------------------------------------------------------------------- the pre-gain rule
def run(rule, measure, g_lo, i_src, target, **kw):
    hist = []
    G = rule(g_lo, i_src, target, hist, **kw)
    while G is not None:
        hist.append((G, measure(G)))
        G = rule(g_lo, i_src, target, hist, **kw)
    return hist


# measured loudness of the limited programme as a function of the pre-gain (dB), for a source at -20 LUFS
MODELS = {
    "linear": lambda G: -20.0 + G,                                              # the limiter takes nothing away
    "soft": lambda G: -20.0 + G - 0.08 * max(G - 3.0, 0.0) ** 1.5,             # .. takes more the harder it is driven
    "flat": lambda G: -20.0 + min(G, 5.0) + 0.1 * max(G - 5.0, 0.0),           # slope 0.1: under the clamp of 1/4
    "steep": lambda G: -20.0 + 1.5 * G,                                        # slope 1.5: over the clamp of 1
    "stuck": lambda G: -18.0,                                                   # slope 0
    "nan": lambda G: math.nan,
}


@pytest.mark.parametrize("model", sorted(MODELS))
@pytest.mark.parametrize("g_lo,target", [(3.0, -14.0), (3.0, -12.0), (0.0, -19.95), (2.0, -10.0), (7.0, -14.0)])
def test_limiter_drive_is_the_restated_rule(model, g_lo, target):
    f = MODELS[model]
    for kw in (dict(), dict(drive_db=3.0, iterations=6, tol=0.01), dict(drive_db=0.0), dict(iterations=1)):
        a = run(native.limiter_drive, f, g_lo, -20.0, target, **kw)
        b = run(lim.drive, f, g_lo, -20.0, target, **kw)
        assert len(a) == len(b) >= 1 and all(x[0] == y[0] for x, y in zip(a, b)), (a, b)
        hi = g_lo + kw.get("drive_db", 6.0)
        assert all(g_lo <= G <= hi for G, _ in a) and len(a) <= kw.get("iterations", 4)
        assert len({G for G, _ in a}) == len(a)                                  # the clamp never repeats a G
        assert a[0][0] == min(max(target + 20.0, g_lo), hi)
        if model != "nan":
            assert native.limiter_best(a, target) == lim.best(b, target)


def test_limiter_drive_steps():
    # G_0, then G_0 + (target - I_0), then the secant step with the slope clamped to [1/4, 1]
    h = [(6.0, -14.5)]
    assert native.limiter_drive(3.0, -20.0, -14.0, [], 6.0, 4, 0.1) == 6.0
    assert native.limiter_drive(3.0, -20.0, -14.0, h, 6.0, 4, 0.1) == 6.5
    h.append((6.5, -14.25))                                                      # slope 1/2: 0.25 / 0.5 more
    assert native.limiter_drive(3.0, -20.0, -14.0, h, 6.0, 4, 0.1) == 7.0
    assert native.limiter_drive(3.0, -20.0, -14.0, h + [(7.0, -14.05)], 6.0, 4, 0.1) is None      # within tol
    assert native.limiter_drive(3.0, -20.0, -14.0, h + [(7.0, -14.2)], 6.0, 3, 0.1) is None       # out of evaluations
    assert native.limiter_drive(3.0, -20.0, -14.0, [(6.0, -14.5), (6.5, -14.49)], 6.0, 4, 0.1) == 6.5 + 0.49 / 0.25
    assert native.limiter_drive(3.0, -20.0, -14.0, [(6.0, -14.5), (6.5, -13.0)], 6.0, 4, 0.1) == 5.5  # slope 3 -> 1
    assert native.limiter_drive(3.0, -20.0, -10.0, [(9.0, -12.0)], 6.0, 4, 0.1) is None           # the clamp repeats 9
    assert native.limiter_best([(6.0, -14.5), (6.5, -13.8), (7.0, -14.2)], -14.0) == 1
    assert native.limiter_best([(6.0, math.nan), (6.5, -13.0)], -14.0) == 1


# ---------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("W", [1, 2, 7])
def test_restatement_hold_and_identity(W):
    g = np.random.default_rng(W)
    r = np.where(g.random(60) < 0.15, g.random(60), 1.0)
    m = lim.hold(r, W)                                                           # (asserts its two ways agree)
    assert m.shape == (60 + 2 * W,) and m[W] == r[:W + 1].min() and m[0] == r[0]
    cv = lim.curve_from_required(r, W)
    far = np.array([not (r[max(0, t - 2 * W):t + 2 * W + 1] < 1.0).any() for t in range(60)])
    assert (cv[far] == 1.0).all() and (cv <= r).all() and (cv >= 0.0).all()
    assert np.array_equal(lim.curve_from_required(np.ones(9), W), np.ones(9))


# ---------------------------------------------------------------------------------------------- the command line
def test_cli_flags_reach_the_options():
    from ditsep_amd import separate as cli

    base = ["in", "out", "--config", "c.json"]
    a = cli.build_parser().parse_args(base)
    assert cli.limit_of(a) is None and cli.loudness_of(a) is None
    a = cli.build_parser().parse_args(base + ["--loudness", "-16", "--limit"])
    assert cli.loudness_of(a) == dict(target=-16.0, peak=-1.0, link="mixture")       # its three keys, as before
    assert native.limit_options(cli.limit_of(a)) == native.LIMIT_DEFAULTS
    a = cli.build_parser().parse_args(base + ["--limit", "--limit-lookahead", "2.5", "--limit-drive", "9",
                                              "--limit-iterations", "6"])
    assert cli.loudness_of(a) is None
    assert native.limit_options(cli.limit_of(a)) == dict(ceiling=None, lookahead_ms=2.5, drive_db=9.0, iterations=6, tol=0.1)
    with pytest.raises(SystemExit):
        cli.build_parser().parse_args(base + ["--limit-iterations", "two"])
