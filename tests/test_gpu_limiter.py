"""dsn_limiter_curve / dsn_apply_curve (csrc/limiter.hip) against the float64 restatement (tests/limiter_restatement.py).

Shapes are the smallest at which the kernels can go wrong: L in {1, W, 2 W + 1, tile - 1, tile + 1, 3 tiles + 5}, the
half-windows W in {1, 2, 80, 1024} (8000, 16000 and 192000 Hz), one and two channels, groups of 1, 2 and 4 rows, a
peak at sample 0, at the last sample, on either side of a tile edge, two peaks W / 2, W + 1 and 2 W + 1 apart, a
whole item over the ceiling.
  envelope  |p - p64| <= dp = (S + 1) 2^-24 sum |h| |y|, the resampler's bound (y = float32(G x) on both sides)
  curve     |g - g64| <= max_{|s - t| <= 2 W} (c dp[s] / p[s]^2) + (2 W + 4) 2^-24: min and max are 1-Lipschitz, the
            smoothing is a convex combination, and the second term holds the roundings of the division, of 1 - m, of
            the 2 W + 1 fmas and of 1 - a, and the float the device lowers r by where r p would round above c
  output    |out - y g64| <= |y| (that bound) + |y g64| 2^-24: one more product
  exactly   float32(g p) <= c at every sample from the device's own g and p; g == 1.0f and out == y bit for bit at every
            sample farther than 2 W from any sample with p > c; an item under the ceiling is apply_gain's bits; the
            statistics are those of the returned curve
and bit for bit: an item in a NaN-padded ragged mixed-rate batch against the item alone, a permuted batch, a second
call, a base pointer one float off, apply_curve against (G x) g in torch, and stems that share a curve still sum to
the curve applied to their sum."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

from ditsep_amd import native
from tests import limiter_restatement as lim
from tests import resample_restatement as rr
from tests.util import make_engine

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = open(os.path.join(ROOT, "ditsep_amd", "csrc", "kernels.h")).read()
TILE = int(re.search(r"#define LIM_TILE (\d+)", HDR).group(1))
U = 2.0 ** -24
CEIL = float(np.float32(10.0 ** (-1.0 / 20.0)))

# W -> (fs, lookahead_ms)
WINDOWS = {1: (8000, 0.125), 2: (8000, 0.25), 80: (16000, 5.0), 1024: (192000, 16.0 / 3.0)}


@pytest.fixture(scope="module")
def eng():
    e = make_engine()
    assert e.cfg.score_kind == native.SCORE_NONE
    yield e
    e.close()


@pytest.fixture(scope="module")
def taps():
    p = native.resample_plan(1, 4)
    assert (p["new"], p["support"]) == (4, 13)
    return p, rr.dense_from_compact(p["k0"], p["taps"], p["K"])


def bed(seed, rows, Cn, L, amp=0.05):
    g = torch.Generator().manual_seed(seed)
    return amp * torch.randn((rows, Cn, L), generator=g)


def with_peaks(x, at, height=1.4):
    """x [rows, C, L]: samples `at` of row 0, channel 0 (and the last row's last channel, smaller) over the ceiling"""
    L = x.shape[-1]
    for k, t in enumerate(at):
        if 0 <= t < L:
            if x.shape[0] * x.shape[1] > 1:
                x[-1, -1, t] = -0.5 * height
            x[0, 0, t] = height * (1.0 if k % 2 == 0 else -0.8)
    return x


_worst = {"curve": 0.0, "out": 0.0, "env": 0.0}


def check(eng, taps, x, W, G=1.0, c=CEIL, what=""):
    """one group x [rows, C, L] float32 through the device against the restatement -> (curve, env, out) on the host"""
    plan, h = taps
    fs, ms = WINDOWS[W]
    assert native.limiter_half_window(ms, fs) == W == lim.half_window(ms, fs)
    rows, Cn, L = x.shape
    G32 = float(np.float32(G))
    curve, info, env = eng.limiter_curve(x, fs, [0] * rows, [G32], c, ms, envelope=True)
    out = eng.apply_curve(x, [0] * rows, [G32], curve)
    y_dev = eng.apply_gain(x, [G32] * rows)
    torch.cuda.synchronize()
    g, p, o, y32 = curve[0].cpu().numpy(), env[0].cpu().numpy(), out.cpu().numpy(), y_dev.cpu().numpy()
    cv = lim.curve(x.reshape(rows * Cn, L).numpy(), G32, c, W, taps=h)
    assert np.array_equal(cv["y"].astype(np.float32).reshape(rows, Cn, L), y32), what          # step 1 is apply_gain
    # the envelope
    dp = (plan["support"] + 1) * U * cv["A"]
    e_env = np.abs(p.astype(np.float64) - cv["p"])
    assert (e_env <= dp).all(), f"{what}: envelope off by {e_env.max():.3e}"
    # the curve and the output
    bound = lim.curve_bound(cv["p"], cv["A"], c, W, plan["support"])
    e_g = np.abs(g.astype(np.float64) - cv["g"])
    ratio = float((e_g / bound).max())
    print(f"{what}: min g = {g.min():.6f}, {int((g < 1).sum())} of {L} samples reduced, worst |g - g64| / bound = {ratio:.3f}")
    assert (e_g <= bound).all(), f"{what}: curve off by {e_g.max():.3e}, {ratio:.3f} of the bound"
    want = cv["y"].reshape(rows, Cn, L) * cv["g"]
    b_out = np.abs(cv["y"]).reshape(rows, Cn, L) * bound + np.abs(want) * U
    e_o = np.abs(o.astype(np.float64) - want)
    assert (e_o <= b_out).all(), f"{what}: output off by {e_o.max():.3e}"
    with np.errstate(invalid="ignore", divide="ignore"):
        _worst["curve"] = max(_worst["curve"], ratio)
        _worst["env"] = max(_worst["env"], float(np.nanmax(np.where(dp > 0, e_env / dp, 0.0))))
        _worst["out"] = max(_worst["out"], float(np.nanmax(np.where(b_out > 0, e_o / b_out, 0.0))))
    # exactly
    assert ((g * p) <= np.float32(c)).all() and (g * p).dtype == np.float32, what
    assert (g >= 0.0).all() and (g <= 1.0).all()
    over = np.flatnonzero(p > np.float32(c))
    far = np.ones(L, dtype=bool)
    for t in over:
        far[max(0, t - 2 * W):t + 2 * W + 1] = False
    assert (g[far] == 1.0).all(), what
    assert np.array_equal(o[..., far].view(np.uint32), y32[..., far].view(np.uint32)), what
    assert np.array_equal(o, (y32 * g).astype(np.float32)), what                                  # (G x) g, two products
    assert float(info["min_gain"][0]) == float(g.min()) and int(info["limited_samples"][0]) == int((g < 1.0).sum())
    assert int(info["nonfinite"][0]) == 0
    return g, p, o


def lengths(W):
    return sorted({1, W, 2 * W + 1, TILE - 1, TILE + 1, 3 * TILE + 5})


CASES = [(W, L) for W in WINDOWS for L in lengths(W)]


@pytest.mark.parametrize("W,L", CASES, ids=lambda v: str(v))
def test_curve_and_output_against_the_restatement(eng, taps, W, L):
    k = CASES.index((W, L))
    Cn, rows = 1 + k % 2, (1, 2, 4)[k % 3]
    x = bed(100 + k, rows, Cn, L)
    # a peak at sample 0, at the last sample, on either side of every tile edge, and two in the middle W + 1 apart
    at = [0, L - 1, TILE - 1, TILE, 2 * TILE - 1, 2 * TILE + 1, L // 2, L // 2 + W + 1]
    g, p, _ = check(eng, taps, with_peaks(x, at), W, G=(1.0, 1.7, 0.8)[k % 3], what=f"W={W} L={L} C={Cn} rows={rows}")
    assert g.min() < 1.0 and g[0] < 1.0 and g[-1] < 1.0


@pytest.mark.parametrize("W", [2, 80, 1024])
@pytest.mark.parametrize("gap", ["W/2", "W+1", "2W+1", "4W+8"])
def test_two_peaks(eng, taps, W, gap):
    d = {"W/2": W // 2, "W+1": W + 1, "2W+1": 2 * W + 1, "4W+8": 4 * W + 8}[gap]
    L = TILE + 4 * W + 40
    t0 = TILE - W // 2 - 3                                                          # the pair straddles a tile edge
    x = with_peaks(bed(W + d, 2, 2, L, 0.02), [t0, t0 + d], height=2.0)
    g, p, _ = check(eng, taps, x, W, what=f"two peaks {gap} apart, W={W}")
    if gap == "4W+8":
        # (the interpolator spreads a peak of this height over one sample on either side)
        assert g[t0 + d // 2] == 1.0                                                # the curve is back at 1 in between
    if gap == "W/2":
        assert (g[t0:t0 + d + 1] < 1.0).all()


@pytest.mark.parametrize("W,L", [(1, 1), (2, 5), (80, TILE + 1), (1024, 2 * TILE + 7)])
def test_whole_item_over_the_ceiling(eng, taps, W, L):
    x = bed(W + L, 2, 1, L, 0.5)
    x[0, 0] = 1.5 * torch.sign(x[0, 0])
    g, p, o = check(eng, taps, x, W, G=2.0, what=f"all over, W={W} L={L}")
    assert (p > CEIL).all() and (g < 1.0).all()


@pytest.mark.parametrize("W,L", [(1, 7), (80, TILE - 1), (80, 3 * TILE + 5), (1024, TILE + 1)])
def test_items_under_the_ceiling_are_apply_gain_bits(eng, taps, W, L):
    x = bed(3 * W + L, 4, 2, L, 0.02)
    g, p, o = check(eng, taps, x, W, G=3.0, what=f"under, W={W} L={L}")
    assert (g == 1.0).all() and float(p.max()) < CEIL
    assert np.array_equal(o, eng.apply_gain(x, [float(np.float32(3.0))] * 4).cpu().numpy())


def test_zero_item_and_pregain_zero(eng):
    fs, ms = WINDOWS[80]
    x = torch.zeros((1, 2, 300))
    curve, info, env = eng.limiter_curve(x, fs, [0], [1.0], CEIL, ms, envelope=True)
    assert bool((curve == 1.0).all()) and bool((env == 0.0).all()) and float(info["min_gain"][0]) == 1.0
    curve, info = eng.limiter_curve(bed(1, 1, 2, 300, 5.0), fs, [0], [0.0], CEIL, ms)
    assert bool((curve == 1.0).all()) and int(info["limited_samples"][0]) == 0


def test_worst_ratios_are_reported(eng):
    print(f"worst error / bound over the cases above: envelope {_worst['env']:.3f}, curve {_worst['curve']:.3f}, "
          f"output {_worst['out']:.3f}")


# ---------------------------------------------------------------------------------------------- bit for bit
# (fs, lookahead ms) is the call's; items: (fs, L, C, rows)
ITEMS = [(16000, 3 * TILE + 5, 1, 2), (192000, TILE + 1, 2, 1), (8000, 1, 1, 1), (44100, TILE - 1, 2, 4),
         (16000, 161, 2, 2), (8000, 2 * TILE, 1, 1)]
MS = 5.0


def item_signal(b):
    fs, L, Cn, rows = ITEMS[b]
    W = native.limiter_half_window(MS, fs)
    return with_peaks(bed(40 + b, rows, Cn, L), [0, L - 1, TILE - 1, TILE, L // 3, L // 3 + W + 1], height=1.2 + 0.1 * b)


@pytest.fixture(scope="module")
def ragged(eng):
    """the mixed-rate batch, padded with NaN past every item's end and in the channels it does not have; and every
    item's curve and output alone"""
    clips = [item_signal(b) for b in range(len(ITEMS))]
    pre = [float(np.float32(1.0 + 0.25 * b)) for b in range(len(ITEMS))]
    alone = []
    for b, c in enumerate(clips):
        rows = c.shape[0]
        curve, info = eng.limiter_curve(c, ITEMS[b][0], [0] * rows, [pre[b]], CEIL, MS)
        alone.append((curve.cpu(), {k: v.clone() for k, v in info.items()},
                      eng.apply_curve(c, [0] * rows, [pre[b]], curve).cpu()))
        assert float(info["min_gain"][0]) < 1.0 or ITEMS[b][1] == 1
    return clips, pre, alone


def batch_of(clips, order):
    Lmax = max(c.shape[-1] for c in clips) + 37
    R = sum(clips[b].shape[0] for b in order)
    x = torch.full((R, 2, Lmax), float("nan"))
    rates, lens, chans, group = [], [], [], []
    r = 0
    for q, b in enumerate(order):
        c = clips[b]
        x[r:r + c.shape[0], :c.shape[1], :c.shape[2]] = c
        for _ in range(c.shape[0]):
            rates.append(ITEMS[b][0]), lens.append(c.shape[2]), chans.append(c.shape[1]), group.append(q)
        r += c.shape[0]
    return x, rates, lens, chans, group


def run_batch(eng, clips, pre, alone, order):
    x, rates, lens, chans, group = batch_of(clips, order)
    pg = [pre[b] for b in order]
    curve, info = eng.limiter_curve(x, rates, group, pg, CEIL, MS, lens, chans)
    out = eng.apply_curve(x, group, pg, curve, lens, chans).cpu()
    curve = curve.cpu()
    assert not torch.isnan(curve).any() and int(info["nonfinite"].sum()) == 0                  # no NaN was read
    r = 0
    for q, b in enumerate(order):
        rows, Cn, L = clips[b].shape
        a_curve, a_info, a_out = alone[b]
        assert torch.equal(curve[q, :L], a_curve[0]), f"item {b} at group {q}"
        assert bool((curve[q, L:] == 1.0).all())
        for k in ("min_gain", "limited_samples", "nonfinite"):
            assert torch.equal(info[k][q:q + 1], a_info[k]), (b, k)
        assert torch.equal(out[r:r + rows, :Cn, :L], a_out), f"item {b}"
        assert bool((out[r:r + rows, :, L:] == 0.0).all()) and bool((out[r:r + rows, Cn:] == 0.0).all())
        r += rows
    return curve, out


def test_ragged_mixed_rate_batch_gives_each_item_its_own_bits(eng, ragged):
    clips, pre, alone = ragged
    order = list(range(len(ITEMS)))
    a = run_batch(eng, clips, pre, alone, order)
    b = run_batch(eng, clips, pre, alone, order)                                               # .. and a second call
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_permuted_batch(eng, ragged):
    clips, pre, alone = ragged
    run_batch(eng, clips, pre, alone, [4, 2, 0, 5, 3, 1])


def test_base_pointer_one_float_off(eng, ragged):
    clips, pre, alone = ragged
    for b in (0, 1, 3):
        c = clips[b]
        rows = c.shape[0]
        flat = torch.full((c.numel() + 5,), float("nan"), device="cuda")
        dst = torch.full((c.numel() + 5,), float("nan"), device="cuda")
        for off in (1, 2, 3):
            v = flat[off:off + c.numel()].view(c.shape)
            v.copy_(c)
            assert v.data_ptr() % 16 == (flat.data_ptr() + 4 * off) % 16 and v.is_contiguous()
            curve, info = eng.limiter_curve(v, ITEMS[b][0], [0] * rows, [pre[b]], CEIL, MS)
            assert torch.equal(curve.cpu(), alone[b][0]), f"item {b}, {off} floats off"
            o = dst[off:off + c.numel()].view(c.shape)
            assert eng.apply_curve(v, [0] * rows, [pre[b]], curve, out=o) is o
            assert torch.equal(o.cpu(), alone[b][2]), f"item {b}, {off} floats off"


@pytest.mark.parametrize("L", [1, 1003, 4096, 2 * 4096 + 6])
def test_apply_curve_is_two_float32_products(eng, L):
    R, Cn, G = 5, 2, 3
    gen = torch.Generator().manual_seed(L)
    x = torch.randn((R, Cn, L), generator=gen).cuda()
    curve = torch.rand((G, L), generator=gen).cuda()
    lens = [L, max(1, L - 1), max(1, L // 2 + 1), 1, max(1, L - 5)]
    chans = [2, 1, 2, 1, 2]
    group = [2, 0, 0, 1, 2]                                                      # any order
    pg = torch.tensor([0.5, 1.2345678, 3.0e-3], dtype=torch.float32)
    want = (x * pg.cuda()[group][:, None, None]) * curve[group][:, None, :]
    for r in range(R):
        want[r, :, lens[r]:] = 0.0
        want[r, chans[r]:] = 0.0
    xn = x.clone()
    for r in range(R):                                                           # nothing there may be read
        xn[r, :, lens[r]:] = float("nan")
        xn[r, chans[r]:] = float("nan")
    assert torch.equal(eng.apply_curve(xn, group, pg.tolist(), curve, lens, chans), want)
    inplace = xn.clone()
    assert eng.apply_curve(inplace, group, pg.tolist(), curve, lens, chans, out=inplace) is inplace
    assert torch.equal(inplace, want)
    flat = torch.zeros(G * L + 3, device="cuda")                                 # the curve one float off
    cv = flat[1:1 + G * L].view(G, L)
    cv.copy_(curve)
    assert torch.equal(eng.apply_curve(xn, group, pg.tolist(), cv, lens, chans), want)


@pytest.mark.parametrize("Cn", [1, 2])
def test_linked_stems_sum_to_the_curve_applied_to_their_sum(eng, Cn):
    """stems on a power-of-two grid, so that their sums and every product with a power-of-two pre-gain are exact before
    the curve: each limited stem is fl(y_i g), and the sum of those is within the product roundings of fl(y g)"""
    fs, ms = WINDOWS[80]
    n, L = 4, TILE + 300
    gen = torch.Generator().manual_seed(17 + Cn)
    stems = torch.randint(-2 ** 10, 2 ** 10, (n, Cn, L), generator=gen).float() * 2.0 ** -13   # |.| < 1/8
    stems[1, 0, TILE - 3] = 0.75
    stems[2, Cn - 1, 77] = -0.625
    mixture = stems.sum(0, keepdim=True)
    assert torch.equal(mixture.double(), stems.double().sum(0, keepdim=True))                   # the sums are exact
    curve, info = eng.limiter_curve(stems, fs, [0] * n, [2.0], CEIL, ms)
    assert float(info["min_gain"][0]) < 1.0
    out = eng.apply_curve(stems, [0] * n, [2.0], curve).cpu().double()
    mix_out = eng.apply_curve(mixture, [0], [2.0], curve).cpu().double()
    g = curve[0].cpu().double()
    # where g == 1 the sum is exact; elsewhere every one of the n + 1 products is off by at most half an ulp
    slack = 2.0 ** -24 * ((2.0 * stems.abs().double()).sum(0) * g + (2.0 * mixture[0].abs().double()) * g)
    diff = (out.sum(0) - mix_out[0]).abs()
    assert bool((diff <= slack).all())
    assert bool((diff[..., g == 1.0] == 0.0).all()) and bool((g == 1.0).any())


def test_nonfinite_samples_are_counted_and_the_curve_is_nan(eng):
    fs, ms = WINDOWS[80]
    x = with_peaks(bed(5, 2, 2, TILE + 9), [50])
    y = x.clone()
    y[1, 1, TILE + 2] = float("nan")
    y[0, 0, 17] = float("inf")
    both = torch.cat([y, x])
    curve, info = eng.limiter_curve(both, fs, [0, 0, 1, 1], [1.0, 1.0], CEIL, ms)
    assert info["nonfinite"].tolist() == [2, 0] and math.isnan(float(info["min_gain"][0]))
    assert bool(torch.isnan(curve[0]).all()) and not bool(torch.isnan(curve[1]).any())
    alone, _ = eng.limiter_curve(x, fs, [0, 0], [1.0], CEIL, ms)                                 # the other group is unharmed
    assert torch.equal(curve[1], alone[0])


# ---------------------------------------------------------------------------------------------- refusals, by name
def test_library_refusals(eng):
    lib = eng.lib
    x = torch.zeros((2, 2, 100), device="cuda")
    cv = torch.zeros((2, 100), device="cuda")
    stats = (C.c_double * 6)()
    i32 = C.c_int32 * 2
    f32 = C.c_float * 2
    ok = dict(x=C.c_void_p(x.data_ptr()), R=2, Cn=2, L=100, lens=i32(100, 100), ch=i32(2, 1), rates=i32(8000, 8000),
              group=i32(0, 0), G=1, pg=f32(1.0, 1.0), c=0.9, ms=5.0, curve=C.c_void_p(cv.data_ptr()))

    def call(**kw):
        a = dict(ok, **kw)
        rc = lib.dsn_limiter_curve(eng.ctx, a["x"], a["R"], a["Cn"], a["L"], a["lens"], a["ch"], a["rates"], a["group"],
                                   a["G"], a["pg"], a["c"], a["ms"], a["curve"], None, stats, None)
        return rc, lib.dsn_last_error(eng.ctx).decode()

    rc, _ = call()
    assert rc == 0
    before = eng.workspace_bytes()
    for kw, msg in [(dict(x=None), "null"), (dict(rates=None), "null"), (dict(group=None), "null"),
                    (dict(pg=None), "null"), (dict(curve=None), "null"), (dict(R=0), "outside [1, 65535]"),
                    (dict(Cn=3), "C = 3"), (dict(ch=i32(2, 3)), "channels[1] = 3"), (dict(lens=i32(100, 101)), "lens[1] = 101"),
                    (dict(rates=i32(7999, 7999)), "rates[0] = 7999"), (dict(L=2 ** 30 + 1), "Lmax"),
                    (dict(G=0), "0 groups"), (dict(G=3), "every group needs a row"),
                    (dict(group=i32(0, 1)), "group[1] = 1 outside"), (dict(group=i32(1, 1), G=2), "non-decreasing"),
                    (dict(group=i32(0, 0), G=2), "not G - 1"), (dict(group=i32(1, 0), G=2), "non-decreasing"),
                    (dict(lens=i32(100, 99)), "disagree on length or rate"),
                    (dict(rates=i32(8000, 16000)), "disagree on length or rate"),
                    (dict(c=0.0), "ceiling"), (dict(c=-1.0), "ceiling"), (dict(c=math.inf), "ceiling"),
                    (dict(c=math.nan), "ceiling"), (dict(ms=128.125), "half-window"), (dict(ms=-1.0), "half-window"),
                    (dict(ms=math.nan), "not finite"), (dict(pg=f32(math.inf, 1.0)), "pregain[0]")]:
        rc, err = call(**kw)
        assert rc == -1 and "dsn_limiter_curve" in err and msg in err, (kw, rc, err)
    assert eng.workspace_bytes() == before                       # nothing was allocated
    rc, _ = call(lens=None, ch=None)
    assert rc == 0
    rc, _ = call(group=i32(0, 1), G=2, lens=i32(100, 50), rates=i32(8000, 192000), ms=128.0 / 24.0)   # W = 1024 at 192 kHz
    assert rc == 0

    def apply(**kw):
        a = dict(dict(ok, out=C.c_void_p(x.data_ptr())), **kw)
        rc = lib.dsn_apply_curve(eng.ctx, a["x"], a["R"], a["Cn"], a["L"], a["lens"], a["ch"], a["group"], a["G"],
                                 a["pg"], a["curve"], a["out"], None)
        return rc, lib.dsn_last_error(eng.ctx).decode()

    assert apply()[0] == 0 and apply(group=i32(1, 0), G=2)[0] == 0
    for kw, msg in [(dict(curve=None), "null"), (dict(group=None), "null"), (dict(pg=None), "null"),
                    (dict(out=C.c_void_p(x.data_ptr() + 4)), "overlaps"), (dict(group=i32(0, 1)), "group[1] = 1 outside"),
                    (dict(group=i32(-1, 0)), "group[0] = -1 outside"), (dict(G=0), "0 groups"), (dict(Cn=3), "C = 3")]:
        rc, err = apply(**kw)
        assert rc == -1 and "dsn_apply_curve" in err and msg in err, (kw, rc, err)
