"""dsn_activity and dsn_activity_gate (ditsep_amd/csrc/activity.hip) through Engine.activity and Engine.activity_gate on
an engine with no score network and no codec, against tests/activity_restatement.py.

Bounds.  The band energies are the only floating-point result that is compared with a tolerance: the device's largest
|E - E64| relative to the item's largest E is at most 8 x that of the float32 CPU run of the same restatement, the
project's standing allowance for another float32 FFT (tests/test_gpu_mask_refine.py).  Everything after the energies is
bit for bit: the restatement's `decide`, in both of its forms, applied to the device's own energies gives the device's
level and act exactly; with the restatement's float64 energies the decisions agree exactly on inputs whose every
comparison is at least 1e-3 away from its threshold (a condition asserted on the input, not a tolerance); the gate
equals the restatement's; ragged, permuted and repeated calls give each item the bits it has alone."""
import numpy as np
import pytest
import torch

from ditsep_amd import native
from tests import activity_restatement as ar
from tests import beamform_restatement as br
from tests.util import make_engine

pytestmark = pytest.mark.gpu

FACTOR = 8.0
# (n_fft, hop, n, L): at 64 / 16 a frame group is 32 frames -- n_fft / 2 + 1 samples, one group - 1, exactly, + 1, three
# groups and a partial hop --, then the default transform and the largest
SHAPES = [(64, 16, 1, 33), (64, 16, 2, 470), (64, 16, 4, 481), (64, 16, 2, 497), (64, 16, 4, 16 * 96 + 5),
          (512, 128, 2, 32000), (2048, 512, 2, 5 * 512 + 100)]
# (half_width, min_on, min_off, pad)
RULES = [(2, 6, 6, 0), (0, 1, 1, 0), (7, 13, 13, 3), (2, 1, 13, 3), (0, 13, 1, 0), (7, 6, 1, 3)]
FS = 16000


@pytest.fixture(scope="module")
def eng():
    e = make_engine()
    assert e.cfg.score_kind == native.SCORE_NONE
    yield e
    e.close()


def bands_of(n_fft):
    """the full band, a one-bin band and the default, in Hz at FS"""
    one = 5.0 * FS / n_fft
    return [(0.0, FS / 2.0), (one, one), (100.0, 4000.0)]


def run(eng, est, **kw):
    """est [n, L] numpy -> the item's (act [n, F], frames_on [n], energy [n, F], level [n, F]) as numpy"""
    res = eng.activity(torch.from_numpy(est)[None], fs=FS, **kw)
    F = res["frames"][0]
    assert res["act"].dtype == torch.uint8 and res["frames_on"].dtype == torch.int32
    assert res["energy"].dtype == res["level"].dtype == torch.float64
    assert F == 1 + -(-est.shape[1] // kw.get("hop", 128)) == res["act"].shape[-1]
    return tuple(res[k][0].cpu().numpy() for k in ("act", "frames_on", "energy", "level"))


def check_decision(act, on, E, lev, hw, mon, moff, pad, what):
    want, wlev, _ = ar.decide_both(E, half_width=hw, consts=ar.constants(), min_on=mon, min_off=moff, pad=pad)
    assert np.array_equal(lev, wlev, equal_nan=True), f"{what}: level"
    assert np.array_equal(act, want), f"{what}: act differs in {int((act != want).sum())} frames"
    assert np.array_equal(on, want.sum(axis=1)), f"{what}: frames_on"


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(str(v) for v in s))
def test_energies_against_float64(eng, shape):
    """The device's largest |E - E64| relative to the item's largest E64, against 8 x that of the float32 CPU run of the
    restatement (torch.stft in float32, as tests/test_gpu_mask_refine.py takes it).  Both runs carry the same kind of
    error on a band of many bins: a radix-2 twiddle table rounded once to float32 by itself -- every other operation
    exact in float64 -- biases a frame's energy by -5.8e-08 at 2048 and -6.4e-08 at 512 points, so the error does not
    average out over the bins.  Measured on an MI355X (device error / float32 CPU
    error): at most 1.59 at 64 / 16, 1.32 at 512 / 128 and 2.09 at 2048 / 512 (one bin: 2.6e-07 against 1.3e-07; the
    full band there 7.6e-08 against 5.2e-08)."""
    n_fft, hop, n, L = shape
    est = ar.burst_case(n_fft + 3 * n + L, n, L, hop)
    worst, missed = 0.0, []
    for band in bands_of(n_fft):
        bins = ar.band_bins(band, FS, n_fft)
        E64 = ar.energies(est, n_fft, hop, bins)
        E32 = ar.energies(est, n_fft, hop, bins, dtype=np.float32)
        _, _, E, _ = run(eng, est, n_fft=n_fft, hop=hop, band=band)
        e_dev = np.max(np.abs(E - E64)) / np.max(E64)
        e_cpu = np.max(np.abs(E32 - E64)) / np.max(E64)
        what = f"n_fft {n_fft} hop {hop} n {n} L {L} bins {bins}"
        print(f"{what}: energy error {e_dev:.3e} (float32 CPU {e_cpu:.3e}, ratio {e_dev / e_cpu:.2f})")
        worst = max(worst, e_dev / e_cpu)
        if not e_dev <= FACTOR * e_cpu:
            missed.append(f"{what}: {e_dev / e_cpu:.2f} x the float32 CPU error")
    print(f"{shape}: worst energy ratio {worst:.2f} (allowed {FACTOR})")
    assert not missed, missed


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(str(v) for v in s))
def test_decisions_bit_for_bit(eng, shape):
    """`decide`, in both forms, on the device's own energies gives the device's level, act and frames_on exactly"""
    n_fft, hop, n, L = shape
    est = ar.burst_case(n_fft + 3 * n + L, n, L, hop)
    for band in bands_of(n_fft):
        first = None
        for hw, mon, moff, pad in RULES:
            act, on, E, lev = run(eng, est, n_fft=n_fft, hop=hop, band=band, half_width=hw, min_on=mon, min_off=moff,
                                  pad=pad)
            what = f"n_fft {n_fft} hop {hop} n {n} L {L} band {band} rules {(hw, mon, moff, pad)}"
            first = E if first is None else first
            assert np.array_equal(E, first), f"{what}: the energies depend on the decision's parameters"
            check_decision(act, on, E, lev, hw, mon, moff, pad, what)


def test_chunked_scans(eng):
    """more than 256 x 8 frames: a thread's chunk is 9 frames, so every scan crosses chunk and summary boundaries and
    the runs (1 to 40 frames) straddle chunk edges"""
    L = 16 * 2100 + 3
    est = ar.burst_case(5, 2, L, 16)
    for hw, mon, moff, pad in RULES:
        act, on, E, lev = run(eng, est, n_fft=64, hop=16, half_width=hw, min_on=mon, min_off=moff, pad=pad)
        assert act.shape[1] == 2102 and 0 < act.sum() < act.size
        check_decision(act, on, E, lev, hw, mon, moff, pad, f"long item, rules {(hw, mon, moff, pad)}")


def test_silence_and_nan(eng):
    est = np.zeros((2, 1000), np.float32)
    act, on, E, lev = run(eng, est, n_fft=64, hop=16)
    assert not act.any() and not on.any() and not E.any() and not lev.any()
    est = ar.burst_case(9, 2, 3000, 16)
    est[1, 1500] = np.nan
    for hw, mon, moff, pad in RULES[:3]:
        act, on, E, lev = run(eng, est, n_fft=64, hop=16, half_width=hw, min_on=mon, min_off=moff, pad=pad)
        assert np.isnan(E[1]).any() and not np.isnan(E[0]).any() and act.any()
        check_decision(act, on, E, lev, hw, mon, moff, pad, f"one NaN sample, rules {(hw, mon, moff, pad)}")


def margin_ok(ratios):
    return bool(np.all(np.abs(ratios - 1.0) > 1e-3))


# (n_fft, hop, n, L, seed): seeds whose closest comparison is 6.5e-2 and 1.8e-2 away from its threshold
SMALL = [(64, 16, 2, 1541, 1), (64, 16, 4, 3000, 4)]


@pytest.mark.parametrize("leak", [0.3, 0.1])
def test_end_to_end_sanity_case(eng, leak):
    _, est, _ = br.sanity_case(leak=leak)
    bins = ar.band_bins((100.0, 4000.0), FS, 512)
    want, _, ratios = ar.decide_both(ar.energies(est, 512, 128, bins), half_width=2, consts=ar.constants(), min_on=6,
                                     min_off=6, pad=0)
    assert margin_ok(ratios), "the input has a comparison within 1e-3 of its threshold"
    act, on, _, _ = run(eng, est, half_width=2, min_on=6, min_off=6)
    assert np.array_equal(act, want) and np.array_equal(on, want.sum(axis=1))


@pytest.mark.parametrize("case", SMALL, ids=lambda s: "x".join(str(v) for v in s))
def test_end_to_end_small(eng, case):
    n_fft, hop, n, L, seed = case
    est = ar.burst_case(seed, n, L, hop)
    bins = ar.band_bins((100.0, 4000.0), FS, n_fft)
    want, _, ratios = ar.decide_both(ar.energies(est, n_fft, hop, bins), half_width=2, consts=ar.constants(), min_on=6,
                                     min_off=6, pad=0)
    assert margin_ok(ratios), "the input has a comparison within 1e-3 of its threshold"
    act, on, _, _ = run(eng, est, n_fft=n_fft, hop=hop, half_width=2, min_on=6, min_off=6)
    assert want.any() and not want.all()
    assert np.array_equal(act, want) and np.array_equal(on, want.sum(axis=1))


# ------------------------------------------------------------------ the gate
def random_rows(g, n, F, lo=1, hi=12):
    act = np.zeros((n, F), np.uint8)
    for i in range(n):
        p, on = 0, bool(g.integers(2))
        while p < F:
            q = p + int(g.integers(lo, hi))
            act[i, p:q] = on
            p, on = q, not on
    return act


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("fade", [0, 1, 80, 4096])
@pytest.mark.parametrize("hop,L", [(128, 9001), (16, 4099), (128, 16384)])
def test_gate_bit_for_bit(eng, fade, hop, L):
    """ramps that overlap (gaps of 1 to 11 frames against fades of up to 4096 samples) and ramps cut by both ends; a
    NaN and a -0 inside a segment stay, a NaN further than `fade` from every segment becomes +0"""
    g = np.random.default_rng(fade + hop + L)
    n, F = 2, 1 + -(-L // hop)
    act = random_rows(g, n, F)
    act[1, :] = 0
    act[1, F // 2:F // 2 + 2] = 1                                # one short segment: both ramps run out (or hit the ends)
    x = g.standard_normal((n, L)).astype(np.float32)
    fr = (np.arange(L) + hop // 2) // hop
    inside = act[:, fr] != 0
    a0 = np.flatnonzero(inside[0])
    x[0, a0[len(a0) // 2]] = np.nan
    x[0, a0[len(a0) // 3]] = -0.0
    far = np.flatnonzero(~inside[1] & (np.abs(np.arange(L) - np.flatnonzero(inside[1]).mean()) > fade + 2 * hop))
    if len(far):
        x[1, far[0]] = np.nan
    out = eng.activity_gate(torch.from_numpy(x)[None], torch.from_numpy(act)[None].cuda(), hop=hop, fade=fade)
    out = out[0].cpu().numpy()
    want = np.stack([ar.gate(x[i], act[i], hop, fade) for i in range(n)])
    assert np.array_equal(bits(out), bits(want))
    assert np.array_equal(bits(out[inside]), bits(x[inside]))
    if len(far):
        assert bits(out[1, far[0]:far[0] + 1])[0] == 0
    if fade == 0:
        assert not bits(out[~inside]).any()


def test_gate_unaligned_and_ragged(eng):
    """a base pointer that is 4-byte aligned only, L % 4 != 0, and a NaN-padded batch against each item alone"""
    g = np.random.default_rng(3)
    n, L, hop, fade = 2, 4099, 16, 80
    lens = [4099, 1030, 33]
    F = 1 + -(-L // hop)
    act = np.stack([random_rows(g, n, F) for _ in lens])
    x = g.standard_normal((len(lens), n, L)).astype(np.float32)
    for b, v in enumerate(lens):
        x[b, :, v:] = np.nan
    buf = torch.full((x.size + 1,), float("nan"), device="cuda")
    xd = buf[1:].view(len(lens), n, L)
    xd.copy_(torch.from_numpy(x))
    assert xd.data_ptr() % 16 == 4
    out = eng.activity_gate(xd, torch.from_numpy(act).cuda(), lens=lens, hop=hop, fade=fade).cpu().numpy()
    again = eng.activity_gate(torch.from_numpy(x), torch.from_numpy(act), lens=lens, hop=hop, fade=fade).cpu().numpy()
    assert np.array_equal(bits(out), bits(again))
    for b, v in enumerate(lens):
        want = np.stack([ar.gate(x[b, i, :v], act[b, i], hop, fade) for i in range(n)])
        assert np.array_equal(bits(out[b, :, :v]), bits(want)) and not bits(out[b, :, v:]).any()
        Fb = 1 + -(-v // hop)
        alone = eng.activity_gate(torch.from_numpy(x[b:b + 1, :, :v].copy()), torch.from_numpy(act[b:b + 1, :, :Fb].copy()),
                                  hop=hop, fade=fade).cpu().numpy()
        assert np.array_equal(bits(alone[0]), bits(out[b, :, :v]))


# ------------------------------------------------------------------ invariances
def test_ragged_permuted_and_repeated(eng):
    n, hop, n_fft = 2, 16, 64
    lens = [3000, 33, 16 * 600 + 7, 1541]
    L = max(lens)
    ests = [ar.burst_case(20 + b, n, v, hop) for b, v in enumerate(lens)]
    x = np.full((len(lens), n, L), np.nan, np.float32)
    for b, e in enumerate(ests):
        x[b, :, :e.shape[1]] = e
    kw = dict(fs=FS, n_fft=n_fft, hop=hop, half_width=2, min_on=6, min_off=6, pad=1)
    keys = ("act", "frames_on", "energy", "level")
    buf = torch.full((x.size + 1,), float("nan"), device="cuda")
    xd = buf[1:].view(x.shape)
    xd.copy_(torch.from_numpy(x))
    res = eng.activity(xd, lens=lens, **kw)
    assert res["frames"] == [1 + -(-v // hop) for v in lens]
    got = {k: res[k].cpu().numpy() for k in keys}
    rerun = eng.activity(torch.from_numpy(x), lens=lens, **kw)
    for k in keys:
        assert np.array_equal(got[k], rerun[k].cpu().numpy(), equal_nan=True), k
    perm = [2, 0, 3, 1]
    shuffled = eng.activity(torch.from_numpy(x[perm]), lens=[lens[p] for p in perm], **kw)
    for k in keys:
        assert np.array_equal(got[k][perm], shuffled[k].cpu().numpy(), equal_nan=True), k
    gated = eng.activity_gate(torch.from_numpy(x), res["act"], lens=lens, hop=hop, fade=8).cpu().numpy()
    for b, e in enumerate(ests):
        alone = eng.activity(torch.from_numpy(e)[None], **kw)
        F = alone["frames"][0]
        for k in keys:
            a, full = alone[k][0].cpu().numpy(), got[k][b]
            assert np.array_equal(a, full[..., :F] if k != "frames_on" else full), (b, k)
            if k != "frames_on":
                assert not full[..., F:].any(), (b, k)
        act = got["act"][b]
        assert np.array_equal(got["frames_on"][b], act.sum(axis=1))
        want = np.stack([ar.gate(e[i], act[i], hop, 8) for i in range(n)])
        assert np.array_equal(bits(gated[b, :, :lens[b]]), bits(want))


def test_refusals_reach_the_library_by_name(eng):
    x = torch.zeros(1, 2, 1000)
    lib, ctx = eng.lib, eng.ctx
    act = torch.zeros(1, 2, 64, dtype=torch.uint8, device="cuda")
    out = torch.zeros(1, 2, 1000, device="cuda")
    xd = x.cuda()
    rc = lib.dsn_activity_gate(ctx, native._ptr(xd), native._ptr(act), 1, 2, 1000, 8, None, 16, 0, None, native._ptr(out),
                               None)
    assert rc != 0 and b"act holds 8 frames per row, 63 needed" in lib.dsn_last_error(ctx)
    with pytest.raises(ValueError, match=r"activity: 4194305 frames \(L = 33554432, hop = 8\) > 2\^22 per item"):
        native.check_activity((1, 1, 1 << 25), n_fft=64, hop=8)
