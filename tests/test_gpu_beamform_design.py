"""The rank-one MVDR and GEV weights (ditsep_amd/csrc/beamform_design.hip) through Engine.beamform(design=) and
Engine.beamform_solve on an engine with no score network and no codec, against tests/beamform_design_restatement.py.

Bounds.  The yardstick of tests/test_gpu_beamform.py: the device's worst output error (of the mixture's peak) and worst
weight error (of the largest weight) against the float64 restatement may be at most 8 x those of the float32-CPU run of
the same restatement on the same input.  Every parity case first asserts two conditions on the restatement: every bin
carries at least 1e-6 of the strongest bin's power, and every (source, bin) has a relative eigenvalue gap
(mu_1 - mu_2) / mu_1 >= 1e-2 (below that the eigenvector, and with it both filters, is ill-conditioned: an error of the
statistics is magnified by 1 / gap).  Silent estimates with n >= 2 cannot meet the second condition -- every class has
the statistics N / n, so G = L^-1 N_i L^-H is (n - 1)^-1 I up to the loading and its gap is of the order of reg --;
they are checked bit for bit instead (n equal outputs), and the kind enters the parity cases with n = 1.
dsn_beamform_solve runs on float64 statistics from the restatement: two fp64 routes to the same weights, held to 1e-10
of the largest weight (the allowance of tests/test_gpu_beamform.py's Cholesky against numpy.linalg.solve).  The
device's own statistics are not handed out by any call, so "Souden on the same statistics" is checked in two halves:
design="souden" through the new entry points has the bits of today's calls, info_w included, and dsn_beamform_solve
with DSN_BEAMFORM_DESIGN_SOUDEN is held to the restatement's Souden weights on the float64 statistics.
Everything else is bit for bit.

Measured on an MI355X: see the README paragraph "Beamformer designs"."""
import numpy as np
import pytest
import torch

from ditsep_amd import native
from tests import beamform_design_restatement as bd
from tests import beamform_restatement as br
from tests.test_gpu_beamform import FACTOR, off_alignment, ratio, same_bits
from tests.test_gpu_mask_refine import span_of
from tests.util import make_engine

pytestmark = pytest.mark.gpu
DESIGNS = ("rank1", "gev")
E32, R32 = float(np.float32(1e-10)), float(np.float32(1e-3))


@pytest.fixture(scope="module")
def eng():
    e = make_engine()
    assert e.cfg.score_kind == native.SCORE_NONE
    yield e
    e.close()


# ------------------------------------------------------------------ 1. parity with the restatement
def conditions(mix, est, what, n_fft, hop, power=2):
    """the two conditions of the module docstring, on the float64 restatement"""
    N = bd.item_statistics(mix, est, n_fft=n_fft, hop=hop, power=power)
    p = np.einsum("nfcc->f", N).real
    assert p.min() >= 1e-6 * p.max() > 0, f"{what}: a bin of the input carries no signal"
    gap = float(bd.gaps(N, est.shape[0], E32, R32).min())
    assert gap >= 1e-2, f"{what}: eigenvalue gap {gap:.2e} < 1e-2"
    return gap


def check(eng, mix, est, what, design, sweeps=10, **kw):
    gap = conditions(mix, est, what, kw.get("n_fft", 512), kw.get("hop", 128))
    ref, iref = bd.beamform(mix, est, design=design, sweeps=sweeps, return_info=True, **kw)
    cpu, icpu = bd.beamform(mix, est, design=design, sweeps=sweeps, dtype=np.float32, return_info=True, **kw)
    m = off_alignment(torch.from_numpy(mix)[None], eng.device)
    e = off_alignment(torch.from_numpy(est)[None], eng.device)
    out, info = eng.beamform(m, e, return_info=True, design=dict(kind=design, sweeps=sweeps), **kw)
    out, w = out[0].cpu().numpy(), info["w"][0].numpy()
    assert out.shape == ref.shape and w.shape == iref["w"].shape
    assert np.all(np.isfinite(out)) and np.all(np.isfinite(w))
    top = float(np.max(np.abs(iref["w"])))
    rel = lambda a: float(np.max(np.abs(a - iref["w"])) / top)
    pairs = {"parity": (br.rel_err(out, ref, mix), br.rel_err(cpu, ref, mix)), "w": (rel(w), rel(icpu["w"]))}
    print(f"{what} {design} sweeps {sweeps} (gap {gap:.3f}): "
          + "; ".join(f"{k} {d:.3e} (float32 CPU {c:.3e}, ratio {ratio(d, c):.2f})" for k, (d, c) in pairs.items()))
    for k, (d, c) in pairs.items():
        assert d <= FACTOR * c, f"{what} {design}: {k} {ratio(d, c):.2f} x the float32 CPU error"


SMALL = dict(n_fft=64, hop=16)
# (what, make_case arguments (seed, kind, n, C, L), keywords): C = 3 leaves empty lanes, 8 x 4 fills them with the last
# channel as the reference, n = 1 has Q = 0 and A = eps I, 33 samples are one reflection of n_fft = 64
CASES = (("2x2", (3, "generic", 2, 2, 700), SMALL), ("3x3", (3, "generic", 3, 3, 700), dict(SMALL, ref=2)),
         ("8x4", (3, "generic", 4, 8, 6000), dict(ref=7)), ("4x1", (3, "generic", 1, 4, 700), dict(SMALL, ref=1)),
         ("shortest", (1, "generic", 2, 2, 33), SMALL), ("dual", (1, "dual", 2, 3, 700), SMALL),
         ("hard", (1, "hard", 2, 4, 700), dict(SMALL, ref=3)), ("silent_ch", (1, "silent_ch", 2, 4, 700), SMALL),
         ("silent_est", (3, "silent_est", 1, 4, 700), SMALL))


@pytest.mark.parametrize("design", DESIGNS)
@pytest.mark.parametrize("what,case,kw", CASES, ids=[c[0] for c in CASES])
def test_against_the_restatement(eng, what, case, kw, design):
    mix, est = br.make_case(*case)
    check(eng, mix, est, what, design, **kw)


@pytest.mark.parametrize("design", DESIGNS)
def test_one_sweep_against_one_sweep(eng, design):
    """an iteration that has not converged is still the same iteration"""
    for what, case, kw in CASES[:2]:
        mix, est = br.make_case(*case)
        check(eng, mix, est, what, design, sweeps=1, **kw)


# ------------------------------------------------------------------ 2. the solver alone, in pure fp64
def solve_case(seed, chans, n, classes, L=700):
    """per item the float64 statistics of a make_case mixture with `classes` estimates -> (N packed for Cmax =
    max(chans), the items' statistics)"""
    Cmax = max(chans)
    stats = [bd.item_statistics(*br.make_case(seed + b, "generic", classes, c, L), **SMALL) for b, c in enumerate(chans)]
    return torch.from_numpy(np.stack([bd.pack(N, Cmax) for N in stats])), stats


@pytest.mark.parametrize("design", DESIGNS + ("souden",))
@pytest.mark.parametrize("extra", [0, 1])
def test_solve_on_float64_statistics(eng, design, extra):
    """C in {1, 2, 3, 5, 8} as the batch's width with every item at full width, then a ragged channel list whose
    missing entries hold NaN; classes = n and n + 1"""
    n = 2
    for chans in ((1,), (2, 2), (3,), (5, 5), (8,), (8, 1, 3, 5, 2)):
        packed, stats = solve_case(11 + len(chans) + chans[0], chans, n, n + extra)
        Cmax, ref = max(chans), 0 if min(chans) == 1 else min(chans) - 1
        ragged = len(set(chans)) > 1
        w = eng.beamform_solve(packed, n=n, channels=list(chans) if ragged else None, ref=ref, design=design).cpu().numpy()
        assert w.shape == (len(chans), n, 33, Cmax)
        for b, (c, N) in enumerate(zip(chans, stats)):
            want = bd.design_weights(N, n, ref, E32, R32, design)
            top = float(np.abs(want).max())
            err = float(np.abs(w[b, :, :, :c] - want).max()) / top
            print(f"{design} classes n + {extra} chans {chans} item {b}: {err:.2e} of the largest weight")
            assert err <= 1e-10, (design, chans, b, err)
            assert np.all(w[b, :, :, c:] == 0)
            if c == 1:
                assert np.all(w[b, :, :, 0] == 1.0)
        again = eng.beamform_solve(packed.flip(0).contiguous(), n=n, channels=list(chans)[::-1] if ragged else None,
                                   ref=ref, design=design)
        assert torch.equal(torch.view_as_real(again.flip(0)).cpu(), torch.view_as_real(torch.from_numpy(w)))


def test_solve_refusals(eng):
    N = torch.zeros((1, 2, 6, 33), dtype=torch.float64)
    for kw, msg in ((dict(design="mvdr"), "design must be"), (dict(design=dict(sweeps=0)), r"sweeps = 0 outside \[1, 30\]"),
                    (dict(design=dict(sweeps=31)), r"sweeps = 31 outside \[1, 30\]"), (dict(n=3), "classes = 2 is not"),
                    (dict(ref=2), r"ref = 2 outside \[0, 2\)"), (dict(reg=-1.0), "reg = -1.0 is not a finite number"),
                    (dict(eps=0.0), "eps = 0.0 is not a finite positive number")):
        with pytest.raises(ValueError, match=msg):
            eng.beamform_solve(N, **kw)
    with pytest.raises(ValueError, match="float64 tensor"):
        eng.beamform_solve(N.float())
    with pytest.raises(ValueError, match="planes per class"):
        eng.beamform_solve(torch.zeros((1, 2, 5, 33), dtype=torch.float64))
    i32 = (native.C.c_int32 * 1)(2)
    dev = N.to(eng.device)
    w = torch.full((1, 2, 33, 2), 7.0, dtype=torch.complex128, device=eng.device)
    call = lambda design, sweeps, classes=2: eng.lib.dsn_beamform_solve(
        eng.ctx, native._ptr(dev), i32, 0, 1, 2, 2, classes, 33, 1e-3, 1e-10, design, sweeps, native._ptr(w),
        eng._stream())
    for args, msg in (((3, 10), "design = 3 is not one of 0 (DSN_BEAMFORM_DESIGN_SOUDEN)"),
                      ((1, 0), "sweeps = 0 outside [1, 30]"), ((2, 31), "sweeps = 31 outside [1, 30]"),
                      ((1, 10, 4), "classes = 4 is not n = 2 or n + 1")):
        assert call(*args) != 0
        assert msg in eng.lib.dsn_last_error(eng.ctx).decode(), eng.lib.dsn_last_error(eng.ctx).decode()
    # more systems than one launch takes: refused before anything is read (items n bins = 2^23 x 2 x 1025)
    assert eng.lib.dsn_beamform_solve(eng.ctx, native._ptr(dev), None, 0, 1 << 23, 2, 2, 2, 1025, 1e-3, 1e-10, 1, 10,
                                      native._ptr(w), eng._stream()) != 0
    assert "systems, more than the 2^31 one launch takes" in eng.lib.dsn_last_error(eng.ctx).decode()
    torch.cuda.synchronize()
    assert bool((w == 7.0).all())


# ------------------------------------------------------------------ 3. exact cases
@pytest.mark.parametrize("design", DESIGNS)
def test_one_channel_is_mask_refine(eng, design):
    """C = 1: w = 1.0 exactly for every design, so the identities of tests/test_gpu_beamform.py hold bit for bit"""
    for n_fft, hop, L in ((512, 128, 2 * span_of(512) + 301), (64, 8, 33)):
        for n in (1, 3):
            mix, est = br.make_case(n_fft + L + n, "generic", n, 1, L)
            m, e = torch.from_numpy(mix)[None].to(eng.device), torch.from_numpy(est)[None].to(eng.device)
            kw = dict(n_fft=n_fft, hop=hop)
            out, info = eng.beamform(m, e, return_info=True, design=design, **kw)
            assert bool((info["w"] == 1.0).all()), (n_fft, n)
            one = eng.mask_refine(m[:, 0], e[:, :1], **kw)
            for i in range(n):
                assert same_bits(out[:, i], one[:, 0]), (n_fft, hop, L, n, i)
            post = eng.beamform(m, e, postfilter="mask", design=design, **kw)
            assert same_bits(post, eng.mask_refine(m[:, 0], e, **kw)), (n_fft, hop, L, n)


@pytest.mark.parametrize("design", DESIGNS)
def test_silent_estimates_give_equal_outputs(eng, design):
    for n_fft, hop, L, C in ((512, 128, 1500, 4), (64, 8, 33, 8)):
        mix, _ = br.make_case(n_fft + L, "generic", 2, C, L)
        for n in (2, 4):
            out, info = eng.beamform(torch.from_numpy(mix)[None], torch.zeros((1, n, L)), n_fft=n_fft, hop=hop,
                                     ref=C - 1, design=design, return_info=True)
            assert float(out.abs().max()) > 0 and bool(torch.isfinite(out).all())
            for i in range(1, n):
                assert same_bits(out[0, i], out[0, 0]), (n_fft, n, i)
                assert torch.equal(torch.view_as_real(info["w"][0, i]), torch.view_as_real(info["w"][0, 0]))


@pytest.mark.parametrize("design", DESIGNS)
def test_nan_estimate_hands_back_the_reference_channel(eng, design):
    """a NaN in an estimate makes the masks of the frames it touches NaN, every statistic of those bins NaN, a pivot
    fails and w = e_ref"""
    mix, est = br.make_case(5, "generic", 2, 3, 700)
    est[1, 300] = np.nan
    out, info = eng.beamform(torch.from_numpy(mix)[None], torch.from_numpy(est)[None], ref=1, design=design,
                             return_info=True, **SMALL)
    want = torch.zeros(3, dtype=torch.complex128)
    want[1] = 1.0
    assert bool((info["w"][0] == want).all())
    assert bool(torch.isfinite(out).all()) and same_bits(out[0, 0], out[0, 1])


@pytest.mark.parametrize("design,n_fft,hop,n,post", [("rank1", 512, 128, 3, None), ("gev", 64, 32, 4, "mask"),
                                                     ("gev", 512, 64, 2, None), ("rank1", 64, 16, 1, "mask")])
def test_ragged(eng, design, n_fft, hop, n, post):
    """5 items of distinct lengths and mixed channel counts, one at the minimum, one over two spans, NaN past every end
    and in every channel an item does not have: each item against the item alone, a permuted batch, a rerun, a base
    pointer one float off, one item per chunk, lists"""
    S, need = span_of(n_fft), n_fft // 2 + 1
    lens = [2 * S + 3 * hop + 5, need, S, S + 1, need + hop + 2]
    chans = [4, 1, 8, 3, 5]
    Lmax, Cmax = max(lens) + 3, 8
    g = np.random.default_rng(n_fft + n)
    mix = torch.full((5, Cmax, Lmax), float("nan"))
    est = torch.full((5, n, Lmax), float("nan"))
    for b, (v, c) in enumerate(zip(lens, chans)):
        m, e = br.make_case(int(g.integers(1 << 30)), br.KINDS[b % 4], n, c, v)
        mix[b, :c, :v], est[b, :, :v] = torch.from_numpy(m), torch.from_numpy(e)
    kw = dict(n_fft=n_fft, hop=hop, postfilter=post, design=design)
    out, info = eng.beamform(mix, est, lens=lens, channels=chans, return_info=True, **kw)
    assert tuple(out.shape) == (5, n, Lmax) and not bool(torch.isnan(out).any())
    assert bool(torch.isfinite(torch.view_as_real(info["w"])).all())
    souden = eng.beamform(mix, est, lens=lens, channels=chans, n_fft=n_fft, hop=hop, postfilter=post)
    assert not same_bits(out, souden)                         # (the design reached the kernel)
    for b, (v, c) in enumerate(zip(lens, chans)):
        alone, ia = eng.beamform(mix[b:b + 1, :c, :v].contiguous(), est[b:b + 1, :, :v].contiguous(), return_info=True,
                                 **kw)
        assert same_bits(out[b, :, :v], alone[0]), f"item {b} differs from the item alone"
        assert torch.equal(torch.view_as_real(info["w"][b, :, :, :c]), torch.view_as_real(ia["w"][0]))
        assert bool((info["w"][b, :, :, c:] == 0).all())
        assert bool((out[b, :, v:] == 0).all()), f"item {b}: not zero past its end"
    perm = [3, 0, 4, 2, 1]
    again = eng.beamform(mix[perm].contiguous(), est[perm].contiguous(), lens=[lens[p] for p in perm],
                         channels=[chans[p] for p in perm], **kw)
    assert same_bits(again, out[perm])
    assert same_bits(eng.beamform(mix, est, lens=lens, channels=chans, **kw), out)
    shifted = eng.beamform(off_alignment(mix, eng.device), off_alignment(est, eng.device), lens=lens, channels=chans, **kw)
    assert same_bits(shifted, out)
    one_item = native.beamform_item_bytes(n_fft, hop, Lmax, Cmax, n)
    assert same_bits(eng.beamform(mix, est, lens=lens, channels=chans, workspace_budget=one_item, **kw), out)
    as_list = eng.beamform([mix[b, :c, :v] for b, (v, c) in enumerate(zip(lens, chans))],
                           [est[b, :, :v] for b, v in enumerate(lens)], **kw)
    for b, v in enumerate(lens):
        assert tuple(as_list[b].shape) == (n, v) and same_bits(as_list[b], out[b, :, :v])


def test_no_design_and_souden_are_todays_calls(eng):
    """design=None is today's call; design="souden" goes through the new entry points and has its bits, weights
    included, in all three calls"""
    mix, est = br.make_case(9, "generic", 2, 4, 1500)
    m, e = torch.from_numpy(mix)[None].to(eng.device), torch.from_numpy(est)[None].to(eng.device)
    for call, kw in ((eng.beamform, dict(postfilter="mask")), (eng.beamform_spatial, dict(iterations=2)),
                     (eng.beamform_track, dict(block_frames=4, context=1))):
        base, ib = call(m, e, return_info=True, **kw)
        for design in (None, "souden", dict(kind="souden", sweeps=3)):
            out, info = call(m, e, return_info=True, design=design, **kw)
            assert same_bits(out, base), (call.__name__, design)
            assert torch.equal(torch.view_as_real(info["w"]), torch.view_as_real(ib["w"])), (call.__name__, design)
        assert not same_bits(call(m, e, design="rank1", **kw), base)


def test_refusals_launch_nothing(eng):
    mix, est = torch.zeros((1, 3, 600), device=eng.device), torch.zeros((1, 2, 600), device=eng.device)
    out = torch.full((1, 2, 600), 7.0, device=eng.device)
    for design, sweeps, msg in ((3, 10, "design = 3 is not one of"), (-1, 10, "design = -1 is not one of"),
                                (1, 0, "sweeps = 0 outside [1, 30]"), (2, 31, "sweeps = 31 outside [1, 30]")):
        head = (eng.ctx, native._ptr(mix), native._ptr(est), 1, 3, 2, 600, None, None, 0, 512, 128, 2, 1e-10, 1e-3, design,
                sweeps)
        for name, tail in (("dsn_beamform_design", (0, 0, native._ptr(out), None, eng._stream())),
                           ("dsn_beamform_spatial_design", (1, 0.1, 0.1, 1e-3, 1e-10, 0, native._ptr(out), None, None, None,
                                                            eng._stream())),
                           ("dsn_beamform_track_design", (0, 100, 1, 1, 0, native._ptr(out), None, eng._stream()))):
            assert getattr(eng.lib, name)(*head, *tail) != 0, (name, design, sweeps)
            text = eng.lib.dsn_last_error(eng.ctx).decode()
            assert msg in text and name + ": " in text, (name, text)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    for call in (eng.beamform, eng.beamform_spatial, eng.beamform_track):
        with pytest.raises(ValueError, match="design must be"):
            call(mix, est, design="mvdr")
        with pytest.raises(ValueError, match=r"design: sweeps = 0 outside \[1, 30\]"):
            call(mix, est, design=dict(sweeps=0))
