"""dsn_beamform_spatial (ditsep_amd/csrc/spatial.hip) through Engine.beamform_spatial on an engine with no score network
and no codec, against the restatement (tests/spatial_restatement.py).

Bounds.  The error of an output is its largest absolute difference from the float64 restatement divided by the peak of
|mix|; the error of the weights is their largest absolute difference from the float64 restatement's divided by its
largest weight; the error of gamma is its largest absolute difference from the float64 restatement's.  Each may be at
most 8 x what the float32 run of the same restatement shows on the same input (float32 pocketfft transforms and masks,
float64 mixture model, statistics and solve: the device's own split of precisions) -- the rule and the factor of
tests/test_gpu_beamform.py, for the same reason.  Every input is one on which the restatement counts no failed bin (that
is asserted first, and that the device counts none) and of which every bin carries at least 1e-6 of the strongest bin's
mixture power.  With iterations = 0, noise = 0 and floor = 0 the weights are within 1e-10 of Engine.beamform's relative
to the largest weight (gamma is M itself; the sums run in another order).
Everything else -- a ragged item against the item alone, a permuted batch, a rerun, a base pointer one float off, a
workspace budget of one item, lists -- is bit for bit.

Measured on an MI355X: see the README paragraph "Spatial mask refinement"."""
import numpy as np
import pytest
import torch

from ditsep_amd import native
from tests import beamform_restatement as br
from tests import spatial_restatement as sp
from tests.test_gpu_beamform import off_alignment, ratio, same_bits
from tests.util import make_engine

pytestmark = pytest.mark.gpu
FACTOR = 8.0


@pytest.fixture(scope="module")
def eng():
    e = make_engine()
    assert e.cfg.score_kind == native.SCORE_NONE
    yield e
    e.close()


def check(eng, mix, est, what, **kw):
    ref, iref = sp.beamform_spatial(mix, est, return_info=True, **kw)
    cpu, icpu = sp.beamform_spatial(mix, est, dtype=np.float32, return_info=True, **kw)
    assert iref["failed"] == 0 and icpu["failed"] == 0, f"{what}: the restatement counts failed bins"
    power = iref["power"]
    assert power.min() >= 1e-6 * power.max() > 0, f"{what}: a bin of the input carries no signal"
    m = off_alignment(torch.from_numpy(mix)[None], eng.device)
    e = off_alignment(torch.from_numpy(est)[None], eng.device)
    out, info = eng.beamform_spatial(m, e, return_info=True, **kw)
    out, w, gamma = out[0].cpu().numpy(), info["w"][0].numpy(), info["gamma"][0].numpy()
    assert int(info["fail"].sum()) == iref["failed"] == 0
    assert out.shape == ref.shape and w.shape == iref["w"].shape and gamma.shape == iref["gamma"].shape
    assert np.all(np.isfinite(out)) and np.all(np.isfinite(w)) and np.all(np.isfinite(gamma))
    top = float(np.max(np.abs(iref["w"])))
    rel = lambda a: float(np.max(np.abs(a - iref["w"])) / top)
    gerr = lambda a: float(np.max(np.abs(a - iref["gamma"])))
    pairs = {"out": (br.rel_err(out, ref, mix), br.rel_err(cpu, ref, mix)), "w": (rel(w), rel(icpu["w"])),
             "gamma": (gerr(gamma), gerr(icpu["gamma"]))}
    print(what + ": " + "; ".join(f"{k} {d:.3e} (float32 CPU {c:.3e}, ratio {ratio(d, c):.2f})"
                                  for k, (d, c) in pairs.items()))
    for k, (d, c) in pairs.items():
        assert d <= FACTOR * c, f"{what}: {k} {ratio(d, c):.2f} x the float32 CPU error"


# n_fft, hop, L, C, n, and the keywords: several frame tiles of the solve launch (607 frames); the largest system with the
# noise class; the longest run of iterations; no noise class; 7 frames of the longest window; the shortest item
CASES = {
    "tiles": (64, 16, 9700, 2, 2, dict(iterations=3, power=1)),
    "largest": (512, 128, 6007, 8, 4, dict(iterations=1, ref=7)),
    "iterations": (512, 128, 5003, 3, 1, dict(iterations=16)),
    "no_noise": (256, 32, 3001, 5, 3, dict(iterations=2, noise=0.0, power=1, ref=4)),
    "long_window": (2048, 512, 3072, 4, 2, dict(iterations=2)),
    "shortest": (512, 128, 257, 2, 2, dict(iterations=2, ref=1)),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_against_the_restatement(eng, name):
    n_fft, hop, L, C, n, kw = CASES[name]
    mix, est = br.make_case(len(name) + L, "generic", n, C, L)
    check(eng, mix, est, f"{name}: n_fft {n_fft} hop {hop} L {L} C {C} n {n} {kw}", n_fft=n_fft, hop=hop, **kw)


def test_sanity_case(eng):
    mix, est, _ = br.sanity_case(leak=0.6, L=8000)
    check(eng, mix, est, "sanity_case(leak=0.6, L=8000) at the defaults")


def test_without_the_model_it_is_beamform(eng):
    """iterations = 0, noise = 0, floor = 0: the statistics path of spatial.hip against that of beamform.hip"""
    for n_fft, hop, L, C, n, power in ((512, 128, 6007, 4, 2, 2), (64, 16, 9700, 8, 4, 1), (2048, 512, 9001, 3, 3, 2)):
        mix, est = br.make_case(n_fft + L, "generic", n, C, L)
        m, e = torch.from_numpy(mix)[None], torch.from_numpy(est)[None]
        kw = dict(n_fft=n_fft, hop=hop, power=power, ref=C - 1)
        _, ib = eng.beamform(m, e, return_info=True, **kw)
        _, isp = eng.beamform_spatial(m, e, iterations=0, noise=0.0, floor=0.0, return_info=True, **kw)
        top = float(ib["w"].abs().max())
        err = float((isp["w"] - ib["w"]).abs().max()) / top
        print(f"n_fft {n_fft} C {C} n {n}: w {err:.3e} of the largest weight from Engine.beamform's")
        assert top > 0 and err <= 1e-10
        assert tuple(isp["gamma"].shape[:3]) == (1, n, n_fft // 2 + 1) and int(isp["fail"].sum()) == 0


@pytest.mark.parametrize("n_fft,hop,n,kw", [(512, 128, 2, dict(iterations=2)),
                                            (64, 16, 4, dict(iterations=1, noise=0.0)),
                                            (2048, 512, 1, dict(iterations=3, floor=0.3))])
def test_ragged(eng, n_fft, hop, n, kw):
    """5 items of distinct lengths and mixed channel counts, a one-channel item and one at the minimum length among them,
    one over several frame tiles, NaN past every end and in every channel an item does not have: each item against the
    item alone, a permuted batch, a rerun, a base pointer one float off, one item per chunk, lists"""
    need = n_fft // 2 + 1
    lens = [300 * hop + 5, need, 700 * hop // (n_fft // 64) + 3, need + hop + 2, 40 * hop + 1]
    chans = [4, 2, 8, 1, 3]
    Lmax, Cmax, B = max(lens) + 3, 8, 5
    g = np.random.default_rng(n_fft + n)
    mix = torch.full((B, Cmax, Lmax), float("nan"))
    est = torch.full((B, n, Lmax), float("nan"))
    for b, (v, c) in enumerate(zip(lens, chans)):
        m, e = br.make_case(int(g.integers(1 << 30)), "generic", n, c, v)
        mix[b, :c, :v], est[b, :, :v] = torch.from_numpy(m), torch.from_numpy(e)
    kw = dict(kw, n_fft=n_fft, hop=hop)
    out, info = eng.beamform_spatial(mix, est, lens=lens, channels=chans, return_info=True, **kw)
    assert tuple(out.shape) == (B, n, Lmax) and not bool(torch.isnan(out).any())
    assert bool(torch.isfinite(torch.view_as_real(info["w"])).all()) and int(info["fail"].sum()) == 0
    for b, (v, c) in enumerate(zip(lens, chans)):
        alone, ia = eng.beamform_spatial(mix[b:b + 1, :c, :v].contiguous(), est[b:b + 1, :, :v].contiguous(),
                                         return_info=True, **kw)
        assert same_bits(out[b, :, :v], alone[0]), f"item {b} differs from the item alone"
        assert torch.equal(torch.view_as_real(info["w"][b, :, :, :c]), torch.view_as_real(ia["w"][0]))
        F = ia["gamma"].shape[-1]
        assert torch.equal(info["gamma"][b, :, :, :F], ia["gamma"][0]) and bool((info["gamma"][b, :, :, F:] == 0).all())
        assert bool((out[b, :, v:] == 0).all()), f"item {b}: not zero past its end"
        assert float(alone.abs().max()) > 0
    perm = [3, 0, 4, 2, 1]
    again = eng.beamform_spatial(mix[perm].contiguous(), est[perm].contiguous(), lens=[lens[p] for p in perm],
                                 channels=[chans[p] for p in perm], **kw)
    assert same_bits(again, out[perm])
    assert same_bits(eng.beamform_spatial(mix, est, lens=lens, channels=chans, **kw), out)
    assert same_bits(eng.beamform_spatial(off_alignment(mix, eng.device), off_alignment(est, eng.device), lens=lens,
                                          channels=chans, **kw), out)
    one_item = native.spatial_item_bytes(n_fft, hop, Lmax, Cmax, n)
    assert same_bits(eng.beamform_spatial(mix, est, lens=lens, channels=chans, workspace_budget=one_item, **kw), out)
    assert same_bits(eng.beamform_spatial(mix, est, lens=lens, channels=chans, workspace_budget=2 * one_item + 8, **kw),
                     out)
    as_list = eng.beamform_spatial([mix[b, :c, :v] for b, (v, c) in enumerate(zip(lens, chans))],
                                   [est[b, :, :v] for b, v in enumerate(lens)], **kw)
    for b, v in enumerate(lens):
        assert tuple(as_list[b].shape) == (n, v) and same_bits(as_list[b], out[b, :, :v])


def test_one_channel_takes_the_priors(eng):
    """C = 1 skips the model: gamma = a, and w = 1.0 exactly, so every source is mask_refine with n = 1"""
    mix, est = br.make_case(5, "generic", 2, 1, 3001)
    m, e = torch.from_numpy(mix)[None].to(eng.device), torch.from_numpy(est)[None].to(eng.device)
    out, info = eng.beamform_spatial(m, e, iterations=3, return_info=True)
    assert bool((info["w"] == 1.0).all()) and int(info["fail"].sum()) == 0
    one = eng.mask_refine(m[:, 0], e[:, :1])
    assert same_bits(out[:, 0], one[:, 0]) and same_bits(out[:, 1], one[:, 0])
    _, iref = sp.beamform_spatial(mix, est, iterations=3, return_info=True)
    _, icpu = sp.beamform_spatial(mix, est, iterations=3, dtype=np.float32, return_info=True)
    err = lambda a: float(np.max(np.abs(a - iref["gamma"])))
    assert err(info["gamma"][0].numpy()) <= FACTOR * err(icpu["gamma"])


def test_a_nan_sample(eng):
    """what the definition gives.  A NaN in an estimate: the priors of the frames it touches are NaN, every bin fails its
    first pivot and is counted, the statistics are NaN and w = e_ref -- the reference channel comes back, finite.  A NaN
    in a channel of the mixture other than the reference: the frames it touches are dead, no bin is counted, the
    statistics are NaN as well and the reference channel comes back."""
    C, n, L, ref = 3, 2, 4001, 1
    mix, est = br.make_case(11, "generic", n, C, L)
    m, e = torch.from_numpy(mix)[None].to(eng.device), torch.from_numpy(est)[None].to(eng.device)
    passed = eng.mask_refine(m[:, ref], e[:, :1])[0, 0]            # the reference channel through the transforms
    bad_e = e.clone()
    bad_e[0, 1, 2000] = float("nan")
    out, info = eng.beamform_spatial(m, bad_e, ref=ref, iterations=2, return_info=True)
    assert int(info["fail"].sum()) == 257 and bool(torch.isfinite(out).all())
    unit = torch.zeros(C, dtype=torch.complex128)
    unit[ref] = 1.0
    assert bool((info["w"] == unit).all())
    assert same_bits(out[0, 0], passed) and same_bits(out[0, 1], passed)
    bad_m = m.clone()
    bad_m[0, 0, 2000] = float("nan")
    out, info = eng.beamform_spatial(bad_m, e, ref=ref, iterations=2, return_info=True)
    assert int(info["fail"].sum()) == 0 and bool((info["w"] == unit).all())
    for i in range(n):   # 0 x NaN in the apply: NaN where the frames that hold the sample reach, the reference elsewhere
        assert bool(torch.isnan(out[0, i, 2000])) and bool(torch.isfinite(out[0, i, :1400]).all())
        assert same_bits(out[0, i, :1400], passed[:1400]) and same_bits(out[0, i, 2600:], passed[2600:])


def test_refusals_launch_nothing(eng):
    B, Cn, n, L = 2, 4, 2, 600
    mix = torch.zeros((B, Cn, L), device=eng.device)
    est = torch.zeros((B, n, L), device=eng.device)
    out = torch.full((B, n, L), 7.0, device=eng.device)
    good = dict(iterations=1, noise=0.1, floor=0.1, mask_reg=1e-3, mask_eps=1e-10, budget=0, n_fft=512, ref=0)

    def call(**kw):
        a = dict(good, **kw)
        return eng.lib.dsn_beamform_spatial(eng.ctx, native._ptr(mix), native._ptr(est), B, Cn, n, L, None, None, a["ref"],
                                            a["n_fft"], 128, 2, 1e-10, 1e-3, a["iterations"], a["noise"], a["floor"],
                                            a["mask_reg"], a["mask_eps"], a["budget"], native._ptr(out), None, None, None,
                                            eng._stream())

    need = native.spatial_item_bytes(512, 128, L, Cn, n)
    for kw, msg in ((dict(iterations=-1), "iterations = -1 outside [0, 16]"),
                    (dict(iterations=17), "iterations = 17 outside [0, 16]"),
                    (dict(noise=-0.1), "noise = -0.1 outside [0, 0.9]"), (dict(noise=0.95), "outside [0, 0.9]"),
                    (dict(noise=float("nan")), "outside [0, 0.9]"),
                    (dict(floor=1.5), "floor = 1.5 outside [0, 1]"), (dict(floor=-1.0), "floor = -1 outside [0, 1]"),
                    (dict(mask_reg=-1.0), "mask_reg = -1 is not a finite number >= 0"),
                    (dict(mask_eps=0.0), "mask_eps = 0 is not a finite positive number"),
                    (dict(n_fft=500), "n_fft = 500 is not a power of two in [64, 2048]"),
                    (dict(ref=4), "ref = 4 outside [0, 4): item 0 has 4 channels"),
                    (dict(budget=-1), "workspace_budget = -1 < 0"),
                    (dict(budget=need - 1), f"is smaller than one item ({need} bytes at C = 4, n = 2")):
        assert call(**kw) != 0, kw
        got = eng.lib.dsn_last_error(eng.ctx).decode()
        assert "dsn_beamform_spatial: " in got and msg in got, (kw, got)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    assert call(budget=need) == 0
    torch.cuda.synchronize()
    assert bool((out == 0.0).all())                 # a silent mixture: every frame is dead, tau = 0, w = e_ref
    with pytest.raises(ValueError, match=r"beamform_spatial: iterations = 17 outside \[0, 16\]"):
        eng.beamform_spatial(torch.zeros(1, 3, 600), torch.zeros(1, 2, 600), iterations=17)
