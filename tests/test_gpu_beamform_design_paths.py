"""The designs of the beamforming weights beyond Engine.beamform: Engine.beamform_spatial(design=) and
Engine.beamform_track(design=) against their restatements with the design's weights substituted
(tests/beamform_design_restatement.py), under the yardstick of tests/test_gpu_beamform_design.py -- at most 8 x the
error of the float32-CPU run of the same restatement, after the same two conditions, the eigenvalue gap taken on the
statistics the weights are solved on (the refined ones, every block's) --, and the `design` keyword of LatentDiffSep
(separate, separate_batch, separate_long in both modes, separate_files) on the tiny test network against the same steps
done by hand: alone, with spatial=, with track=, with dereverb= and with activity=.  The keyword paths are bit for bit
(byte for byte for the files); design=None returns the bits and bytes of the call without the keyword."""
import numpy as np
import pytest
import torch

from ditsep_amd import files, native, wavio
from tests import beamform_design_restatement as bd
from tests import beamform_restatement as br
from tests import pcm_restatement as pr
from tests.test_gpu_beamform import FACTOR, off_alignment, ratio
from tests.test_gpu_beamform_paths import fit
from tests.test_gpu_mask_refine import FS, N_STEPS, model  # noqa: F401  (`model` is a fixture)
from tests.util import make_engine

pytestmark = pytest.mark.gpu
SMALL = dict(n_fft=64, hop=16)
DESIGNS = ("rank1", "gev")


@pytest.fixture(scope="module")
def eng():
    e = make_engine()
    yield e
    e.close()


# ------------------------------------------------------------------ 1. the two other engine calls against their restatements
def check(call, restated, mix, est, what, design, **kw):
    seen = []
    ref, iref = restated(mix, est, design=design, record=seen, return_info=True, **kw)
    cpu, icpu = restated(mix, est, design=design, dtype=np.float32, return_info=True, **kw)
    power = np.asarray(iref["power"])
    assert power.min() >= 1e-6 * power.max() > 0, f"{what}: a bin of the input carries no signal"
    assert min(seen) >= 1e-2, f"{what}: eigenvalue gap {min(seen):.2e} < 1e-2"
    m, e = torch.from_numpy(mix)[None], torch.from_numpy(est)[None]
    out, info = call(off_alignment(m, "cuda"), off_alignment(e, "cuda"), return_info=True, design=design, **kw)
    out, w = out[0].cpu().numpy(), info["w"][0].numpy()
    assert out.shape == ref.shape and w.shape == iref["w"].shape and np.all(np.isfinite(out)) and np.all(np.isfinite(w))
    top = float(np.max(np.abs(iref["w"])))
    rel = lambda a: float(np.max(np.abs(a - iref["w"])) / top)
    pairs = {"out": (br.rel_err(out, ref, mix), br.rel_err(cpu, ref, mix)), "w": (rel(w), rel(icpu["w"]))}
    print(f"{what} {design} (gap {min(seen):.3f}): "
          + "; ".join(f"{k} {d:.3e} (float32 CPU {c:.3e}, ratio {ratio(d, c):.2f})" for k, (d, c) in pairs.items()))
    for k, (d, c) in pairs.items():
        assert d <= FACTOR * c, f"{what} {design}: {k} {ratio(d, c):.2f} x the float32 CPU error"


@pytest.mark.parametrize("design", DESIGNS)
def test_spatial_against_the_restatement(eng, design):
    """the noise class enters Q and gets no filter (classes = n + 1), and without it (classes = n)"""
    for seed, C, kw in ((4, 3, dict(iterations=2, ref=2)), (7, 2, dict(iterations=1, noise=0.0))):
        mix, est = br.make_case(seed, "generic", 2, C, 700)
        check(eng.beamform_spatial, bd.beamform_spatial, mix, est, f"spatial C {C} {kw}", design, **SMALL, **kw)


@pytest.mark.parametrize("design", DESIGNS)
def test_track_against_the_restatement(eng, design):
    """three blocks of 15 frames, interpolated and held; the post-filter is untouched"""
    for seed, C, kw in ((3, 3, dict(block_frames=15, context=1, ref=1)),
                        (7, 2, dict(block_frames=15, context=1, interpolate=False, postfilter="mask"))):
        mix, est = br.make_case(seed, "generic", 2, C, 700)
        check(eng.beamform_track, bd.beamform_track, mix, est, f"track C {C} {kw}", design, **SMALL, **kw)


# ------------------------------------------------------------------ 2. the keyword against the steps done by hand
BLOCK = 5 * 16 / FS                                    # seconds: 5 frames of 16 samples at the model's rate
GEV = dict(kind="gev", sweeps=6)


def test_separate_with_design(model):
    eng = model.engine
    g = torch.Generator().manual_seed(91)
    mix = 0.3 * torch.randn((2, 4, 600), generator=g)
    dev = mix.to(eng.device)
    plain, nfe = model.separate(dev[:, 1:2].contiguous(), seed=3)
    beam = dict(SMALL, ref=1)
    bf = model.separate(mix, seed=3, beamform=beam)[0]
    for design in ("rank1", GEV):
        got, nfe_s = model.separate(mix, seed=3, beamform=beam, design=design)
        assert nfe_s == nfe == 2 * N_STEPS and tuple(got.shape) == (2, 2, 608)
        assert torch.equal(got, eng.beamform(fit(dev, 608), plain, design=design, **beam)) and not torch.equal(got, bf)
        got = model.separate(mix, seed=3, beamform=beam, design=design, spatial=dict(iterations=2))[0]
        assert torch.equal(got, eng.beamform_spatial(fit(dev, 608), plain, design=design, iterations=2, **beam))
        got = model.separate(mix, seed=3, beamform=beam, design=design, track=BLOCK)[0]
        assert torch.equal(got, eng.beamform_track(fit(dev, 608), plain, design=design, block_frames=5, **beam))
    # design=None and "souden" are the call without the keyword
    assert torch.equal(model.separate(mix, seed=3, beamform=beam, design=None)[0], bf)
    assert torch.equal(model.separate(mix, seed=3, beamform=beam, design="souden")[0], bf)
    one = dev[:, 1:2].contiguous()
    assert torch.equal(model.separate(one, seed=3, design=None)[0], model.separate(one, seed=3)[0])
    # with dereverb=: the first step, on the channels, which the beamforming step then sees
    dopts = dict(taps=2, delay=1, iterations=1, n_fft=64, hop=16)
    dry = eng.dereverb(dev, **dopts)
    sep = model.separate(dry[:, 1:2].contiguous(), seed=3)[0]
    got = model.separate(mix, seed=3, beamform=beam, design=GEV, dereverb=dopts)[0]
    assert torch.equal(got, eng.beamform(fit(dry, 608), sep, design=GEV, **beam))
    # with activity=: decided on the beamformed estimates
    got = model.separate(mix, seed=3, beamform=beam, design="rank1", activity="gate")[0]
    r1 = eng.beamform(fit(dev, 608), plain, design="rank1", **beam)
    assert torch.equal(got, model._activity_step(r1, native.activity_options("gate")))
    # with loudness= and limit=: the last step, on the mono outputs, link "mixture" measuring channel ref
    got, _, info = model.separate(mix, seed=3, beamform=beam, design="rank1", loudness=-23.0, limit=True, return_info=True)
    hand, hinfo = eng.loudness_normalize([dev[b, 1:2] for b in range(2)], [r1[b] for b in range(2)], FS,
                                         **native.level_options(-23.0, True))
    assert torch.equal(got, torch.stack(hand)) and info["gain_db"] == hinfo["gain_db"]
    for kw, msg in ((dict(beamform=None), "design= picks the filter of the beamformer: it needs beamform="),
                    (dict(stems="mask"), "beamform= does not go with stems="),
                    (dict(intermediate=True), "beamform= does not go with intermediate"),
                    (dict(design=True), "design must be None, 'rank1', 'gev', 'souden' or a dict"),
                    (dict(design={"sweeps": 31}), r"design: sweeps = 31 outside \[1, 30\]")):
        with pytest.raises(ValueError, match=msg):
            model.separate(mix, **dict(dict(beamform=beam, design="gev"), **kw))
    with pytest.raises(ValueError, match="with latent=True there is no mixture to filter"):
        model.separate(torch.zeros(1, 64, 75), latent=True, beamform=True, design="gev")


def test_separate_batch_and_long_with_design(model):
    eng = model.engine
    g = torch.Generator().manual_seed(93)
    mixes = [0.3 * torch.randn((c, L), generator=g) for c, L in ((4, 300), (2, 611), (8, 417))]
    on_dev = [m.to(eng.device) for m in mixes]
    ones = [m[1:2].contiguous() for m in on_dev]
    beam = dict(ref=1, n_fft=64, hop=16)
    plain, nfe = model.separate_batch(ones, seed=7)
    old, _ = model.separate_batch(mixes, seed=7, beamform=beam)
    for extra, hand in ((dict(), lambda: eng.beamform(on_dev, plain, design=GEV, **beam)),
                        (dict(spatial=True), lambda: eng.beamform_spatial(on_dev, plain, design=GEV, **beam)),
                        (dict(track=BLOCK), lambda: eng.beamform_track(on_dev, plain, design=GEV, block_frames=5, **beam))):
        got, nfe_s = model.separate_batch(mixes, seed=7, beamform=beam, design=GEV, **extra)
        want = hand()
        assert nfe == nfe_s
        for b, m in enumerate(mixes):
            assert tuple(got[b].shape) == (2, m.shape[-1]) and torch.equal(got[b], want[b])
        assert not torch.equal(got[0], old[0])
    again, _ = model.separate_batch(mixes, seed=7, beamform=beam, design=None)
    assert all(torch.equal(a, p) for a, p in zip(again, old))
    # with dereverb= at other rates, and with activity=
    rates = [32000, FS, 8000]
    dopts = dict(taps=2, delay=1, iterations=1, n_fft=64, hop=16)
    got, _ = model.separate_batch(mixes, seed=7, sample_rates=rates, beamform=beam, design="rank1", dereverb=dopts)
    mc = eng.dereverb(eng.to_model_rate(mixes, rates, FS, downmix=False), **dopts)
    est, _ = model.separate_batch([m[1:2].contiguous() for m in mc], seed=7)
    hand = eng.from_model_rate(eng.beamform(list(mc), est, design="rank1", **beam), rates, FS,
                               [m.shape[-1] for m in mixes])
    assert all(torch.equal(a, b) for a, b in zip(got, hand))
    got, _ = model.separate_batch(mixes, seed=7, beamform=beam, design="rank1", activity="gate")
    hand = model._activity_step(list(eng.beamform(on_dev, plain, design="rank1", **beam)), native.activity_options("gate"))
    assert all(torch.equal(a, b) for a, b in zip(got, hand))
    # long recordings, both modes
    rec = [0.3 * torch.randn((3, 700), generator=g), 0.3 * torch.randn((2, 450), generator=g)]
    rdev = [r.to(eng.device) for r in rec]
    for mode in ("stitch", "score"):
        kw = dict(window=256, overlap=64, mode=mode, batch=3, seed=9)
        plain, nfe = model.separate_long([r[:1].contiguous() for r in rdev], **kw)
        old, _ = model.separate_long(rec, beamform=SMALL, **kw)
        for extra, hand in ((dict(), lambda: eng.beamform(rdev, plain, design="rank1", **SMALL)),
                            (dict(spatial=True), lambda: eng.beamform_spatial(rdev, plain, design="rank1", **SMALL)),
                            (dict(track=BLOCK),
                             lambda: eng.beamform_track(rdev, plain, design="rank1", block_frames=5, **SMALL))):
            got, nfe_s = model.separate_long(rec, beamform=SMALL, design="rank1", **extra, **kw)
            assert nfe == nfe_s and all(torch.equal(a, b) for a, b in zip(got, hand()))
            assert not torch.equal(got[0], old[0])
        again, _ = model.separate_long(rec, beamform=SMALL, design=None, **kw)
        assert all(torch.equal(a, b) for a, b in zip(again, old))
        dry = eng.dereverb(rdev, **dopts)
        sep, _ = model.separate_long([r[:1].contiguous() for r in dry], **kw)
        got, _ = model.separate_long(rec, beamform=SMALL, design=GEV, dereverb=dopts, **kw)
        assert all(torch.equal(a, b) for a, b in zip(got, eng.beamform(list(dry), sep, design=GEV, **SMALL)))
        got, _ = model.separate_long(rec, beamform=SMALL, design=GEV, activity=True, **kw)
        assert all(torch.equal(a, b) for a, b in zip(got, eng.beamform(rdev, plain, design=GEV, **SMALL)))
    with pytest.raises(ValueError, match="design= picks the filter of the beamformer: it needs beamform="):
        model.separate_batch(mixes, design="gev")
    with pytest.raises(ValueError, match="beamform= does not go with stems="):
        model.separate_batch(mixes, beamform=True, design="gev", stems="mask")
    with pytest.raises(ValueError, match="design= picks the filter of the beamformer: it needs beamform="):
        model.separate_long(rec, window=256, design="gev")
    with pytest.raises(ValueError, match="does not go with intermediate"):
        model.separate_long(rec, window=256, beamform=True, design="gev", intermediate=True)


def test_separate_files_with_design(model, tmp_path):
    eng = model.engine
    g = np.random.default_rng(97)
    src = tmp_path / "in"
    src.mkdir()
    wavio.write_wav(src / "a.wav", (0.3 * g.standard_normal(4 * 900) * 2 ** 15).astype("<i2").tobytes(), 44100, 4, "s16")
    wavio.write_wav(src / "b.wav", (0.3 * g.standard_normal(2 * 300) * 2 ** 15).astype("<i2").tobytes(), FS, 2, "s16")
    wavio.write_wav(src / "c.wav", (0.3 * g.standard_normal(8 * 260)).astype("<f4").tobytes(), 8000, 8, "f32")
    paths = sorted(src.glob("*.wav"))
    hs = [wavio.read_header(p) for p in paths]
    beam = dict(ref=1, n_fft=128, hop=32)
    trk = dict(block=4 * 32 / FS, context=1, interpolate=True)
    for kw, msg in ((dict(design="gev"), "design= picks the filter of the beamformer: it needs beamform="),
                    (dict(design="gev", beamform=beam, stems="mask"), "beamform= does not go with stems="),
                    (dict(design={"rank": 1}, beamform=beam), r"design: unknown keys \['rank'\]")):
        with pytest.raises(ValueError, match=msg):
            model.separate_files(paths, tmp_path / "never", **kw)
    assert not (tmp_path / "never").exists()
    plan = files.plan_files(hs, FS, 8, batch=2)

    def by_hand(step, dopts):
        want = {}
        for k, idx in enumerate(plan["batches"]):
            clips = [torch.from_numpy(pr.decode(wavio.read_payload(paths[i], hs[i]), hs[i].frames, hs[i].channels,
                                                hs[i].encoding)) for i in idx]
            rates, frames = [hs[i].rate for i in idx], [hs[i].frames for i in idx]
            mc = eng.to_model_rate(clips, rates, FS, downmix=False)
            if dopts is not None:
                mc = eng.dereverb(list(mc), **dopts)
            one = [m[1:2].contiguous() for m in mc]
            est, _ = model.separate_batch(one, codec="padded", seed=5 + k)
            back = eng.from_model_rate(step(list(mc), eng.mask_refine(one, est)), rates, FS, frames)
            for j, i in enumerate(idx):
                want[i] = [pr.quantise(back[j][s].cpu().numpy(), "s16") for s in range(2)]
        return want

    dere = dict(taps=2, delay=1, iterations=1, n_fft=128, hop=32)
    assert native.activity_options(True)["gate"] is False                    # (segments only: the bytes are the design's)
    for tag, extra, dopts, step in (
            ("alone", dict(), None, lambda mc, est: eng.beamform(mc, est, design=GEV, **beam)),
            ("spatial", dict(spatial=True), None, lambda mc, est: eng.beamform_spatial(mc, est, design=GEV, **beam)),
            ("track", dict(track=trk), None,
             lambda mc, est: eng.beamform_track(mc, est, design=GEV, block_frames=4, context=1, **beam)),
            ("dry", dict(dereverb=dere), dere, lambda mc, est: eng.beamform(mc, est, design=GEV, **beam)),
            ("activity", dict(activity=True), None, lambda mc, est: eng.beamform(mc, est, design=GEV, **beam))):
        out = tmp_path / tag
        recs = model.separate_files(paths, out, batch=2, seed=5, refine=True, beamform=beam, design=GEV, **extra)
        want = by_hand(step, dopts)
        for i, p in enumerate(paths):
            assert recs[i]["beamform"] == 1 and recs[i]["design"] == native.design_options(GEV)
            assert ("activity" in recs[i]) == (tag == "activity") and (out / (p.stem + ".rttm")).exists() == (tag == "activity")
            for s in range(2):
                q = out / f"s{s}" / p.name
                ho = wavio.read_header(q)
                assert ho[:4] == (hs[i].rate, 1, hs[i].frames, "s16")
                assert wavio.read_payload(q, ho) == want[i][s][0], f"{q} is not the quantised estimate of the design"
    # design=None: the keys and the bytes of the call without the keyword
    a = model.separate_files(paths, tmp_path / "none", batch=2, seed=5, refine=True, beamform=beam, design=None)
    b = model.separate_files(paths, tmp_path / "old", batch=2, seed=5, refine=True, beamform=beam)
    assert set(a[0]) == set(b[0]) and "design" not in a[0]
    for p in paths:
        for s in range(2):
            assert (tmp_path / "none" / f"s{s}" / p.name).read_bytes() == (tmp_path / "old" / f"s{s}" / p.name).read_bytes()
            assert (tmp_path / "none" / f"s{s}" / p.name).read_bytes() != (tmp_path / "alone" / f"s{s}" / p.name).read_bytes()
