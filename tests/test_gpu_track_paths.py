"""The `track` keyword of LatentDiffSep (separate, separate_batch, separate_long, separate_files) on the tiny test
network against the same steps done by hand: with beamform=, the beamforming step is Engine.beamform_track in place of
Engine.beamform, on the same inputs and in the same place -- after combine and refine and before rescale, the resampling
back, loudness and limit; dereverb= stays the first step.  The block length is given in seconds and converted at the
model's rate.  Everything is bit for bit (byte for byte for the files); track=None returns the bits and bytes of the call
without the keyword."""
import numpy as np
import pytest
import torch

from ditsep_amd import files, native, wavio
from tests import pcm_restatement as pr
from tests.test_gpu_beamform_paths import fit
from tests.test_gpu_mask_refine import FS, N_STEPS, model  # noqa: F401  (`model` is a fixture)

pytestmark = pytest.mark.gpu
SMALL = dict(n_fft=64, hop=16)
BLOCK = 5 * 16 / FS                                    # seconds: 5 frames of 16 samples at the model's rate
TRACK = dict(block=BLOCK, context=1)


def test_the_block_length_in_frames():
    assert native.track_block_frames(BLOCK, FS, 16) == 5 and native.track_block_frames(BLOCK, FS, 32) == 4
    assert native.track_block_frames(0.8, FS, 128) == 100


def test_separate_with_track(model):
    eng = model.engine
    g = torch.Generator().manual_seed(81)
    mix = 0.3 * torch.randn((2, 4, 600), generator=g)
    dev = mix.to(eng.device)                                                            # 608 samples: 39 frames, 8 blocks
    for beamform, track, ref, kw in (
            (dict(SMALL), TRACK, 0, dict(SMALL, block_frames=5, context=1, interpolate=True)),
            (dict(SMALL, ref=2, power=1, reg=1e-2, postfilter="mask"), dict(block=BLOCK, context=0, interpolate=False), 2,
             dict(SMALL, power=1, reg=1e-2, postfilter="mask", block_frames=5, context=0, interpolate=False)),
            (dict(SMALL, ref=1), 2 * BLOCK, 1, dict(SMALL, block_frames=10, context=1, interpolate=True))):
        plain, nfe = model.separate(dev[:, ref:ref + 1].contiguous(), seed=3)
        got, nfe_s = model.separate(mix, seed=3, beamform=beamform, track=track)
        assert nfe_s == nfe == 2 * N_STEPS and tuple(got.shape) == (2, 2, 608)
        want = eng.beamform_track(fit(dev, 608), plain, ref=ref, **kw)
        assert torch.equal(got, want)
        assert not torch.equal(got, model.separate(mix, seed=3, beamform=beamform)[0])
    # track=None is the call without the keyword
    bf = model.separate(mix, seed=3, beamform=1)[0]
    assert torch.equal(model.separate(mix, seed=3, beamform=1, track=None)[0], bf)
    one = dev[:, 1:2].contiguous()
    assert torch.equal(model.separate(one, seed=3, track=None)[0], model.separate(one, seed=3)[0])
    # with dereverb=: the first step, on the channels, which the beamforming step then sees
    dopts = dict(taps=2, delay=1, iterations=1, n_fft=64, hop=16)
    dry = eng.dereverb(dev, **dopts)
    sep = model.separate(dry[:, :1].contiguous(), seed=3)[0]
    got = model.separate(mix, seed=3, beamform=SMALL, track=TRACK, dereverb=dopts)[0]
    assert torch.equal(got, eng.beamform_track(fit(dry, 608), sep, block_frames=5, **SMALL))
    # with loudness=: the last step, on the mono outputs, link "mixture" measuring channel ref
    got, _, info = model.separate(mix, seed=3, beamform=SMALL, track=TRACK, loudness=-23.0, return_info=True)
    tr_out = model.separate(mix, seed=3, beamform=SMALL, track=TRACK)[0]
    hand, hinfo = eng.loudness_normalize([dev[b, :1] for b in range(2)], [tr_out[b] for b in range(2)], FS,
                                         **native.level_options(-23.0, None))
    assert torch.equal(got, torch.stack(hand)) and info["gain_db"] == hinfo["gain_db"]
    # at another rate: the blocks are counted at the model's rate
    got = model.separate(mix, seed=3, sample_rate=32000, beamform=SMALL, track=TRACK)[0]
    mc = eng.resample(mix, 32000, FS)
    est = model.separate(mc[:, :1].contiguous(), seed=3)[0]
    hand = eng.resample(eng.beamform_track(fit(mc, int(est.shape[-1])), est, block_frames=5, **SMALL), FS, 32000)[..., :600]
    assert torch.equal(got, hand)
    for kw, msg in ((dict(beamform=None), "track= adapts the weights of the beamformer block by block: it needs beamform="),
                    (dict(spatial=True), "track= does not go with spatial=: the cACGMM sums its statistics"),
                    (dict(stems="mask"), "does not go with stems="),
                    (dict(intermediate=True), "does not go with intermediate"),
                    (dict(track=False), "track must be None, True, a block length in seconds or a dict"),
                    (dict(track={"context": 65}), r"track: context = 65 outside \[0, 64\]")):
        with pytest.raises(ValueError, match=msg):
            model.separate(mix, **dict(dict(beamform=SMALL, track=True), **kw))
    with pytest.raises(ValueError, match="with latent=True there is no mixture to filter"):
        model.separate(torch.zeros(1, 64, 75), latent=True, beamform=True, track=True)


def test_separate_batch_and_long_with_track(model):
    eng = model.engine
    g = torch.Generator().manual_seed(83)
    mixes = [0.3 * torch.randn((c, L), generator=g) for c, L in ((4, 300), (2, 611), (8, 417))]
    ones = [m[1:2].to(eng.device).contiguous() for m in mixes]
    beam = dict(ref=1, n_fft=64, hop=16)
    hand_kw = dict(beam, block_frames=5, context=1, interpolate=True)
    plain, nfe = model.separate_batch(ones, seed=7)
    got, nfe_s = model.separate_batch(mixes, seed=7, beamform=beam, track=TRACK)
    want = eng.beamform_track([m.to(eng.device) for m in mixes], plain, **hand_kw)
    assert nfe == nfe_s
    for b, m in enumerate(mixes):
        assert tuple(got[b].shape) == (2, m.shape[-1]) and torch.equal(got[b], want[b])
        assert torch.equal(got[b], eng.beamform_track(m[None], plain[b][None], **hand_kw)[0])
    old, _ = model.separate_batch(mixes, seed=7, beamform=beam)
    again, _ = model.separate_batch(mixes, seed=7, beamform=beam, track=None)
    assert all(torch.equal(a, p) for a, p in zip(again, old)) and not torch.equal(old[0], got[0])
    # with dereverb= and loudness= at other rates
    rates = [32000, FS, 8000]
    dopts = dict(taps=2, delay=1, iterations=1, n_fft=64, hop=16)
    got, _ = model.separate_batch(mixes, seed=7, sample_rates=rates, beamform=beam, track=TRACK, dereverb=dopts)
    mc = eng.dereverb(eng.to_model_rate(mixes, rates, FS, downmix=False), **dopts)
    est, _ = model.separate_batch([m[1:2].contiguous() for m in mc], seed=7)
    hand = eng.from_model_rate(eng.beamform_track(list(mc), est, **hand_kw), rates, FS, [m.shape[-1] for m in mixes])
    for b, m in enumerate(mixes):
        assert tuple(got[b].shape) == (2, m.shape[-1]) and torch.equal(got[b], hand[b])
    lev, _ = model.separate_batch(mixes, seed=7, beamform=beam, track=TRACK, loudness=-23.0)
    base, _ = model.separate_batch(mixes, seed=7, beamform=beam, track=TRACK)
    hand, _ = eng.loudness_normalize(ones, base, FS, **native.level_options(-23.0, None))
    assert all(torch.equal(a, b) for a, b in zip(lev, hand))
    # long recordings, both modes
    rec = [0.3 * torch.randn((3, 700), generator=g), 0.3 * torch.randn((2, 450), generator=g)]
    for mode in ("stitch", "score"):
        kw = dict(window=256, overlap=64, mode=mode, batch=3, seed=9)
        plain, nfe = model.separate_long([r[:1].to(eng.device).contiguous() for r in rec], **kw)
        got, nfe_s = model.separate_long(rec, beamform=SMALL, track=TRACK, **kw)
        want = eng.beamform_track([r.to(eng.device) for r in rec], plain, block_frames=5, **SMALL)
        assert nfe == nfe_s and all(torch.equal(a, b) for a, b in zip(got, want))
        old, _ = model.separate_long(rec, beamform=True, **kw)
        again, _ = model.separate_long(rec, beamform=True, track=None, **kw)
        assert all(torch.equal(a, b) for a, b in zip(again, old))
        assert not torch.equal(got[0], model.separate_long(rec, beamform=SMALL, **kw)[0][0])
        # with loudness=: the last step, on the tracked outputs, link "mixture" measuring channel ref
        lev, *_ = model.separate_long(rec, beamform=SMALL, track=TRACK, loudness=-23.0, **kw)
        hand, _ = eng.loudness_normalize([r[:1].to(eng.device).contiguous() for r in rec], list(got), FS,
                                         **native.level_options(-23.0, None))
        assert all(torch.equal(a, b) for a, b in zip(lev, hand))
        untracked, *_ = model.separate_long(rec, beamform=SMALL, loudness=-23.0, **kw)
        assert not torch.equal(lev[0], untracked[0])
        dry = eng.dereverb([r.to(eng.device) for r in rec], **dopts)
        sep, _ = model.separate_long([r[:1].contiguous() for r in dry], **kw)
        got, _ = model.separate_long(rec, beamform=SMALL, track=TRACK, dereverb=dopts, **kw)
        want = eng.beamform_track(list(dry), sep, block_frames=5, **SMALL)
        assert all(torch.equal(a, b) for a, b in zip(got, want))
    with pytest.raises(ValueError, match="track= adapts the weights of the beamformer block by block: it needs beamform="):
        model.separate_batch(mixes, track=True)
    with pytest.raises(ValueError, match="does not go with stems="):
        model.separate_batch(mixes, beamform=True, track=True, stems="mask")
    with pytest.raises(ValueError, match="does not go with intermediate"):
        model.separate_long(rec, window=256, beamform=True, track=True, intermediate=True)
    with pytest.raises(ValueError, match="track= does not go with spatial="):
        model.separate_long(rec, window=256, beamform=True, track=True, spatial=True)


def test_separate_files_with_track(model, tmp_path):
    eng = model.engine
    g = np.random.default_rng(87)
    src = tmp_path / "in"
    src.mkdir()
    wavio.write_wav(src / "a.wav", (0.3 * g.standard_normal(4 * 900) * 2 ** 15).astype("<i2").tobytes(), 44100, 4, "s16")
    wavio.write_wav(src / "b.wav", (0.3 * g.standard_normal(2 * 300) * 2 ** 15).astype("<i2").tobytes(), FS, 2, "s16")
    wavio.write_wav(src / "c.wav", (0.3 * g.standard_normal(8 * 260)).astype("<f4").tobytes(), 8000, 8, "f32")
    paths = sorted(src.glob("*.wav"))
    hs = [wavio.read_header(p) for p in paths]
    beam, trk = dict(ref=1, n_fft=128, hop=32), dict(block=4 * 32 / FS, context=1, interpolate=True)
    assert native.track_block_frames(trk["block"], FS, 32) == 4
    for kw, msg in ((dict(track=trk), "track= adapts the weights of the beamformer block by block: it needs beamform="),
                    (dict(track=trk, beamform=beam, spatial=True), "track= does not go with spatial="),
                    (dict(track=trk, beamform=beam, stems="mask"), "track= does not go with stems="),
                    (dict(track={"frames": 2}, beamform=beam), r"track: unknown keys \['frames'\]")):
        with pytest.raises(ValueError, match=msg):
            model.separate_files(paths, tmp_path / "never", **kw)
    assert not (tmp_path / "never").exists()
    plan = files.plan_files(hs, FS, 8, batch=2)

    def by_hand(loud, dopts):
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
            est = eng.beamform_track(list(mc), eng.mask_refine(one, est), block_frames=4, context=1, interpolate=True,
                                     **beam)
            back = eng.from_model_rate(est, rates, FS, frames)
            if loud is not None:
                back, _ = eng.loudness_normalize([c[1:2].to(eng.device).contiguous() for c in clips], back, rates,
                                                 **native.level_options(loud, None))
            for j, i in enumerate(idx):
                want[i] = [pr.quantise(back[j][s].cpu().numpy(), "s16") for s in range(2)]
        return want

    dere = dict(taps=2, delay=1, iterations=1, n_fft=128, hop=32)
    for tag, loud, dopts in (("plain", None, None), ("levelled", -23.0, None), ("dry", None, dere)):
        out = tmp_path / tag
        recs = model.separate_files(paths, out, batch=2, seed=5, refine=True, beamform=beam, track=trk, loudness=loud,
                                    dereverb=dopts)
        want = by_hand(loud, dopts)
        for i, p in enumerate(paths):
            assert recs[i]["beamform"] == 1 and recs[i]["track"] == native.track_options(trk)
            for s in range(2):
                q = out / f"s{s}" / p.name
                ho = wavio.read_header(q)
                assert ho[:4] == (hs[i].rate, 1, hs[i].frames, "s16")
                assert wavio.read_payload(q, ho) == want[i][s][0], f"{q} is not the quantised tracked estimate"
    # track=None: the keys and the bytes of the call without the keyword
    a = model.separate_files(paths, tmp_path / "none", batch=2, seed=5, refine=True, beamform=beam, track=None)
    b = model.separate_files(paths, tmp_path / "old", batch=2, seed=5, refine=True, beamform=beam)
    assert set(a[0]) == set(b[0]) and "track" not in a[0]
    for p in paths:
        for s in range(2):
            assert (tmp_path / "none" / f"s{s}" / p.name).read_bytes() == (tmp_path / "old" / f"s{s}" / p.name).read_bytes()
            assert (tmp_path / "none" / f"s{s}" / p.name).read_bytes() != (tmp_path / "plain" / f"s{s}" / p.name).read_bytes()
