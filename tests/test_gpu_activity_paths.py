"""The `activity` keyword of LatentDiffSep (separate, separate_batch, separate_long in both modes, separate_files) on the
tiny test network against the same steps done by hand: Engine.activity on the final mono estimates at the model's rate
-- after combine, refine and the beamforming step, before rescale, the resampling back and loudness --, the segments by
native.activity_segments, and with gate=True Engine.activity_gate.  Everything is bit for bit (byte for byte for the
files, character for character for the .rttm); activity=None returns the bits and bytes of the call without the keyword."""
import numpy as np
import pytest
import torch

from ditsep_amd import files, native, wavio
from tests import activity_restatement as ar
from tests import pcm_restatement as pr
from tests.test_gpu_mask_refine import FS, N_STEPS, model  # noqa: F401  (`model` is a fixture)

pytestmark = pytest.mark.gpu
SMALL = dict(n_fft=64, hop=16)
# thresholds close enough to make the tiny network's noise-like stems switch: 3 frames of smoothing, runs and gaps of at
# least 2 frames, a fade of 8 samples
OPTS = dict(SMALL, dominance_db=0.5, hysteresis_db=0.25, smooth=3 * 16 / FS, min_on=2 * 16 / FS, min_off=2 * 16 / FS,
            fade_ms=8000.0 / FS)
GATE = dict(OPTS, gate=True)


def by_hand(eng, est, lens=None, gate=False):
    """est [B, n, L] at the model's rate -> (the estimates, gated or not; per item the segments per source)"""
    opts = native.activity_options(GATE if gate else OPTS)
    fr = native.activity_frames(opts, FS)
    assert fr == dict(min_on=2, min_off=2, pad=0, half_width=1, fade=8)
    res = eng.activity(est, lens=lens, fs=FS, band=opts["band"], half_width=1, range_db=40.0, dominance_db=0.5,
                       hysteresis_db=0.25, min_on=2, min_off=2, pad=0, **SMALL)
    act = res["act"].cpu().numpy()
    B, n, L = est.shape
    segs = [[native.activity_segments(act[b, i], res["frames"][b], 16, L if lens is None else lens[b]) for i in range(n)]
            for b in range(B)]
    out = eng.activity_gate(est, res["act"], lens=lens, hop=16, fade=8) if gate else est
    return out, segs, res


def by_hand_list(eng, ests, gate=False):
    ln = [int(e.shape[-1]) for e in ests]
    ep = torch.zeros((len(ests), 2, max(ln)), device=eng.device)
    for b, e in enumerate(ests):
        ep[b, :, :ln[b]] = e
    out, segs, _ = by_hand(eng, ep, lens=ln, gate=gate)
    return [out[b, :, :ln[b]] for b in range(len(ests))], segs


def check_last(model, segs, gate):
    last = model.last_activity
    assert len(last) == len(segs)
    for item, want in zip(last, segs):
        assert item["segments"] == want and item["options"] == native.activity_options(GATE if gate else OPTS)
        assert item["seconds"] == [[(s / FS, e / FS) for s, e in row] for row in want]
        assert item["active"] == [sum(e - s for s, e in row) / FS for row in want]
        assert len(item["frames_on"]) == 2


def test_separate_with_activity(model):
    eng = model.engine
    g = torch.Generator().manual_seed(91)
    mix = 0.3 * torch.randn((2, 1, 600), generator=g)
    plain, nfe = model.separate(mix, seed=3)
    for gate in (False, True):
        got, nfe_a = model.separate(mix, seed=3, activity=GATE if gate else OPTS)
        want, segs, res = by_hand(eng, plain, gate=gate)
        assert nfe_a == nfe == 2 * N_STEPS and torch.equal(got, want)
        check_last(model, segs, gate)
        on = res["frames_on"].cpu().numpy()
        assert 0 < on.sum() < res["act"].numel()                           # the thresholds do switch these stems
        assert torch.equal(got, plain) != gate
    # the restatement on the device's energies agrees with what the keyword decided
    E = res["energy"][0].cpu().numpy()
    act, _, _ = ar.decide_both(E, half_width=1, consts=ar.constants(40.0, 0.5, 0.25), min_on=2, min_off=2, pad=0)
    assert model.last_activity[0]["segments"] == [ar.segments(act[i], act.shape[1], 16, plain.shape[-1]) for i in range(2)]
    # activity=None is the call without the keyword
    assert torch.equal(model.separate(mix, seed=3, activity=None)[0], plain)
    # with refine=: after it
    ref = model.separate(mix, seed=3, refine=SMALL)[0]
    got = model.separate(mix, seed=3, refine=SMALL, activity=GATE)[0]
    want, segs, _ = by_hand(eng, ref, gate=True)
    assert torch.equal(got, want)
    check_last(model, segs, True)
    # with samples=: after the combine
    comb = model.separate(mix, seed=3, samples=2)[0]
    assert torch.equal(model.separate(mix, seed=3, samples=2, activity=GATE)[0], by_hand(eng, comb, gate=True)[0])
    # with beamform= and track=: after the beamforming step
    arr = 0.3 * torch.randn((2, 4, 600), generator=g)
    trk = dict(block=5 * 16 / FS, context=1)
    bf = model.separate(arr, seed=3, beamform=SMALL, track=trk)[0]
    got = model.separate(arr, seed=3, beamform=SMALL, track=trk, activity=GATE)[0]
    want, segs, _ = by_hand(eng, bf, gate=True)
    assert torch.equal(got, want)
    check_last(model, segs, True)
    sp = model.separate(arr, seed=3, beamform=SMALL, spatial=True)[0]
    assert torch.equal(model.separate(arr, seed=3, beamform=SMALL, spatial=True, activity=GATE)[0],
                       by_hand(eng, sp, gate=True)[0])
    # with loudness=: before it
    got = model.separate(mix, seed=3, activity=GATE, loudness=-23.0)[0]
    gated = by_hand(eng, plain, gate=True)[0]
    hand, _ = eng.loudness_normalize([mix[b].to(eng.device) for b in range(2)], [gated[b] for b in range(2)], FS,
                                     **native.level_options(-23.0, None))
    assert torch.equal(got, torch.stack(hand))
    # at another rate: decided at the model's rate, before the resampling back
    got = model.separate(mix, seed=3, sample_rate=32000, activity=GATE)[0]
    m = eng.resample(mix, 32000, FS, downmix=True)
    est = model.separate(m, seed=3)[0]
    want, segs, _ = by_hand(eng, est, gate=True)
    assert torch.equal(got, eng.resample(want, FS, 32000)[..., :600])
    check_last(model, segs, True)
    # with dereverb=: the first step
    dopts = dict(taps=2, delay=1, iterations=1, n_fft=64, hop=16)
    dry = model.separate(mix, seed=3, dereverb=dopts)[0]
    assert torch.equal(model.separate(mix, seed=3, dereverb=dopts, activity=GATE)[0], by_hand(eng, dry, gate=True)[0])
    for kw, msg in ((dict(stems="mask"), "activity= does not go with stems="),
                    (dict(intermediate=True), "activity= does not go with intermediate"),
                    (dict(activity=False), "activity must be None, True, 'gate' or a dict"),
                    (dict(activity={"n_fft": 4096}), "activity: n_fft = 4096 is not a power of two in")):
        with pytest.raises(ValueError, match=msg):
            model.separate(arr if "stems" in kw else mix, **dict(dict(activity=True), **kw))
    with pytest.raises(ValueError, match="activity= decides on waveforms: with latent=True"):
        model.separate(torch.zeros(1, 64, 75), latent=True, activity=True)


def test_separate_batch_and_long_with_activity(model):
    eng = model.engine
    g = torch.Generator().manual_seed(93)
    mixes = [0.3 * torch.randn((1, L), generator=g) for L in (300, 611, 417)]
    plain, nfe = model.separate_batch(mixes, seed=7)
    for gate in (False, True):
        got, nfe_a = model.separate_batch(mixes, seed=7, activity=GATE if gate else OPTS)
        want, segs = by_hand_list(eng, plain, gate)
        assert nfe == nfe_a and all(torch.equal(a, b) for a, b in zip(got, want))
        check_last(model, segs, gate)
        for b, e in enumerate(plain):                                      # .. and each item what it gets alone
            alone, s1, _ = by_hand(eng, e[None].contiguous(), gate=gate)
            assert torch.equal(alone[0], got[b]) and s1[0] == segs[b]
    again, _ = model.separate_batch(mixes, seed=7, activity=None)
    assert all(torch.equal(a, p) for a, p in zip(again, plain))
    ref, _ = model.separate_batch(mixes, seed=7, refine=SMALL)
    got, _ = model.separate_batch(mixes, seed=7, refine=SMALL, activity=GATE)
    assert all(torch.equal(a, b) for a, b in zip(got, by_hand_list(eng, ref, True)[0]))
    rates = [32000, FS, 8000]
    got, _ = model.separate_batch(mixes, seed=7, sample_rates=rates, activity=GATE)
    at_fs = eng.to_model_rate(mixes, rates, FS)
    est, _ = model.separate_batch(at_fs, seed=7)
    want, segs = by_hand_list(eng, est, True)
    hand = eng.from_model_rate(want, rates, FS, [m.shape[-1] for m in mixes])
    assert all(torch.equal(a, b) for a, b in zip(got, hand))
    check_last(model, segs, True)
    arrs = [0.3 * torch.randn((c, L), generator=g) for c, L in ((4, 300), (2, 611))]
    trk = dict(block=5 * 16 / FS, context=1)
    bf, _ = model.separate_batch(arrs, seed=7, beamform=SMALL, track=trk)
    got, _ = model.separate_batch(arrs, seed=7, beamform=SMALL, track=trk, activity=GATE, loudness=-23.0)
    gated = by_hand_list(eng, bf, True)[0]
    hand, _ = eng.loudness_normalize([a[:1].to(eng.device).contiguous() for a in arrs], gated, FS,
                                     **native.level_options(-23.0, None))
    assert all(torch.equal(a, b) for a, b in zip(got, hand))
    # long recordings, both modes: over the whole recording, after the stitch
    rec = [0.3 * torch.randn((1, 700), generator=g), 0.3 * torch.randn((1, 450), generator=g)]
    for mode in ("stitch", "score"):
        kw = dict(window=256, overlap=64, mode=mode, batch=3, seed=9)
        plain, nfe = model.separate_long(rec, **kw)
        for gate in (False, True):
            got, nfe_a = model.separate_long(rec, activity=GATE if gate else OPTS, **kw)
            want, segs = by_hand_list(eng, plain, gate)
            assert nfe == nfe_a and all(torch.equal(a, b) for a, b in zip(got, want))
            check_last(model, segs, gate)
        one, _ = model.separate_long(rec[0], activity=GATE, **kw)
        assert torch.is_tensor(one) and torch.equal(one, by_hand_list(eng, [model.separate_long(rec[0], **kw)[0]], True)[0][0])
        again, _ = model.separate_long(rec, activity=None, **kw)
        assert all(torch.equal(a, b) for a, b in zip(again, plain))
        ref, _ = model.separate_long(rec, refine=SMALL, **kw)
        got, _ = model.separate_long(rec, refine=SMALL, activity=GATE, **kw)
        assert all(torch.equal(a, b) for a, b in zip(got, by_hand_list(eng, ref, True)[0]))
    with pytest.raises(ValueError, match="activity= does not go with stems="):
        model.separate_batch(arrs, activity=True, stems="mask")
    with pytest.raises(ValueError, match="activity= does not go with intermediate"):
        model.separate_long(rec, window=256, activity=True, intermediate=True)
    with pytest.raises(ValueError, match=r"activity: item 0 has 20 samples, outside \[n_fft / 2 \+ 1 = 33"):
        eng.activity(torch.zeros(1, 2, 20), **SMALL)


def test_separate_files_with_activity(model, tmp_path):
    eng = model.engine
    g = np.random.default_rng(97)
    src = tmp_path / "in"
    src.mkdir()
    wavio.write_wav(src / "a.wav", (0.3 * g.standard_normal(900) * 2 ** 15).astype("<i2").tobytes(), 44100, 1, "s16")
    wavio.write_wav(src / "b.wav", (0.3 * g.standard_normal(300) * 2 ** 15).astype("<i2").tobytes(), FS, 1, "s16")
    wavio.write_wav(src / "c.wav", (0.3 * g.standard_normal(260)).astype("<f4").tobytes(), 8000, 1, "f32")
    paths = sorted(src.glob("*.wav"))
    hs = [wavio.read_header(p) for p in paths]
    for kw, msg in ((dict(activity=True, stems="mask"), "activity= does not go with stems="),
                    (dict(activity={"frames": 2}), r"activity: unknown keys \['frames'\]"),
                    (dict(activity=dict(n_fft=2048, hop=512)), "samples at the model's rate; activity= needs at least "
                                                               "n_fft / 2 \\+ 1 = 1025")):
        with pytest.raises(ValueError, match=msg):
            model.separate_files(paths, tmp_path / "never", **kw)
    assert not (tmp_path / "never").exists()
    plan = files.plan_files(hs, FS, 8, batch=2)

    def hand(gate, rescale, loud):
        want, lines = {}, {}
        for k, idx in enumerate(plan["batches"]):
            clips = [torch.from_numpy(pr.decode(wavio.read_payload(paths[i], hs[i]), hs[i].frames, hs[i].channels,
                                                hs[i].encoding)) for i in idx]
            rates, frames = [hs[i].rate for i in idx], [hs[i].frames for i in idx]
            at_fs = eng.to_model_rate(clips, rates, FS)
            est, _ = model.separate_batch(at_fs, codec="padded", seed=5 + k)
            est = eng.mask_refine(at_fs, est, **SMALL)
            est, segs = by_hand_list(eng, list(est), gate)
            if rescale:
                sep, lens = files._padded(est, eng.device)
                scaled, _ = eng.scale_output(files._padded(at_fs, eng.device)[0], sep, lens)
                est = [scaled[j, :, :lens[j]] for j in range(len(idx))]
            back = eng.from_model_rate(est, rates, FS, frames)
            if loud is not None:
                back, _ = eng.loudness_normalize(clips, back, rates, **native.level_options(loud, None))
            for j, i in enumerate(idx):
                want[i] = [pr.quantise(back[j][s].cpu().numpy(), "s16") for s in range(2)]
                lines[i] = (ar.rttm_lines(paths[i].stem, segs[j], FS), segs[j])
        return want, lines

    for tag, gate, rescale, loud in (("seg", False, False, None), ("gate", True, False, None), ("scaled", True, True, None),
                                     ("level", True, False, -23.0)):
        out = tmp_path / tag
        recs = model.separate_files(paths, out, batch=2, seed=5, refine=SMALL, activity=GATE if gate else OPTS,
                                    rescale=rescale, loudness=loud)
        want, lines = hand(gate, rescale, loud)
        for i, p in enumerate(paths):
            text, segs = lines[i]
            assert (out / (p.stem + ".rttm")).read_text() == "".join(t + "\n" for t in text)
            assert recs[i]["activity"] == dict(segments=[[(s / FS, e / FS) for s, e in row] for row in segs],
                                               active=[sum(e - s for s, e in row) / FS for row in segs])
            for s in range(2):
                q = out / f"s{s}" / p.name
                assert wavio.read_payload(q, wavio.read_header(q)) == want[i][s][0], f"{q}: not the hand-made output"
    # without the keyword: no record entry, no .rttm, and with gate=False the bytes of the call without it
    old = model.separate_files(paths, tmp_path / "old", batch=2, seed=5, refine=SMALL)
    none = model.separate_files(paths, tmp_path / "none", batch=2, seed=5, refine=SMALL, activity=None)
    assert "activity" not in old[0] and set(old[0]) == set(none[0]) and not list((tmp_path / "old").glob("*.rttm"))
    differs = False
    for p in paths:
        for s in range(2):
            a = (tmp_path / "old" / f"s{s}" / p.name).read_bytes()
            assert a == (tmp_path / "none" / f"s{s}" / p.name).read_bytes() == (tmp_path / "seg" / f"s{s}" / p.name).read_bytes()
            differs = differs or a != (tmp_path / "gate" / f"s{s}" / p.name).read_bytes()
    assert differs
    # a file with no active speaker gets an empty .rttm
    wavio.write_wav(src / "z.wav", np.zeros(400, "<i2").tobytes(), FS, 1, "s16")
    recs = model.separate_files([src / "z.wav"], tmp_path / "quiet", seed=5, activity=dict(OPTS, range_db=0.0, min_on=1.0))
    assert (tmp_path / "quiet" / "z.rttm").read_text() == "" and recs[0]["activity"]["segments"] == [[], []]
