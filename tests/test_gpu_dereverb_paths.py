"""The `dereverb` keyword of LatentDiffSep (separate, separate_batch, separate_long, separate_files) on the tiny test
network against the same steps done by hand: the mixture goes to the model's rate with its channels kept,
Engine.dereverb runs once per recording, the existing call runs on the result at the model's rate (on native.downmix of
the channels, or on the channels with stems= and beamform=), and the outputs go back; loudness stays the last step and
keeps measuring the input as given.  Everything is bit for bit (byte for byte for the files); dereverb=None returns the
bits and bytes of the call without the keyword."""
import numpy as np
import pytest
import torch

from ditsep_amd import files, native, wavio
from tests import pcm_restatement as pr
from tests.test_gpu_mask_refine import FS, N_STEPS, model  # noqa: F401  (`model` is a fixture)

pytestmark = pytest.mark.gpu
OPTS = dict(taps=3, delay=1, iterations=2, n_fft=64, hop=16)
FULL = dict(native.DEREVERB_DEFAULTS, **OPTS)


def test_separate_with_dereverb(model):
    eng = model.engine
    g = torch.Generator().manual_seed(71)
    mix = 0.3 * torch.randn((2, 4, 600), generator=g)
    dev = mix.to(eng.device)
    dry = eng.dereverb(dev, **OPTS)
    assert not torch.equal(dry, dev)
    # alone: the model separates the downmix of the dereverberated channels
    plain, nfe = model.separate(native.downmix(dry), seed=3)
    got, nfe_d = model.separate(mix, seed=3, dereverb=OPTS)
    assert nfe_d == nfe == 2 * N_STEPS and tuple(got.shape) == (2, 2, 608) and torch.equal(got, plain)
    assert not torch.equal(got, model.separate(native.downmix(dev), seed=3)[0])
    # the defaults, and a mono mixture [B, L] as one channel
    long = 0.3 * torch.randn((1, 2, 1200), generator=g)
    want = model.separate(native.downmix(eng.dereverb(long.to(eng.device))), seed=3)[0]
    assert torch.equal(model.separate(long, seed=3, dereverb=True)[0], want)
    mono = mix[:, 0].contiguous()
    want = model.separate(eng.dereverb(mono[:, None].to(eng.device), **OPTS), seed=3)[0]
    assert torch.equal(model.separate(mono, seed=3, dereverb=OPTS)[0], want)
    # with samples= and refine=: they see the dereverberated downmix
    want, _, info = model.separate(native.downmix(dry), seed=3, samples=2, refine=True, return_info=True)
    got, _, info_d = model.separate(mix, seed=3, samples=2, refine=True, return_info=True, dereverb=OPTS)
    assert torch.equal(got, want) and sorted(info_d) == sorted(info)
    # with beamform= and stems=: they see the dereverberated channels
    assert torch.equal(model.separate(mix, seed=3, dereverb=OPTS, beamform=2)[0], model.separate(dry, seed=3, beamform=2)[0])
    st = model.separate(mix, seed=3, dereverb=OPTS, stems="mask")[0]
    assert tuple(st.shape) == (2, 2, 4, 608) and torch.equal(st, model.separate(dry, seed=3, stems="mask")[0])
    # dereverb=None is the old path
    one = dev[:, :1].contiguous()
    assert torch.equal(model.separate(one, seed=3, dereverb=None)[0], model.separate(one, seed=3)[0])
    # at another rate: the channels are resampled with the channels kept, the outputs taken back
    x = 0.3 * torch.randn((1, 3, 1300), generator=g)
    mc = eng.dereverb(eng.resample(x, 32000, FS), **OPTS)
    sep = model.separate(native.downmix(mc), seed=5)[0]
    assert torch.equal(model.separate(x, seed=5, sample_rate=32000, dereverb=OPTS)[0],
                       eng.resample(sep, FS, 32000)[..., :1300])
    sep = model.separate(mc, seed=5, stems="mask")[0]
    hand = eng.resample(sep.reshape(1, 6, -1), FS, 32000)[..., :1300].reshape(1, 2, 3, 1300)
    assert torch.equal(model.separate(x, seed=5, sample_rate=32000, dereverb=OPTS, stems="mask")[0], hand)
    # loudness is the last step; link "mixture" measures the mixture as given
    x2 = mix[:, :2].contiguous()
    got, _, info = model.separate(x2, seed=3, dereverb=OPTS, loudness=-23.0, return_info=True)
    est = model.separate(x2, seed=3, dereverb=OPTS)[0]
    hand, hinfo = eng.loudness_normalize([x2[b].to(eng.device) for b in range(2)], [est[b] for b in range(2)], FS,
                                         **native.level_options(-23.0, None))
    assert torch.equal(got, torch.stack(hand)) and info["gain_db"] == hinfo["gain_db"]
    for kw, msg in ((dict(intermediate=True), "dereverb= does not go with intermediate"),
                    (dict(dereverb=False), "dereverb must be None, True or a dict"),
                    (dict(dereverb={"window": 1}), r"dereverb: unknown keys \['window'\]")):
        with pytest.raises(ValueError, match=msg):
            model.separate(mix, **dict(dict(dereverb=OPTS), **kw))
    with pytest.raises(ValueError, match=r"needs at least n_fft / 2 \+ 1 = 257"):
        model.separate(mix[..., :200], dereverb=True)
    with pytest.raises(ValueError, match="with latent=True there is no mixture to filter"):
        model.separate(torch.zeros(1, 64, 75), latent=True, dereverb=True)
    with pytest.raises(ValueError, match=r"item 0 has 9 channels, outside \[1, 8\]"):
        model.separate(torch.zeros(1, 9, 600), dereverb=OPTS)


def test_separate_batch_and_long_with_dereverb(model):
    eng = model.engine
    g = torch.Generator().manual_seed(73)
    mixes = [0.3 * torch.randn((c, L), generator=g) for c, L in ((4, 300), (2, 611), (8, 417))]
    dry = eng.dereverb([m.to(eng.device) for m in mixes], **OPTS)
    down = [native.downmix(d[None])[0] for d in dry]
    plain, nfe = model.separate_batch(down, seed=7)
    got, nfe_d = model.separate_batch(mixes, seed=7, dereverb=OPTS)
    assert nfe == nfe_d
    for b, m in enumerate(mixes):
        assert tuple(got[b].shape) == (2, m.shape[-1]) and torch.equal(got[b], plain[b])
        assert torch.equal(dry[b], eng.dereverb(m[None], **OPTS)[0])                    # .. and the item alone
    ones = [m[:1].to(eng.device).contiguous() for m in mixes]
    old, _ = model.separate_batch(ones, seed=7)
    again, _ = model.separate_batch(ones, seed=7, dereverb=None)
    assert all(torch.equal(a, p) for a, p in zip(again, old))
    # with beamform= and stems=, at other rates, mixed channel counts
    rates = [32000, FS, 8000]
    mc = eng.dereverb(eng.to_model_rate(mixes, rates, FS, downmix=False), **OPTS)
    lengths = [m.shape[-1] for m in mixes]
    est, _ = model.separate_batch([native.downmix(m[None])[0] for m in mc], seed=7)
    got, _ = model.separate_batch(mixes, seed=7, sample_rates=rates, dereverb=OPTS)
    hand = eng.from_model_rate(est, rates, FS, lengths)
    assert all(torch.equal(a, b) for a, b in zip(got, hand))
    bopts = dict(ref=1, n_fft=128, hop=32)
    got, _ = model.separate_batch(mixes, seed=7, sample_rates=rates, dereverb=OPTS, beamform=bopts)
    hand = eng.from_model_rate(model.separate_batch(mc, seed=7, beamform=bopts)[0], rates, FS, lengths)
    assert all(tuple(a.shape) == (2, L) and torch.equal(a, b) for a, b, L in zip(got, hand, lengths))
    sopts = dict(mode="mask", n_fft=128, hop=32)
    got, _ = model.separate_batch(mixes, seed=7, sample_rates=rates, dereverb=OPTS, stems=sopts)
    hand = eng.stems_from_model_rate(model.separate_batch(mc, seed=7, stems=sopts)[0], rates, FS, lengths)
    assert all(tuple(a.shape) == (2, m.shape[0], m.shape[1]) and torch.equal(a, b) for a, b, m in zip(got, hand, mixes))
    # loudness: the last step, on the mixtures as given
    two = [m[:2].to(eng.device).contiguous() for m in mixes]
    got, _, info = model.separate_batch(two, seed=7, dereverb=OPTS, loudness=-20.0, return_info=True)
    est, _ = model.separate_batch(two, seed=7, dereverb=OPTS)
    hand, hinfo = eng.loudness_normalize(two, est, FS, **native.level_options(-20.0, None))
    assert all(torch.equal(a, b) for a, b in zip(got, hand)) and info["gain_db"] == hinfo["gain_db"]
    # long recordings: dereverberated whole, before any windowing, in both modes
    rec = [0.3 * torch.randn((3, 700), generator=g), 0.3 * torch.randn((1, 450), generator=g)]
    dry = eng.dereverb([r.to(eng.device) for r in rec], **OPTS)
    for mode in ("stitch", "score"):
        kw = dict(window=256, overlap=64, mode=mode, batch=3, seed=9)
        plain, nfe = model.separate_long([native.downmix(d[None])[0] for d in dry], **kw)
        got, nfe_d = model.separate_long(rec, dereverb=OPTS, **kw)
        assert nfe == nfe_d and all(torch.equal(a, b) for a, b in zip(got, plain))
        one, _ = model.separate_long(rec[0], dereverb=OPTS, **kw)
        alone, _ = model.separate_long(native.downmix(dry[0][None])[0], **kw)            # (its windows, pooled alone)
        assert tuple(one.shape) == (2, 700) and torch.equal(one, alone)
        got, _ = model.separate_long(rec, dereverb=OPTS, beamform=True, **kw)
        want, _ = model.separate_long(list(dry), beamform=True, **kw)
        assert all(torch.equal(a, b) for a, b in zip(got, want))
        mono = [r[:1].to(eng.device).contiguous() for r in rec]
        old, _ = model.separate_long(mono, **kw)
        again, _ = model.separate_long(mono, dereverb=None, **kw)
        assert all(torch.equal(a, b) for a, b in zip(again, old))
    with pytest.raises(ValueError, match=r"dereverb: item 1 has 9 channels, outside \[1, 8\]"):
        model.separate_batch([mixes[0], torch.zeros(9, 300)], dereverb=OPTS)
    with pytest.raises(ValueError, match="dereverb= does not go with intermediate"):
        model.separate_long(rec, window=256, dereverb=OPTS, intermediate=True)
    with pytest.raises(ValueError, match=r"dereverb: item 0 has 150 samples at the model's rate; dereverb= needs at "
                                         r"least n_fft / 2 \+ 1 = 257"):
        model.separate_batch(mixes, sample_rates=rates, dereverb=True)


def test_separate_files_with_dereverb(model, tmp_path):
    eng = model.engine
    g = np.random.default_rng(77)
    src = tmp_path / "in"
    src.mkdir()
    wavio.write_wav(src / "a.wav", (0.3 * g.standard_normal(4 * 900) * 2 ** 15).astype("<i2").tobytes(), 44100, 4, "s16")
    wavio.write_wav(src / "b.wav", (0.3 * g.standard_normal(2 * 300) * 2 ** 15).astype("<i2").tobytes(), FS, 2, "s16")
    wavio.write_wav(src / "c.wav", (0.3 * g.standard_normal(8 * 260)).astype("<f4").tobytes(), 8000, 8, "f32")
    paths = sorted(src.glob("*.wav"))
    hs = [wavio.read_header(p) for p in paths]
    for kw, msg in ((dict(dereverb={"n_fft": 1024, "hop": 256}), r"dereverb= needs at least n_fft / 2 \+ 1 = 513"),
                    (dict(dereverb={"taps": 11}), r"dereverb: C taps = 8 x 11 = 88 unknowns per bin"),
                    (dict(dereverb={"reg": -1.0}), "dereverb: reg = -1.0 is not a finite number >= 0"),
                    (dict(dereverb=False), "dereverb must be None, True or a dict")):
        with pytest.raises(ValueError, match=msg):
            model.separate_files(paths, tmp_path / "never", **kw)
    assert not (tmp_path / "never").exists()
    plan = files.plan_files(hs, FS, 8, batch=2)
    assert sorted(i for b in plan["batches"] for i in b) == [0, 1, 2] and len(plan["batches"]) == 2
    bopts = dict(ref=1, n_fft=128, hop=32)
    sopts = dict(mode="mask", n_fft=128, hop=32)

    def by_hand(beam, stems, loud):
        want = {}
        for k, idx in enumerate(plan["batches"]):
            clips = [torch.from_numpy(pr.decode(wavio.read_payload(paths[i], hs[i]), hs[i].frames, hs[i].channels,
                                                hs[i].encoding)) for i in idx]
            rates, frames = [hs[i].rate for i in idx], [hs[i].frames for i in idx]
            mc = eng.dereverb(eng.to_model_rate(clips, rates, FS, downmix=False), **OPTS)
            one = [m[1:2].contiguous() for m in mc] if beam else [native.downmix(m[None])[0] for m in mc]
            est, _ = model.separate_batch(one, codec="padded", seed=5 + k)
            if stems:
                back = eng.stems_from_model_rate(eng.stems(mc, est, **sopts), rates, FS, frames)
            else:
                back = eng.from_model_rate(eng.beamform(mc, est, **bopts) if beam else est, rates, FS, frames)
            if loud is not None:
                back, _ = eng.loudness_normalize([c.to(eng.device) for c in clips], back, rates,
                                                 **native.level_options(loud, None))
            for j, i in enumerate(idx):
                if stems:    # interleaved frames
                    want[i] = [pr.quantise(back[j][s].t().contiguous().cpu().numpy().reshape(-1), "s16") for s in range(2)]
                else:
                    want[i] = [pr.quantise(back[j][s].cpu().numpy(), "s16") for s in range(2)]
        return want

    for tag, beam, stems, loud in (("plain", False, False, None), ("beam", True, False, None),
                                   ("stems", False, True, None)):
        out = tmp_path / tag
        recs = model.separate_files(paths, out, batch=2, seed=5, dereverb=OPTS, beamform=bopts if beam else None,
                                    stems=sopts if stems else None, loudness=loud)
        want = by_hand(beam, stems, loud)
        for i, p in enumerate(paths):
            assert recs[i]["dereverb"] == FULL and recs[i]["channels"] == hs[i].channels
            for s in range(2):
                q = out / f"s{s}" / p.name
                ho = wavio.read_header(q)
                assert ho[:4] == (hs[i].rate, hs[i].channels if stems else 1, hs[i].frames, "s16")
                assert wavio.read_payload(q, ho) == want[i][s][0], f"{q} is not the quantised estimate done by hand"
    # with loudness= (link "mixture" measures the file as given: at most 2 channels)
    out = tmp_path / "levelled"
    recs = model.separate_files(paths[1:2], out, batch=2, seed=5, dereverb=OPTS, loudness=-23.0)
    clip = torch.from_numpy(pr.decode(wavio.read_payload(paths[1], hs[1]), hs[1].frames, 2, "s16"))
    mc = eng.dereverb([clip.to(eng.device)], **OPTS)
    est, _ = model.separate_batch([native.downmix(mc[0][None])[0]], codec="padded", seed=5)
    back, info = eng.loudness_normalize([clip.to(eng.device)], est, [FS], **native.level_options(-23.0, None))
    assert recs[0]["gain_db"] == info["gain_db"][0]
    for s in range(2):
        q = out / f"s{s}" / paths[1].name
        assert wavio.read_payload(q, wavio.read_header(q)) == pr.quantise(back[0][s].cpu().numpy(), "s16")[0]
    # dereverb=None: the keys and the bytes of the call without the keyword
    a = model.separate_files(paths, tmp_path / "none", batch=2, seed=5, dereverb=None)
    b = model.separate_files(paths, tmp_path / "old", batch=2, seed=5)
    assert set(a[0]) == set(b[0]) == {"path", "rate", "channels", "frames", "outputs", "clipped", "batch"}
    for p in paths:
        for s in range(2):
            assert (tmp_path / "none" / f"s{s}" / p.name).read_bytes() == (tmp_path / "old" / f"s{s}" / p.name).read_bytes()
            assert (tmp_path / "none" / f"s{s}" / p.name).read_bytes() != (tmp_path / "plain" / f"s{s}" / p.name).read_bytes()
