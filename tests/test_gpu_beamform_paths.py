"""The `beamform` keyword of LatentDiffSep (separate, separate_batch, separate_long, separate_files) on the tiny test
network against the same steps done by hand: the model separates channel `ref`, Engine.beamform filters all channels at
the model's rate after combine and refine and before rescale, the resampling back, loudness and limit.  Everything is
bit for bit (byte for byte for the files); beamform=None returns the bits and bytes of the call without the keyword."""
import numpy as np
import pytest
import torch

from ditsep_amd import files, native, wavio
from tests import pcm_restatement as pr
from tests.test_gpu_mask_refine import FS, N_STEPS, model  # noqa: F401  (`model` is a fixture)

pytestmark = pytest.mark.gpu


def fit(x, L):
    return torch.nn.functional.pad(x, (0, L - x.shape[-1])) if x.shape[-1] < L else x[..., :L]


def test_separate_with_beamform(model):
    eng = model.engine
    g = torch.Generator().manual_seed(61)
    mix = 0.3 * torch.randn((2, 4, 600), generator=g)
    dev = mix.to(eng.device)
    for beamform, ref, kw in ((True, 0, {}), (2, 2, {}),
                              (dict(ref=3, n_fft=64, hop=16, power=1, reg=1e-2, postfilter="mask"), 3,
                               dict(n_fft=64, hop=16, power=1, reg=1e-2, postfilter="mask"))):
        plain, nfe = model.separate(dev[:, ref:ref + 1].contiguous(), seed=3)
        got, nfe_b = model.separate(mix, seed=3, beamform=beamform)
        assert nfe_b == nfe == 2 * N_STEPS and tuple(got.shape) == (2, 2, 608)
        want = eng.beamform(fit(dev, 608), plain, ref=ref, **kw)
        assert torch.equal(got, want) and not torch.equal(got, plain)
    # with samples= and refine=: on the mono estimates of channel ref, before the beamformer
    one = dev[:, 1:2].contiguous()
    comb, _, info = model.separate(one, seed=3, samples=2, refine=True, return_info=True)
    got, _, info_b = model.separate(mix, seed=3, samples=2, refine=True, return_info=True, beamform=1)
    assert torch.equal(got, eng.beamform(fit(dev, 608), comb, ref=1)) and sorted(info_b) == sorted(info)
    # beamform=None is the old path, before and after
    plain, _ = model.separate(one, seed=3)
    assert torch.equal(model.separate(one, seed=3, beamform=None)[0], plain)
    assert torch.equal(model.separate(one, seed=3)[0], plain)
    # at another rate: the channels are resampled with the channels kept, the outputs taken back
    x = 0.3 * torch.randn((1, 3, 1300), generator=g)
    mc = eng.resample(x, 32000, FS)
    sep = model.separate(mc[:, 2:3].contiguous(), seed=5)[0]
    hand = eng.resample(eng.beamform(fit(mc, sep.shape[-1]), sep, ref=2), FS, 32000)[..., :1300]
    assert torch.equal(model.separate(x, seed=5, sample_rate=32000, beamform=2)[0], hand)
    # loudness and limit see the mono estimates; link "mixture" measures channel ref at the rate of the call
    got, _, info = model.separate(mix, seed=3, beamform=2, loudness=-23.0, limit=True, return_info=True)
    bf = model.separate(mix, seed=3, beamform=2)[0]
    hand, hinfo = eng.loudness_normalize([dev[b, 2:3] for b in range(2)], [bf[b] for b in range(2)], FS,
                                         **native.level_options(-23.0, True))
    assert torch.equal(got, torch.stack(hand)) and info["gain_db"] == hinfo["gain_db"]
    for kw, msg in ((dict(stems="mask"), "beamform= does not go with stems="),
                    (dict(intermediate=True), "beamform= does not go with intermediate"),
                    (dict(beamform=4), r"beamform: ref = 4 outside \[0, 4\): item 0 has 4 channels"),
                    (dict(beamform=False), "beamform must be None, True, a reference channel or a dict"),
                    (dict(beamform={"postfilter": "wiener"}), "beamform: postfilter must be")):
        with pytest.raises(ValueError, match=msg):
            model.separate(mix, **dict(dict(beamform=True), **kw))
    with pytest.raises(ValueError, match="with latent=True there is no mixture to filter"):
        model.separate(torch.zeros(1, 64, 75), latent=True, beamform=True)
    with pytest.raises(ValueError, match=r"beamform= takes mix \[B, C, L\]"):
        model.separate(torch.zeros(2, 600), beamform=True)
    with pytest.raises(ValueError, match=r"item 0 has 9 channels, outside \[1, 8\]"):
        model.separate(torch.zeros(1, 9, 600), beamform=True)


def test_separate_batch_and_long_with_beamform(model):
    eng = model.engine
    g = torch.Generator().manual_seed(63)
    mixes = [0.3 * torch.randn((c, L), generator=g) for c, L in ((4, 300), (2, 611), (8, 417))]
    ones = [m[1:2].to(eng.device).contiguous() for m in mixes]
    plain, nfe = model.separate_batch(ones, seed=7)
    got, nfe_b = model.separate_batch(mixes, seed=7, beamform=1)
    want = eng.beamform([m.to(eng.device) for m in mixes], plain, ref=1)
    assert nfe == nfe_b
    for b, m in enumerate(mixes):
        assert tuple(got[b].shape) == (2, m.shape[-1]) and torch.equal(got[b], want[b])
        assert torch.equal(got[b], eng.beamform(m[None], plain[b][None], ref=1)[0])      # .. and the item alone
    again, _ = model.separate_batch(ones, seed=7)
    assert all(torch.equal(a, p) for a, p in zip(again, plain))
    again, _ = model.separate_batch(ones, seed=7, beamform=None)
    assert all(torch.equal(a, p) for a, p in zip(again, plain))
    # at other rates, mixed channel counts
    rates = [32000, FS, 8000]
    opts = dict(ref=1, n_fft=128, hop=32, postfilter="mask")                            # 300 samples at 32 kHz are 150
    got, _ = model.separate_batch(mixes, seed=7, sample_rates=rates, beamform=opts)
    mc = eng.to_model_rate(mixes, rates, FS, downmix=False)
    est, _ = model.separate_batch([m[1:2].contiguous() for m in mc], seed=7)
    hand = eng.from_model_rate(eng.beamform(mc, est, **opts), rates, FS, [m.shape[-1] for m in mixes])
    for b, m in enumerate(mixes):
        assert tuple(got[b].shape) == (2, m.shape[-1]) and torch.equal(got[b], hand[b])
    # long recordings: after the stitch (or the single decode of mode="score")
    rec = [0.3 * torch.randn((3, 700), generator=g), 0.3 * torch.randn((1, 450), generator=g)]
    for mode in ("stitch", "score"):
        kw = dict(window=256, overlap=64, mode=mode, batch=3, seed=9)
        plain, nfe = model.separate_long([r[:1].to(eng.device).contiguous() for r in rec], **kw)
        got, nfe_b = model.separate_long(rec, beamform=True, **kw)
        want = eng.beamform([r.to(eng.device) for r in rec], plain)
        assert nfe == nfe_b and all(torch.equal(a, b) for a, b in zip(got, want))
        one, _ = model.separate_long(rec[0], beamform=True, **kw)
        alone, _ = model.separate_long(rec[0][:1].to(eng.device).contiguous(), **kw)     # (its windows, pooled alone)
        assert tuple(one.shape) == (2, 700) and torch.equal(one, eng.beamform(rec[0][None], alone[None])[0])
        again, _ = model.separate_long([r[:1].to(eng.device).contiguous() for r in rec], beamform=None, **kw)
        assert all(torch.equal(a, b) for a, b in zip(again, plain))
    with pytest.raises(ValueError, match="beamform= does not go with stems="):
        model.separate_batch(mixes, beamform=True, stems="mask")
    with pytest.raises(ValueError, match=r"beamform: ref = 2 outside \[0, 2\): item 1 has 2 channels"):
        model.separate_batch(mixes, beamform=2)
    with pytest.raises(ValueError, match="beamform= does not go with intermediate"):
        model.separate_long(rec, window=256, beamform=True, intermediate=True)
    with pytest.raises(ValueError, match=r"beamform: ref = 1 outside \[0, 1\): item 1 has 1 channels"):
        model.separate_long(rec, window=256, beamform=1)


def test_separate_files_with_beamform(model, tmp_path):
    eng = model.engine
    g = np.random.default_rng(67)
    src = tmp_path / "in"
    src.mkdir()
    wavio.write_wav(src / "a.wav", (0.3 * g.standard_normal(4 * 900) * 2 ** 15).astype("<i2").tobytes(), 44100, 4, "s16")
    wavio.write_wav(src / "b.wav", (0.3 * g.standard_normal(2 * 300) * 2 ** 15).astype("<i2").tobytes(), FS, 2, "s16")
    wavio.write_wav(src / "c.wav", (0.3 * g.standard_normal(8 * 260)).astype("<f4").tobytes(), 8000, 8, "f32")
    paths = sorted(src.glob("*.wav"))
    hs = [wavio.read_header(p) for p in paths]
    assert [(h.rate, h.channels, h.encoding) for h in hs] == [(44100, 4, "s16"), (FS, 2, "s16"), (8000, 8, "f32")]
    opts = dict(ref=1, n_fft=128, hop=32)                                               # c.wav has 520 samples at 16 kHz
    for kw, msg in ((dict(beamform=opts, stems="mask"), "beamform= does not go with stems="),
                    (dict(beamform=2), r"b\.wav: 2 channels; beamform= has ref = 2 outside \[0, 2\)"),
                    (dict(beamform={"n_fft": 1024, "hop": 256}), r"beamform= needs at least n_fft / 2 \+ 1 = 513"),
                    (dict(beamform={"postfilter": "wiener"}), "beamform: postfilter must be"),
                    (dict(beamform={"reg": -1.0}), "beamform: reg = -1.0 is not a finite number >= 0")):
        with pytest.raises(ValueError, match=msg):
            model.separate_files(paths, tmp_path / "never", **kw)
    assert not (tmp_path / "never").exists()
    plan = files.plan_files(hs, FS, 8, batch=2)
    assert sorted(i for b in plan["batches"] for i in b) == [0, 1, 2] and len(plan["batches"]) == 2

    def by_hand(rescale, loud):
        want = {}
        for k, idx in enumerate(plan["batches"]):
            clips = [torch.from_numpy(pr.decode(wavio.read_payload(paths[i], hs[i]), hs[i].frames, hs[i].channels,
                                                hs[i].encoding)) for i in idx]
            rates, frames = [hs[i].rate for i in idx], [hs[i].frames for i in idx]
            mc = eng.to_model_rate(clips, rates, FS, downmix=False)
            one = [m[1:2].contiguous() for m in mc]
            est, _ = model.separate_batch(one, codec="padded", seed=5 + k)
            est = eng.beamform(mc, eng.mask_refine(one, est), **opts)
            if rescale:
                lens = [int(e.shape[-1]) for e in est]
                sep = torch.zeros((len(idx), 2, max(lens)), device=eng.device)
                mono = torch.zeros((len(idx), 1, max(lens)), device=eng.device)
                for j, e in enumerate(est):
                    sep[j, :, :lens[j]], mono[j, :, :lens[j]] = e, one[j]
                scaled, _ = eng.scale_output(mono, sep, lens)
                est = [scaled[j, :, :lens[j]] for j in range(len(idx))]
            back = eng.from_model_rate(est, rates, FS, frames)
            if loud is not None:
                back, _ = eng.loudness_normalize([c[1:2].to(eng.device).contiguous() for c in clips], back, rates,
                                                 **native.level_options(loud, None))
            for j, i in enumerate(idx):
                want[i] = [pr.quantise(back[j][s].cpu().numpy(), "s16") for s in range(2)]
        return want

    for tag, rescale, loud in (("plain", False, None), ("levelled", True, -23.0)):
        out = tmp_path / tag
        recs = model.separate_files(paths, out, batch=2, seed=5, refine=True, beamform=opts, rescale=rescale,
                                    loudness=loud)
        want = by_hand(rescale, loud)
        for i, p in enumerate(paths):
            assert recs[i]["beamform"] == 1 and recs[i]["channels"] == hs[i].channels
            for s in range(2):
                q = out / f"s{s}" / p.name
                ho = wavio.read_header(q)
                assert ho[:4] == (hs[i].rate, 1, hs[i].frames, "s16")                    # mono, the input's rate and frames
                assert wavio.read_payload(q, ho) == want[i][s][0], f"{q} is not the quantised beamformed estimate"
                assert recs[i]["clipped"][s] == want[i][s][1]
    # beamform=None: the keys and the bytes of the call without the keyword
    a = model.separate_files(paths, tmp_path / "none", batch=2, seed=5, beamform=None)
    b = model.separate_files(paths, tmp_path / "old", batch=2, seed=5)
    assert set(a[0]) == set(b[0]) == {"path", "rate", "channels", "frames", "outputs", "clipped", "batch"}
    for p in paths:
        for s in range(2):
            assert (tmp_path / "none" / f"s{s}" / p.name).read_bytes() == (tmp_path / "old" / f"s{s}" / p.name).read_bytes()
            assert (tmp_path / "none" / f"s{s}" / p.name).read_bytes() != (tmp_path / "plain" / f"s{s}" / p.name).read_bytes()
