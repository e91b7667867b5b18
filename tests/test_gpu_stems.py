"""dsn_stems and dsn_pcm_encode_frames (ditsep_amd/csrc/maskrefine.hip, pcm.hip) through Engine.stems and
Engine.pcm_encode_frames on an engine with no score network and no codec, against the restatement
(tests/stems_restatement.py), and the `stems` keyword of LatentDiffSep against the same steps done by hand.

Bounds.  The error of a result is its largest absolute difference from the float64 restatement divided by the peak of
|mix|; the consistency error is that of sum_i out_i against the mixture, per channel.  Each may be at most 8 x what the
float32 run of the same restatement shows on the same input (float32 pocketfft transforms and masks, float64 statistics
and solve: the device's own split of precisions) -- the rule and the factor of tests/test_gpu_mask_refine.py, for the
same reason: the device's radix-2 butterfly order and its fused multiply-adds differ from pocketfft's.  The spatial
covariances and their denominators are held to the same rule relative to their largest entry.  Everything else -- mask
mode against Engine.mask_refine per channel, silent estimates, a ragged item against the item alone, a permuted batch,
a rerun, the encoder's bytes, the keyword against the calls done by hand -- is bit for bit.

Measured on an MI355X: see the README paragraph "Stereo stems"."""
import wave

import numpy as np
import pytest
import torch

from ditsep_amd import files, native, wavio
from tests import pcm_restatement as pr
from tests import stems_restatement as sr
from tests.test_gpu_mask_refine import FS, N_STEPS, model, span_of  # noqa: F401  (`model` is a fixture)
from tests.util import make_engine

pytestmark = pytest.mark.gpu
FACTOR = 8.0
KINDS = ("generic", "dual", "hard", "silent_ch", "silent_est")


@pytest.fixture(scope="module")
def eng():
    e = make_engine()
    assert e.cfg.score_kind == native.SCORE_NONE
    yield e
    e.close()


def off_alignment(x, device):
    """x on the device at a base pointer one float past a 16-byte boundary"""
    buf = torch.empty(x.numel() + 1, device=device, dtype=torch.float32)
    view = buf[1:].view(x.shape)
    view.copy_(x)
    assert view.data_ptr() % 16 == 4
    return view


def lengths_of(n_fft, hop):
    return (n_fft // 2 + 1, 5 * n_fft + 7, 3 * span_of(n_fft) + 2 * hop + 37)


# ------------------------------------------------------------------ 1. mask mode
@pytest.mark.parametrize("n_fft", [64, 128, 256, 512, 1024, 2048])
def test_mask_mode_is_mask_refine_per_channel(eng, n_fft):
    cases = []
    for r in (2, 4, 8):
        for L in lengths_of(n_fft, n_fft // r):
            q = len(cases)
            cases.append((r, L, (1, 2, 3, 8)[q % 4], 1 + (q // 2) % 4, 1 + q % 2))
    # every size at one of the ratios: two channels and two sources over two span boundaries, L % 4 != 0
    cases.append(({64: 2, 128: 4, 256: 8, 512: 2, 1024: 4, 2048: 8}[n_fft], 2 * span_of(n_fft) + 37, 2, 2, 2))
    for r, L, C, n, power in cases:
        hop = n_fft // r
        mix, est = sr.make_case(n_fft + 13 * r + L, "generic", n, C, L)
        m = off_alignment(torch.from_numpy(mix)[None], eng.device)
        e = off_alignment(torch.from_numpy(est)[None], eng.device)
        out = eng.stems(m, e, mode="mask", n_fft=n_fft, hop=hop, power=power)
        assert tuple(out.shape) == (1, n, C, L) and float(out.abs().max()) > 0
        for c in range(C):
            want = eng.mask_refine(m[:, c].contiguous(), e, n_fft=n_fft, hop=hop, power=power)
            assert torch.equal(out[:, :, c].view(torch.int32), want.view(torch.int32)), (n_fft, hop, L, C, n, c)


# ------------------------------------------------------------------ 2. wiener mode against the restatement
def ratio(dev, cpu):
    return dev / cpu if cpu > 0 else (0.0 if dev == 0 else float("inf"))


def check_wiener(eng, mix, est, n_fft, hop, power, what):
    kw = dict(n_fft=n_fft, hop=hop, power=power)
    ref, iref = sr.stems(mix, est, return_info=True, **kw)
    cpu, icpu = sr.stems(mix, est, dtype=np.float32, return_info=True, **kw)
    m = off_alignment(torch.from_numpy(mix)[None], eng.device)
    e = off_alignment(torch.from_numpy(est)[None], eng.device)
    out, info = eng.stems(m, e, mode="wiener", return_info=True, **kw)
    out = out[0].cpu().numpy()
    assert out.shape == ref.shape and np.all(np.isfinite(out))
    rel = lambda a, b: float(np.max(np.abs(a - b)) / np.max(np.abs(b)))
    pairs = {"parity": (sr.rel_err(out, ref, mix), sr.rel_err(cpu, ref, mix)),
             "consistency": (sr.rel_err(out.astype(np.float64).sum(axis=0), mix, mix),
                             sr.rel_err(cpu.astype(np.float64).sum(axis=0), mix, mix)),
             "R": (rel(info["R"][0].numpy(), iref["R"]), rel(icpu["R"], iref["R"])),
             "den": (rel(info["den"][0].numpy(), iref["den"]), rel(icpu["den"], iref["den"]))}
    print(what + ": " + "; ".join(f"{k} {d:.3e} (float32 CPU {c:.3e}, ratio {ratio(d, c):.2f})"
                                  for k, (d, c) in pairs.items()))
    for k, (d, c) in pairs.items():
        assert d <= FACTOR * c, f"{what}: {k} {ratio(d, c):.2f} x the float32 CPU error"
    return {k: ratio(d, c) for k, (d, c) in pairs.items()}


@pytest.mark.parametrize("n_fft", [64, 512, 2048])
def test_wiener_against_the_restatement(eng, n_fft):
    """every hop ratio and length (one reflection only, a partial last hop, statistics over several workgroups'
    partials), every source count, both powers and every kind of mixture, the two-channel kinds with C = 2"""
    worst, q = {}, 0
    for r in (2, 4, 8):
        hop = n_fft // r
        for L in lengths_of(n_fft, hop):
            for n in (1, 2, 3, 4):
                kind = KINDS[q % 5]
                C = 2 if kind in ("dual", "hard", "silent_ch") else 1 + (q // 5) % 2
                power = 1 + (q // 3) % 2
                q += 1
                mix, est = sr.make_case(n_fft + 31 * r + 7 * n + L, kind, n, C, L)
                got = check_wiener(eng, mix, est, n_fft, hop, power,
                                   f"n_fft {n_fft} hop {hop} L {L} n {n} C {C} power {power} {kind}")
                worst = {k: max(v, worst.get(k, 0.0)) for k, v in got.items()}
    print(f"n_fft {n_fft}: worst ratios " + ", ".join(f"{k} {v:.2f}" for k, v in worst.items())
          + f" (allowed {FACTOR})")


@pytest.mark.parametrize("kind", KINDS)
def test_wiener_every_kind_in_stereo(eng, kind):
    for C in (1, 2):
        mix, est = sr.make_case(len(kind) + C, kind, 3, C, 2 * span_of(512) + 301)
        check_wiener(eng, mix, est, 512, 128, 2, f"{kind} C {C}")


# ------------------------------------------------------------------ 3. exact cases
@pytest.mark.parametrize("mode", ["mask", "wiener"])
def test_silent_estimates_give_equal_outputs(eng, mode):
    for n_fft, hop, L in ((512, 128, 2 * span_of(512) + 301), (64, 8, 33), (2048, 1024, 3000)):
        mix, _ = sr.make_case(n_fft + L, "generic", 2, 2, L)
        for n in (2, 3, 4):
            out = eng.stems(torch.from_numpy(mix)[None], torch.zeros((1, n, L)), mode=mode, n_fft=n_fft, hop=hop)
            assert float(out.abs().max()) > 0
            for i in range(1, n):
                assert torch.equal(out[0, i].view(torch.int32), out[0, 0].view(torch.int32)), (n_fft, n, i)


@pytest.mark.parametrize("mode,n_fft,hop,n", [("wiener", 512, 128, 3), ("wiener", 2048, 256, 2), ("wiener", 64, 32, 4),
                                              ("mask", 512, 256, 4), ("mask", 64, 8, 1)])
def test_ragged(eng, mode, n_fft, hop, n):
    """5 items of distinct lengths and mixed channel counts, one at the minimum, one over two spans, NaN past every end
    and in every unused channel"""
    S, need = span_of(n_fft), n_fft // 2 + 1
    lens = [2 * S + 3 * hop + 5, need, S, S + 1, need + hop + 2]
    chans = [2, 1, 2, 1, 2]
    Lmax = max(lens) + 3
    g = np.random.default_rng(n_fft + n)
    mix = torch.full((5, 2, Lmax), float("nan"))
    est = torch.full((5, n, Lmax), float("nan"))
    for b, (v, c) in enumerate(zip(lens, chans)):
        m, e = sr.make_case(int(g.integers(1 << 30)), KINDS[b % 4], n, c, v)
        mix[b, :c, :v], est[b, :, :v] = torch.from_numpy(m), torch.from_numpy(e)
    kw = dict(mode=mode, n_fft=n_fft, hop=hop)
    out = eng.stems(mix, est, lens=lens, channels=chans, **kw)
    assert tuple(out.shape) == (5, n, 2, Lmax) and not bool(torch.isnan(out).any())
    for b, (v, c) in enumerate(zip(lens, chans)):
        alone = eng.stems(mix[b:b + 1, :c, :v].contiguous(), est[b:b + 1, :, :v].contiguous(), **kw)
        assert torch.equal(out[b, :, :c, :v].view(torch.int32), alone[0].view(torch.int32)), f"item {b} differs from the item alone"
        assert bool((out[b, :, :, v:] == 0).all()), f"item {b}: not zero past its end"
        assert bool((out[b, :, c:] == 0).all()), f"item {b}: not zero in the channels it does not have"
        assert float(alone.abs().max()) > 0
    perm = [3, 0, 4, 2, 1]
    again = eng.stems(mix[perm].contiguous(), est[perm].contiguous(), lens=[lens[p] for p in perm],
                      channels=[chans[p] for p in perm], **kw)
    assert torch.equal(again.view(torch.int32), out[perm].view(torch.int32))
    twice, info = eng.stems(mix, est, lens=lens, channels=chans, return_info=True, **kw)
    assert torch.equal(twice.view(torch.int32), out.view(torch.int32))
    assert bool(torch.isfinite(info["den"]).all()) and bool(torch.isfinite(torch.view_as_real(info["R"])).all())
    # lists are padded once and come back as a list
    as_list = eng.stems([mix[b, :c, :v] for b, (v, c) in enumerate(zip(lens, chans))],
                        [est[b, :, :v] for b, v in enumerate(lens)], **kw)
    for b, (v, c) in enumerate(zip(lens, chans)):
        assert tuple(as_list[b].shape) == (n, c, v) and torch.equal(as_list[b], out[b, :, :c, :v])


# ------------------------------------------------------------------ 4. refusals
def test_refusals_launch_nothing(eng):
    B, Cn, n, L = 2, 2, 2, 600
    mix = torch.zeros((B, Cn, L), device=eng.device)
    est = torch.zeros((B, n, L), device=eng.device)
    out = torch.full((B, n, Cn, L), 7.0, device=eng.device)
    good = dict(mix=mix, est=est, B=B, C=Cn, n=n, Lmax=L, lens=None, channels=None, mode=1, n_fft=512, hop=128, power=2,
                eps=1e-10, reg=1e-3, out=out)

    def call(**kw):
        a = dict(good, **kw)
        i32 = lambda v: None if v is None else (native.C.c_int32 * len(v))(*v)
        return eng.lib.dsn_stems(eng.ctx, native._ptr(a["mix"]), native._ptr(a["est"]), a["B"], a["C"], a["n"], a["Lmax"],
                                 i32(a["lens"]), i32(a["channels"]), a["mode"], a["n_fft"], a["hop"], a["power"],
                                 a["eps"], a["reg"], native._ptr(a["out"]), None, None, eng._stream())

    flat = torch.zeros(B * (Cn + n + n * Cn) * L + 8, device=eng.device)
    for kw, msg in ((dict(mix=None), "mix, est or out is null"), (dict(est=None), "mix, est or out is null"),
                    (dict(out=None), "mix, est or out is null"),
                    (dict(mode=2), "mode = 2 is not one of 0 (DSN_STEMS_MASK), 1 (DSN_STEMS_WIENER)"),
                    (dict(mode=-1), "mode = -1 is not one of"),
                    (dict(B=0), "B = 0 outside [1, 65535]"),
                    (dict(C=0), "C = 0 outside [1, 2]"), (dict(C=3), "C = 3 outside [1, 2] (DSN_STEMS_WIENER"),
                    (dict(C=9, mode=0), "C = 9 outside [1, 8] (DSN_STEMS_MASK)"),
                    (dict(n=0), "n = 0 outside [1, 4]"), (dict(n=5), "n = 5 outside [1, 4]"),
                    (dict(n_fft=32, hop=8), "n_fft = 32 is not a power of two in [64, 2048]"),
                    (dict(n_fft=4096, hop=1024), "n_fft = 4096 is not a power of two in [64, 2048]"),
                    (dict(hop=512), "n_fft / hop = 512 / 512 is not one of 2, 4, 8"),
                    (dict(hop=0), "n_fft / hop = 512 / 0 is not one of 2, 4, 8"),
                    (dict(power=3), "power = 3 is not 1 or 2"),
                    (dict(eps=0.0), "eps = 0 is not a finite positive number"),
                    (dict(eps=float("nan")), "is not a finite positive number"),
                    (dict(reg=-1.0), "reg = -1 is not a finite number >= 0"),
                    (dict(reg=float("inf")), "is not a finite number >= 0"),
                    (dict(reg=float("nan")), "is not a finite number >= 0"),
                    (dict(lens=[600, 256]), "item 1 has 256 samples, outside [n_fft / 2 + 1 = 257, Lmax = 600]"),
                    (dict(lens=[601, 600]), "item 0 has 601 samples, outside"),
                    (dict(channels=[2, 3]), "channels[1] = 3 outside [1, C = 2]"),
                    (dict(channels=[0, 1]), "channels[0] = 0 outside [1, C = 2]"),
                    (dict(mix=out[0, 1]), "out overlaps mix or est"),
                    (dict(est=flat[4:], out=flat), "out overlaps mix or est"),
                    (dict(est=out), "out overlaps mix or est")):
        assert call(**kw) != 0, kw
        assert msg in eng.lib.dsn_last_error(eng.ctx).decode(), (kw, eng.lib.dsn_last_error(eng.ctx).decode())
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((flat == 0.0).all())
    for mode in (0, 1):
        out.fill_(7.0)
        assert call(mode=mode, reg=0.0) == 0
        torch.cuda.synchronize()
        assert bool((out == 0.0).all())             # a silent mixture gives silence
    # the refusals of the Python layer come first
    with pytest.raises(ValueError, match=r"stems: C = 3 outside \[1, 2\] for mode 'wiener'"):
        eng.stems(torch.zeros(1, 3, 600), torch.zeros(1, 2, 600))


# ------------------------------------------------------------------ 5. the interleaving encoder
@pytest.mark.parametrize("encoding", ["s16", "s24", "f32"])
def test_pcm_encode_frames(eng, encoding):
    w = native.PCM_SAMPLE_BYTES[encoding]
    g = np.random.default_rng(w)
    R, Cn, Lmax = 5, 3, 2500
    lens, chans = [2500, 1, 1025, 2047, 300], [3, 2, 1, 3, 2]
    x = (0.4 * g.standard_normal((R, Cn, Lmax))).astype(np.float32)
    x[0, 1, 5], x[0, 2, 6], x[3, 0, 2046], x[4, 1, 0] = 1.0, -1.5, np.nan, np.inf     # 1.0 saturates: 2^(b-1) is out of range
    x[1, 2, :], x[2, 1:, :], x[4, :, 300:] = np.nan, 7.0, -9.0                          # unused channels and tails
    want = [sr.encode_frames(x[r], lens[r], chans[r], encoding) for r in range(R)]
    xt = torch.from_numpy(x)
    payloads, clipped = eng.pcm_encode_frames(xt, lens, chans, encoding)
    for r in range(R):
        assert len(payloads[r]) == lens[r] * chans[r] * w
        assert payloads[r] == want[r][0], f"row {r}"
        assert clipped[r] == want[r][1]
    if encoding != "f32":
        assert clipped[0] >= 2 and clipped[3] >= 1 and clipped[4] >= 1
    # odd offsets with gaps, in a buffer of the caller's: the bytes between the rows stay as they were
    offsets, o = [], 3
    for r in range(R):
        offsets.append(o)
        o += lens[r] * chans[r] * w + (1, 7, 2, 13, 5)[r]
    buf = torch.full((o,), 0xAA, dtype=torch.uint8, device=eng.device)
    got, _ = eng.pcm_encode_frames(xt, lens, chans, encoding, offsets=offsets, out=buf)
    host = buf.cpu().numpy()
    own = np.zeros(o, dtype=bool)
    for r in range(R):
        assert got[r] == want[r][0]
        own[offsets[r]:offsets[r] + len(want[r][0])] = True
    assert bool((host[~own] == 0xAA).all())
    # one channel: the bytes of pcm_encode
    mono, mclip = eng.pcm_encode(xt[:, 0].contiguous(), lens, encoding)
    one, oclip = eng.pcm_encode_frames(xt[:, :1].contiguous(), lens, None, encoding)
    assert one == mono and oclip == mclip
    with pytest.raises(ValueError, match=r"row 1: channels = 4 outside \[1, C = 3\]"):
        eng.pcm_encode_frames(xt, lens, [3, 4, 1, 3, 2], encoding)
    wide = native.PCM_MAX_FRAME_BYTES // w + 1
    with pytest.raises(ValueError, match="wider than PCM_MAX_FRAME_BYTES"):
        eng.pcm_encode_frames(torch.zeros(1, wide, 8), None, None, encoding)
    i64 = native.C.c_int64 * 1
    assert eng.lib.dsn_pcm_encode_frames(eng.ctx, native._ptr(torch.zeros(1, wide, 8, device=eng.device)), 1, wide, 8,
                                         None, None, native.PCM_ENCODINGS[encoding], native._ptr(buf), buf.numel(),
                                         i64(0), None, eng._stream()) != 0
    assert "more than DSN_PCM_MAX_FRAME_BYTES" in eng.lib.dsn_last_error(eng.ctx).decode()


# ------------------------------------------------------------------ 6. the stems keyword of LatentDiffSep
def fit(x, L):
    return torch.nn.functional.pad(x, (0, L - x.shape[-1])) if x.shape[-1] < L else x[..., :L]


def test_separate_with_stems(model):
    eng = model.engine
    g = torch.Generator().manual_seed(51)
    mix = 0.3 * torch.randn((2, 2, 600), generator=g)
    mono = native.downmix(mix.to(eng.device))
    assert torch.equal(mono[:, 0], (mix[:, 0] + mix[:, 1]).to(eng.device) / 2)
    plain, nfe = model.separate(mono, seed=3)
    for stems, kw in (("wiener", dict(mode="wiener")), ("mask", dict(mode="mask")),
                      (dict(mode="wiener", n_fft=64, hop=16, power=1, reg=1e-2),) * 2):
        got, nfe_s = model.separate(mix, seed=3, stems=stems)
        assert nfe_s == nfe == 2 * N_STEPS and tuple(got.shape) == (2, 2, 2, 608)
        assert torch.equal(got, eng.stems(fit(mix.to(eng.device), 608), plain, **kw))
    got = model.separate(mix, seed=3, stems="wiener")[0]
    peak = float(mix.abs().max())
    assert float((got.sum(dim=1)[..., :600].cpu() - mix).abs().max()) < 1e-5 * peak       # stems sum to every channel
    # with refine: on the mono estimates, before the stems
    refined = eng.mask_refine(fit(mono, 608), plain)
    assert torch.equal(model.separate(mix, seed=3, refine=True, stems="mask")[0],
                       eng.stems(fit(mix.to(eng.device), 608), refined, mode="mask"))
    # stems=None is the old path, before and after
    assert torch.equal(model.separate(mono, seed=3)[0], plain)
    assert torch.equal(model.separate(mono, seed=3, stems=None)[0], plain)
    # at another rate: filtered at the model's rate against the channels resampled without downmix, then taken back
    x = 0.3 * torch.randn((1, 2, 1300), generator=g)
    mc, m1 = eng.resample(x, 32000, FS), eng.resample(x, 32000, FS, downmix=True)
    sep = model.separate(m1, seed=5)[0]
    st = eng.stems(fit(mc, sep.shape[-1]), sep)
    hand = eng.resample(st.reshape(1, 4, -1), FS, 32000)[..., :1300].reshape(1, 2, 2, 1300)
    assert torch.equal(model.separate(x, seed=5, sample_rate=32000, stems="wiener")[0], hand)
    with pytest.raises(ValueError, match="with latent=True there is no mixture to filter"):
        model.separate(torch.zeros(1, 64, 75), latent=True, stems="mask")
    with pytest.raises(ValueError, match="stems= does not go with intermediate"):
        model.separate(mix, stems="mask", intermediate=True)
    with pytest.raises(ValueError, match=r"item 0 has 3 channels, outside \[1, 2\] for mode 'wiener'"):
        model.separate(torch.zeros(1, 3, 600), stems="wiener")
    with pytest.raises(ValueError, match=r"stems= takes mix \[B, C, L\]"):
        model.separate(torch.zeros(2, 600), stems="wiener")


def test_separate_batch_and_long_with_stems(model):
    eng = model.engine
    g = torch.Generator().manual_seed(53)
    mixes = [0.3 * torch.randn((c, L), generator=g) for c, L in ((2, 300), (1, 611), (2, 417))]
    monos = [native.downmix(m[None].to(eng.device))[0] for m in mixes]
    plain, nfe = model.separate_batch(monos, seed=7)
    got, nfe_s = model.separate_batch(mixes, seed=7, stems="wiener")
    want = eng.stems([m.to(eng.device) for m in mixes], plain)
    assert nfe == nfe_s
    for b, m in enumerate(mixes):
        assert tuple(got[b].shape) == (2,) + tuple(m.shape) and torch.equal(got[b], want[b])
        assert torch.equal(got[b], eng.stems(m[None], plain[b][None])[0])                # .. and the item alone
    again, _ = model.separate_batch(monos, seed=7)
    assert all(torch.equal(a, p) for a, p in zip(again, plain))
    # at other rates, mixed channel counts: back through one resample call per (rate, channel count)
    rates = [32000, FS, 8000]
    opts = dict(mode="mask", n_fft=128, hop=32)                                          # 300 samples at 32 kHz are 150
    got, _ = model.separate_batch(mixes, seed=7, sample_rates=rates, stems=opts)
    at_fs = eng.to_model_rate(mixes, rates, FS)
    mc = eng.to_model_rate(mixes, rates, FS, downmix=False)
    assert [tuple(a.shape) for a in mc] == [(m.shape[0], a.shape[-1]) for m, a in zip(mixes, at_fs)]
    est, _ = model.separate_batch(at_fs, seed=7)
    hand = eng.stems_from_model_rate(eng.stems(mc, est, **opts), rates, FS, [m.shape[-1] for m in mixes])
    for b, m in enumerate(mixes):
        assert tuple(got[b].shape) == (2,) + tuple(m.shape) and torch.equal(got[b], hand[b])
    # long recordings: after the stitch
    rec = [0.3 * torch.randn((2, 700), generator=g), 0.3 * torch.randn((1, 450), generator=g)]
    kw = dict(window=256, overlap=64, batch=3, seed=9)
    plain, nfe = model.separate_long([native.downmix(r[None].to(eng.device))[0] for r in rec], **kw)
    got, nfe_s = model.separate_long(rec, stems="wiener", **kw)
    want = eng.stems([r.to(eng.device) for r in rec], plain)
    assert nfe == nfe_s and all(torch.equal(a, b) for a, b in zip(got, want))
    one, _ = model.separate_long(rec[0], stems="wiener", **kw)
    alone, _ = model.separate_long(native.downmix(rec[0][None].to(eng.device))[0], **kw)   # (its windows, pooled alone)
    assert tuple(one.shape) == (2, 2, 700) and torch.equal(one, eng.stems(rec[0][None], alone[None])[0])


def test_separate_files_with_stems(model, tmp_path):
    eng = model.engine
    g = np.random.default_rng(57)
    src = tmp_path / "in"
    src.mkdir()
    wavio.write_wav(src / "a.wav", (0.3 * g.standard_normal(2 * 900) * 2 ** 15).astype("<i2").tobytes(), 44100, 2, "s16")
    wavio.write_wav(src / "b.wav", (0.3 * g.standard_normal(300) * 2 ** 15).astype("<i2").tobytes(), FS, 1, "s16")
    half = np.clip(128 + 40 * g.standard_normal(260), 0, 255).astype(np.uint8)
    with wave.open(str(src / "c.wav"), "wb") as f:                                       # 8 kHz dual-mono u8
        f.setnchannels(2)
        f.setsampwidth(1)
        f.setframerate(8000)
        f.writeframes(np.repeat(half, 2).tobytes())
    paths = sorted(src.glob("*.wav"))
    hs = [wavio.read_header(p) for p in paths]
    assert [(h.rate, h.channels, h.encoding) for h in hs] == [(44100, 2, "s16"), (FS, 1, "s16"), (8000, 2, "u8")]
    with pytest.raises(ValueError, match="stems= does not go with rescale"):
        model.separate_files(paths, tmp_path / "never", stems="wiener", rescale=True)
    with pytest.raises(ValueError, match=r"stems= needs at least n_fft / 2 \+ 1 = 513"):
        model.separate_files(paths, tmp_path / "never", stems={"n_fft": 1024, "hop": 256})
    assert not (tmp_path / "never").exists()
    out = tmp_path / "out"
    recs = model.separate_files(paths, out, batch=2, seed=5, stems="wiener")
    assert set(recs[0]) == {"path", "rate", "channels", "frames", "outputs", "clipped", "batch", "stems"}
    plan = files.plan_files(hs, FS, 8, batch=2)
    assert sorted(i for b in plan["batches"] for i in b) == [0, 1, 2] and len(plan["batches"]) == 2
    for k, idx in enumerate(plan["batches"]):
        clips = [torch.from_numpy(pr.decode(wavio.read_payload(paths[i], hs[i]), hs[i].frames, hs[i].channels,
                                            hs[i].encoding)) for i in idx]
        rates = [hs[i].rate for i in idx]
        at_fs = eng.to_model_rate(clips, rates, FS)
        est, _ = model.separate_batch(at_fs, codec="padded", seed=5 + k)
        st = eng.stems(eng.to_model_rate(clips, rates, FS, downmix=False), est)
        back = eng.stems_from_model_rate(st, rates, FS, [hs[i].frames for i in idx])
        for j, i in enumerate(idx):
            assert tuple(back[j].shape) == (2, hs[i].channels, hs[i].frames)
            for s in range(2):
                p = out / f"s{s}" / paths[i].name
                with wave.open(str(p), "rb") as f:
                    assert (f.getnchannels(), f.getframerate(), f.getnframes(), f.getsampwidth()) == (
                        hs[i].channels, hs[i].rate, hs[i].frames, 2)
                    payload = f.readframes(hs[i].frames)
                want, clipped = sr.encode_frames(back[j][s].cpu().numpy(), hs[i].frames, hs[i].channels, "s16")
                assert payload == want, f"{p} is not the quantised stem"
                assert recs[i]["clipped"][s] == clipped and recs[i]["stems"] == "wiener"
    # the dual-mono file comes back dual-mono
    with wave.open(str(out / "s0" / "c.wav"), "rb") as f:
        lr = np.frombuffer(f.readframes(260), dtype="<i2").reshape(260, 2)
    assert np.array_equal(lr[:, 0], lr[:, 1]) and np.abs(lr).max() > 0
    # without stems: mono files, the old keys, the bytes of the steps the call has always taken
    old = tmp_path / "old"
    recs = model.separate_files(paths, old, batch=2, seed=5)
    assert set(recs[0]) == {"path", "rate", "channels", "frames", "outputs", "clipped", "batch"}
    for k, idx in enumerate(plan["batches"]):
        clips = [torch.from_numpy(pr.decode(wavio.read_payload(paths[i], hs[i]), hs[i].frames, hs[i].channels,
                                            hs[i].encoding)) for i in idx]
        at_fs = eng.to_model_rate(clips, [hs[i].rate for i in idx], FS)
        est, _ = model.separate_batch(at_fs, codec="padded", seed=5 + k)
        back = eng.from_model_rate(est, [hs[i].rate for i in idx], FS, [hs[i].frames for i in idx])
        for j, i in enumerate(idx):
            for s in range(2):
                ho = wavio.read_header(old / f"s{s}" / paths[i].name)
                assert ho[:4] == (hs[i].rate, 1, hs[i].frames, "s16")
                assert wavio.read_payload(old / f"s{s}" / paths[i].name, ho) == pr.quantise(back[j][s].cpu().numpy(),
                                                                                             "s16")[0]
