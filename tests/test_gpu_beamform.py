"""dsn_beamform (ditsep_amd/csrc/beamform.hip) through Engine.beamform on an engine with no score network and no codec,
against the restatement (tests/beamform_restatement.py).

Bounds.  The error of an output is its largest absolute difference from the float64 restatement divided by the peak of
|mix|; the error of the weights is their largest absolute difference from the float64 restatement's divided by its
largest weight.  Each may be at most 8 x what the float32 run of the same restatement shows on the same input (float32
pocketfft transforms and masks, float64 statistics and solve: the device's own split of precisions) -- the rule and the
factor of tests/test_gpu_mask_refine.py and tests/test_gpu_stems.py, for the same reason: the device's radix-2 butterfly
order and its fused multiply-adds differ from pocketfft's.  The weights are compared in every bin; the test first
asserts that every bin of its input carries at least 1e-6 of the strongest bin's mixture power (all sources are white).
Everything else -- C = 1 against Engine.mask_refine, silent estimates, a ragged item against the item alone, a permuted
batch, a rerun, a workspace budget of one item, lists -- is bit for bit.

Measured on an MI355X: see the README paragraph "Beamforming"."""
import numpy as np
import pytest
import torch

from ditsep_amd import native
from tests import beamform_restatement as br
from tests.test_gpu_mask_refine import span_of
from tests.util import make_engine

pytestmark = pytest.mark.gpu
FACTOR = 8.0
CHANNELS = (1, 2, 3, 4, 8)


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
    """one reflection only; a partial last hop; several spans; one span more than the owner cap holds, so that an owner
    of the statistics launch takes two spans of frames"""
    S = span_of(n_fft)
    return (n_fft // 2 + 1, 5 * n_fft + 7, 3 * S + 2 * hop + 37, native.BEAMFORM_MAX_OWNERS * S + hop + 5)


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ------------------------------------------------------------------ 1. parity with the restatement
def ratio(dev, cpu):
    return dev / cpu if cpu > 0 else (0.0 if dev == 0 else float("inf"))


def check(eng, mix, est, what, **kw):
    ref, iref = br.beamform(mix, est, return_info=True, **kw)
    cpu, icpu = br.beamform(mix, est, dtype=np.float32, return_info=True, **kw)
    power = iref["power"]
    assert power.min() >= 1e-6 * power.max() > 0, f"{what}: a bin of the input carries no signal"
    m = off_alignment(torch.from_numpy(mix)[None], eng.device)
    e = off_alignment(torch.from_numpy(est)[None], eng.device)
    out, info = eng.beamform(m, e, return_info=True, **kw)
    out, w = out[0].cpu().numpy(), info["w"][0].numpy()
    assert out.shape == ref.shape and w.shape == iref["w"].shape
    assert np.all(np.isfinite(out)) and np.all(np.isfinite(w))
    top = float(np.max(np.abs(iref["w"])))
    rel = lambda a: float(np.max(np.abs(a - iref["w"])) / top) if top > 0 else float(np.max(np.abs(a)))
    pairs = {"parity": (br.rel_err(out, ref, mix), br.rel_err(cpu, ref, mix)), "w": (rel(w), rel(icpu["w"]))}
    print(what + ": " + "; ".join(f"{k} {d:.3e} (float32 CPU {c:.3e}, ratio {ratio(d, c):.2f})"
                                  for k, (d, c) in pairs.items()))
    for k, (d, c) in pairs.items():
        assert d <= FACTOR * c, f"{what}: {k} {ratio(d, c):.2f} x the float32 CPU error"
    return {k: ratio(d, c) for k, (d, c) in pairs.items()}


@pytest.mark.parametrize("n_fft", [64, 512, 2048])
def test_against_the_restatement(eng, n_fft):
    """every hop ratio and length, every channel and source count, both powers, both post-filters, both ends of the
    reference channel and every kind of mixture"""
    worst, q = {}, {64: 0, 512: 1, 2048: 2}[n_fft]
    for r in (2, 4, 8):
        hop = n_fft // r
        for L in lengths_of(n_fft, hop):
            C, kind, n = CHANNELS[q % 5], br.KINDS[(q + q // 5) % 5], 1 + q % 4
            power, post, ref = 1 + (q // 2) % 2, (None, "mask")[(q // 3) % 2], (0, C - 1)[(q // 2 + q) % 2]
            q += 1
            mix, est = br.make_case(n_fft + 31 * r + 7 * n + L, kind, n, C, L)
            got = check(eng, mix, est, f"n_fft {n_fft} hop {hop} L {L} C {C} n {n} power {power} post {post} ref {ref} "
                        f"{kind}", ref=ref, n_fft=n_fft, hop=hop, power=power, postfilter=post)
            worst = {k: max(v, worst.get(k, 0.0)) for k, v in got.items()}
    print(f"n_fft {n_fft}: worst ratios " + ", ".join(f"{k} {v:.2f}" for k, v in worst.items())
          + f" (allowed {FACTOR})")


@pytest.mark.parametrize("kind", br.KINDS)
def test_every_kind_on_an_array(eng, kind):
    worst = {}
    for C, n, ref, post in ((4, 2, 3, None), (8, 4, 0, "mask"), (2, 3, 0, None), (3, 1, 2, "mask")):
        mix, est = br.make_case(len(kind) + C, kind, n, C, 2 * span_of(512) + 301)
        got = check(eng, mix, est, f"{kind} C {C} n {n} ref {ref} post {post}", ref=ref, postfilter=post)
        worst = {k: max(v, worst.get(k, 0.0)) for k, v in got.items()}
    print(f"{kind}: worst ratios " + ", ".join(f"{k} {v:.2f}" for k, v in worst.items()) + f" (allowed {FACTOR})")


# ------------------------------------------------------------------ 2. exact cases
def test_one_channel_is_mask_refine(eng):
    """C = 1: w = Z / Z = 1.0, so every source is mask_refine with n = 1 (the mixture's own transform handed back), and
    with the mask post-filter mask_refine itself"""
    every = tuple((n_fft, n_fft // r, 2 * span_of(n_fft) + 37)   # every size, over two span boundaries, L % 4 != 0
                  for n_fft, r in ((64, 2), (128, 4), (256, 8), (512, 2), (1024, 4), (2048, 8)))
    for n_fft, hop, L in ((512, 128, 2 * span_of(512) + 301), (64, 8, 33), (2048, 1024, 3 * span_of(2048) + 17),
                          (256, 64, native.BEAMFORM_MAX_OWNERS * span_of(256) + 77)) + every:
        for n, power in ((1, 2), (2, 1), (3, 2), (4, 2)):
            mix, est = br.make_case(n_fft + L + n, "generic", n, 1, L)
            m, e = torch.from_numpy(mix)[None].to(eng.device), torch.from_numpy(est)[None].to(eng.device)
            kw = dict(n_fft=n_fft, hop=hop, power=power)
            out, info = eng.beamform(m, e, return_info=True, **kw)
            assert bool((info["w"] == 1.0).all()), (n_fft, n)
            one = eng.mask_refine(m[:, 0], e[:, :1], **kw)
            assert float(one.abs().max()) > 0
            for i in range(n):
                assert same_bits(out[:, i], one[:, 0]), (n_fft, hop, L, n, i)
            post = eng.beamform(m, e, postfilter="mask", **kw)
            assert same_bits(post, eng.mask_refine(m[:, 0], e, **kw)), (n_fft, hop, L, n)


@pytest.mark.parametrize("post", [None, "mask"])
def test_silent_estimates_give_equal_outputs(eng, post):
    for n_fft, hop, L, C in ((512, 128, 2 * span_of(512) + 301, 4), (64, 8, 33, 8), (2048, 1024, 3000, 3)):
        mix, _ = br.make_case(n_fft + L, "generic", 2, C, L)
        for n in (2, 3, 4):
            out = eng.beamform(torch.from_numpy(mix)[None], torch.zeros((1, n, L)), n_fft=n_fft, hop=hop, ref=C - 1,
                               postfilter=post)
            assert float(out.abs().max()) > 0
            for i in range(1, n):
                assert same_bits(out[0, i], out[0, 0]), (n_fft, n, i)


@pytest.mark.parametrize("n_fft,hop,n,post", [(512, 128, 3, None), (2048, 256, 2, "mask"), (64, 32, 4, None),
                                              (256, 32, 1, "mask")])
def test_ragged(eng, n_fft, hop, n, post):
    """6 items of distinct lengths and mixed channel counts, one at the minimum, one over two spans, one past the owner
    cap, NaN past every end and in every channel an item does not have: each item against the item alone, a permuted
    batch, a rerun, one item per chunk, lists"""
    S, need = span_of(n_fft), n_fft // 2 + 1
    lens = [2 * S + 3 * hop + 5, need, S, native.BEAMFORM_MAX_OWNERS * S + 3, S + 1, need + hop + 2]
    chans = [4, 1, 8, 2, 3, 5]
    Lmax, Cmax = max(lens) + 3, 8
    g = np.random.default_rng(n_fft + n)
    mix = torch.full((6, Cmax, Lmax), float("nan"))
    est = torch.full((6, n, Lmax), float("nan"))
    for b, (v, c) in enumerate(zip(lens, chans)):
        m, e = br.make_case(int(g.integers(1 << 30)), br.KINDS[b % 4], n, c, v)
        mix[b, :c, :v], est[b, :, :v] = torch.from_numpy(m), torch.from_numpy(e)
    kw = dict(n_fft=n_fft, hop=hop, postfilter=post)
    out, info = eng.beamform(mix, est, lens=lens, channels=chans, return_info=True, **kw)
    assert tuple(out.shape) == (6, n, Lmax) and not bool(torch.isnan(out).any())
    assert bool(torch.isfinite(torch.view_as_real(info["w"])).all())
    for b, (v, c) in enumerate(zip(lens, chans)):
        alone, ia = eng.beamform(mix[b:b + 1, :c, :v].contiguous(), est[b:b + 1, :, :v].contiguous(), return_info=True,
                                 **kw)
        assert same_bits(out[b, :, :v], alone[0]), f"item {b} differs from the item alone"
        assert torch.equal(torch.view_as_real(info["w"][b, :, :, :c]), torch.view_as_real(ia["w"][0]))
        assert bool((info["w"][b, :, :, c:] == 0).all())
        assert bool((out[b, :, v:] == 0).all()), f"item {b}: not zero past its end"
        assert float(alone.abs().max()) > 0
    perm = [3, 0, 5, 4, 2, 1]
    again = eng.beamform(mix[perm].contiguous(), est[perm].contiguous(), lens=[lens[p] for p in perm],
                         channels=[chans[p] for p in perm], **kw)
    assert same_bits(again, out[perm])
    assert same_bits(eng.beamform(mix, est, lens=lens, channels=chans, **kw), out)
    one_item = native.beamform_item_bytes(n_fft, hop, Lmax, Cmax, n)
    assert same_bits(eng.beamform(mix, est, lens=lens, channels=chans, workspace_budget=one_item, **kw), out)
    assert same_bits(eng.beamform(mix, est, lens=lens, channels=chans, workspace_budget=2 * one_item + 8, **kw), out)
    as_list = eng.beamform([mix[b, :c, :v] for b, (v, c) in enumerate(zip(lens, chans))],
                           [est[b, :, :v] for b, v in enumerate(lens)], **kw)
    for b, v in enumerate(lens):
        assert tuple(as_list[b].shape) == (n, v) and same_bits(as_list[b], out[b, :, :v])


# ------------------------------------------------------------------ 3. refusals
def test_refusals_launch_nothing(eng):
    B, Cn, n, L = 2, 4, 2, 600
    mix = torch.zeros((B, Cn, L), device=eng.device)
    est = torch.zeros((B, n, L), device=eng.device)
    out = torch.full((B, n, L), 7.0, device=eng.device)
    good = dict(mix=mix, est=est, B=B, C=Cn, n=n, Lmax=L, lens=None, channels=None, ref=0, n_fft=512, hop=128, power=2,
                eps=1e-10, reg=1e-3, post=0, budget=0, out=out)

    def call(**kw):
        a = dict(good, **kw)
        i32 = lambda v: None if v is None else (native.C.c_int32 * len(v))(*v)
        return eng.lib.dsn_beamform(eng.ctx, native._ptr(a["mix"]), native._ptr(a["est"]), a["B"], a["C"], a["n"],
                                    a["Lmax"], i32(a["lens"]), i32(a["channels"]), a["ref"], a["n_fft"], a["hop"],
                                    a["power"], a["eps"], a["reg"], a["post"], a["budget"], native._ptr(a["out"]), None,
                                    eng._stream())

    flat = torch.zeros(B * (Cn + 2 * n) * L + 8, device=eng.device)
    need = native.beamform_item_bytes(512, 128, L, Cn, n)
    for kw, msg in ((dict(mix=None), "mix, est or out is null"), (dict(est=None), "mix, est or out is null"),
                    (dict(out=None), "mix, est or out is null"),
                    (dict(post=2), "postfilter = 2 is not one of 0 (DSN_BEAMFORM_POST_NONE), 1 (DSN_BEAMFORM_POST_MASK)"),
                    (dict(post=-1), "postfilter = -1 is not one of"),
                    (dict(B=0), "B = 0 outside [1, 65535]"),
                    (dict(C=0), "C = 0 outside [1, 8]"), (dict(C=9), "C = 9 outside [1, 8]"),
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
                    (dict(channels=[2, 5]), "channels[1] = 5 outside [1, C = 4]"),
                    (dict(channels=[0, 1]), "channels[0] = 0 outside [1, C = 4]"),
                    (dict(ref=4), "ref = 4 outside [0, 4): item 0 has 4 channels"),
                    (dict(ref=-1), "ref = -1 outside [0, 4): item 0"),
                    (dict(ref=2, channels=[4, 2]), "ref = 2 outside [0, 2): item 1 has 2 channels"),
                    (dict(budget=-1), "workspace_budget = -1 < 0"),
                    (dict(budget=need - 1), f"is smaller than one item ({need} bytes at C = 4, n = 2"),
                    (dict(mix=out), "out overlaps mix or est"),
                    (dict(est=flat[4:], out=flat), "out overlaps mix or est"),
                    (dict(est=out), "out overlaps mix or est")):
        assert call(**kw) != 0, kw
        assert msg in eng.lib.dsn_last_error(eng.ctx).decode(), (kw, eng.lib.dsn_last_error(eng.ctx).decode())
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((flat == 0.0).all())
    for post in (0, 1):
        out.fill_(7.0)
        assert call(post=post, budget=need) == 0
        torch.cuda.synchronize()
        assert bool((out == 0.0).all())             # a silent mixture: tau = 0, w = e_ref, silence
    # the refusals of the Python layer come first
    with pytest.raises(ValueError, match=r"beamform: ref = 3 outside \[0, 3\): item 0 has 3 channels"):
        eng.beamform(torch.zeros(1, 3, 600), torch.zeros(1, 2, 600), ref=3)
    with pytest.raises(ValueError, match=r"beamform: C = 9 outside \[1, 8\]"):
        eng.beamform(torch.zeros(1, 9, 600), torch.zeros(1, 2, 600))
