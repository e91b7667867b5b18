"""dsn_beamform_track (ditsep_amd/csrc/beamform_track.hip) through Engine.beamform_track on an engine with no score
network and no codec, against the restatement (tests/beamform_track_restatement.py).

Bounds.  The rule and the factor of tests/test_gpu_beamform.py: the error of an output is its largest absolute
difference from the float64 restatement divided by the peak of |mix|; the error of the weights is their largest absolute
difference from the float64 restatement's over all blocks and bins divided by its largest weight.  Each may be at most
8 x what the float32 run of the same restatement shows on the same input.  Each case first asserts that every (context
window, bin) of its input carries at least 1e-6 of the strongest one's mixture power (all sources are white).  One block
per item is within 1e-10 of Engine.beamform's weights (another order of the sums).  Everything else -- C = 1 against
Engine.mask_refine, silent estimates, a context over all blocks, a ragged item against the item alone, a permuted batch,
a rerun, a workspace budget of one item, lists -- is bit for bit.

Measured on an MI355X: see the README paragraph "Tracking moving speakers"."""
import numpy as np
import pytest
import torch

from ditsep_amd import native
from tests import beamform_restatement as br
from tests import beamform_track_restatement as tr
from tests.test_gpu_beamform import FACTOR, off_alignment, ratio, same_bits
from tests.test_gpu_mask_refine import span_of
from tests.util import make_engine

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    e = make_engine()
    assert e.cfg.score_kind == native.SCORE_NONE
    yield e
    e.close()


# ------------------------------------------------------------------ 1. parity with the restatement
def check(eng, mix, est, what, **kw):
    """both interpolation modes of one case (the blocks' weights do not depend on the mode) -> the worst ratios"""
    worst = {}
    for interp in (True, False):
        ref, iref = tr.beamform_track(mix, est, interpolate=interp, return_info=True, **kw)
        cpu, icpu = tr.beamform_track(mix, est, interpolate=interp, dtype=np.float32, return_info=True, **kw)
        power = iref["power"]
        assert power.min() >= 1e-6 * power.max() > 0, f"{what}: a bin of a context window carries no signal"
        m = off_alignment(torch.from_numpy(mix)[None], eng.device)
        e = off_alignment(torch.from_numpy(est)[None], eng.device)
        out, info = eng.beamform_track(m, e, interpolate=interp, return_info=True, **kw)
        out, w = out[0].cpu().numpy(), info["w"][0].numpy()
        assert out.shape == ref.shape and w.shape == iref["w"].shape, (w.shape, iref["w"].shape)
        assert np.all(np.isfinite(out)) and np.all(np.isfinite(w))
        top = float(np.max(np.abs(iref["w"])))
        rel = lambda a: float(np.max(np.abs(a - iref["w"])) / top) if top > 0 else float(np.max(np.abs(a)))
        pairs = {"parity": (br.rel_err(out, ref, mix), br.rel_err(cpu, ref, mix)), "w": (rel(w), rel(icpu["w"]))}
        print(f"{what} interpolate {interp} K {w.shape[0]}: "
              + "; ".join(f"{k} {d:.3e} (float32 CPU {c:.3e}, ratio {ratio(d, c):.2f})" for k, (d, c) in pairs.items()))
        for k, (d, c) in pairs.items():
            assert d <= FACTOR * c, f"{what}: {k} {ratio(d, c):.2f} x the float32 CPU error"
            worst[k] = max(worst.get(k, 0.0), ratio(d, c))
    return worst


CASES = {
    # n_fft, hop, L, block_frames, context, C, n, further keywords
    "small-2x2-ctx0": (64, 16, 3 * 2048 + 16 + 5, 5, 0, 2, 2, dict()),
    "small-3x3-ctx2": (64, 16, 3 * 2048 + 16 + 5, 5, 2, 3, 3, dict(power=1)),
    "array-Tb9": (512, 128, 2 * 2048 + 301, 9, 1, 8, 4, dict(postfilter="mask", ref=7)),
    "array-Tb100": (512, 128, 2 * 2048 + 301, 100, 1, 8, 4, dict(postfilter="mask", ref=7)),
    "one-source": (1024, 512, 2048 + 5 * 512 + 3, 4, 1, 4, 1, dict(power=1)),
    "short-last-block": (2048, 512, 6 * 512 - 100, 4, 0, 3, 2, dict(ref=2)),                # 7 frames: blocks of 4 and 3
    "one-frame-pair": (512, 128, 257, 100, 1, 4, 2, dict(ref=3)),                           # 4 frames, one block
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_against_the_restatement(eng, name):
    n_fft, hop, L, Tb, ctx, C, n, kw = CASES[name]
    assert span_of(64) == span_of(512) == span_of(1024) == 2048
    if name == "short-last-block":
        assert 1 + -(-L // hop) == 7
    mix, est = br.make_case(n_fft + 7 * n + L + Tb, "generic", n, C, L)
    got = check(eng, mix, est, f"{name}: n_fft {n_fft} hop {hop} L {L} Tb {Tb} ctx {ctx} C {C} n {n} {kw}", n_fft=n_fft,
                hop=hop, block_frames=Tb, context=ctx, **kw)
    print(f"{name}: worst ratios " + ", ".join(f"{k} {v:.2f}" for k, v in got.items()) + f" (allowed {FACTOR})")


@pytest.mark.parametrize("kind", br.KINDS)
def test_every_kind_on_an_array(eng, kind):
    """the cases of test_gpu_beamform.py's test of the same name, in blocks of 12 frames"""
    worst = {}
    for C, n, ref, post in ((4, 2, 3, None), (8, 4, 0, "mask"), (2, 3, 0, None), (3, 1, 2, "mask")):
        mix, est = br.make_case(len(kind) + C, kind, n, C, 2 * span_of(512) + 301)
        got = check(eng, mix, est, f"{kind} C {C} n {n} ref {ref} post {post}", ref=ref, postfilter=post, block_frames=12)
        worst = {k: max(v, worst.get(k, 0.0)) for k, v in got.items()}
    print(f"{kind}: worst ratios " + ", ".join(f"{k} {v:.2f}" for k, v in worst.items()) + f" (allowed {FACTOR})")


# ------------------------------------------------------------------ 2. one block: Engine.beamform up to the sum order
def test_one_block_is_beamform(eng):
    worst = 0.0
    for n_fft, hop, L, C, n, post in ((512, 128, 2 * span_of(512) + 301, 4, 2, None), (64, 16, 5000, 8, 4, "mask"),
                                      (2048, 512, 3 * span_of(2048) + 17, 3, 3, None)):
        mix, est = br.make_case(n_fft + L, "generic", n, C, L)
        m, e = torch.from_numpy(mix)[None].to(eng.device), torch.from_numpy(est)[None].to(eng.device)
        kw = dict(n_fft=n_fft, hop=hop, ref=C - 1, postfilter=post)
        F = 1 + -(-L // hop)
        fixed, ifix = eng.beamform(m, e, return_info=True, **kw)
        for Tb in (F, 1 << 20):
            out, info = eng.beamform_track(m, e, block_frames=Tb, return_info=True, **kw)
            assert tuple(info["w"].shape) == (1, 1) + tuple(ifix["w"].shape[1:])
            d = float((info["w"][:, 0] - ifix["w"]).abs().max() / ifix["w"].abs().max())
            worst = max(worst, d)
            assert d <= 1e-10, (n_fft, Tb, d)
            ref = br.beamform(mix, est, **kw)
            cpu = br.beamform(mix, est, dtype=np.float32, **kw)
            assert br.rel_err(out[0].cpu().numpy(), ref, mix) <= FACTOR * br.rel_err(cpu, ref, mix)
    print(f"one block against Engine.beamform: weights within {worst:.3e} of the largest (allowed 1e-10)")


# ------------------------------------------------------------------ 3. exact cases
def test_one_channel_is_mask_refine(eng):
    """C = 1: every block's w is 1.0 and w0 + alpha (w1 - w0) = 1.0, so every source is mask_refine with n = 1, and with
    the mask post-filter mask_refine itself"""
    for n_fft, hop, L in ((512, 128, 2 * span_of(512) + 301), (64, 16, 1033), (2048, 1024, 3 * span_of(2048) + 17)):
        for n, power in ((1, 2), (2, 1), (4, 2)):
            mix, est = br.make_case(n_fft + L + n, "generic", n, 1, L)
            m, e = torch.from_numpy(mix)[None].to(eng.device), torch.from_numpy(est)[None].to(eng.device)
            kw = dict(n_fft=n_fft, hop=hop, power=power)
            out, info = eng.beamform_track(m, e, block_frames=5, interpolate=True, return_info=True, **kw)
            assert info["w"].shape[1] == -(-(1 + -(-L // hop)) // 5) > 1 and bool((info["w"] == 1.0).all()), (n_fft, n)
            one = eng.mask_refine(m[:, 0], e[:, :1], **kw)
            assert float(one.abs().max()) > 0
            for i in range(n):
                assert same_bits(out[:, i], one[:, 0]), (n_fft, hop, L, n, i)
            post = eng.beamform_track(m, e, block_frames=5, interpolate=True, postfilter="mask", **kw)
            assert same_bits(post, eng.mask_refine(m[:, 0], e, **kw)), (n_fft, hop, L, n)


@pytest.mark.parametrize("post", [None, "mask"])
def test_silent_estimates_give_equal_outputs(eng, post):
    for n_fft, hop, L, C in ((512, 128, 2 * span_of(512) + 301, 4), (64, 8, 333, 8), (2048, 1024, 9000, 3)):
        mix, _ = br.make_case(n_fft + L, "generic", 2, C, L)
        for n in (2, 4):
            out = eng.beamform_track(torch.from_numpy(mix)[None], torch.zeros((1, n, L)), n_fft=n_fft, hop=hop, ref=C - 1,
                                     postfilter=post, block_frames=4)
            assert float(out.abs().max()) > 0
            for i in range(1, n):
                assert same_bits(out[0, i], out[0, 0]), (n_fft, n, i)


def test_a_context_over_all_blocks_needs_no_interpolation(eng):
    for n_fft, hop, L, C, n, Tb in ((512, 128, 2 * span_of(512) + 301, 4, 2, 6), (64, 16, 1033, 3, 3, 4)):
        mix, est = br.make_case(n_fft + L, "generic", n, C, L)
        K = -(-(1 + -(-L // hop)) // Tb)
        assert 1 < K - 1 <= native.TRACK_MAX_CONTEXT
        kw = dict(n_fft=n_fft, hop=hop, block_frames=Tb, context=K - 1, return_info=True)
        on, ion = eng.beamform_track(torch.from_numpy(mix)[None], torch.from_numpy(est)[None], interpolate=True, **kw)
        off, ioff = eng.beamform_track(torch.from_numpy(mix)[None], torch.from_numpy(est)[None], interpolate=False, **kw)
        w = torch.view_as_real(ion["w"])
        assert torch.equal(w, torch.view_as_real(ioff["w"])) and all(torch.equal(w[:, k], w[:, 0]) for k in range(K))
        assert same_bits(on, off) and float(on.abs().max()) > 0
        less = eng.beamform_track(torch.from_numpy(mix)[None], torch.from_numpy(est)[None], n_fft=n_fft, hop=hop,
                                  block_frames=Tb, context=0)
        assert not same_bits(less, on)


@pytest.mark.parametrize("n_fft,hop,n,post,Tb,ctx,interp", [(512, 128, 3, None, 7, 1, True),
                                                            (2048, 256, 2, "mask", 4, 0, False),
                                                            (64, 32, 4, None, 5, 2, True)])
def test_ragged(eng, n_fft, hop, n, post, Tb, ctx, interp):
    """6 items of distinct lengths and mixed channel counts (one with one channel, one at the minimum length, several
    with fewer blocks than the longest), NaN past every end and in every channel an item does not have: each item
    against the item alone, a permuted batch, a rerun, a base pointer one float off, one item per chunk, lists"""
    S, need = span_of(n_fft), n_fft // 2 + 1
    lens = [2 * S + 3 * hop + 5, need, S, S + Tb * hop + 3, S + 1, need + hop + 2]
    chans = [4, 1, 8, 2, 3, 5]
    Lmax, Cmax = max(lens) + 3, 8
    g = np.random.default_rng(n_fft + n)
    mix = torch.full((6, Cmax, Lmax), float("nan"))
    est = torch.full((6, n, Lmax), float("nan"))
    for b, (v, c) in enumerate(zip(lens, chans)):
        m, e = br.make_case(int(g.integers(1 << 30)), br.KINDS[b % 4], n, c, v)
        mix[b, :c, :v], est[b, :, :v] = torch.from_numpy(m), torch.from_numpy(e)
    kw = dict(n_fft=n_fft, hop=hop, postfilter=post, block_frames=Tb, context=ctx, interpolate=interp)
    blocks = [-(-(1 + -(-v // hop)) // Tb) for v in lens]
    Kmax = -(-(1 + -(-Lmax // hop)) // Tb)
    assert len(set(blocks)) > 2 and max(blocks) <= Kmax
    out, info = eng.beamform_track(mix, est, lens=lens, channels=chans, return_info=True, **kw)
    assert tuple(out.shape) == (6, n, Lmax) and not bool(torch.isnan(out).any())
    assert tuple(info["w"].shape) == (6, Kmax, n, n_fft // 2 + 1, Cmax)
    assert bool(torch.isfinite(torch.view_as_real(info["w"])).all())
    for b, (v, c) in enumerate(zip(lens, chans)):
        alone, ia = eng.beamform_track(mix[b:b + 1, :c, :v].contiguous(), est[b:b + 1, :, :v].contiguous(),
                                       return_info=True, **kw)
        assert same_bits(out[b, :, :v], alone[0]), f"item {b} differs from the item alone"
        assert ia["w"].shape[1] == blocks[b]
        assert torch.equal(torch.view_as_real(info["w"][b, :blocks[b], :, :, :c]), torch.view_as_real(ia["w"][0]))
        assert bool((info["w"][b, :, :, :, c:] == 0).all()), f"item {b}: weights in channels it does not have"
        assert bool((info["w"][b, blocks[b]:] == 0).all()), f"item {b}: weights in blocks it does not have"
        assert bool((info["w"][b, :blocks[b], :, :, :c] != 0).any())
        assert bool((out[b, :, v:] == 0).all()), f"item {b}: not zero past its end"
        assert float(alone.abs().max()) > 0
    perm = [3, 0, 5, 4, 2, 1]
    again = eng.beamform_track(mix[perm].contiguous(), est[perm].contiguous(), lens=[lens[p] for p in perm],
                               channels=[chans[p] for p in perm], **kw)
    assert same_bits(again, out[perm])
    assert same_bits(eng.beamform_track(mix, est, lens=lens, channels=chans, **kw), out)
    shifted = eng.beamform_track(off_alignment(mix, eng.device), off_alignment(est, eng.device), lens=lens, channels=chans,
                                 **kw)
    assert same_bits(shifted, out)
    one_item = native.track_item_bytes(n_fft, hop, Lmax, Cmax, n, Tb)
    chunked, ic = eng.beamform_track(mix, est, lens=lens, channels=chans, workspace_budget=one_item, return_info=True, **kw)
    assert same_bits(chunked, out) and torch.equal(torch.view_as_real(ic["w"]), torch.view_as_real(info["w"]))
    assert same_bits(eng.beamform_track(mix, est, lens=lens, channels=chans, workspace_budget=2 * one_item + 8, **kw), out)
    as_list = eng.beamform_track([mix[b, :c, :v] for b, (v, c) in enumerate(zip(lens, chans))],
                                 [est[b, :, :v] for b, v in enumerate(lens)], **kw)
    for b, v in enumerate(lens):
        assert tuple(as_list[b].shape) == (n, v) and same_bits(as_list[b], out[b, :, :v])


# ------------------------------------------------------------------ 4. refusals
def test_refusals_launch_nothing(eng):
    B, Cn, n, L = 2, 4, 2, 600
    mix = torch.zeros((B, Cn, L), device=eng.device)
    est = torch.zeros((B, n, L), device=eng.device)
    out = torch.full((B, n, L), 7.0, device=eng.device)
    good = dict(mix=mix, est=est, B=B, C=Cn, n=n, Lmax=L, lens=None, channels=None, ref=0, n_fft=512, hop=128, power=2,
                eps=1e-10, reg=1e-3, post=0, block=4, context=1, interp=1, budget=0, out=out)

    def call(**kw):
        a = dict(good, **kw)
        i32 = lambda v: None if v is None else (native.C.c_int32 * len(v))(*v)
        return eng.lib.dsn_beamform_track(eng.ctx, native._ptr(a["mix"]), native._ptr(a["est"]), a["B"], a["C"], a["n"],
                                          a["Lmax"], i32(a["lens"]), i32(a["channels"]), a["ref"], a["n_fft"], a["hop"],
                                          a["power"], a["eps"], a["reg"], a["post"], a["block"], a["context"], a["interp"],
                                          a["budget"], native._ptr(a["out"]), None, eng._stream())

    flat = torch.zeros(B * (Cn + 2 * n) * L + 8, device=eng.device)
    need = native.track_item_bytes(512, 128, L, Cn, n, 4)
    for kw, msg in ((dict(mix=None), "mix, est or out is null"), (dict(est=None), "mix, est or out is null"),
                    (dict(out=None), "mix, est or out is null"),
                    (dict(post=2), "postfilter = 2 is not one of 0 (DSN_BEAMFORM_POST_NONE), 1 (DSN_BEAMFORM_POST_MASK)"),
                    (dict(B=0), "B = 0 outside [1, 65535]"),
                    (dict(C=0), "C = 0 outside [1, 8]"), (dict(C=9), "C = 9 outside [1, 8]"),
                    (dict(n=0), "n = 0 outside [1, 4]"), (dict(n=5), "n = 5 outside [1, 4]"),
                    (dict(n_fft=32, hop=8), "n_fft = 32 is not a power of two in [64, 2048]"),
                    (dict(hop=512), "n_fft / hop = 512 / 512 is not one of 2, 4, 8"),
                    (dict(power=3), "power = 3 is not 1 or 2"),
                    (dict(eps=0.0), "eps = 0 is not a finite positive number"),
                    (dict(reg=-1.0), "reg = -1 is not a finite number >= 0"),
                    (dict(reg=float("nan")), "is not a finite number >= 0"),
                    (dict(lens=[600, 256]), "item 1 has 256 samples, outside [n_fft / 2 + 1 = 257, Lmax = 600]"),
                    (dict(channels=[2, 5]), "channels[1] = 5 outside [1, C = 4]"),
                    (dict(ref=4), "ref = 4 outside [0, 4): item 0 has 4 channels"),
                    (dict(ref=2, channels=[4, 2]), "ref = 2 outside [0, 2): item 1 has 2 channels"),
                    (dict(block=3), "block_frames = 3 outside [4, 2^20]"),
                    (dict(block=(1 << 20) + 1), "block_frames = 1048577 outside [4, 2^20]"),
                    (dict(context=-1), "context = -1 outside [0, 64]"),
                    (dict(context=65), "context = 65 outside [0, 64]"),
                    (dict(interp=2), "interpolate = 2 is not 0 or 1"), (dict(interp=-1), "interpolate = -1 is not 0 or 1"),
                    (dict(Lmax=4 * 128 * 4096), "4097 blocks of block_frames = 4 frames at Lmax = 2097152, hop = 128: more "
                                                "than 4096"),
                    (dict(budget=-1), "workspace_budget = -1 < 0"),
                    (dict(budget=need - 1), f"is smaller than one item ({need} bytes at C = 4, n = 2"),
                    (dict(mix=out), "out overlaps mix or est"),
                    (dict(est=flat[4:], out=flat), "out overlaps mix or est")):
        assert call(**kw) != 0, kw
        text = eng.lib.dsn_last_error(eng.ctx).decode()
        assert msg in text and "dsn_beamform_track: " in text, (kw, text)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((flat == 0.0).all())
    for post in (0, 1):
        out.fill_(7.0)
        assert call(post=post, budget=need) == 0
        torch.cuda.synchronize()
        assert bool((out == 0.0).all())             # a silent mixture: tau = 0, w = e_ref, silence
    # the refusals of the Python layer come first
    with pytest.raises(ValueError, match=r"beamform_track: ref = 3 outside \[0, 3\): item 0 has 3 channels"):
        eng.beamform_track(torch.zeros(1, 3, 600), torch.zeros(1, 2, 600), ref=3)
    with pytest.raises(ValueError, match=r"beamform_track: block_frames = 3 outside \[4, 2\^20\]"):
        eng.beamform_track(torch.zeros(1, 3, 600), torch.zeros(1, 2, 600), block_frames=3)
    with pytest.raises(ValueError, match="a list of mixtures goes with a list of as many estimates"):
        eng.beamform_track([torch.zeros(3, 600)], torch.zeros(1, 2, 600))
