"""dsn_dereverb (ditsep_amd/csrc/dereverb.hip) through Engine.dereverb on an engine with no score network and no codec,
against the restatement (tests/dereverb_restatement.py).

Bounds.  The error of an output is its largest absolute difference from the float64 restatement divided by the peak of
|mix|; the error of the filter is its largest absolute difference from the float64 restatement's divided by that
item's largest |G|.  Each may be at most 8 x what the float32 run of the same restatement shows on the same input
(float32 pocketfft transforms, float64 solve: the device's own split of precisions) -- the rule and the factor of
tests/test_gpu_beamform.py and tests/test_gpu_stems.py, for the same reason: the device's radix-2 butterfly order and
its fused multiply-adds differ from pocketfft's.  Every such case first asserts on the restatement that the worst
bin's cond(A) is at most 1e7 at reg = 1e-4 (above that an error ratio stops meaning anything; measured: at most 8.0e5)
and that no bin passed through.  Everything else -- items with F <= D and a silent item against Engine.mask_refine, a
power-of-two scale, ragged NaN-padded items with mixed channel counts against each item alone, a permuted batch, a
rerun, a base pointer one float off, a workspace budget of one item, lists -- is bit for bit.

Measured on an MI355X: see the README paragraph "Dereverberation"."""
import numpy as np
import pytest
import torch

from ditsep_amd import native
from tests import dereverb_restatement as dr
from tests.util import make_engine

pytestmark = pytest.mark.gpu
FACTOR = 8.0
COND_CAP = 1e7

# n_fft, hop, C, taps, delay, L, iterations: the smallest shapes at which each part can go wrong
CASES = {
    "tiles": (64, 16, 2, 4, 1, 6000, 3),          # 376 frames: more than one frame tile, the halo across tiles
    "largest": (512, 128, 8, 10, 3, 4000, 3),     # 80 unknowns, 33 frames: loading-dominated
    "array": (512, 128, 4, 10, 3, 16000, 3),
    "few_frames": (2048, 512, 3, 2, 2, 3000, 3),  # 7 frames
    "one_channel": (512, 128, 1, 10, 3, 6000, 3),
    "one_tap": (512, 128, 4, 1, 3, 5000, 3),
    "delay_8": (512, 128, 2, 6, 8, 5000, 3),
    "one_iteration": (512, 128, 4, 10, 3, 5000, 1),
    "odd_system": (256, 32, 3, 5, 2, 4001, 2),    # 15 unknowns: no multiple of the 4 x 4 register block
}


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


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def ratio(dev, cpu):
    return dev / cpu if cpu > 0 else (0.0 if dev == 0 else float("inf"))


# ------------------------------------------------------------------ 1. parity with the restatement
@pytest.mark.parametrize("name", sorted(CASES))
def test_against_the_restatement(eng, name):
    n_fft, hop, C, K, D, L, I = CASES[name]
    kw = dict(taps=K, delay=D, iterations=I, n_fft=n_fft, hop=hop)
    mix, _ = dr.reverb_case(n_fft + C + K, C, L)
    ref, iref = dr.dereverb(mix, return_info=True, return_cond=True, **kw)
    assert iref["cond"] <= COND_CAP, f"{name}: cond(A) = {iref['cond']:.2e} on the restatement"
    assert iref["fail"] == 0
    cpu, icpu = dr.dereverb(mix, dtype=np.float32, return_info=True, **kw)
    out, info = eng.dereverb(off_alignment(torch.from_numpy(mix)[None], eng.device), return_info=True, **kw)
    out, G = out[0].cpu().numpy(), info["G"][0].numpy()
    assert out.shape == ref.shape and G.shape == iref["G"].shape
    assert np.all(np.isfinite(out)) and np.all(np.isfinite(G))
    assert int(info["fail"][0]) == iref["fail"] == 0
    top = float(np.max(np.abs(iref["G"])))
    assert top > 0
    rel = lambda a: float(np.max(np.abs(a - iref["G"])) / top)
    pairs = {"parity": (dr.rel_err(out, ref, mix), dr.rel_err(cpu, ref, mix)), "G": (rel(G), rel(icpu["G"]))}
    print(f"{name}: cond {iref['cond']:.2e}; " + "; ".join(
        f"{k} {d:.3e} (float32 CPU {c:.3e}, ratio {ratio(d, c):.2f})" for k, (d, c) in pairs.items()))
    for k, (d, c) in pairs.items():
        assert d <= FACTOR * c, f"{name}: {k} {ratio(d, c):.2f} x the float32 CPU error"


# ------------------------------------------------------------------ 2. exact cases
def test_short_and_silent_items_are_the_round_trip(eng):
    """F <= D: P = 0, G = 0, X = Y; so is a silent item.  Every channel is mask_refine of that channel with n = 1"""
    g = torch.Generator().manual_seed(5)
    for n_fft, hop, D, L, C in ((512, 128, 8, 700, 3), (2048, 1024, 4, 2500, 2), (64, 32, 3, 33, 8),
                                (128, 64, 8, 401, 2), (256, 128, 8, 799, 2), (1024, 512, 8, 3001, 2)):
        F = 1 + (L + hop - 1) // hop
        assert F <= D
        x = (0.3 * torch.randn((1, C, L), generator=g)).to(eng.device)
        out, info = eng.dereverb(x, taps=4, delay=D, n_fft=n_fft, hop=hop, return_info=True)
        assert bool((info["G"] == 0).all()) and int(info["fail"][0]) == 0
        assert float(out.abs().max()) > 0
        for c in range(C):
            one = eng.mask_refine(x[:, c], x[:, c:c + 1], n_fft=n_fft, hop=hop)
            assert same_bits(out[:, c], one[:, 0]), (n_fft, c)
    x = torch.zeros((1, 4, 5000), device=eng.device)
    out, info = eng.dereverb(x, return_info=True)
    assert bool((out == 0).all()) and bool((info["G"] == 0).all()) and int(info["fail"][0]) == 0
    one = eng.mask_refine(x[:, 0], x[:, :1])
    assert same_bits(out[:, 0], one[:, 0])


def test_a_power_of_two_scale_commutes(eng):
    for name in ("array", "tiles", "few_frames"):
        n_fft, hop, C, K, D, L, I = CASES[name]
        kw = dict(taps=K, delay=D, iterations=I, n_fft=n_fft, hop=hop)
        x = torch.from_numpy(dr.reverb_case(3, C, L)[0])[None].to(eng.device)
        a, ia = eng.dereverb(x, return_info=True, **kw)
        b, ib = eng.dereverb(4.0 * x, return_info=True, **kw)
        assert float(a.abs().max()) > 0 and float(ia["G"].abs().max()) > 0
        assert torch.equal(torch.view_as_real(ia["G"]), torch.view_as_real(ib["G"])), name
        assert same_bits(b, 4.0 * a), name


@pytest.mark.parametrize("n_fft,hop,K,D,I", [(512, 128, 10, 3, 3), (64, 16, 4, 1, 2), (2048, 512, 2, 2, 3)])
def test_ragged(eng, n_fft, hop, K, D, I):
    """5 items of distinct lengths and mixed channel counts, one at the minimum, one with F <= D + K, NaN past every end
    and in every channel an item does not have: each item against the item alone, a permuted batch, a rerun, a base
    pointer one float off, one item per chunk, lists"""
    need = n_fft // 2 + 1
    lens = [70 * hop + 5, need, 9 * hop, 40 * hop + 3, need + hop + 2]
    chans = [4, 1, 8, 2, 3]
    Lmax, Cmax = max(lens) + 3, 8
    mix = torch.full((5, Cmax, Lmax), float("nan"))
    for b, (v, c) in enumerate(zip(lens, chans)):
        mix[b, :c, :v] = torch.from_numpy(dr.reverb_case(n_fft + b, c, v)[0])
    kw = dict(taps=K, delay=D, iterations=I, n_fft=n_fft, hop=hop)
    mixd = mix.to(eng.device)
    out, info = eng.dereverb(mixd, lens=lens, channels=chans, return_info=True, **kw)
    assert tuple(out.shape) == (5, Cmax, Lmax) and not bool(torch.isnan(out).any())
    assert bool(torch.isfinite(torch.view_as_real(info["G"])).all())
    for b, (v, c) in enumerate(zip(lens, chans)):
        alone, ia = eng.dereverb(mixd[b:b + 1, :c, :v].contiguous(), return_info=True, **kw)
        assert same_bits(out[b, :c, :v], alone[0]), f"item {b} differs from the item alone"
        Gb = info["G"][b]
        assert torch.equal(torch.view_as_real(Gb[:, :c * K, :c]), torch.view_as_real(ia["G"][0]))
        assert bool((Gb[:, c * K:] == 0).all()) and bool((Gb[:, :, c:] == 0).all())
        assert int(info["fail"][b]) == int(ia["fail"][0])
        assert bool((out[b, :, v:] == 0).all()) and bool((out[b, c:] == 0).all()), f"item {b}: not zero outside"
        assert float(alone.abs().max()) > 0
    perm = [3, 0, 4, 2, 1]
    again = eng.dereverb(mixd[perm].contiguous(), lens=[lens[p] for p in perm], channels=[chans[p] for p in perm], **kw)
    assert same_bits(again, out[perm])
    assert same_bits(eng.dereverb(mixd, lens=lens, channels=chans, **kw), out)
    assert same_bits(eng.dereverb(off_alignment(mix, eng.device), lens=lens, channels=chans, **kw), out)
    one_item = native.dereverb_item_bytes(n_fft, hop, Lmax, Cmax, K)
    assert same_bits(eng.dereverb(mixd, lens=lens, channels=chans, workspace_budget=one_item, **kw), out)
    o2, i2 = eng.dereverb(mixd, lens=lens, channels=chans, workspace_budget=2 * one_item + 8, return_info=True, **kw)
    assert same_bits(o2, out) and torch.equal(torch.view_as_real(i2["G"]), torch.view_as_real(info["G"]))
    assert torch.equal(i2["fail"], info["fail"])
    as_list = eng.dereverb([mix[b, :c, :v] for b, (v, c) in enumerate(zip(lens, chans))], **kw)
    for b, (v, c) in enumerate(zip(lens, chans)):
        assert tuple(as_list[b].shape) == (c, v) and same_bits(as_list[b], out[b, :c, :v])


def test_a_failed_pivot_passes_the_bin_through(eng):
    """one NaN sample inside an item: every bin's lambda, R and first pivot are NaN, so every bin is counted and passes
    through with G = 0 (the restatement counts the same bins); the item next to it is untouched"""
    mix, _ = dr.reverb_case(11, 2, 3000)
    bad = mix.copy()
    bad[1, 1500] = np.nan
    _, iref = dr.dereverb(bad, taps=4, return_info=True)
    assert iref["fail"] == 257
    both = torch.from_numpy(np.stack([bad, mix]))
    out, info = eng.dereverb(both, taps=4, return_info=True)
    assert [int(v) for v in info["fail"]] == [257, 0]
    assert bool((info["G"][0] == 0).all()) and float(info["G"][1].abs().max()) > 0
    assert same_bits(out[1:], eng.dereverb(both[1:], taps=4))


# ------------------------------------------------------------------ 3. refusals
def test_refusals_launch_nothing(eng):
    B, Cn, L = 2, 4, 600
    mix = torch.zeros((B, Cn, L), device=eng.device)
    out = torch.full((B, Cn, L), 7.0, device=eng.device)
    good = dict(mix=mix, B=B, C=Cn, Lmax=L, lens=None, channels=None, n_fft=512, hop=128, taps=10, delay=3, iterations=3,
                reg=1e-4, eps=1e-10, budget=0, out=out)

    def call(**kw):
        a = dict(good, **kw)
        i32 = lambda v: None if v is None else (native.C.c_int32 * len(v))(*v)
        return eng.lib.dsn_dereverb(eng.ctx, native._ptr(a["mix"]), a["B"], a["C"], a["Lmax"], i32(a["lens"]),
                                    i32(a["channels"]), a["n_fft"], a["hop"], a["taps"], a["delay"], a["iterations"],
                                    a["reg"], a["eps"], a["budget"], native._ptr(a["out"]), None, None, eng._stream())

    flat = torch.zeros(2 * B * Cn * L + 8, device=eng.device)
    need = native.dereverb_item_bytes(512, 128, L, Cn, 10)
    for kw, msg in ((dict(mix=None), "mix or out is null"), (dict(out=None), "mix or out is null"),
                    (dict(B=0), "B = 0 outside [1, 65535]"),
                    (dict(C=0), "C = 0 outside [1, 8]"), (dict(C=9), "C = 9 outside [1, 8]"),
                    (dict(taps=0), "taps = 0 outside [1, 16]"), (dict(taps=17), "taps = 17 outside [1, 16]"),
                    (dict(delay=0), "delay = 0 outside [1, 8]"), (dict(delay=9), "delay = 9 outside [1, 8]"),
                    (dict(C=8, taps=11), "C taps = 8 x 11 = 88 unknowns per bin, more than 80"),
                    (dict(iterations=0), "iterations = 0 outside [1, 8]"),
                    (dict(iterations=9), "iterations = 9 outside [1, 8]"),
                    (dict(n_fft=32, hop=8), "n_fft = 32 is not a power of two in [64, 2048]"),
                    (dict(n_fft=4096, hop=1024), "n_fft = 4096 is not a power of two in [64, 2048]"),
                    (dict(hop=512), "n_fft / hop = 512 / 512 is not one of 2, 4, 8"),
                    (dict(hop=0), "n_fft / hop = 512 / 0 is not one of 2, 4, 8"),
                    (dict(eps=0.0), "eps = 0 is not a finite positive number"),
                    (dict(eps=float("nan")), "is not a finite positive number"),
                    (dict(reg=-1.0), "reg = -1 is not a finite number >= 0"),
                    (dict(reg=float("inf")), "is not a finite number >= 0"),
                    (dict(reg=float("nan")), "is not a finite number >= 0"),
                    (dict(lens=[600, 256]), "item 1 has 256 samples, outside [n_fft / 2 + 1 = 257, Lmax = 600]"),
                    (dict(lens=[601, 600]), "item 0 has 601 samples, outside"),
                    (dict(channels=[2, 5]), "channels[1] = 5 outside [1, C = 4]"),
                    (dict(channels=[0, 1]), "channels[0] = 0 outside [1, C = 4]"),
                    (dict(budget=-1), "workspace_budget = -1 < 0"),
                    (dict(budget=need - 1), f"is smaller than one item ({need} bytes at C = 4, taps = 10"),
                    (dict(mix=out), "out overlaps mix"),
                    (dict(mix=flat[4:], out=flat), "out overlaps mix")):
        assert call(**kw) != 0, kw
        assert msg in eng.lib.dsn_last_error(eng.ctx).decode(), (kw, eng.lib.dsn_last_error(eng.ctx).decode())
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((flat == 0.0).all())
    assert call(budget=need) == 0
    torch.cuda.synchronize()
    assert bool((out == 0.0).all())             # a silent mixture passes through: silence
    # the refusals of the Python layer come first
    with pytest.raises(ValueError, match=r"dereverb: C = 9 outside \[1, 8\]"):
        eng.dereverb(torch.zeros(1, 9, 600))
    with pytest.raises(ValueError, match=r"dereverb: C taps = 8 x 11 = 88 unknowns"):
        eng.dereverb(torch.zeros(1, 8, 600), taps=11)
