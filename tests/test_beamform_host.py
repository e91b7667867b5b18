"""The `beamform` keyword without a GPU: the float64 restatement's own properties (tests/beamform_restatement.py), the
option parsing and refusals of ditsep_amd.native, and the command line."""
import numpy as np
import pytest

from ditsep_amd import native, separate
from tests import beamform_restatement as br
from tests import mask_refine_restatement as mr


@pytest.mark.parametrize("C", [2, 4, 8])
def test_the_two_solvers_agree(C):
    """numpy.linalg.solve against the explicit Cholesky: A = Q + lambda I has a condition number of about 1 / reg = 1e3
    at the worst (dual-mono, hard pans), so the two may differ by about 1e3 x 2^-53 x a modest factor; 1e-9 relative to
    the largest weight is the bound, the largest difference seen is 3e-12"""
    for k, kind in enumerate(br.KINDS):
        for n in (1, 2, 4):
            mix, est = br.make_case(7 * C + k + n, kind, n, C, 900)
            a, ia = br.beamform(mix, est, n_fft=256, hop=64, return_info=True)
            b, ib = br.beamform(mix, est, n_fft=256, hop=64, solver="solve", return_info=True)
            assert np.all(np.isfinite(ia["w"])) and np.all(np.isfinite(a))
            top = np.max(np.abs(ia["w"]))
            assert np.max(np.abs(ia["w"] - ib["w"])) <= 1e-9 * top, (kind, n)
            assert br.rel_err(a, b, mix) < 1e-9, (kind, n)
            assert ia["power"].min() >= 1e-6 * ia["power"].max()          # every bin carries signal


def test_the_filter_is_distortionless_in_the_statistics():
    """w^H N_i e_ref = tr(Z)^-1 e_ref^H Z^H N_i e_ref: with a rank-one N_i = p d d^H and Q of full rank the MVDR
    constraint w^H d = d_ref holds, which the rank-one single-source case shows to rounding"""
    g = np.random.default_rng(3)
    C, bins = 4, 5
    d = g.standard_normal((bins, C)) + 1j * g.standard_normal((bins, C))
    Ni = 2.5 * np.einsum("fc,fd->fcd", d, d.conj())
    V = g.standard_normal((bins, C, 3 * C)) + 1j * g.standard_normal((bins, C, 3 * C))
    Nj = np.einsum("fck,fdk->fcd", V, V.conj())
    for ref in (0, 3):
        w = br.weights(np.stack([Ni, Nj]), ref, 0.0, 0.0)[0]
        got = np.einsum("fc,fc->f", w.conj(), d)
        assert np.allclose(got, d[:, ref], rtol=1e-9, atol=0)


@pytest.mark.parametrize("post", [None, "mask"])
def test_one_channel_has_unit_weights(post):
    """C = 1: w = Z / Z = 1.0 exactly, the output is the mixture's own transform handed back (mask_refine with n = 1),
    and with the mask post-filter mask_refine itself"""
    for n in (1, 2, 4):
        mix, est = br.make_case(21 + n, "generic", n, 1, 1000)
        for dtype in (np.float64, np.float32):
            out, info = br.beamform(mix, est, n_fft=256, hop=64, postfilter=post, dtype=dtype, return_info=True)
            assert np.all(info["w"] == 1.0)
            if post is None:
                want = mr.refine_torch(mix[0], est[:1], 256, 64, dtype=dtype)
                assert all(np.array_equal(out[i], want[0]) for i in range(n))
            else:
                assert np.array_equal(out, mr.refine_torch(mix[0], est, 256, 64, dtype=dtype))


def test_scaling_the_mixture_leaves_the_weights():
    """N_i and Q_i scale alike and lambda with them as eps -> 0, so w does not change (the scale of N_i cancels)"""
    mix, est = br.make_case(31, "generic", 3, 4, 1500)
    kw = dict(n_fft=256, hop=64, eps=1e-30, ref=2, return_info=True)
    _, a = br.beamform(mix, est, **kw)
    _, b = br.beamform(8.0 * mix.astype(np.float64), est, **kw)       # (a power of two: the products scale exactly)
    _, c = br.beamform(3.7 * mix.astype(np.float64), est, **kw)
    top = np.max(np.abs(a["w"]))
    assert np.max(np.abs(a["w"] - b["w"])) <= 1e-12 * top
    assert np.max(np.abs(a["w"] - c["w"])) <= 1e-9 * top             # condition number x float64 rounding


def test_dual_mono_gives_the_channel_average_and_silence_the_reference():
    mix, est = br.make_case(41, "dual", 2, 4, 1200)
    _, info = br.beamform(mix, est, n_fft=256, hop=64, return_info=True)
    assert np.allclose(info["w"], 0.25, atol=1e-6)                     # no spatial information: the average
    out, info = br.beamform(np.zeros((3, 600), np.float32), np.zeros((2, 600), np.float32), ref=1, n_fft=256, hop=64,
                            return_info=True)
    assert np.array_equal(info["w"], np.broadcast_to(np.array([0, 1, 0], np.complex128), info["w"].shape))
    assert not out.any()


def test_silent_estimates_give_equal_outputs():
    mix, est = br.make_case(13, "silent_est", 4, 3, 800)
    out = br.beamform(mix, est, n_fft=128, hop=64)
    for i in range(1, 4):
        assert np.array_equal(out[i], out[0])


def test_float32_mode_is_close_to_float64():
    mix, est = br.make_case(5, "generic", 2, 4, 3000)
    ref, iref = br.beamform(mix, est, return_info=True)
    f32, i32 = br.beamform(mix, est, dtype=np.float32, return_info=True)
    assert f32.dtype == np.float32 and 1e-9 < br.rel_err(f32, ref, mix) < 1e-5
    assert 1e-9 < np.max(np.abs(i32["w"] - iref["w"])) / np.max(np.abs(iref["w"])) < 1e-4


def test_sanity_beamforming_beats_the_single_channel_mask():
    """4 channels, 2 burst-noise sources, 24-tap random mixing filters, estimates with 30 % leakage: the SI-SDR of every
    beamformed source against its image at the reference microphone exceeds that of the mask post-filter alone on the
    reference channel (C = 1).  The restatement's figures for this case: 19.15 / 14.21 dB beamformed (13.98 / 11.17 dB
    with the mask post-filter on top) against 10.58 / 9.53 dB for the mask on channel 0; the estimates themselves are
    at 11.34 / 9.61 dB.  A sanity figure on synthetic data, not a quality claim."""
    mix, est, img0 = br.sanity_case(0)
    bf = br.beamform(mix, est)
    mask = br.beamform(mix[:1], est, postfilter="mask")
    got = [br.si_sdr(bf[i], img0[i]) for i in range(2)]
    base = [br.si_sdr(mask[i], img0[i]) for i in range(2)]
    print("beamformed", got, "mask at C = 1", base)
    assert got == pytest.approx([19.15, 14.21], abs=0.05) and base == pytest.approx([10.58, 9.53], abs=0.05)
    assert all(a > b for a, b in zip(got, base))


def test_beamform_options():
    assert native.beamform_options(None) is None
    assert native.BEAMFORM_DEFAULTS == dict(ref=0, n_fft=512, hop=128, power=2, eps=1e-10, reg=1e-3, postfilter=None)
    assert all(native.BEAMFORM_DEFAULTS[k] == native.STEMS_DEFAULTS[k] for k in ("n_fft", "hop", "power", "eps", "reg"))
    assert native.beamform_options(True) == native.BEAMFORM_DEFAULTS
    assert native.beamform_options(3) == dict(native.BEAMFORM_DEFAULTS, ref=3)
    assert native.beamform_options(0) == native.BEAMFORM_DEFAULTS
    assert native.beamform_options({"ref": 1, "n_fft": 1024, "hop": 256, "postfilter": "mask"}) == dict(
        ref=1, n_fft=1024, hop=256, power=2, eps=1e-10, reg=1e-3, postfilter="mask")
    for bad, msg in ((False, "beamform must be None, True, a reference channel or a dict"), ("mvdr", "beamform must be"),
                     (1.5, "beamform must be"), (-1, "beamform: the reference channel -1 is negative"),
                     ({"window": 3}, r"beamform: unknown keys \['window'\]"),
                     ({"postfilter": "wiener"}, r"beamform: postfilter must be None, 'none' or 'mask' \(got 'wiener'\)")):
        with pytest.raises(ValueError, match=msg):
            native.beamform_options(bad)


def test_check_beamform():
    good = native.check_beamform((3, 4, 600), (3, 2, 600), [600, 300, 257], [4, 2, 3], ref=1, postfilter="mask")
    assert good == ((3, 4, 2, 600), [600, 300, 257], [4, 2, 3], 1, 512, 128, 2, 1e-10, 1e-3, 1, 0)
    assert native.check_beamform((1, 8, 600), (1, 1, 600), ref=7)[:4] == ((1, 8, 1, 600), None, None, 7)
    need = native.beamform_item_bytes(512, 128, 600, 2, 2)
    assert need == 8 * (1 + 1) * 2 * 2 * 3 * 257
    # one span more than the cap holds: still 16 owners, each with two spans
    assert native.beamform_item_bytes(512, 128, 17 * 2048, 8, 4) == 8 * (16 + 1) * 4 * 72 * 257
    assert native.check_beamform((1, 2, 600), (1, 2, 600), workspace_budget=need)[-1] == need
    for args, kw, msg in (
            (((2, 600), (2, 2, 600)), {}, r"beamform: mix must be \[B, C, L\] and est \[B, n, L\]"),
            (((2, 2, 600), (2, 2, 601)), {}, "beamform: mix must be"),
            (((1, 9, 600), (1, 2, 600)), {}, r"beamform: C = 9 outside \[1, 8\]"),
            (((1, 2, 600), (1, 5, 600)), {}, r"beamform: n = 5 outside \[1, 4\]"),
            (((1, 2, 600), (1, 2, 600)), dict(n_fft=384), "beamform: n_fft = 384 is not a power of two"),
            (((1, 2, 600), (1, 2, 600)), dict(hop=512), "beamform: n_fft / hop = 512 / 512 is not one of 2, 4, 8"),
            (((1, 2, 600), (1, 2, 600)), dict(power=3), "beamform: power = 3 is not 1 or 2"),
            (((1, 2, 600), (1, 2, 600)), dict(eps=0.0), "beamform: eps = 0.0 is not a finite positive number"),
            (((1, 2, 600), (1, 2, 600)), dict(reg=-1e-3), "beamform: reg = -0.001 is not a finite number >= 0"),
            (((1, 2, 600), (1, 2, 600)), dict(reg=float("nan")), "beamform: reg = nan is not a finite number"),
            (((1, 2, 600), (1, 2, 600)), dict(postfilter="wiener"), "beamform: postfilter must be None, 'none' or 'mask'"),
            (((1, 2, 600), (1, 2, 600)), dict(lens=[256]),
             r"beamform: item 0 has 256 samples, outside \[n_fft / 2 \+ 1 = 257"),
            (((2, 2, 600), (2, 2, 600)), dict(channels=[2]), "beamform: channels must hold one channel count per item"),
            (((2, 2, 600), (2, 2, 600)), dict(channels=[2, 3]),
             r"beamform: item 1 has channels = 3, outside \[1, C = 2\]"),
            (((2, 4, 600), (2, 2, 600)), dict(ref=4), r"beamform: ref = 4 outside \[0, 4\): item 0 has 4 channels"),
            (((2, 4, 600), (2, 2, 600)), dict(ref=-1), r"beamform: ref = -1 outside \[0, 4\)"),
            (((2, 4, 600), (2, 2, 600)), dict(ref=2, channels=[3, 2]),
             r"beamform: ref = 2 outside \[0, 2\): item 1 has 2 channels"),
            (((2, 4, 600), (2, 2, 600)), dict(ref=1.5), "beamform: ref = 1.5 is not a channel index"),
            (((1, 2, 600), (1, 2, 600)), dict(workspace_budget=-1), "beamform: workspace_budget = -1 < 0"),
            (((1, 2, 600), (1, 2, 600)), dict(workspace_budget=need - 1),
             rf"beamform: workspace_budget = {need - 1} bytes is smaller than one item \({need} bytes at C = 2, n = 2")):
        with pytest.raises(ValueError, match=msg):
            native.check_beamform(*args, **kw)


def test_command_line_flags():
    p = separate.build_parser()
    base = ["in", "out", "--config", "c.json"]
    a = p.parse_args(base)
    assert a.beamform is False and separate.beamform_of(a) is None
    a = p.parse_args(base + ["--beamform"])
    assert separate.beamform_of(a) == dict(ref=0, n_fft=512, hop=128, reg=1e-3, postfilter=None)
    assert native.beamform_options(separate.beamform_of(a)) == native.BEAMFORM_DEFAULTS
    a = p.parse_args(base + ["--beamform", "--beamform-ref", "3", "--beamform-nfft", "1024", "--beamform-hop", "256",
                             "--beamform-reg", "0.01", "--beamform-post", "mask"])
    assert separate.beamform_of(a) == dict(ref=3, n_fft=1024, hop=256, reg=0.01, postfilter="mask")
    assert separate.beamform_of(p.parse_args(base + ["--beamform", "--beamform-post", "none"]))["postfilter"] is None
    for bad in (["--beamform-post", "wiener"], ["--beamform-ref", "x"]):
        with pytest.raises(SystemExit):
            p.parse_args(base + bad)
