"""The restatement of dsn_beamform_spatial (tests/spatial_restatement.py) against itself and against
tests/beamform_restatement.py, and the host side of the `spatial` keyword: options, refusals, command-line flags."""
import numpy as np
import pytest
import torch

from ditsep_amd import native, separate
from ditsep_amd.latent import LatentDiffSep
from tests import beamform_restatement as br
from tests import spatial_restatement as sp
from tests import stems_restatement as sr


@pytest.fixture(scope="module")
def sanity():
    """sanity_case(leak=0.6) cut to 8000 samples, and its float64 run at 3 iterations"""
    mix, est, img = br.sanity_case(leak=0.6, L=8000)
    out, info = sp.beamform_spatial(mix, est, iterations=3, return_info=True)
    return mix, est, img, out, info


def test_the_two_solvers_agree(sanity):
    """q and log det by numpy.linalg against the explicit Cholesky: the classes' covariances are loaded to a condition
    number of at most about 1 / reg = 1e3, so both are good to about 1e3 x 2^-53 = 1e-13 relative; gamma, a ratio of
    exponentials of C log q, to about C x that.  Measured: gamma 2.8e-13, w 2.5e-13 of the largest weight.  Bounded at
    1e-10."""
    mix, est, _, out, info = sanity
    other, io = sp.beamform_spatial(mix, est, iterations=3, solver="solve", return_info=True)
    dg = float(np.max(np.abs(io["gamma"] - info["gamma"])))
    dw = float(np.max(np.abs(io["w"] - info["w"])) / np.max(np.abs(info["w"])))
    print(f"solve against cholesky: gamma {dg:.3e}, w {dw:.3e} of the largest weight, out {br.rel_err(other, out, mix):.3e}")
    assert dg <= 1e-10 and dw <= 1e-10 and io["failed"] == info["failed"] == 0
    for C, n in ((8, 4), (3, 1)):
        mix, est = br.make_case(C, "generic", n, C, 4001)
        _, ia = sp.beamform_spatial(mix, est, iterations=2, return_info=True)
        _, ib = sp.beamform_spatial(mix, est, iterations=2, solver="solve", return_info=True)
        dg = float(np.max(np.abs(ia["gamma"] - ib["gamma"])))
        dw = float(np.max(np.abs(ia["w"] - ib["w"])) / np.max(np.abs(ia["w"])))
        print(f"C {C} n {n}: gamma {dg:.3e}, w {dw:.3e}")
        assert dg <= 1e-10 and dw <= 1e-10


def test_without_the_model_it_is_beamform():
    """iterations = 0, noise = 0, floor = 0: gamma = a = M; the statistics are summed by another expression"""
    for mix, est in (br.sanity_case(leak=0.6, L=8000)[:2], br.make_case(3, "generic", 3, 5, 3001)):
        got, info = sp.beamform_spatial(mix, est, iterations=0, noise=0.0, floor=0.0, return_info=True)
        err = br.rel_err(got, br.beamform(mix, est), mix)
        print(f"against beamform_restatement.beamform: {err:.3e} of the peak")
        assert err <= 1e-12 and info["gamma"].shape[0] == est.shape[0]


def test_the_posteriors_sum_to_one(sanity):
    info = sanity[4]
    assert info["gamma"].shape[0] == 3                                    # the noise class
    assert float(np.max(np.abs(info["gamma"].sum(axis=0) - 1.0))) <= 1e-12
    _, i0 = sp.beamform_spatial(sanity[0], sanity[1], iterations=2, noise=0.0, return_info=True)
    assert i0["gamma"].shape[0] == 2 and float(np.max(np.abs(i0["gamma"].sum(axis=0) - 1.0))) <= 1e-12


@pytest.mark.parametrize("reg", [0.0, 1e-3])
def test_the_log_likelihood_does_not_decrease(sanity, reg):
    """expectation-maximisation: with mask_reg = 0 (and a loading of 1e-30) a theorem; it also holds at 1e-3 here"""
    mix, est = sanity[:2]
    for kw in (dict(), dict(noise=0.0, floor=0.0), dict(noise=0.3, floor=0.5)):
        _, info = sp.beamform_spatial(mix, est, iterations=10, mask_reg=reg, mask_eps=1e-30 if reg == 0 else 1e-10,
                                      return_info=True, **kw)
        ll = np.array(info["ll"])
        assert len(ll) == 11 and info["failed"] == 0
        steps = np.diff(ll)
        print(f"reg {reg} {kw}: log-likelihood {ll[0]:.6e} -> {ll[-1]:.6e}, smallest step {steps.min():.3e}")
        assert np.all(steps >= -1e-9 * np.abs(ll[1:]))


def test_one_channel_takes_the_priors():
    mix, est = br.make_case(5, "generic", 2, 1, 3001)
    out, info = sp.beamform_spatial(mix, est, iterations=3, return_info=True)
    Z, _, _ = sr._stft(np.concatenate([mix, est]).astype(np.float64), 512, 128, np.float64)
    M = sr._masks(Z[1:], 2, 2, 1e-10, torch.float64).numpy()
    a = sp.priors(M, float(np.float32(0.1)), float(np.float32(0.1)))
    assert np.array_equal(info["gamma"], a) and info["failed"] == 0 and info["ll"] == []
    assert np.all(info["w"] == 1.0)


def test_dead_frames_take_the_prior():
    """a mixture that is silent for a while: the frames inside the gap have p = 0 in every bin"""
    mix, est = br.make_case(7, "generic", 2, 3, 6000)
    mix[:, 2000:4000] = 0.0
    out, info = sp.beamform_spatial(mix, est, iterations=2, return_info=True)
    Z, _, _ = sr._stft(np.concatenate([mix, est]).astype(np.float64), 512, 128, np.float64)
    X = Z[:3].numpy()
    dead = (np.abs(X) ** 2).sum(axis=0) == 0
    assert dead[:, 19:29].all() and not dead[:, :12].any()
    a = sp.priors(sr._masks(Z[3:], 2, 2, 1e-10, torch.float64).numpy(), float(np.float32(0.1)), float(np.float32(0.1)))
    assert np.array_equal(info["gamma"][:, dead], a[:, dead]) and not np.array_equal(info["gamma"], a)
    assert info["failed"] == 0 and np.all(np.isfinite(out))


def test_a_class_with_a_zero_prior_resets_to_the_identity():
    """floor = 0, no noise class, a silent estimate beside a loud one and the smallest float32 eps: in the float32 mode
    (the device's masks) the silent source's mask underflows to zero in every frame.  The definition: log a = -inf,
    gamma = 0, sum gamma = 0, so B_k is the identity (plus its loading) after every M-step -- nothing fails, the class
    stays empty, its statistics are zero and its weights are e_ref."""
    mix, est = br.make_case(9, "generic", 2, 3, 3001)
    est = np.stack([1000.0 * est[0], np.zeros_like(est[1])])
    Z, _, _ = sr._stft(np.concatenate([mix, est]), 512, 128, np.float32)
    M = sr._masks(Z[3:], 2, 2, 1e-45, torch.float32).numpy()
    assert np.all(M[1] == 0) and np.all(M[0] == 1)
    out, info = sp.beamform_spatial(mix, est, ref=1, eps=1e-45, iterations=3, noise=0.0, floor=0.0, dtype=np.float32,
                                    return_info=True)
    assert info["failed"] == 0 and np.all(info["gamma"][1] == 0) and np.all(info["gamma"][0] == 1)
    assert np.all(np.isfinite(out)) and np.all(info["w"][1] == np.array([0, 1, 0]))
    # the M-step itself: an empty class gives the loaded identity
    C = 3
    B = sp.m_step(np.stack([np.ones((4, 9)), np.zeros((4, 9))]), np.ones((2, 4, 9)),
                  np.ones((4, 9, C)) / np.sqrt(C), np.ones((4, 9), dtype=bool), 1e-3, 1e-10)
    assert np.allclose(B[:, 1], (1 + 1e-3 + 1e-10) * np.eye(C), rtol=0, atol=1e-15)


def test_a_failed_pivot_resets_the_bin():
    """a NaN in an estimate: every bin fails its first pivot, is counted once, and falls back to the identity"""
    mix, est = br.make_case(11, "generic", 2, 3, 4001)
    est[1, 2000] = np.nan
    out, info = sp.beamform_spatial(mix, est, ref=1, iterations=2, return_info=True)
    assert info["failed"] == 257 and np.all(np.isfinite(out))
    assert np.all(info["w"] == np.array([0, 1, 0]))


def test_sanity_refinement_recovers_poor_estimates():
    """sanity_case(leak=0.6) at the defaults: every source gains more than 2 dB over the beamformer on the estimates'
    own masks (measured: +8.3 and +5.1 dB).  The table of the README, printed in full."""
    rows = ((0.3, 1, 0.1, 0.1), (0.6, 1, 0.1, 0.1), (0.6, 1, 0.0, 0.0), (0.6, 3, 0.1, 0.1), (0.6, 10, 0.1, 0.1))
    table = {}
    for leak, it, nu, phi in rows:
        mix, est, img = br.sanity_case(leak=leak)
        base = br.beamform(mix, est)
        got = sp.beamform_spatial(mix, est, iterations=it, noise=nu, floor=phi)
        table[leak, it, nu, phi] = ([br.si_sdr(base[i], img[i]) for i in range(2)],
                                    [br.si_sdr(got[i], img[i]) for i in range(2)])
        b, g = table[leak, it, nu, phi]
        print(f"leak {leak} iterations {it} noise {nu} floor {phi}: beamform {b[0]:.2f} / {b[1]:.2f} dB, "
              f"with refinement {g[0]:.2f} / {g[1]:.2f} dB")
    base, got = table[0.6, 1, 0.1, 0.1]
    assert native.SPATIAL_DEFAULTS == dict(iterations=1, noise=0.1, floor=0.1, reg=1e-3, eps=1e-10)
    assert all(g > b + 2.0 for g, b in zip(got, base))
    assert base == pytest.approx([11.89, 9.91], abs=0.05) and got == pytest.approx([20.18, 14.98], abs=0.05)


def test_float32_mode_is_close_to_float64(sanity):
    mix, est, _, out, info = sanity
    cpu, ic = sp.beamform_spatial(mix, est, iterations=3, dtype=np.float32, return_info=True)
    dg = float(np.max(np.abs(ic["gamma"] - info["gamma"])))
    dw = float(np.max(np.abs(ic["w"] - info["w"])) / np.max(np.abs(info["w"])))
    print(f"float32 transforms against float64: gamma {dg:.3e}, w {dw:.3e}, out {br.rel_err(cpu, out, mix):.3e}")
    assert 0 < dg <= 1e-3 and 0 < dw <= 1e-4 and 0 < br.rel_err(cpu, out, mix) <= 1e-5


# ------------------------------------------------------------------ the host side of the keyword
def test_spatial_options():
    assert native.spatial_options(None) is None
    assert native.spatial_options(True) == native.SPATIAL_DEFAULTS
    assert native.spatial_options({"iterations": 3, "noise": 0.0}) == dict(iterations=3, noise=0.0, floor=0.1, reg=1e-3,
                                                                           eps=1e-10)
    for bad, msg in ((False, "spatial must be None, True or a dict"), ("cacgmm", "spatial must be"), (2, "spatial must be"),
                     ({"taps": 3}, r"spatial: unknown keys \['taps'\]")):
        with pytest.raises(ValueError, match=msg):
            native.spatial_options(bad)
    beam = native.beamform_options({"ref": 2, "n_fft": 1024, "hop": 256})
    kw = native.spatial_beamform_keywords(beam, native.spatial_options({"iterations": 4, "reg": 1e-2}))
    assert kw == dict(ref=2, n_fft=1024, hop=256, power=2, eps=1e-10, reg=1e-3, iterations=4, noise=0.1, floor=0.1,
                      mask_reg=1e-2, mask_eps=1e-10)
    assert native.spatial_beamform_keywords(beam, None) == beam
    native.check_spatial((1, 4, 3000), (1, 2, 3000), **kw)
    with pytest.raises(ValueError, match="spatial= refines the masks of the beamformer: it needs beamform="):
        native.spatial_beamform_keywords(None, native.SPATIAL_DEFAULTS)
    with pytest.raises(ValueError, match="spatial= does not go with postfilter='mask'"):
        native.spatial_beamform_keywords(native.beamform_options({"postfilter": "mask"}), native.SPATIAL_DEFAULTS)


def test_the_entry_points_refuse_by_name():
    spat, beam = native.spatial_options(True), native.beamform_options(True)
    refuse = LatentDiffSep._spatial_refusals
    assert refuse(spat, beam) == native.spatial_beamform_keywords(beam, spat)
    for kw, msg in ((dict(stems="mask"), "spatial= does not go with stems="),
                    (dict(latent=True), "spatial= refines the masks of waveforms: with latent=True"),
                    (dict(intermediate=True), "spatial= does not go with intermediate")):
        with pytest.raises(ValueError, match=msg):
            refuse(spat, beam, **kw)
    with pytest.raises(ValueError, match="spatial= refines the masks of the beamformer: it needs beamform="):
        refuse(spat, None)
    with pytest.raises(ValueError, match="spatial= does not go with postfilter='mask'"):
        refuse(spat, native.beamform_options({"postfilter": "mask"}))


def test_check_spatial():
    good = native.check_spatial((3, 4, 600), (3, 2, 600), [600, 300, 257], [4, 2, 3], ref=1, iterations=0, noise=0)
    assert good == ((3, 4, 2, 600), [600, 300, 257], [4, 2, 3], 1, 512, 128, 2, 1e-10, 1e-3, 0, 0.0, 0.1, 1e-3, 1e-10, 0)
    need = native.spatial_item_bytes(512, 128, 600, 2, 2)
    assert need == 257 * (8 * 3 * 2 * 3 + 6 * (8 * 2 + 4 * 2) + 4)
    assert native.check_spatial((1, 2, 600), (1, 2, 600), workspace_budget=need)[-1] == need
    one = ((1, 2, 600), (1, 2, 600))
    for args, kw, msg in (
            (((2, 600), (2, 2, 600)), {}, r"beamform_spatial: mix must be \[B, C, L\] and est \[B, n, L\]"),
            (((1, 9, 600), (1, 2, 600)), {}, r"beamform_spatial: C = 9 outside \[1, 8\]"),
            (((1, 2, 600), (1, 5, 600)), {}, r"beamform_spatial: n = 5 outside \[1, 4\]"),
            (one, dict(n_fft=384), "beamform_spatial: n_fft = 384 is not a power of two"),
            (one, dict(power=3), "beamform_spatial: power = 3 is not 1 or 2"),
            (one, dict(reg=-1e-3), "beamform_spatial: reg = -0.001 is not a finite number >= 0"),
            (one, dict(ref=2), r"beamform_spatial: ref = 2 outside \[0, 2\): item 0 has 2 channels"),
            (one, dict(iterations=17), r"beamform_spatial: iterations = 17 outside \[0, 16\]"),
            (one, dict(iterations=-1), r"beamform_spatial: iterations = -1 outside \[0, 16\]"),
            (one, dict(iterations=1.5), r"beamform_spatial: iterations = 1.5 outside \[0, 16\]"),
            (one, dict(iterations=True), r"beamform_spatial: iterations = True outside \[0, 16\]"),
            (one, dict(noise=0.91), r"beamform_spatial: noise = 0.91 outside \[0, 0.9\]"),
            (one, dict(noise=-0.1), r"beamform_spatial: noise = -0.1 outside \[0, 0.9\]"),
            (one, dict(noise=float("nan")), r"beamform_spatial: noise = nan outside \[0, 0.9\]"),
            (one, dict(floor=1.1), r"beamform_spatial: floor = 1.1 outside \[0, 1\]"),
            (one, dict(floor=-0.5), r"beamform_spatial: floor = -0.5 outside \[0, 1\]"),
            (one, dict(mask_reg=-1.0), "beamform_spatial: mask_reg = -1.0 is not a finite number >= 0"),
            (one, dict(mask_eps=0.0), "beamform_spatial: mask_eps = 0.0 is not a finite positive number"),
            (one, dict(workspace_budget=-1), "beamform_spatial: workspace_budget = -1 < 0"),
            (one, dict(workspace_budget=need - 1),
             rf"beamform_spatial: workspace_budget = {need - 1} bytes is smaller than one item \({need} bytes at C = 2")):
        with pytest.raises(ValueError, match=msg):
            native.check_spatial(*args, **kw)


def test_command_line_flags():
    p = separate.build_parser()
    base = ["in", "out", "--config", "c.json"]
    a = p.parse_args(base)
    assert a.spatial is False and separate.spatial_of(a) is None
    a = p.parse_args(base + ["--beamform", "--spatial"])
    assert separate.spatial_of(a) == dict(iterations=1, noise=0.1, floor=0.1, reg=1e-3)
    assert native.spatial_options(separate.spatial_of(a)) == native.SPATIAL_DEFAULTS
    assert separate.beamform_of(a) == dict(ref=0, n_fft=512, hop=128, reg=1e-3, postfilter=None)
    a = p.parse_args(base + ["--spatial", "--spatial-iterations", "3", "--spatial-noise", "0", "--spatial-floor", "0.25",
                             "--spatial-reg", "0.01"])
    assert separate.spatial_of(a) == dict(iterations=3, noise=0.0, floor=0.25, reg=0.01)
    assert separate.beamform_of(a) is None
    for bad in (["--spatial-iterations", "x"], ["--spatial-noise", "much"]):
        with pytest.raises(SystemExit):
            p.parse_args(base + bad)
