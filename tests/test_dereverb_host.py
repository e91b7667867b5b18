"""The restatement of dsn_dereverb (tests/dereverb_restatement.py) and the host side of the `dereverb` keyword, on the
CPU: the properties the definition promises, option parsing, every refusal of check_dereverb by name, the workspace
formula, the command-line flags and the keyword's own refusals."""
import types

import numpy as np
import pytest

from ditsep_amd import native, separate
from ditsep_amd.latent import LatentDiffSep
from tests import dereverb_restatement as dr


def test_the_two_solvers_agree():
    """numpy.linalg.solve against the explicit Cholesky, on the shapes of tests/test_gpu_dereverb.py.  Measured: the
    filters at most 3.4e-11 of the largest entry apart, the outputs at most 2.1e-12 of the peak, at cond(A) <= 8.0e5."""
    worst = [0.0, 0.0, 0.0]
    for n_fft, hop, C, K, D, L in ((64, 16, 2, 4, 1, 6000), (512, 128, 8, 10, 3, 4000), (2048, 512, 3, 2, 2, 3000)):
        mix, _ = dr.reverb_case(n_fft + C + K, C, L)
        kw = dict(taps=K, delay=D, n_fft=n_fft, hop=hop, return_info=True)
        a, ia = dr.dereverb(mix, solver="cholesky", return_cond=True, **kw)
        b, ib = dr.dereverb(mix, solver="solve", **kw)
        assert ia["fail"] == ib["fail"] == 0 and ia["cond"] <= 1e7
        top = np.abs(ia["G"]).max()
        worst = [max(worst[0], np.abs(ia["G"] - ib["G"]).max() / top), max(worst[1], dr.rel_err(a, b, mix)),
                 max(worst[2], ia["cond"])]
    print(f"solve against cholesky: G {worst[0]:.2e}, output {worst[1]:.2e}, worst cond(A) {worst[2]:.2e}")
    assert worst[0] <= 1e-7 and worst[1] <= 1e-9      # cond(A) times the unit roundoff, with room


def test_short_and_silent_items_are_the_round_trip():
    g = np.random.default_rng(1)
    x = 0.3 * g.standard_normal((3, 700))             # 7 frames
    for dtype in (np.float64, np.float32):
        out, info = dr.dereverb(x, taps=4, delay=8, dtype=dtype, return_info=True)
        assert np.array_equal(out, dr.round_trip(x, dtype=dtype)) and not info["G"].any() and info["fail"] == 0
    out, info = dr.dereverb(np.zeros((2, 3000)), return_info=True)
    assert not out.any() and not info["G"].any() and info["fail"] == 0


def test_a_power_of_two_scale_commutes():
    mix, _ = dr.reverb_case(2, 3, 5000)
    a, ia = dr.dereverb(mix, taps=5, return_info=True)
    b, ib = dr.dereverb(8.0 * mix, taps=5, return_info=True)
    assert np.array_equal(ia["G"], ib["G"]) and np.array_equal(b, 8.0 * a) and ia["G"].any()
    a32 = dr.dereverb(mix, taps=5, dtype=np.float32)
    assert np.array_equal(dr.dereverb(0.25 * mix, taps=5, dtype=np.float32), np.float32(0.25) * a32)


def test_a_huge_loading_tends_to_the_input():
    mix, _ = dr.reverb_case(3, 2, 5000)
    far = dr.rel_err(dr.dereverb(mix, iterations=1), dr.round_trip(mix), mix)
    errs = [dr.rel_err(dr.dereverb(mix, iterations=1, reg=reg), dr.round_trip(mix), mix) for reg in (1e2, 1e4, 1e6)]
    print("distance from the input at reg = 1e-4, 1e2, 1e4, 1e6:", far, errs)
    assert far > 1e-2 and errs[0] < far and errs[0] > errs[1] > errs[2] and errs[2] < 1e-5


def test_a_failed_pivot_is_counted_and_passes_through():
    mix, _ = dr.reverb_case(4, 2, 3000)
    bad = mix.copy()
    bad[0, 1000] = np.nan
    with np.errstate(invalid="ignore"):
        _, info = dr.dereverb(bad, taps=4, return_info=True)
    assert info["fail"] == 257 and not info["G"].any()


def test_sanity_on_synthetic_reverberation():
    """Burst noise through exponentially decaying random 0.3 s responses, sensor noise at 1e-3, 4 channels, 2 s, the
    defaults: channel 0's SI-SDR against the source convolved with the first 20 ms of its response rises from 2.05 dB to
    13.73 dB (+11.68 dB).  A sanity figure on synthetic data, not a quality claim."""
    mix, early = dr.reverb_case(0, 4, 32000)
    out, info = dr.dereverb(mix, return_info=True)
    before, after = dr.si_sdr(mix[0], early), dr.si_sdr(out[0], early)
    print(f"SI-SDR of channel 0 against the early part: {before:.2f} dB -> {after:.2f} dB")
    assert info["fail"] == 0 and after - before > 3.0


def test_dereverb_options():
    assert native.dereverb_options(None) is None
    assert native.DEREVERB_DEFAULTS == dict(taps=10, delay=3, iterations=3, n_fft=512, hop=128, reg=1e-4, eps=1e-10)
    assert native.DEREVERB_DEFAULTS == dr.DEFAULTS
    assert native.dereverb_options(True) == native.DEREVERB_DEFAULTS
    assert native.dereverb_options(True) is not native.DEREVERB_DEFAULTS
    assert native.dereverb_options({"taps": 5, "n_fft": 1024, "hop": 256}) == dict(
        taps=5, delay=3, iterations=3, n_fft=1024, hop=256, reg=1e-4, eps=1e-10)
    for bad, msg in ((False, "dereverb must be None, True or a dict"), ("wpe", "dereverb must be"),
                     (3, "dereverb must be"), ({"window": 3}, r"dereverb: unknown keys \['window'\]")):
        with pytest.raises(ValueError, match=msg):
            native.dereverb_options(bad)


def test_check_dereverb():
    good = native.check_dereverb((3, 4, 600), [600, 300, 257], [4, 2, 3], taps=5, delay=2, iterations=1)
    assert good == ((3, 4, 600), [600, 300, 257], [4, 2, 3], 5, 2, 1, 512, 128, 1e-4, 1e-10, 0)
    assert native.check_dereverb((1, 8, 600))[:3] == ((1, 8, 600), None, None)
    assert native.check_dereverb((1, 5, 600), taps=16)[3] == 16
    need = native.dereverb_item_bytes(512, 128, 600, 2, 10)
    assert need == 257 * (8 * (2 * 20 * 2 + 6 + 2 * 2 * 6) + 4)          # 600 samples: 1 + 5 frames
    assert native.dereverb_item_bytes(64, 16, 33, 1, 1) == 33 * (8 * (2 + 4 + 2 * 4) + 4)
    assert native.check_dereverb((1, 2, 600), workspace_budget=need)[-1] == need
    assert native.check_dereverb((1, 2, 600), workspace_budget=None)[-1] == 0
    for shape, kw, msg in (
            ((2, 600), {}, r"dereverb: mix must be \[B, C, L\]"),
            ((1, 9, 600), {}, r"dereverb: C = 9 outside \[1, 8\]"),
            ((1, 0, 600), {}, r"dereverb: C = 0 outside \[1, 8\]"),
            ((1, 2, 600), dict(taps=0), r"dereverb: taps = 0 outside \[1, 16\]"),
            ((1, 2, 600), dict(taps=17), r"dereverb: taps = 17 outside \[1, 16\]"),
            ((1, 2, 600), dict(taps=2.5), r"dereverb: taps = 2.5 outside \[1, 16\]"),
            ((1, 2, 600), dict(delay=0), r"dereverb: delay = 0 outside \[1, 8\]"),
            ((1, 2, 600), dict(delay=9), r"dereverb: delay = 9 outside \[1, 8\]"),
            ((1, 2, 600), dict(iterations=0), r"dereverb: iterations = 0 outside \[1, 8\]"),
            ((1, 2, 600), dict(iterations=9), r"dereverb: iterations = 9 outside \[1, 8\]"),
            ((1, 2, 600), dict(iterations=True), r"dereverb: iterations = True outside \[1, 8\]"),
            ((1, 8, 600), dict(taps=11), r"dereverb: C taps = 8 x 11 = 88 unknowns per bin, more than 80"),
            ((1, 2, 600), dict(n_fft=384), "dereverb: n_fft = 384 is not a power of two"),
            ((1, 2, 600), dict(hop=512), "dereverb: n_fft / hop = 512 / 512 is not one of 2, 4, 8"),
            ((1, 2, 600), dict(eps=0.0), "dereverb: eps = 0.0 is not a finite positive number"),
            ((1, 2, 600), dict(eps=float("inf")), "dereverb: eps = inf is not a finite positive number"),
            ((1, 2, 600), dict(reg=-1e-3), "dereverb: reg = -0.001 is not a finite number >= 0"),
            ((1, 2, 600), dict(reg=float("nan")), "dereverb: reg = nan is not a finite number"),
            ((1, 2, 600), dict(lens=[256]), r"dereverb: item 0 has 256 samples, outside \[n_fft / 2 \+ 1 = 257"),
            ((1, 2, 256), {}, r"dereverb: item 0 has 256 samples, outside \[n_fft / 2 \+ 1 = 257"),
            ((2, 2, 600), dict(channels=[2]), "dereverb: channels must hold one channel count per item"),
            ((2, 2, 600), dict(channels=[2, 3]), r"dereverb: item 1 has channels = 3, outside \[1, C = 2\]"),
            ((2, 2, 600), dict(channels=[0, 2]), r"dereverb: item 0 has channels = 0, outside \[1, C = 2\]"),
            ((1, 2, 600), dict(workspace_budget=-1), "dereverb: workspace_budget = -1 < 0"),
            ((1, 2, 600), dict(workspace_budget=need - 1),
             rf"dereverb: workspace_budget = {need - 1} bytes is smaller than one item \({need} bytes at C = 2, taps = 10")):
        with pytest.raises(ValueError, match=msg):
            native.check_dereverb(shape, **kw)


def test_command_line_flags():
    p = separate.build_parser()
    base = ["in", "out", "--config", "c.json"]
    a = p.parse_args(base)
    assert a.dereverb is False and separate.dereverb_of(a) is None
    a = p.parse_args(base + ["--dereverb"])
    assert separate.dereverb_of(a) == dict(taps=10, delay=3, iterations=3, n_fft=512, hop=128, reg=1e-4)
    assert native.dereverb_options(separate.dereverb_of(a)) == native.DEREVERB_DEFAULTS
    a = p.parse_args(base + ["--dereverb", "--dereverb-taps", "6", "--dereverb-delay", "2", "--dereverb-iterations", "5",
                             "--dereverb-nfft", "1024", "--dereverb-hop", "256", "--dereverb-reg", "0.001"])
    assert separate.dereverb_of(a) == dict(taps=6, delay=2, iterations=5, n_fft=1024, hop=256, reg=0.001)
    assert separate.beamform_of(a) is None and separate.stems_of(a) is None
    for bad in (["--dereverb-taps", "x"], ["--dereverb-reg", "small"]):
        with pytest.raises(SystemExit):
            p.parse_args(base + bad)


def test_the_keyword_refusals():
    """LatentDiffSep._dereverb_refusals, which every entry point calls before any device work"""
    model = types.SimpleNamespace(_model_rate=lambda what: 16000)
    refuse = lambda *a, **kw: LatentDiffSep._dereverb_refusals(model, native.dereverb_options(True), *a, **kw)
    refuse([(1, 257), (8, 4000)])
    refuse([(2, 514)], [32000])
    with pytest.raises(ValueError, match="dereverb= filters waveforms: with latent=True"):
        refuse([], latent=True)
    with pytest.raises(ValueError, match="dereverb= does not go with intermediate"):
        refuse([(1, 4000)], intermediate=True)
    with pytest.raises(ValueError, match=r"dereverb: item 1 has 9 channels, outside \[1, 8\]"):
        refuse([(2, 4000), (9, 4000)])
    with pytest.raises(ValueError, match=r"dereverb: item 0 has 256 samples at the model's rate; dereverb= needs at "
                                         r"least n_fft / 2 \+ 1 = 257"):
        refuse([(2, 256)])
    with pytest.raises(ValueError, match=r"dereverb: item 1 has 250 samples at the model's rate"):
        refuse([(2, 4000), (2, 500)], [16000, 32000])
