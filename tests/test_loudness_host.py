"""Host-side checks of the loudness step (no GPU): the K-weighting coefficients the library forms against the
standard's table, the float64 restatement (tests/loudness_restatement.py) against published readings, the gain rule,
the option parsing and every refusal."""
import math

import numpy as np
import pytest

from ditsep_amd import native
from tests import loudness_restatement as lr


def test_kweight_coeffs_match_the_standards_table_at_48k():
    c = native.kweight_coeffs(48000)
    want = np.array(lr.TABLE_48K["shelf_b"] + lr.TABLE_48K["shelf_a"] + (1.0, -2.0, 1.0) + lr.TABLE_48K["highpass_a"])
    assert np.abs(c - want).max() <= 1e-12, np.abs(c - want).max()


@pytest.mark.parametrize("fs", [8000, 11025, 16000, 22050, 44100, 48000, 96000, 192000])
def test_kweight_coeffs_match_the_restatement(fs):
    assert np.abs(native.kweight_coeffs(fs) - lr.coeffs(fs)).max() <= 1e-14


@pytest.mark.parametrize("fs", [7999, 192001, 0, -48000, 44100.5, True])
def test_kweight_coeffs_refuse_a_rate_outside_the_range(fs):
    with pytest.raises(ValueError, match="kweight_coeffs"):
        native.kweight_coeffs(fs)


def test_block_step_is_libebur128s():
    assert [lr.block_step(fs) for fs in (8000, 11025, 22050, 44100, 48000)] == [800, 1103, 2205, 4410, 4800]


def test_full_scale_997_hz_sine_reads_minus_3_01():
    m = lr.measure(lr.sine(997.0, 0.0, 20.0, 48000), 48000, true_peak=False)
    print(f"0 dBFS 997 Hz mono, 48 kHz: {m['loudness']:.4f} LKFS")
    assert abs(m["loudness"] - (-3.01)) <= 0.005
    assert m["blocks"] == (20 * 48000 - 4 * 4800) // 4800 + 1 == m["gated_blocks"]


@pytest.mark.parametrize("fs", [8000, 11025, 16000, 22050, 44100])
def test_the_sine_reads_the_same_at_other_rates(fs):
    m = lr.measure(lr.sine(997.0, 0.0, 20.0, fs), fs, true_peak=False)
    print(f"0 dBFS 997 Hz mono, {fs} Hz: {m['loudness']:.4f} LKFS")
    assert abs(m["loudness"] - (-3.01)) <= 0.05


def _tone(parts, fs=48000):
    return np.concatenate([lr.sine(1000.0, db, sec, fs, channels=2) for db, sec in parts], axis=1)


EBU_3341 = {
    "case1": ([(-23.0, 20.0)], -23.0),
    "case3": ([(-36.0, 10.0), (-23.0, 60.0), (-36.0, 10.0)], -23.0),
    "case4": ([(-72.0, 10.0), (-36.0, 10.0), (-23.0, 60.0), (-36.0, 10.0), (-72.0, 10.0)], -23.0),
    "case5": ([(-26.0, 20.0), (-20.0, 20.1), (-26.0, 20.0)], -23.0),
}


@pytest.mark.parametrize("case", sorted(EBU_3341))
def test_ebu_tech_3341_integrated_loudness(case):
    parts, want = EBU_3341[case]
    m = lr.measure(_tone(parts), 48000, true_peak=False)
    print(f"EBU Tech 3341 {case}: {m['loudness']:.4f} LUFS ({m['gated_blocks']} of {m['blocks']} blocks)")
    assert abs(m["loudness"] - want) <= 0.1


def test_ebu_cases_3_and_4_read_the_same():
    a = lr.measure(_tone(EBU_3341["case3"][0]), 48000, true_peak=False)["loudness"]
    b = lr.measure(_tone(EBU_3341["case4"][0]), 48000, true_peak=False)["loudness"]
    assert abs(a - b) <= 1e-3


def test_too_short_and_silent_items_read_minus_infinity():
    rng = np.random.default_rng(0)
    assert lr.measure(rng.standard_normal((1, 3199)), 8000, true_peak=False)["loudness"] == -math.inf
    m = lr.measure(np.zeros((2, 8000)), 8000)
    assert m["loudness"] == -math.inf and m["blocks"] == 7 and m["gated_blocks"] == 0 and m["true_peak"] == 0.0


def test_true_peak_readings_on_quarter_rate_sines_are_recorded():
    """fs / 4 sines whose samples miss the crest (EBU Tech 3341 cases 15 to 19 use such signals).  The interpolator is
    the project's resampler, not the standard's 48-tap table, and the tones start abruptly: the readings are printed,
    and only that they are not below the sample peak and within 0.5 dB of the crest is asserted -- conformance to EBU's
    +0.2 / -0.4 dB window is not claimed."""
    fs = 48000
    t = np.arange(fs // 2, dtype=np.float64)
    for amp, phase in ((0.5, 0.0), (0.5, 45.0), (0.5, 60.0), (0.5, 67.0), (1.41, 45.0)):
        x = amp * np.sin(2.0 * np.pi * t / 4.0 + np.deg2rad(phase))
        m = lr.measure(x[None], fs)
        over = 20.0 * math.log10(m["true_peak"] / amp)
        print(f"fs/4 sine, amplitude {amp}, phase {phase:4.1f} deg: sample peak {20 * math.log10(m['sample_peak']):+.3f} "
              f"dBFS, true peak {20 * math.log10(m['true_peak']):+.3f} dBTP ({over:+.3f} dB against the crest)")
        assert m["true_peak"] >= m["sample_peak"] * (1.0 - 1e-6) and abs(over) <= 0.5


# ---------------------------------------------------------------------------------------------- the gain rule
def test_gain_rule_ceiling_slack_and_binding():
    g = native.loudness_gain([-30.0, -30.0], [0.1, 0.9], None, -23.0, -1.0)
    assert g["gain_db"][0] == 7.0 and not g["limited"][0]                               # 0.1 -> -20 dBTP: 19 dB of room
    want = -1.0 - 20.0 * math.log10(0.9)
    assert g["gain_db"][1] == want and g["limited"][1] and want < 7.0
    assert g["gain"][1] == float(np.float32(10.0 ** (want / 20.0)))
    assert g["gain"][0] == float(np.float32(10.0 ** (7.0 / 20.0)))
    for r in range(2):
        assert g["gain_db"][r] == lr.gain_db(-30.0, [0.1, 0.9][r], -23.0, -1.0)
    free = native.loudness_gain([-30.0], [0.9], None, -23.0, None)
    assert free["gain_db"] == [7.0] and free["limited"] == [False]


def test_gain_rule_minus_infinity_and_nan_sources_stay_at_0_db():
    g = native.loudness_gain([-math.inf, -20.0, math.nan, -20.0], [0.0, 0.5, 0.5, math.nan], None, -23.0, -1.0)
    assert g["gain_db"] == [0.0, -3.0, 0.0, 0.0] and g["gain"][0] == 1.0 and g["gain"][2] == 1.0
    assert g["silent"] == [0] and g["nonfinite"] == [2, 3]


def test_gain_rule_linked_group_shares_the_smallest_room():
    # two items of two stems, each item one gain from its mixture; the loudest stem's peak sets the ceiling
    g = native.loudness_gain([-30.0, -30.0, -25.0, -25.0], [0.2, 0.95, 0.1, 0.2], [0, 0, 1, 1], -23.0, -1.0)
    want = -1.0 - 20.0 * math.log10(0.95)
    assert g["gain_db"][:2] == [want, want] and g["limited"][:2] == [True, True]
    assert g["gain_db"][2:] == [2.0, 2.0] and g["limited"][2:] == [False, False]
    with pytest.raises(ValueError, match="do not share one gain source"):
        native.loudness_gain([-30.0, -29.0], [0.2, 0.2], [0, 0], -23.0, -1.0)
    with pytest.raises(ValueError, match="group labels"):
        native.loudness_gain([-30.0, -29.0], [0.2, 0.2], [0], -23.0, -1.0)
    with pytest.raises(ValueError, match="sources but"):
        native.loudness_gain([-30.0], [0.2, 0.2], None, -23.0, -1.0)


def test_silent_rows_have_no_ceiling():
    assert native.loudness_gain([-30.0], [0.0], None, -23.0, -1.0)["gain_db"] == [7.0]


# ---------------------------------------------------------------------------------------------- options and refusals
def test_loudness_options():
    assert native.loudness_options(None) is None
    assert native.loudness_options(True) == native.LOUDNESS_DEFAULTS == dict(target=-23.0, peak=-1.0, link="mixture")
    assert native.loudness_options(-16) == dict(target=-16.0, peak=-1.0, link="mixture")
    assert native.loudness_options(-14.5)["target"] == -14.5
    assert native.loudness_options({"peak": None, "link": "stem"}) == dict(target=-23.0, peak=None, link="stem")
    assert native.loudness_options(True) is not native.LOUDNESS_DEFAULTS


@pytest.mark.parametrize("spec,msg", [
    (False, "loudness must be None, True"), ("loud", "loudness must be None, True"), ([-23.0], "loudness must be"),
    ({"lufs": -23.0}, "unknown keys"), ({"link": "item"}, "link must be one of"),
    ({"target": None}, "target = None"), ({"target": math.nan}, "not a finite number"),
    ({"target": "-23"}, "not a finite number"), ({"peak": math.inf}, "peak = inf"), ({"peak": True}, "peak = True"),
    (math.inf, "target = inf"),
])
def test_loudness_options_refusals(spec, msg):
    with pytest.raises(ValueError, match=msg):
        native.loudness_options(spec)


def test_check_loudness():
    assert native.check_loudness((5,), 8000) == ((1, 1, 5), [8000], None, None)
    assert native.check_loudness((2, 7), 44100) == ((1, 2, 7), [44100], None, None)
    assert native.check_loudness((3, 2, 9), [8000, 192000, 11025], [9, 1, 4], [1, 2, 2]) == \
        ((3, 2, 9), [8000, 192000, 11025], [9, 1, 4], [1, 2, 2])


@pytest.mark.parametrize("args,msg", [
    (((2, 2, 2, 2), 8000), r"x must be \[L\]"), (((0, 1, 5), 8000), "B = 0"), (((65536, 1, 5), 8000), "B = 65536"),
    (((1, 3, 5), 8000), "C = 3 outside"), (((1, 0, 5), 8000), "C = 0 outside"), (((1, 1, 0), 8000), "L = 0 outside"),
    (((1, 1, 2 ** 30 + 1), 8000), "L = 1073741825 outside"), (((2, 1, 5), [8000]), "one sample rate per item"),
    (((1, 1, 5), 7999), "rates\\[0\\] = 7999"), (((1, 1, 5), [192001]), "rates\\[0\\] = 192001"),
    (((1, 1, 5), [44100.5]), "rates\\[0\\] = 44100.5"), (((2, 1, 5), 8000, [5]), "lens"),
    (((2, 1, 5), 8000, [5, 6]), "lens"), (((2, 1, 5), 8000, [5, 0]), "lens"),
    (((2, 2, 5), 8000, None, [1]), "one channel count per item"), (((2, 2, 5), 8000, None, [1, 3]), "channels = 3"),
    (((2, 2, 5), 8000, None, [0, 1]), "channels = 0"),
])
def test_check_loudness_refusals(args, msg):
    with pytest.raises(ValueError, match=msg):
        native.check_loudness(*args)


def test_cli_flags_reach_the_options():
    from ditsep_amd import separate as cli

    base = ["in", "out", "--config", "c.json"]
    assert cli.loudness_of(cli.build_parser().parse_args(base)) is None
    a = cli.build_parser().parse_args(base + ["--loudness", "-16"])
    assert native.loudness_options(cli.loudness_of(a)) == dict(target=-16.0, peak=-1.0, link="mixture")
    a = cli.build_parser().parse_args(base + ["--loudness", "-23", "--true-peak", "-2", "--loudness-link", "stem"])
    assert native.loudness_options(cli.loudness_of(a)) == dict(target=-23.0, peak=-2.0, link="stem")
    with pytest.raises(SystemExit):
        cli.build_parser().parse_args(base + ["--loudness", "-23", "--loudness-link", "item"])
