"""The host side of dsn_activity and dsn_activity_gate: the options, shorthands and refusals of the `activity` keyword,
the seconds -> frames conversion, the frame and sample map against a brute-force labelling, the run rules of the
restatement (tests/activity_restatement.py, both forms) on hand-written rows, and the synthetic sanity case the README
reports."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

from ditsep_amd import files, native, separate
from ditsep_amd.latent import LatentDiffSep
from tests import activity_restatement as ar
from tests import beamform_restatement as br


# ------------------------------------------------------------------ options
def test_activity_options():
    d = native.ACTIVITY_DEFAULTS
    assert d == dict(gate=False, n_fft=512, hop=128, band=(100.0, 4000.0), smooth=0.04, range_db=40.0, dominance_db=6.0,
                     hysteresis_db=3.0, min_on=0.1, min_off=0.1, pad=0.0, fade_ms=5.0)
    assert native.activity_options(None) is None
    assert native.activity_options(True) == d
    assert native.activity_options("gate") == dict(d, gate=True)
    assert native.activity_options({"gate": True, "band": [300, 3400], "pad": 1}) == dict(d, gate=True,
                                                                                          band=(300.0, 3400.0), pad=1.0)
    for bad, msg in ((False, "activity must be None, True, 'gate' or a dict"), ("vad", "activity must be"),
                     ({"frames": 3}, r"activity: unknown keys \['frames'\]"),
                     ({"gate": 1}, "activity: gate = 1 is not True or False"),
                     ({"hop": 128.0}, "activity: hop = 128.0 is not an integer"),
                     ({"band": 4000.0}, "activity: band = 4000.0 is not a pair"),
                     ({"band": (4000.0, 100.0)}, "the high edge is below the low edge"),
                     ({"band": (-1.0, 100.0)}, r"activity: band\[0\] = -1.0 < 0.0"),
                     ({"range_db": -1}, "activity: range_db = -1 < 0.0"),
                     ({"dominance_db": float("nan")}, "activity: dominance_db = nan is not a finite number"),
                     ({"hysteresis_db": "3"}, "activity: hysteresis_db = '3' is not a finite number"),
                     ({"smooth": -0.1}, "activity: smooth = -0.1 < 0.0"),
                     ({"min_on": 0}, "activity: min_on = 0.0 s is not positive"),
                     ({"min_off": -1}, "activity: min_off = -1 < 0.0"),
                     ({"pad": True}, "activity: pad = True is not a finite number"),
                     ({"fade_ms": float("inf")}, "activity: fade_ms = inf is not a finite number")):
        with pytest.raises(ValueError, match=msg):
            native.activity_options(bad)


def test_seconds_to_frames():
    d = native.ACTIVITY_DEFAULTS
    assert native.activity_frames(d, 16000) == dict(min_on=13, min_off=13, pad=0, half_width=2, fade=80)   # 12.5 -> 13
    assert native.activity_frames(dict(d, hop=256), 16000) == dict(min_on=6, min_off=6, pad=0, half_width=1, fade=80)
    assert native.activity_frames(dict(d, min_on=1e-6, pad=0.004, smooth=0.0, fade_ms=0.0), 8000) == dict(
        min_on=1, min_off=6, pad=0, half_width=0, fade=0)                                  # pad 0.25 frames -> 0
    assert native.activity_frames(dict(d, pad=0.05, smooth=0.1), 44100)["pad"] == 17        # 17.2
    assert native.activity_frames(dict(d, smooth=0.1), 44100)["half_width"] == 17           # 34.45 -> 34 -> 17
    kw = native.activity_keywords(d, 16000)
    assert kw == dict(fs=16000, n_fft=512, hop=128, band=(100.0, 4000.0), half_width=2, range_db=40.0, dominance_db=6.0,
                      hysteresis_db=3.0, min_on=13, min_off=13, pad=0)
    assert set(kw) == set(inspect.signature(native.Engine.activity).parameters) - {"self", "est", "lens"}
    for k, v in kw.items():
        assert inspect.signature(native.Engine.activity).parameters[k].default == v, k
    assert inspect.signature(native.Engine.activity_gate).parameters["fade"].default == 80
    assert native.activity_band((100.0, 4000.0), 16000, 512) == (4, 128) == ar.band_bins((100.0, 4000.0), 16000, 512)
    assert native.activity_band((0.0, 8000.0), 16000, 64) == (0, 32)
    assert native.activity_band((0.0, 1e6), 16000, 64) == (0, 32)
    assert native.activity_band((1250.0, 1250.0), 16000, 64) == (5, 5)
    assert native.activity_constants(40.0, 6.0, 3.0) == ar.constants(40.0, 6.0, 3.0)
    assert native.activity_constants(40.0, 6.0, 3.0)[0] == 1e-4
    for fade in (0, 1, 80, 4096):
        r = native.activity_ramp(fade)
        assert r.dtype == np.float32 and r.shape == (fade,) and np.array_equal(r, ar.ramp(fade))
        assert np.all(np.diff(r) < 0) and np.all((r > 0) & (r < 1))
    with pytest.raises(ValueError, match=r"activity_gate: fade = 4097 samples outside \[0, 4096\]"):
        native.activity_ramp(4097)


def test_check_activity():
    good = native.check_activity((3, 2, 600), [600, 300, 257])
    assert good == ((3, 2, 600), [600, 300, 257], 512, 128, (4, 128), ar.constants(), 6)
    one = (1, 2, 600)
    for shape, kw, msg in (
            ((2, 600), {}, r"activity: est must be \[B, n, L\]"),
            ((1, 5, 600), {}, r"activity: n = 5 outside \[1, 4\]"),
            (one, dict(n_fft=384), "activity: n_fft = 384 is not a power of two"),
            (one, dict(hop=512), "activity: n_fft / hop = 512 / 512 is not one of 2, 4, 8"),
            (one, dict(lens=[256]), r"activity: item 0 has 256 samples, outside \[n_fft / 2 \+ 1 = 257, L = 600\]"),
            (one, dict(fs=0), "activity: fs = 0 is not a positive integer"),
            (one, dict(fs=16000.5), "activity: fs = 16000.5 is not a positive integer"),
            (one, dict(band=(10.0, 20.0)), r"activity: the band \(10.0, 20.0\) Hz holds no bin of an n_fft = 512 "
                                           r"transform at 16000 Hz \(bins 1 .. 0\)"),
            (one, dict(band=(9000.0, 9500.0)), "holds no bin"),
            (one, dict(band=100.0), "activity: band = 100.0 is not a pair"),
            (one, dict(half_width=-1), r"activity: half_width = -1 outside \[0, 1024\]"),
            (one, dict(half_width=1025), r"activity: half_width = 1025 outside \[0, 1024\]"),
            (one, dict(half_width=1.5), "activity: half_width = 1.5 is not an integer number of frames"),
            (one, dict(range_db=-1.0), "activity: range_db = -1.0 < 0.0"),
            (one, dict(dominance_db=float("inf")), "activity: dominance_db = inf is not a finite number"),
            (one, dict(hysteresis_db=-3), "activity: hysteresis_db = -3 < 0.0"),
            (one, dict(min_on=0), "activity: min_on = 0 or min_off = 13 < 1 frame"),
            (one, dict(min_off=0), "activity: min_on = 13 or min_off = 0 < 1 frame"),
            (one, dict(pad=-1), "activity: pad = -1 < 0"),
            ((1, 1, 1 << 25), dict(n_fft=64, hop=8), r"activity: 4194305 frames \(L = 33554432, hop = 8\) > 2\^22 per item")):
        with pytest.raises(ValueError, match=msg):
            native.check_activity(shape, **kw)
    native.check_activity((1, 1, (1 << 25) - 8), n_fft=64, hop=8)                  # 2^22 frames
    assert native.check_activity_gate((2, 2, 600), (2, 2, 6), [600, 1]) == ((2, 2, 600), 6, [600, 1])
    for x, a, kw, msg in (((600,), (1, 1, 6), {}, r"activity_gate: x must be \[B, n, L\]"),
                          ((1, 5, 600), (1, 5, 6), {}, r"activity_gate: n = 5 outside \[1, 4\]"),
                          ((1, 2, 600), (1, 2, 4), {}, r"activity_gate: act must be \[B, n, F\] with x's B and n and "
                                                       r"F >= 6 frames \(L = 600, hop = 128; got \(1, 2, 4\)\)"),
                          ((1, 2, 600), (1, 3, 6), {}, "activity_gate: act must be"),
                          ((1, 2, 600), (1, 2, 6), dict(hop=4), r"activity_gate: hop = 4 outside \[8, 65536\]"),
                          ((1, 2, 600), (1, 2, 6), dict(fade=4097), r"activity_gate: fade = 4097 samples outside"),
                          ((1, 2, 600), (1, 2, 6), dict(fade=-1), r"activity_gate: fade = -1 samples outside"),
                          ((1, 2, 600), (1, 2, 6), dict(lens=[601]), r"sample count lens\[0\] = 601 outside")):
        with pytest.raises(ValueError, match=msg):
            native.check_activity_gate(x, a, **kw)


# ------------------------------------------------------------------ frames and samples
@pytest.mark.parametrize("hop,n_fft", [(16, 64), (128, 512)])
def test_segments_against_a_per_sample_labelling(hop, n_fft):
    """frame t owns [t hop - hop / 2, (t + 1) hop - hop / 2) of [0, L): every L from n_fft / 2 + 1 over three hops, the
    multiples of hop among them"""
    g = np.random.default_rng(hop)
    for L in range(n_fft // 2 + 1, n_fft // 2 + 2 + 3 * hop):
        F = 1 + -(-L // hop)
        for row in (g.integers(0, 2, F), np.ones(F, np.uint8), np.zeros(F, np.uint8), np.eye(F, dtype=np.uint8)[F - 1]):
            label = np.array([row[(m + hop // 2) // hop] != 0 for m in range(L)])
            want = ar.runs_of(label)
            padded = np.concatenate([row, [1, 1, 1]])                  # (frames past F are not the item's)
            assert native.activity_segments(padded, F, hop, L) == want == ar.segments(padded, F, hop, L), (L, row)
    assert native.activity_segments([1, 1, 0, 1], 4, 128, 300) == [(0, 192)]       # the last frame owns no sample


# ------------------------------------------------------------------ the run rules
def rules(bits, min_on=1, min_off=1, pad=0):
    a = np.array([c == "1" for c in bits])
    x, y = ar.rules_loops(a, min_on, min_off, pad), ar.rules_scans(a, min_on, min_off, pad)
    assert np.array_equal(x, y), bits
    return "".join("1" if v else "0" for v in x)


def test_run_rules_on_hand_written_rows():
    assert rules("0110001100", min_off=3) == "0110001100"               # a gap of exactly min_off stays
    assert rules("0110001100", min_off=4) == "0111111100"               # .. of min_off - 1 is closed
    assert rules("0011100", min_on=3) == "0011100"                      # a run of exactly min_on stays
    assert rules("0011100", min_on=4) == "0000000"                      # .. of min_on - 1 is cleared
    assert rules("0011000", min_off=9) == "0011000"                     # leading and trailing stretches never close
    assert rules("1100000", min_off=9) == "1100000"
    assert rules("0000011", min_off=9) == "0000011"
    assert rules("1101011", min_on=3, min_off=2) == "1111111"           # gaps first: the single frame survives
    assert rules("0101000", min_on=2, min_off=2) == "0111000"
    assert rules("0100010", min_on=2, min_off=2) == "0000000"
    assert rules("0010000100", pad=1) == "0111001110"
    assert rules("0010000100", pad=2) == "1111111111"                   # padding merges the runs and is cut at both ends
    assert rules("1000000001", pad=3) == "1111001111"
    assert rules("0000100000", min_on=2, pad=3) == "0000000000"         # the run is cleared before it is padded
    assert rules("0000000000", pad=3) == "0000000000"
    assert rules("", pad=3) == ""
    g = np.random.default_rng(0)
    for _ in range(200):
        bits = "".join(g.choice(["0", "1"], size=int(g.integers(1, 40))))
        rules(bits, int(g.integers(1, 6)), int(g.integers(1, 6)), int(g.integers(0, 4)))


def test_hysteresis_forms_agree():
    g = np.random.default_rng(1)
    for _ in range(200):
        F = int(g.integers(1, 50))
        on, stay = g.integers(0, 2, F).astype(bool), g.integers(0, 2, F).astype(bool)     # (stay need not contain on)
        assert np.array_equal(ar.hysteresis_loops(on, stay), ar.hysteresis_scans(on, stay))
    on, stay = np.array([0, 1, 0, 0, 0, 1, 0], bool), np.array([1, 1, 1, 0, 1, 0, 1], bool)
    assert ar.hysteresis_loops(on, stay).tolist() == [False, True, True, False, False, True, True]


def test_nan_and_silence_in_the_decision():
    E = np.ones((2, 20))
    E[1, 8] = np.nan
    act, lev, _ = ar.decide_both(E, half_width=1, min_on=1, min_off=1)
    assert np.isnan(lev[1, 7:10]).all() and not act[1, 7:10].any() and act[0].all() and act[1, :7].all()
    act, lev, _ = ar.decide_both(np.zeros((2, 9)), half_width=7, min_on=1, min_off=1)
    assert not act.any() and not lev.any()


def test_the_two_routes_of_the_spectra():
    """float64: the explicit framing with numpy's rfft equals torch.stft in float64 to rounding; float32 is a run of the
    transform in float32 (torch.stft), not the float64 result rounded once: its band energies differ from float64 by
    more than one rounding of a sum and by less than 1e-6"""
    est = ar.burst_case(1, 2, 3000, 16)
    S = ar.spectra(est, 64, 16)
    x = np.zeros((2, 3008))
    x[:, :3000] = est
    Z = torch.stft(torch.from_numpy(x), 64, hop_length=16, window=torch.from_numpy(ar.mrr.window(64)), center=True,
                   pad_mode="reflect", return_complex=True).numpy().transpose(0, 2, 1)
    assert S.shape == Z.shape == (2, 189, 33) and np.abs(S - Z).max() <= 1e-13 * np.abs(S).max()
    S32 = ar.spectra(est, 64, 16, dtype=np.float32)
    assert S32.dtype == np.complex64 and S32.shape == S.shape
    assert not np.array_equal(S32, S.astype(np.complex64))
    E, E32 = ar.energies(est, 64, 16), ar.energies(est, 64, 16, dtype=np.float32)
    assert 1e-9 < np.max(np.abs(E32 - E)) / np.max(E) < 1e-6


# ------------------------------------------------------------------ the sanity case
@pytest.mark.parametrize("leak,most", [(0.3, 0.12), (0.1, 0.12), (0.6, None)])
def test_sanity_case(leak, most):
    """Two burst-noise sources, each off for one burst of 2000 samples in three; 512 / 128, half-width 2, min_on =
    min_off = 6 frames.  Measured: 24 / 19 of 251 frames wrong (9.6 / 7.6 %) at 30 % leakage, 18 / 13 (7.2 / 5.2 %) at
    10 %, every one of them within three frames of one of the ten edges; at 60 % (-4.4 dB, above the 6 dB dominance
    threshold) both sources are active throughout."""
    _, est, _ = br.sanity_case(leak=leak)
    n, L = est.shape
    E = ar.energies(est, 512, 128, ar.band_bins((100.0, 4000.0), 16000, 512))
    act, _, ratios = ar.decide_both(E, half_width=2, consts=ar.constants(), min_on=6, min_off=6, pad=0)
    on = np.stack([(np.arange(L) // 2000 + i) % (n + 1) != 0 for i in range(n)])
    truth = ar.truth_frames(on, 128)
    wrong = (act != truth).sum(axis=1)
    print(f"leak {leak}: {wrong.tolist()} of {act.shape[1]} frames wrong, closest ratio {np.min(np.abs(ratios - 1)):.1e}")
    if most is None:
        assert act.all()
        return
    assert np.all(wrong <= most * act.shape[1]), wrong
    edges = np.flatnonzero(np.diff(truth.astype(np.int8), axis=1)[0]).tolist() \
        + np.flatnonzero(np.diff(truth.astype(np.int8), axis=1)[1]).tolist()
    for i in range(n):
        for t in np.flatnonzero(act[i] != truth[i]):
            assert min(abs(t - e) for e in edges) <= 3, (i, t)


# ------------------------------------------------------------------ the keyword's host side
def test_the_entry_points_refuse_by_name(tmp_path):
    a = native.activity_options(True)
    refuse = LatentDiffSep._activity_refusals
    assert refuse(a) is None
    for kw, msg in ((dict(stems="mask"), "activity= does not go with stems="),
                    (dict(latent=True), "activity= decides on waveforms: with latent=True"),
                    (dict(intermediate=True), "activity= does not go with intermediate")):
        with pytest.raises(ValueError, match=msg):
            refuse(a, **kw)
    m = object.__new__(LatentDiffSep)           # no engine to touch: the refusals come first
    m.engine = None
    assert m.last_activity is None
    mix, clips = torch.zeros(1, 2, 4000), [torch.zeros(2, 4000)]
    calls = (lambda **kw: m.separate(mix, **kw), lambda **kw: m.separate_batch(clips, **kw),
             lambda **kw: m.separate_long(clips, 2048, **kw), lambda **kw: m.separate_long(clips, 2048, mode="score", **kw))
    for call in calls:
        with pytest.raises(ValueError, match="activity= does not go with stems="):
            call(activity=True, stems="mask")
        with pytest.raises(ValueError, match="activity= does not go with intermediate"):
            call(activity="gate", intermediate=True)
        with pytest.raises(ValueError, match=r"activity: unknown keys \['frames'\]"):
            call(activity={"frames": 3})
        with pytest.raises(ValueError, match="activity must be None, True, 'gate' or a dict"):
            call(activity=False)
    with pytest.raises(ValueError, match="activity= decides on waveforms: with latent=True"):
        m.separate(mix, activity=True, latent=True)

    class NoDevice:
        engine, hop_length, n_src = None, 8, 2

        def _model_rate(self, what):
            return 16000

    for kw, msg in ((dict(activity=True, stems="mask"), "activity= does not go with stems="),
                    (dict(activity={"min_on": 0}), "activity: min_on = 0.0 s is not positive"),
                    (dict(activity="vad"), "activity must be None, True, 'gate' or a dict")):
        with pytest.raises(ValueError, match=msg):
            files.separate_files(NoDevice(), [tmp_path / "a.wav"], tmp_path / "never", **kw)
    assert not (tmp_path / "never").exists()
    for fn in (LatentDiffSep.separate, LatentDiffSep.separate_batch, LatentDiffSep.separate_long,
               LatentDiffSep.separate_files, files.separate_files):
        assert inspect.signature(fn).parameters["activity"].default is None


def test_rttm_lines():
    segs = [[(0, 1600), (32000, 40000)], [(800, 2400)], []]
    want = ["SPEAKER rec 1 0.000 0.100 <NA> <NA> s0 <NA> <NA>", "SPEAKER rec 1 0.050 0.100 <NA> <NA> s1 <NA> <NA>",
            "SPEAKER rec 1 2.000 0.500 <NA> <NA> s0 <NA> <NA>"]
    assert native.activity_rttm("rec", segs, 16000) == want == ar.rttm_lines("rec", segs, 16000)
    assert native.activity_rttm("rec", [[(5, 9)], [(5, 7)]], 16000)[0].endswith("s0 <NA> <NA>")     # onset, then source
    assert native.activity_rttm("rec", [[], []], 16000) == []


def test_symbols_declared_exported_and_built():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "ditsep_hip.h")).read()
    assert re.search(r"\bint dsn_activity\(dsn_ctx\* ctx, const float\* est, int B, int n, int Lmax, const int32_t\* lens,",
                     hdr)
    assert re.search(r"\bint dsn_activity_gate\(dsn_ctx\* ctx, const float\* x, const uint8_t\* act, int B, int n,", hdr)
    lib = native.load_library()
    for name, nargs in (("dsn_activity", 23), ("dsn_activity_gate", 13)):
        assert name in native.EXPORTS and hasattr(lib, name) and len(getattr(lib, name).argtypes) == nargs
    src = open(os.path.join(root, "ditsep_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS = .*\bactivity\.hip\b", src, flags=re.M)
    assert os.path.exists(os.path.join(root, "ditsep_amd", "csrc", "activity.hip"))


def test_command_line_flags():
    p = separate.build_parser()
    base = ["in", "out", "--config", "c.json"]
    a = p.parse_args(base)
    assert a.activity is False and a.activity_gate is False and separate.activity_of(a) is None
    a = p.parse_args(base + ["--activity"])
    assert native.activity_options(separate.activity_of(a)) == native.ACTIVITY_DEFAULTS
    a = p.parse_args(base + ["--activity-gate"])
    assert native.activity_options(separate.activity_of(a)) == native.activity_options("gate")
    a = p.parse_args(base + ["--activity", "--activity-range", "30", "--activity-dominance", "3", "--activity-hysteresis",
                             "1", "--activity-min-on", "0.2", "--activity-min-off", "0.3", "--activity-pad", "0.05",
                             "--activity-smooth", "0.1", "--activity-band", "300", "3400", "--activity-fade", "2.5"])
    assert separate.activity_of(a) == dict(gate=False, band=(300.0, 3400.0), smooth=0.1, range_db=30.0, dominance_db=3.0,
                                           hysteresis_db=1.0, min_on=0.2, min_off=0.3, pad=0.05, fade_ms=2.5)
    for bad in (["--activity-band", "300"], ["--activity-range", "wide"], ["--activity-fade", "fast"]):
        with pytest.raises(SystemExit):
            p.parse_args(base + bad)
