"""The host side of dsn_beamform_track: its float64 restatement (tests/beamform_track_restatement.py) against
beamform_restatement where the two must agree, the interpolation table, the options, refusals and flags of the `track`
keyword, and the moving-source sanity case the README's table reports."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

from ditsep_amd import files, native, separate
from ditsep_amd.latent import LatentDiffSep
from tests import beamform_restatement as br
from tests import beamform_track_restatement as tr


@pytest.fixture(scope="module")
def sanity():
    return br.sanity_case()


# ------------------------------------------------------------------ the restatement
def test_one_block_is_the_time_invariant_beamformer(sanity):
    mix, est, _ = sanity
    for kw in (dict(), dict(ref=2, postfilter="mask", power=1)):
        ref, iref = br.beamform(mix, est, return_info=True, **kw)
        F = 1 + -(-mix.shape[-1] // 128)
        for Tb, ctx, interp in ((F, 0, True), (F + 7, 3, False), (1 << 20, 1, True)):
            out, info = tr.beamform_track(mix, est, block_frames=Tb, context=ctx, interpolate=interp, return_info=True,
                                          **kw)
            assert info["w"].shape == (1,) + iref["w"].shape
            assert np.array_equal(info["w"][0], iref["w"]) and np.array_equal(out, ref)
            assert np.allclose(info["power"][0], iref["power"], rtol=1e-12, atol=0)      # (a diagnostic: another sum order)


def test_a_context_over_all_blocks_gives_every_block_the_same_weights(sanity):
    mix, est, _ = sanity
    mix, est = mix[:, :9000], est[:, :9000]
    F = 1 + -(-9000 // 128)
    Tb = 9
    K = -(-F // Tb)
    on, ion = tr.beamform_track(mix, est, block_frames=Tb, context=K - 1, interpolate=True, return_info=True)
    off, ioff = tr.beamform_track(mix, est, block_frames=Tb, context=K - 1, interpolate=False, return_info=True)
    assert ion["w"].shape[0] == K > 3
    for k in range(1, K):
        assert np.array_equal(ion["w"][k], ion["w"][0])
    assert np.array_equal(ion["w"], ioff["w"]) and np.array_equal(on, off)
    # ... and a smaller context does not
    less, iless = tr.beamform_track(mix, est, block_frames=Tb, context=1, return_info=True)
    assert not np.array_equal(iless["w"][0], iless["w"][K - 1]) and not np.array_equal(less, on)


@pytest.mark.parametrize("Tb", [4, 5, 100])
def test_the_interpolation_table(Tb):
    """native.track_plan and the restatement's frame_plan against the centre-to-centre interpolation in float64: block
    k's centre is at (k Tb + (Tb - 1) / 2) frames whatever the last block's length, a frame between two centres takes
    alpha = (t - centre_k0) / Tb, a frame before the first or at or after the last centre holds"""
    for F in range(1, 3 * Tb + 2):
        K = -(-F // Tb)
        k0, alpha = native.track_plan(F, Tb, True)
        k0, alpha = k0.numpy(), alpha.numpy()
        rk, ra = tr.frame_plan(F, Tb, True)
        assert np.array_equal(k0, rk) and np.array_equal(alpha, ra)
        assert k0.shape == alpha.shape == (F,) and np.all((alpha >= 0) & (alpha < 1)) and np.all((k0 >= 0) & (k0 < K))
        for t in range(F):
            pos = (t - (Tb - 1) / 2.0) / Tb                       # in blocks, from the first centre
            want_k, want_a = (0, 0.0) if pos <= 0 else (K - 1, 0.0) if pos >= K - 1 else (int(pos), pos - int(pos))
            assert k0[t] == want_k and abs(alpha[t] - want_a) <= 1e-15, (F, t)
        half = (Tb - 1) // 2 + 1                                   # the frames up to the first centre hold block 0
        assert np.all(k0[:half] == 0) and np.all(alpha[:half] == 0)
        last = (K - 1) * Tb + Tb // 2                              # .. and from the last centre on the last block
        assert np.all(k0[last:] == K - 1) and np.all(alpha[last:] == 0)
        hk, ha = native.track_plan(F, Tb, False)
        assert np.array_equal(hk.numpy(), np.arange(F) // Tb) and not ha.any()
        assert np.array_equal(tr.frame_plan(F, Tb, False)[0], np.arange(F) // Tb)


def test_float32_mode_is_close_to_float64(sanity):
    mix, est, _ = sanity
    mix, est = mix[:, :9000], est[:, :9000]
    ref, iref = tr.beamform_track(mix, est, block_frames=20, return_info=True)
    cpu, icpu = tr.beamform_track(mix, est, block_frames=20, dtype=np.float32, return_info=True)
    assert cpu.dtype == np.float32 and br.rel_err(cpu, ref, mix) < 1e-5
    assert np.max(np.abs(icpu["w"] - iref["w"])) / np.max(np.abs(iref["w"])) < 1e-4


# ------------------------------------------------------------------ the sanity case
def test_tracking_gains_on_a_moving_source():
    """C = 3, 4 positions of source 0, L = 128000, leak 0.3, the defaults (100 frames, one block of context each side,
    interpolated): both sources gain at least 3 dB SI-SDR over the time-invariant beamformer on the same input.
    Measured: 6.76 / 8.18 dB time-invariant, 12.20 / 16.91 dB tracked (the estimates themselves: 9.55 / 11.34 dB)."""
    mix, est, img = tr.moving_case()
    assert mix.shape == (3, 128000) and est.shape == img.shape == (2, 128000)
    fixed = br.beamform(mix, est)
    tracked = tr.beamform_track(mix, est, **tr.DEFAULTS)
    for i in range(2):
        a, b = br.si_sdr(fixed[i], img[i]), br.si_sdr(tracked[i], img[i])
        print(f"source {i}: estimate {br.si_sdr(est[i], img[i]):.2f} dB, time-invariant {a:.2f} dB, tracked {b:.2f} dB")
        assert b >= a + 3.0, (i, a, b)


def test_the_moving_case_is_the_sanity_case_with_one_position():
    a, b = tr.moving_case(L=9000, C=4, pos=1), br.sanity_case(L=9000)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    c = tr.moving_case(L=9000, C=4, pos=3)
    # the moving source's image: the first segment keeps sanity_case's filter, the others have their own
    assert np.array_equal(c[2][0][:3000], a[2][0][:3000]) and not np.array_equal(c[2][0][3000:], a[2][0][3000:])
    assert np.array_equal(c[2][1], a[2][1])                       # the other source stays where it is


# ------------------------------------------------------------------ the host side of the keyword
def test_track_options():
    assert native.TRACK_DEFAULTS == dict(block=0.8, context=1, interpolate=True)
    assert set(native.BEAMFORM_DEFAULTS).isdisjoint(native.TRACK_DEFAULTS)
    assert native.track_options(None) is None
    assert native.track_options(True) == native.TRACK_DEFAULTS
    assert native.track_options(0.5) == dict(block=0.5, context=1, interpolate=True)
    assert native.track_options(2) == dict(block=2.0, context=1, interpolate=True)
    assert native.track_options({"context": 0, "interpolate": False}) == dict(block=0.8, context=0, interpolate=False)
    for bad, msg in ((False, "track must be None, True, a block length in seconds or a dict"), ("blocks", "track must be"),
                     ({"frames": 100}, r"track: unknown keys \['frames'\]"),
                     ({"block": 0}, "track: block = 0 is not a positive number of seconds"),
                     ({"block": -1.0}, "track: block = -1.0 is not a positive number"),
                     ({"block": float("nan")}, "track: block = nan is not a positive number"),
                     ({"block": "1"}, "track: block = '1' is not a positive number"),
                     ({"context": 65}, r"track: context = 65 outside \[0, 64\]"),
                     ({"context": -1}, r"track: context = -1 outside \[0, 64\]"),
                     ({"context": 1.5}, r"track: context = 1.5 outside \[0, 64\]"),
                     ({"context": True}, r"track: context = True outside \[0, 64\]"),
                     ({"interpolate": 1}, "track: interpolate = 1 is not True or False")):
        with pytest.raises(ValueError, match=msg):
            native.track_options(bad)


def test_seconds_to_frames():
    assert native.track_block_frames(0.8, 16000, 128) == 100
    assert native.track_block_frames(0.8, 16000, 256) == 50
    assert native.track_block_frames(0.5, 44100, 128) == 172          # 172.27
    assert native.track_block_frames(0.02, 16000, 128) == 4           # 2.5 rounds up to 3; the floor of 4 holds
    assert native.track_block_frames(0.036, 16000, 128) == 5          # 4.5 rounds up
    assert native.track_block_frames(1e-6, 16000, 128) == 4
    beam = native.beamform_options({"ref": 2, "n_fft": 1024, "hop": 256, "postfilter": "mask"})
    kw = native.track_beamform_keywords(beam, native.track_options({"context": 2}), 16000)
    assert kw == dict(ref=2, n_fft=1024, hop=256, power=2, eps=1e-10, reg=1e-3, postfilter="mask", block_frames=50,
                      context=2, interpolate=True)
    native.check_track((1, 4, 3000), (1, 2, 3000), **kw)
    assert native.track_beamform_keywords(beam, native.TRACK_DEFAULTS, None)["block_frames"] is None
    with pytest.raises(ValueError, match="track= adapts the weights of the beamformer block by block: it needs beamform="):
        native.track_beamform_keywords(None, native.TRACK_DEFAULTS, 16000)
    with pytest.raises(ValueError, match="track= does not go with spatial=: the cACGMM sums its statistics inside its "
                                         "solve workgroup"):
        native.track_beamform_keywords(beam, native.TRACK_DEFAULTS, 16000, native.SPATIAL_DEFAULTS)


def test_check_track():
    good = native.check_track((3, 4, 600), (3, 2, 600), [600, 300, 257], [4, 2, 3], ref=1, block_frames=4, context=0,
                              interpolate=False)
    assert good == ((3, 4, 2, 600), [600, 300, 257], [4, 2, 3], 1, 512, 128, 2, 1e-10, 1e-3, 0, 4, 0, 0, 2, 0)
    # F = 1 + ceil(600 / 128) = 6 frames, 2 blocks of 4: partials and sums 2 x 2 x 257 x (2 x 3) doubles each, weights
    # 2 x 257 x 2 complex doubles, one int32 -- per block
    need = native.track_item_bytes(512, 128, 600, 2, 2, 4)
    assert need == 2 * (8 * (2 * 2 * 257 * 6 + 2 * 257 * 2 * 2) + 4)
    assert native.track_item_bytes(512, 128, 600, 2, 2, 6) * 2 == need
    assert native.track_item_bytes(2048, 512, 1 << 20, 8, 4, 100) == 21 * (8 * 4 * 1025 * (144 + 16) + 4)
    assert native.check_track((1, 2, 600), (1, 2, 600), block_frames=4, workspace_budget=need)[-1] == need
    assert native.check_track((1, 2, 600), (1, 2, 600), interpolate=1)[-3] == 1
    one = ((1, 2, 600), (1, 2, 600))
    for args, kw, msg in (
            (((2, 600), (2, 2, 600)), {}, r"beamform_track: mix must be \[B, C, L\] and est \[B, n, L\]"),
            (((1, 9, 600), (1, 2, 600)), {}, r"beamform_track: C = 9 outside \[1, 8\]"),
            (((1, 2, 600), (1, 5, 600)), {}, r"beamform_track: n = 5 outside \[1, 4\]"),
            (one, dict(n_fft=384), "beamform_track: n_fft = 384 is not a power of two"),
            (one, dict(hop=512), "beamform_track: n_fft / hop = 512 / 512 is not one of 2, 4, 8"),
            (one, dict(power=3), "beamform_track: power = 3 is not 1 or 2"),
            (one, dict(eps=0.0), "beamform_track: eps = 0.0 is not a finite positive number"),
            (one, dict(reg=-1e-3), "beamform_track: reg = -0.001 is not a finite number >= 0"),
            (one, dict(ref=2), r"beamform_track: ref = 2 outside \[0, 2\): item 0 has 2 channels"),
            (one, dict(lens=[256]), r"beamform_track: item 0 has 256 samples, outside \[n_fft / 2 \+ 1 = 257, L = 600\]"),
            (one, dict(channels=[3]), r"beamform_track: item 0 has channels = 3, outside \[1, C = 2\]"),
            (one, dict(postfilter="wiener"), "beamform: postfilter must be None, 'none' or 'mask'"),
            (one, dict(block_frames=3), r"beamform_track: block_frames = 3 outside \[4, 2\^20\]"),
            (one, dict(block_frames=(1 << 20) + 1), r"beamform_track: block_frames = 1048577 outside \[4, 2\^20\]"),
            (one, dict(block_frames=4.5), r"beamform_track: block_frames = 4.5 outside \[4, 2\^20\]"),
            (one, dict(block_frames=True), r"beamform_track: block_frames = True outside \[4, 2\^20\]"),
            (one, dict(context=65), r"beamform_track: context = 65 outside \[0, 64\]"),
            (one, dict(context=-1), r"beamform_track: context = -1 outside \[0, 64\]"),
            (one, dict(interpolate=2), "beamform_track: interpolate = 2 is not 0 or 1"),
            (one, dict(interpolate="yes"), "beamform_track: interpolate = 'yes' is not 0 or 1"),
            (((1, 2, 4 * 128 * 4096), (1, 2, 4 * 128 * 4096)), dict(block_frames=4),
             r"beamform_track: 4097 blocks of block_frames = 4 frames at L = 2097152, hop = 128: more than 4096"),
            (one, dict(workspace_budget=-1), "beamform_track: workspace_budget = -1 < 0"),
            (one, dict(block_frames=4, workspace_budget=need - 1),
             rf"beamform_track: workspace_budget = {need - 1} bytes is smaller than one item \({need} bytes at C = 2, "
             rf"n = 2, n_fft = 512, hop = 128, L = 600, block_frames = 4\)")):
        with pytest.raises(ValueError, match=msg):
            native.check_track(*args, **kw)
    native.check_track((1, 2, 4 * 128 * 4096 - 128), (1, 2, 4 * 128 * 4096 - 128), block_frames=4)   # 4096 blocks


def test_the_entry_points_refuse_by_name(tmp_path):
    trk, beam, spat = native.track_options(True), native.beamform_options(True), native.spatial_options(True)
    refuse = LatentDiffSep._track_refusals
    assert refuse(trk, beam, None) is None
    for args, kw, msg in (((trk, beam, None), dict(stems="mask"), "track= does not go with stems="),
                          ((trk, beam, None), dict(latent=True), "track= adapts the filter of waveforms: with latent=True"),
                          ((trk, beam, None), dict(intermediate=True), "track= does not go with intermediate"),
                          ((trk, None, None), {}, "track= adapts the weights of the beamformer block by block: it needs "
                                                  "beamform="),
                          ((trk, beam, spat), {}, "track= does not go with spatial=: the cACGMM sums its statistics")):
        with pytest.raises(ValueError, match=msg):
            refuse(*args, **kw)

    m = object.__new__(LatentDiffSep)           # no engine to touch: the refusals come first
    m.engine = None
    mix, clips = torch.zeros(1, 3, 4000), [torch.zeros(3, 4000)]
    calls = (lambda **kw: m.separate(mix, **kw), lambda **kw: m.separate_batch(clips, **kw),
             lambda **kw: m.separate_long(clips, 2048, **kw), lambda **kw: m.separate_long(clips, 2048, mode="score", **kw))
    for call in calls:
        with pytest.raises(ValueError, match="track= adapts the weights of the beamformer block by block: it needs "
                                             "beamform="):
            call(track=True)
        with pytest.raises(ValueError, match="track= does not go with spatial=: the cACGMM sums its statistics inside "
                                             "its solve workgroup"):
            call(track=True, beamform=True, spatial=True)
        with pytest.raises(ValueError, match="beamform= does not go with stems=|track= does not go with stems="):
            call(track=True, beamform=True, stems="mask")
        with pytest.raises(ValueError, match="does not go with intermediate"):
            call(track=True, beamform=True, intermediate=True)
        with pytest.raises(ValueError, match=r"track: unknown keys \['frames'\]"):
            call(track={"frames": 3}, beamform=True)
    with pytest.raises(ValueError, match="with latent=True there is no mixture to filter"):
        m.separate(mix, track=True, beamform=True, latent=True)

    class NoDevice:
        engine, hop_length, n_src = None, 8, 2

        def _model_rate(self, what):
            return 16000

    for kw, msg in ((dict(track=True), "track= adapts the weights of the beamformer block by block: it needs beamform="),
                    (dict(track=True, beamform=True, spatial=True), "track= does not go with spatial="),
                    (dict(track=True, beamform=True, stems="mask"), "track= does not go with stems="),
                    (dict(track={"block": 0}, beamform=True), "track: block = 0 is not a positive number")):
        with pytest.raises(ValueError, match=msg):
            files.separate_files(NoDevice(), [tmp_path / "a.wav"], tmp_path / "never", **kw)
    assert not (tmp_path / "never").exists()
    for fn in (LatentDiffSep.separate, LatentDiffSep.separate_batch, LatentDiffSep.separate_long,
               LatentDiffSep.separate_files, files.separate_files):
        assert inspect.signature(fn).parameters["track"].default is None
    assert "track" not in inspect.signature(native.Engine.beamform).parameters


def test_symbol_declared_exported_and_built():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "ditsep_hip.h")).read()
    assert re.search(r"\bint dsn_beamform_track\(dsn_ctx\* ctx, const float\* mix, const float\* est, int B, int C, int n, "
                     r"int Lmax,\s+const int32_t\* lens, const int32_t\* channels, int ref, int n_fft, int hop, int power, "
                     r"float eps,\s+float reg, int postfilter, int block_frames, int context, int interpolate,\s+"
                     r"int64_t workspace_budget, float\* out, double\* info_w, void\* stream\);", hdr)
    lib = native.load_library()
    assert "dsn_beamform_track" in native.EXPORTS and hasattr(lib, "dsn_beamform_track")
    assert len(lib.dsn_beamform_track.argtypes) == 23
    src = open(os.path.join(root, "ditsep_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS = .*\bbeamform_track\.hip\b", src, flags=re.M)
    assert os.path.exists(os.path.join(root, "ditsep_amd", "csrc", "beamform_track.hip"))


def test_command_line_flags():
    p = separate.build_parser()
    base = ["in", "out", "--config", "c.json"]
    a = p.parse_args(base)
    assert a.track is False and separate.track_of(a) is None
    a = p.parse_args(base + ["--beamform", "--track"])
    assert separate.track_of(a) == dict(block=0.8, context=1, interpolate=True)
    assert native.track_options(separate.track_of(a)) == native.TRACK_DEFAULTS
    assert separate.beamform_of(a) == dict(ref=0, n_fft=512, hop=128, reg=1e-3, postfilter=None)
    a = p.parse_args(base + ["--track", "--track-block", "1.5", "--track-context", "0", "--track-hold"])
    assert separate.track_of(a) == dict(block=1.5, context=0, interpolate=False)
    assert separate.beamform_of(a) is None and separate.spatial_of(a) is None
    for bad in (["--track-block", "long"], ["--track-context", "1.5"]):
        with pytest.raises(SystemExit):
            p.parse_args(base + bad)
