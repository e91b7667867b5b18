"""The `stems` keyword without a GPU: the float64 restatement's own properties (tests/stems_restatement.py), the option
parsing and refusals of ditsep_amd.native, the command line, and the interleaved encoder's restatement against Python's
`wave` module."""
import io
import wave

import numpy as np
import pytest

from ditsep_amd import native, separate
from tests import mask_refine_restatement as mr
from tests import stems_restatement as sr

KINDS = ("generic", "dual", "hard", "silent_ch", "silent_est")


@pytest.mark.parametrize("C", [1, 2])
@pytest.mark.parametrize("n", [1, 2, 3])
def test_wiener_outputs_sum_to_every_channel(C, n):
    for k, kind in enumerate(KINDS):
        mix, est = sr.make_case(100 * C + 10 * n + k, kind, n, C, 700)
        for solver in ("adjugate", "solve"):
            out = sr.stems(mix, est, n_fft=128, hop=32, solver=solver)
            assert out.shape == (n, C, 700) and np.all(np.isfinite(out))
            # float64 throughout: lambda's remainder is handed out equally, so the sum is the mixture
            assert sr.rel_err(out.sum(axis=0), mix, mix) < 1e-12, (kind, solver)


@pytest.mark.parametrize("C", [1, 2])
def test_the_two_solvers_agree(C):
    for k, kind in enumerate(KINDS):
        mix, est = sr.make_case(7 * C + k, kind, 3, C, 900)
        a, ia = sr.stems(mix, est, n_fft=256, hop=64, return_info=True)
        b, ib = sr.stems(mix, est, n_fft=256, hop=64, solver="solve", return_info=True)
        # dual-mono: Sigma + lambda I has condition number about 1 / reg = 1e3
        assert sr.rel_err(a, b, mix) < 1e-10, kind
        assert np.array_equal(ia["R"], ib["R"]) and np.array_equal(ia["den"], ib["den"])
        R = ia["R"]
        assert np.allclose(R, np.conj(np.swapaxes(R, -1, -2)), atol=1e-15)             # Hermitian
        assert np.allclose(np.einsum("ifcc->if", R).real, C)                           # tr R_i = C: d_i is tr N_i / C


def test_float32_mode_is_close_to_float64():
    mix, est = sr.make_case(5, "generic", 2, 2, 3000)
    ref = sr.stems(mix, est)
    f32 = sr.stems(mix, est, dtype=np.float32)
    assert f32.dtype == np.float32 and 1e-9 < sr.rel_err(f32, ref, mix) < 1e-5


@pytest.mark.parametrize("power", [1, 2])
def test_mask_mode_is_the_mono_restatement_per_channel(power):
    mix, est = sr.make_case(11, "generic", 3, 3, 1000)
    for dtype in (np.float64, np.float32):
        out = sr.stems(mix, est, mode="mask", n_fft=256, hop=128, power=power, dtype=dtype)
        for c in range(3):
            want = mr.refine_torch(mix[c], est, 256, 128, power, dtype=dtype)
            assert np.array_equal(out[:, c], want), (c, dtype)


@pytest.mark.parametrize("mode", ["mask", "wiener"])
def test_silent_estimates_give_equal_outputs(mode):
    mix, est = sr.make_case(13, "silent_est", 4, 2, 800)
    out = sr.stems(mix, est, mode=mode, n_fft=128, hop=64)
    for i in range(1, 4):
        assert np.array_equal(out[i], out[0])
    assert sr.rel_err(4 * out[0], mix, mix) < 1e-12


def test_stems_options():
    assert native.stems_options(None) is None
    assert native.STEMS_DEFAULTS == dict(mode="wiener", n_fft=512, hop=128, power=2, eps=1e-10, reg=1e-3)
    assert native.stems_options("mask") == dict(native.STEMS_DEFAULTS, mode="mask")
    assert native.stems_options("wiener") == native.STEMS_DEFAULTS
    assert native.stems_options({"mode": "mask", "n_fft": 1024, "hop": 256, "reg": 0.0}) == dict(
        mode="mask", n_fft=1024, hop=256, power=2, eps=1e-10, reg=0.0)
    for bad, msg in ((True, "stems must be None, 'mask', 'wiener' or a dict"), (False, "stems must be"),
                     ("mwf", "stems must be"), ({"window": 3}, r"stems: unknown keys \['window'\]"),
                     ({"mode": "em"}, r"stems: mode must be one of \['mask', 'wiener'\] \(got 'em'\)")):
        with pytest.raises(ValueError, match=msg):
            native.stems_options(bad)


def test_check_stems():
    good = native.check_stems((3, 2, 600), (3, 4, 600), [600, 300, 257], [2, 1, 2])
    assert good == ((3, 2, 4, 600), [600, 300, 257], [2, 1, 2], 1, 512, 128, 2, 1e-10, 1e-3)
    assert native.check_stems((1, 8, 600), (1, 1, 600), mode="mask")[:4] == ((1, 8, 1, 600), None, None, 0)
    for args, kw, msg in (
            (((1, 2, 600), (1, 2, 600)), dict(mode="em"), "stems: mode must be one of"),
            (((2, 600), (2, 2, 600)), {}, r"stems: mix must be \[B, C, L\] and est \[B, n, L\]"),
            (((2, 2, 600), (2, 2, 601)), {}, "stems: mix must be"),
            (((1, 3, 600), (1, 2, 600)), {}, r"stems: C = 3 outside \[1, 2\] for mode 'wiener' \(the Wiener filter"),
            (((1, 9, 600), (1, 2, 600)), dict(mode="mask"), r"stems: C = 9 outside \[1, 8\] for mode 'mask'"),
            (((1, 2, 600), (1, 5, 600)), {}, r"stems: n = 5 outside \[1, 4\]"),
            (((1, 2, 600), (1, 2, 600)), dict(n_fft=384), "stems: n_fft = 384 is not a power of two"),
            (((1, 2, 600), (1, 2, 600)), dict(hop=512), "stems: n_fft / hop = 512 / 512 is not one of 2, 4, 8"),
            (((1, 2, 600), (1, 2, 600)), dict(power=3), "stems: power = 3 is not 1 or 2"),
            (((1, 2, 600), (1, 2, 600)), dict(eps=0.0), "stems: eps = 0.0 is not a finite positive number"),
            (((1, 2, 600), (1, 2, 600)), dict(reg=-1e-3), "stems: reg = -0.001 is not a finite number >= 0"),
            (((1, 2, 600), (1, 2, 600)), dict(reg=float("nan")), "stems: reg = nan is not a finite number"),
            (((1, 2, 600), (1, 2, 600)), dict(lens=[256]), r"stems: item 0 has 256 samples, outside \[n_fft / 2 \+ 1 = 257"),
            (((2, 2, 600), (2, 2, 600)), dict(channels=[2]), "stems: channels must hold one channel count per item"),
            (((2, 2, 600), (2, 2, 600)), dict(channels=[2, 3]), r"stems: item 1 has channels = 3, outside \[1, C = 2\]"),
            (((2, 2, 600), (2, 2, 600)), dict(channels=[0, 1]), r"stems: item 0 has channels = 0, outside")):
        with pytest.raises(ValueError, match=msg):
            native.check_stems(*args, **kw)


def test_command_line_flags():
    p = separate.build_parser()
    base = ["in", "out", "--config", "c.json"]
    a = p.parse_args(base)
    assert a.stems is None and separate.stems_of(a) is None
    a = p.parse_args(base + ["--stems", "wiener"])
    assert separate.stems_of(a) == dict(mode="wiener", n_fft=512, hop=128, power=2, reg=1e-3)
    assert native.stems_options(separate.stems_of(a)) == native.STEMS_DEFAULTS
    a = p.parse_args(base + ["--stems", "mask", "--stems-nfft", "1024", "--stems-hop", "256", "--stems-power", "1",
                             "--stems-reg", "0.01"])
    assert separate.stems_of(a) == dict(mode="mask", n_fft=1024, hop=256, power=1, reg=0.01)
    for bad in (["--stems", "em"], ["--stems-power", "3"], ["--stems"]):
        with pytest.raises(SystemExit):
            p.parse_args(base + bad)


@pytest.mark.parametrize("C", [1, 2, 3])
def test_interleave_against_the_wave_module(C):
    g = np.random.default_rng(C)
    x = (0.1 * g.standard_normal((C + 1, 50))).astype(np.float32)
    x[0, 3], x[C - 1, 7], x[0, 9] = 1.5, -2.0, np.nan                                  # two clamped, one not finite
    for frames in (50, 17):
        payload, clipped = sr.encode_frames(x, frames, C, "s16")
        assert len(payload) == frames * C * 2
        assert clipped == 3                                                            # all three lie before frame 17
        buf = io.BytesIO()
        with wave.open(buf, "wb") as f:
            f.setnchannels(C)
            f.setsampwidth(2)
            f.setframerate(8000)
            f.writeframes(payload)
        buf.seek(0)
        with wave.open(buf, "rb") as f:
            assert (f.getnchannels(), f.getnframes()) == (C, frames)
            got = np.frombuffer(f.readframes(frames), dtype="<i2").reshape(frames, C)
        want = np.clip(np.rint(np.nan_to_num(x[:C, :frames].astype(np.float64)) * 32768.0), -32768, 32767).T
        assert np.array_equal(got, want.astype(np.int16))
    # the unused channel and the frames past the end take no part
    y = x.copy()
    y[C:], y[:, 17:] = 9.0, 9.0
    assert sr.encode_frames(y, 17, C, "s16") == sr.encode_frames(x, 17, C, "s16")
    for enc, w in (("s24", 3), ("f32", 4)):
        payload, _ = sr.encode_frames(x, 50, C, enc)
        assert len(payload) == 50 * C * w
    assert sr.encode_frames(x, 50, C, "f32")[0] == np.ascontiguousarray(x[:C].T).tobytes()
