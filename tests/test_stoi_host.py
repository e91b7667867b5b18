"""CPU-only: the float64 STOI / ESTOI restatement (tests/stoi_restatement.py) that dsn_stoi is tested against, and the
dsn_stoi C-ABI binding."""
import ctypes
import os
import re

import numpy as np
import pytest

from ditsep_amd import native, synthetic
from tests import stoi_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("fs,L", [(8000, 8000), (16000, 16000), (44100, 11025)])
def test_resampler_equals_scipy_resample_poly(fs, L):
    from scipy.signal import resample_poly

    x = np.random.default_rng(fs).standard_normal(L)
    h = R.resample_window(R.FS, fs)
    want = resample_poly(x, R.FS, fs, window=h / h.sum())
    got = R.resample(x, fs)
    assert got.shape == want.shape == (-(-L * R.FS // fs),)
    assert np.abs(got - want).max() < 1e-12


def test_resample_filter_lengths():
    assert R.resample_window(10000, 16000).size == 581
    assert R.resample_window(10000, 8000).size == 365


def test_band_edges():
    assert R.band_edges() == [(7, 9), (9, 11), (11, 14), (14, 17), (17, 22), (22, 27), (27, 34), (34, 43), (43, 55),
                              (55, 69), (69, 87), (87, 109), (109, 138), (138, 174), (174, 219)]


@pytest.mark.parametrize("fs", [10000, 16000])
@pytest.mark.parametrize("extended", [False, True])
def test_identical_signals_score_one(fs, extended):
    x = synthetic.synthetic_sources(1, 1, 3 * fs, fs=fs, seed=5)[0, 0].double().numpy()
    assert abs(R.stoi(x, x, fs, extended) - 1.0) < 1e-12


def test_stft_frames_are_kept_frames_minus_one():
    """A silence-removed signal of K kept frames has (K-1)*128 + 256 samples and K - 1 STFT frames: the last frame
    that fits is excluded from the STFT (strict <), but included by the silent-frame removal."""
    rng = np.random.default_rng(3)
    x = rng.standard_normal(20000)
    x[6000:11000] *= 1e-3          # a -60 dB gap: its frames are removed
    y = x + 0.1 * rng.standard_normal(x.size)
    xs, ys, mask = R.remove_silent_frames(x, y)
    K = int(mask.sum())
    assert 0 < K < mask.size
    assert xs.size == ys.size == (K - 1) * R.HOP + R.N_FRAME
    assert R.stft(xs).shape == (K - 1, R.NFFT // 2 + 1)
    score, frames, k2 = R.stoi_details(x, y, R.FS)
    assert frames == K - 1 and k2 == K and 0 < score < 1


def test_short_input_returns_floor():
    x = np.random.default_rng(4).standard_normal(3000)
    score, frames, _ = R.stoi_details(x, x, R.FS, True)
    assert frames < R.N and score == 1e-5


def _c_to_ctypes(param: str):
    """ctypes type of one dsn_stoi parameter: device arrays are c_void_p, host arrays typed pointers."""
    param = " ".join(param.split())
    if param.startswith("dsn_ctx*") or param.startswith("void*") or param.startswith("const float*"):
        return ctypes.c_void_p
    if param.startswith("float*"):
        return ctypes.POINTER(ctypes.c_float)
    if param.startswith("const int*") or param.startswith("int*"):
        return ctypes.POINTER(ctypes.c_int)
    if param.startswith("int "):
        return ctypes.c_int
    raise AssertionError(f"unexpected parameter {param!r}")


def test_dsn_stoi_binding_matches_header():
    hdr = open(os.path.join(ROOT, "include", "ditsep_hip.h")).read()
    m = re.search(r"\bint\s+dsn_stoi\s*\(([^)]*)\)\s*;", hdr)
    assert m, "dsn_stoi is not declared in include/ditsep_hip.h"
    params = [p.strip() for p in m.group(1).split(",")]
    names = [re.findall(r"\w+", p)[-1] for p in params]
    assert names == ["ctx", "ref", "est", "B", "n", "L", "fs", "extended", "perm", "out", "frames_out", "stream"]
    assert "dsn_stoi" in native.EXPORTS
    lib = native.load_library()
    assert list(lib.dsn_stoi.argtypes) == [_c_to_ctypes(p) for p in params]
