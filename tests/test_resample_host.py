"""The sinc resampler's host side (no GPU): the plan of csrc/resample_plan.h through dsn_resample_plan against the
float64 restatement (tests/resample_restatement.py), the restatement against itself, the refusals, and the binding."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

from ditsep_amd import native
from tests import resample_restatement as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("dsn_resample_plan", "dsn_resample_length", "dsn_resample")


def test_the_pairs_are_the_28():
    assert len(rr.PAIRS) == 28 and (44100, 16000) in rr.PAIRS and (16000, 44100) in rr.PAIRS


@pytest.mark.parametrize("fs_in,fs_out", rr.PAIRS, ids=lambda v: str(v))
def test_plan_against_the_restatement(fs_in, fs_out):
    o, n, _, width, K = rr.params(fs_in, fs_out)
    plan = native.resample_plan(fs_in, fs_out)
    assert (plan["orig"], plan["new"], plan["width"], plan["K"]) == (o, n, width, K)
    h = rr.dense_taps(fs_in, fs_out)
    k0, S, c = rr.compact(h)                 # (asserts that every dropped tap is exactly 0.0)
    for p in range(n):
        run = np.zeros(K, dtype=bool)
        run[k0[p]:k0[p] + S] = True
        assert np.all(h[p, ~run] == 0.0)
    assert plan["support"] == S and S <= 73 and n * S * 4 <= 32.5 * 1024
    assert plan["k0"].dtype == np.int32 and np.array_equal(plan["k0"], k0)
    assert plan["taps"].dtype == np.float32 and plan["taps"].shape == (n, S)
    # C's sin / cos and numpy's may differ in the last float64 bit: one float32 ulp
    d = np.abs(plan["taps"].astype(np.float64) - c.astype(np.float64))
    assert np.all(d <= 2.0 ** -23 * np.abs(c.astype(np.float64)))
    # the table the compact one stands for is the dense one where the restatement's is not zero, and zero elsewhere
    assert np.array_equal(rr.dense_from_compact(plan["k0"], plan["taps"], K) != 0.0, h != 0.0)


@pytest.mark.parametrize("fs_in,fs_out", rr.PAIRS, ids=lambda v: str(v))
def test_length(fs_in, fs_out):
    o, n, *_ = rr.params(fs_in, fs_out)
    for L in list(range(1, 3 * o + 3)) + [479999, 480000, 480001]:
        assert native.resample_length(fs_in, fs_out, L) == -(-n * L // o)


@pytest.mark.parametrize("fs_in,fs_out", [(8000, 16000), (16000, 8000), (48000, 16000), (44100, 16000), (16000, 44100),
                                          (11025, 16000), (48000, 8000), (22050, 8000)], ids=lambda v: str(v))
def test_restatements_agree(fs_in, fs_out):
    """the two routes round the float64 argument differently, so a tap may differ by one float32 ulp; an indexing
    mistake shows as an error of order 1"""
    o = rr.params(fs_in, fs_out)[0]
    x = np.random.default_rng(o).standard_normal(3 * o + 17)
    a, A = rr.resample_a(x, fs_in, fs_out)
    b, _ = rr.resample_b(x, fs_in, fs_out)
    assert a.shape == b.shape == (rr.length(*rr.params(fs_in, fs_out)[:2], x.shape[0]),)
    assert np.all(np.abs(a - b) <= 2.0 ** -22 * A)
    assert np.abs(a).max() > 0.1


@pytest.mark.parametrize("fs_in,fs_out", rr.PAIRS, ids=lambda v: str(v))
def test_a_sine_stays_a_sine(fs_in, fs_out):
    """a sanity cap on the restatement itself: 440 Hz, 0.25 s, within 1e-3 of the analytic sine at the output rate once
    the first and last 20 ms are excluded (the filter's own pass-band gain error is below 5e-4 on these pairs)"""
    L = fs_in // 4
    x = np.sin(2 * np.pi * 440.0 * np.arange(L) / fs_in)
    y, _ = rr.resample_a(x, fs_in, fs_out)
    want = np.sin(2 * np.pi * 440.0 * np.arange(y.shape[0]) / fs_out)
    e = int(0.02 * fs_out)
    err = float(np.abs(y - want)[e:-e].max())
    print(f"{fs_in} -> {fs_out}: worst deviation from the analytic sine {err:.2e}")
    assert err <= 1e-3


def test_plan_refusals():
    for bad in ((0, 16000), (16000, 0), (-8000, 16000), (16000, -1)):
        with pytest.raises(ValueError, match="sample rates must be positive integers"):
            native.resample_plan(*bad)
        with pytest.raises(ValueError, match="sample rates must be positive integers"):
            native.resample_length(*bad, 100)
        assert native.load_library().dsn_resample_plan(*bad, None, None, None, None, None, None) != 0
        assert native.load_library().dsn_resample_length(*bad, 100) == -1
    with pytest.raises(ValueError, match="sample rates must be positive integers"):
        native.resample_plan(44100.5, 16000)


class _Untouchable:
    """stands in for the loaded library: any use fails the test"""

    def __getattr__(self, name):
        raise AssertionError(f"the library was touched ({name}) before the refusal")


def _engine():
    e = object.__new__(native.Engine)
    e.cfg = native.DsnConfig()
    e.lib, e.ctx, e.n_src, e.latent_dim = _Untouchable(), None, 2, 64
    return e


def test_engine_refusals_before_the_library():
    e = _engine()
    x = torch.zeros(3, 2, 500)
    with pytest.raises(ValueError, match=r"sample rates must be positive integers \(fs_in = 0\)"):
        e.resample(x, 0, 16000)
    with pytest.raises(ValueError, match=r"sample rates must be positive integers \(fs_out = -16000\)"):
        e.resample(x, 8000, -16000)
    with pytest.raises(ValueError, match=r"x must be \[L\], \[C, L\] or \[B, C, L\]"):
        e.resample(torch.zeros(1, 3, 2, 500), 8000, 16000)
    with pytest.raises(ValueError, match=r"C = 0 < 1"):
        e.resample(torch.zeros(3, 0, 500), 8000, 16000)
    with pytest.raises(ValueError, match=r"L = 0 < 1"):
        e.resample(torch.zeros(3, 2, 0), 8000, 16000)
    for bad, msg in (((500, 0, 400), r"lens\[1\] = 0 outside \[1, Lmax = 500\]"),
                     ((500, 400, 501), r"lens\[2\] = 501 outside \[1, Lmax = 500\]"),
                     ((500, 400), r"one sample count per item \(B = 3\)")):
        with pytest.raises(ValueError, match=msg):
            e.resample(x, 8000, 16000, lens=bad)
    with pytest.raises(ValueError, match=r"one sample rate per clip is needed \(2 clips, 1 rates\)"):
        e.to_model_rate([torch.zeros(100), torch.zeros(100)], [8000], 16000)
    with pytest.raises(ValueError, match=r"clip 0 must be \[L\], \[C, L\] or \[1, C, L\]"):
        e.to_model_rate([torch.zeros(2, 2, 100)], 8000, 16000)


class _NoRate:
    """a LatentDiffSep whose configuration has no model.fs; its engine may not be touched"""

    def __new__(cls):
        from ditsep_amd import LatentDiffSep

        m = object.__new__(LatentDiffSep)
        m.fs, m.engine, m.config = None, _engine(), {}
        return m


def test_a_rate_needs_the_models_rate():
    m = _NoRate()
    clip = torch.zeros(2, 1000)
    with pytest.raises(ValueError, match="config.model.fs is missing"):
        m.separate(clip[None], sample_rate=44100)
    with pytest.raises(ValueError, match="config.model.fs is missing"):
        m.separate_batch([clip], sample_rates=44100)
    with pytest.raises(ValueError, match="config.model.fs is missing"):
        m.separate_long([clip], 4096, sample_rates=[44100])
    with pytest.raises(ValueError, match="config.model.fs is missing"):
        m.preprocess_audio_list_for_encoder([clip], 44100)
    with pytest.raises(ValueError, match="config.model.fs is missing"):
        m.preprocess_audio_for_encoder(clip, 44100)
    m.fs = 16000
    with pytest.raises(ValueError, match="a latent has no sample rate"):
        m.separate(torch.zeros(1, 1, 64, 4), latent=True, sample_rate=44100)
    with pytest.raises(ValueError, match="same length of audio_list"):
        m.preprocess_audio_list_for_encoder([clip, clip], [44100])


def test_abi_and_keywords():
    hdr = open(os.path.join(ROOT, "include", "ditsep_hip.h")).read()
    lib = native.load_library()
    for name in NAMES:
        assert re.search(r"\bint %s\(" % name, hdr) and name in native.EXPORTS and hasattr(lib, name)
    assert "int dsn_resample(dsn_ctx* ctx, const float* x, int B, int C, int L, const int32_t* lens, int fs_in, " \
           "int fs_out,\n                 int downmix, float* out, int Lout, void* stream);" in hdr
    assert len(lib.dsn_resample.argtypes) == 12 and len(lib.dsn_resample_plan.argtypes) == 8
    from ditsep_amd import LatentDiffSep

    assert inspect.signature(LatentDiffSep.separate).parameters["sample_rate"].default is None
    assert inspect.signature(LatentDiffSep.separate_batch).parameters["sample_rates"].default is None
    assert inspect.signature(LatentDiffSep.separate_long).parameters["sample_rates"].default is None
    sig = inspect.signature(native.Engine.resample).parameters
    assert sig["lens"].default is None and sig["downmix"].default is False
    # the source file and its plan header are part of the build
    mk = open(os.path.join(ROOT, "ditsep_amd", "csrc", "Makefile")).read()
    assert "resample.hip" in mk and "resample_plan.h" in mk
