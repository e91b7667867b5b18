"""CPU-only: the float64 restatement of LLR / WSS / segmental SNR (tests/composite_restatement.py) against the
reference's own functions (tests/golden/composite.npz, scripts/make_golden_composite.py), the host-side arithmetic of
the composite measures, and the dsn_composite C-ABI binding."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest

from ditsep_amd import evaluate, native
from tests import composite_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "composite.npz")

# max |restatement - golden| measured on the golden's float32 inputs (fs16k / fs8k, 6 items of 263 frames each).  The
# reference rounds its LPC output and lags to float32 and forms the LLR's quadratic forms in float32 (per-frame LLR
# values of 3e-4 .. 0.84); it removes the means and rescales in float32 before the segmental SNR; its WSS is float64
# like the restatement.  Bounds: 4x the measured maximum, the margin for other seeds.
#                      fs16k     fs8k
#   llr  per frame     5.8e-7    5.9e-7       aggregate  1.7e-8   1.8e-8
#   wss  per frame     4.3e-14   7.1e-14      aggregate  3.6e-15  7.1e-15
#   ssnr per frame     7.7e-6    3.0e-6       aggregate  2.3e-6   4.7e-7     overall snr  2.2e-6  2.7e-6
MEASURED_GOLDEN_FRAME = {"llr": 5.9e-7, "wss": 7.2e-14, "segsnr": 7.7e-6}
MEASURED_GOLDEN_AGG = {"llr": 1.9e-8, "wss": 7.2e-15, "segsnr": 2.3e-6, "snr": 2.7e-6}
TOL_GOLDEN_FRAME = {k: 4 * v for k, v in MEASURED_GOLDEN_FRAME.items()}
TOL_GOLDEN_AGG = {k: 4 * v for k, v in MEASURED_GOLDEN_AGG.items()}
FRAME_KEYS = {"llr": "llr_frames", "wss": "wss_frames", "segsnr": "ssnr_frames"}


@functools.lru_cache(maxsize=None)
def golden_case(name):
    g = np.load(GOLDEN)
    fs, n, L, rows = R.CASES[name]
    assert g[f"{name}_shape"].tolist() == [fs, len(rows), n, L] and g[f"{name}_rows"].tolist() == [list(r) for r in rows]
    ref, est = R.make_items(n, L, fs, rows)
    ref, est = ref.numpy(), est.numpy()
    # generator drift would show here
    assert np.array_equal(ref[..., :16], g[f"{name}_ref_head"]) and np.array_equal(est[..., :16], g[f"{name}_est_head"])
    assert np.array_equal(ref.astype(np.float64).sum(-1), g[f"{name}_ref_sum"])
    assert np.array_equal(est.astype(np.float64).sum(-1), g[f"{name}_est_sum"])
    out = [[R.measures(ref[b, i], est[b, i], fs) for i in range(n)] for b in range(len(rows))]
    return g, ref, est, fs, out


@pytest.mark.parametrize("name", ["fs16k", "fs8k"])
def test_restatement_matches_reference(name):
    g, ref, est, fs, out = golden_case(name)
    bad = []
    for k, fk in FRAME_KEYS.items():
        got = np.array([[o[fk] for o in row] for row in out])
        assert got.shape == g[f"{name}_{fk}"].shape == (3, 2, 263)
        err = float(np.abs(got - g[f"{name}_{fk}"]).max())
        print(f"{name}: {k} per frame max |restatement - reference| = {err:.3e} (bound {TOL_GOLDEN_FRAME[k]:.3e})")
        if not err <= TOL_GOLDEN_FRAME[k]:
            bad.append((fk, err))
    for k in ("llr", "wss", "segsnr", "snr"):
        got = np.array([[o[k] for o in row] for row in out])
        err = float(np.abs(got - g[f"{name}_{k}"]).max())
        print(f"{name}: {k} max |restatement - reference| = {err:.3e} (bound {TOL_GOLDEN_AGG[k]:.3e})")
        if not err <= TOL_GOLDEN_AGG[k]:
            bad.append((k, err))
    assert not bad, bad


def test_composites_match_reference_and_pesq_conditioning():
    g, ref, est, fs, out = golden_case("fs16k")
    for b in range(3):
        for i in range(2):
            o = out[b][i]
            got = R.composites(o["llr"], o["wss"], o["segsnr"], float(g["fs16k_pesq"][b, i]))
            assert np.abs(np.array(got) - g["fs16k_composite"][b, i]).max() < 1e-6
            # what the reference handed to its PESQ call: evaluate.condition_for_pesq reproduces it bit for bit
            r, e = evaluate.condition_for_pesq(ref[b, i], est[b, i])
            assert r.dtype == e.dtype == np.float32
            assert np.array_equal(r[:16], g["fs16k_pesq_in_head"][b, i, 0])
            assert np.array_equal(e[:16], g["fs16k_pesq_in_head"][b, i, 1])
            assert r.astype(np.float64).sum() == g["fs16k_pesq_in_sums"][b, i, 0]
            assert np.abs(e.astype(np.float64)).sum() == g["fs16k_pesq_in_sums"][b, i, 1]


def test_trimmed_count_is_pythons_round():
    lib = ctypes.CDLL(None)
    lib.nearbyint.restype = ctypes.c_double
    lib.nearbyint.argtypes = [ctypes.c_double]
    for F in range(1, 4001):
        assert R.trimmed_count(F) == round(F * 0.95) == int(lib.nearbyint(F * 0.95)), F
    assert R.trimmed_count(10) == 10 and R.trimmed_count(30) == 28 and R.trimmed_count(1) == 1
    assert round(9.5) == 10 and round(28.5) == 28            # half to even


@pytest.mark.parametrize("fs,L,F", [(16000, 32061, 263), (16000, 32040, 263), (16000, 32039, 262), (16000, 600, 1),
                                    (16000, 599, 0), (16000, 480, 0), (8000, 16061, 263), (8000, 299, 0),
                                    (8000, 300, 1), (16000, 30 * 16000, 3996)])
def test_frame_count(fs, L, F):
    assert R.num_frames(L, fs) == F
    win, hop, _, _ = R.geometry(fs)
    assert F == max(L // hop - win // hop, 0)               # the integer form dsn_composite uses
    if F:
        assert (F - 1) * hop + win <= L                     # the last frame lies inside the signal
        assert R.frames(np.zeros(L), fs).shape == (F, win)


def test_geometry_and_band_table():
    assert R.geometry(16000) == (480, 120, 1024, 16) and R.geometry(8000) == (240, 60, 512, 10)
    for fs in (8000, 16000):
        nfft = R.geometry(fs)[2]
        tab = R.band_table(fs)
        assert len(tab) == 25
        for (s, w), fc in zip(tab, R.CENT_FREQ):
            assert 0 <= s and s + w.size <= nfft // 2 and w.min() > np.exp(-30.0 / (2 * 2.303))
            assert s <= int(fc / (fs / 2) * (nfft // 2)) < s + w.size


@pytest.mark.parametrize("fs", [8000, 16000])
def test_identical_signals(fs):
    x = R.make_items(1, 2 * fs, fs, ((5, 6),))[0][0, 0].numpy()
    m = R.measures(x, x.copy(), fs)
    assert np.all(m["llr_frames"] == 0.0) and np.all(m["wss_frames"] == 0.0) and np.all(m["ssnr_frames"] == 35.0)
    assert m["llr"] == 0.0 and m["wss"] == 0.0 and m["segsnr"] == 35.0


def test_silence_and_zero_estimate():
    x = R.make_items(1, 8000, 16000, ((5, 6),))[0][0, 0].numpy()
    z = np.zeros_like(x)
    m = R.measures(z, z, 16000)
    assert np.all(m["llr_frames"] == 0.0) and np.all(m["wss_frames"] == 0.0)
    m = R.measures(x, z, 16000)         # the reference rescales by max|est| = 0: NaN; LLR and WSS read the raw signals
    assert np.isnan(m["segsnr"]) and np.isnan(m["snr"]) and np.isfinite(m["llr"]) and np.isfinite(m["wss"])
    assert R.wss_slope_margin_db(z, z, 16000) == np.inf


def test_composite_formulas_and_clip():
    assert R.composites(0.0, 0.0, 0.0, 0.0) == (3.093, 1.634, 1.594)
    c = R.composites(0.25, 30.0, 5.0, 2.5)
    assert abs(c[0] - (3.093 - 1.029 * 0.25 + 0.603 * 2.5 - 0.009 * 30.0)) < 1e-15
    assert abs(c[1] - (1.634 + 0.478 * 2.5 - 0.007 * 30.0 + 0.063 * 5.0)) < 1e-15
    assert abs(c[2] - (1.594 + 0.805 * 2.5 - 0.512 * 0.25 - 0.007 * 30.0)) < 1e-15
    assert R.composites(0.0, 0.0, 35.0, 4.5) == (5.0, 5.0, 5.0)
    assert R.composites(3.0, 200.0, -10.0, 1.0) == (1.0, 1.0, 1.0)
    c = R.composites(0.1, 10.0, float("nan"), 2.0)
    assert np.isnan(c[1]) and np.isfinite(c[0]) and np.isfinite(c[2])


def _c_to_ctypes(param: str):
    """ctypes type of one dsn_composite parameter: device arrays are c_void_p, host arrays typed pointers."""
    param = " ".join(param.split())
    if param.startswith("const DsnCompositeOut*"):
        return ctypes.POINTER(native.DsnCompositeOut)
    if param.startswith("dsn_ctx*") or param.startswith("void*"):
        return ctypes.c_void_p
    if param.startswith("const float* ref") or param.startswith("const float* est"):
        return ctypes.c_void_p
    if param.startswith("const float*"):
        return ctypes.POINTER(ctypes.c_float)
    if param.startswith("const int*"):
        return ctypes.POINTER(ctypes.c_int)
    if param.startswith("int "):
        return ctypes.c_int
    raise AssertionError(f"unexpected parameter {param!r}")


def test_dsn_composite_binding_matches_header():
    hdr = open(os.path.join(ROOT, "include", "ditsep_hip.h")).read()
    m = re.search(r"\bint\s+dsn_composite\s*\(([^)]*)\)\s*;", hdr)
    assert m, "dsn_composite is not declared in include/ditsep_hip.h"
    params = [p.strip() for p in m.group(1).split(",")]
    names = [re.findall(r"\w+", p)[-1] for p in params]
    assert names == ["ctx", "ref", "est", "B", "n", "L", "fs", "perm", "pesq", "out", "stream"]
    s = re.search(r"typedef\s+struct\s+DsnCompositeOut\s*\{(.*?)\}\s*DsnCompositeOut\s*;", hdr, re.S)
    assert s, "DsnCompositeOut is not declared in include/ditsep_hip.h"
    fields = []
    for decl in re.sub(r"/\*.*?\*/", "", s.group(1), flags=re.S).split(";"):
        decl = decl.strip()
        if decl:
            ctype = ctypes.c_float if decl.startswith("float") else ctypes.c_int
            assert decl.startswith(("float", "int"))
            fields += [(nm, ctypes.POINTER(ctype)) for nm in re.findall(r"\*\s*(\w+)", decl)]
    assert fields == list(native.DsnCompositeOut._fields_)
    assert "dsn_composite" in native.EXPORTS
    lib = native.load_library()
    assert list(lib.dsn_composite.argtypes) == [_c_to_ctypes(p) for p in params]
