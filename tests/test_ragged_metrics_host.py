"""CPU-only: the C-ABI bindings of the ragged metric calls (dsn_si_bss_eval_ragged, dsn_stoi_ragged,
dsn_composite_ragged) against include/ditsep_hip.h, the refusals Engine.si_bss_eval / stoi / composite raise for lens=
before the library is touched, and what evaluate_batches still refuses for a list batch."""
import ctypes
import os
import re

import pytest
import torch

from ditsep_amd import evaluate, native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RAGGED = {
    "dsn_si_bss_eval_ragged": ["ctx", "ref", "est", "B", "n", "L", "lens", "perm_by", "clamp_db", "si_sdr_out",
                               "si_sir_out", "si_sar_out", "perm_out", "stream"],
    "dsn_stoi_ragged": ["ctx", "ref", "est", "B", "n", "L", "lens", "fs", "extended", "perm", "out", "frames_out",
                        "stream"],
    "dsn_composite_ragged": ["ctx", "ref", "est", "B", "n", "L", "lens", "fs", "perm", "pesq", "out", "stream"],
}
DENSE = {"dsn_si_bss_eval_ragged": "dsn_si_bss_eval", "dsn_stoi_ragged": "dsn_stoi",
         "dsn_composite_ragged": "dsn_composite"}


def _c_to_ctypes(param: str):
    """ctypes type of one parameter: device arrays (ref, est) are c_void_p, host arrays typed pointers (the approach of
    tests/test_stoi_host.py, with const int32_t* for lens and the composite call's pesq and out)"""
    param = " ".join(param.split())
    name = re.findall(r"\w+", param)[-1]
    if param.startswith("dsn_ctx*") or param.startswith("void*"):
        return ctypes.c_void_p
    if param.startswith("const float*"):
        return ctypes.POINTER(ctypes.c_float) if name == "pesq" else ctypes.c_void_p
    if param.startswith("float*"):
        return ctypes.POINTER(ctypes.c_float)
    if param.startswith("const int32_t*"):
        return ctypes.POINTER(ctypes.c_int32)
    if param.startswith("const int*") or param.startswith("int*"):
        return ctypes.POINTER(ctypes.c_int)
    if param.startswith("const DsnCompositeOut*"):
        return ctypes.POINTER(native.DsnCompositeOut)
    if param.startswith("int "):
        return ctypes.c_int
    if param.startswith("float "):
        return ctypes.c_float
    raise AssertionError(f"unexpected parameter {param!r}")


def _params(hdr, name):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr)
    assert m, f"{name} is not declared in include/ditsep_hip.h"
    return [p.strip() for p in m.group(1).split(",")]


@pytest.mark.parametrize("name", sorted(RAGGED))
def test_ragged_metric_binding_matches_header(name):
    hdr = open(os.path.join(ROOT, "include", "ditsep_hip.h")).read()
    params = _params(hdr, name)
    names = [re.findall(r"\w+", p)[-1] for p in params]
    assert names == RAGGED[name]
    # the dense call's arguments, L read as Lmax, plus lens
    dense = _params(hdr, DENSE[name])
    assert [p for p in params if not p.startswith("const int32_t* lens")] == dense
    assert name in native.EXPORTS
    lib = native.load_library()
    assert list(getattr(lib, name).argtypes) == [_c_to_ctypes(p) for p in params]


class _Untouchable:
    """stands in for the loaded library: any use fails the test"""

    def __getattr__(self, name):
        raise AssertionError(f"the library was touched ({name}) before the refusal")


def _engine():
    e = object.__new__(native.Engine)
    e.cfg = native.DsnConfig()
    e.lib, e.ctx, e.n_src, e.latent_dim = _Untouchable(), None, 2, 64
    return e


def test_lens_refusals_before_the_library():
    B, n, Lmax = 3, 2, 5000
    ref, est = torch.zeros(B, n, Lmax), torch.zeros(B, n, Lmax)
    e = _engine()
    calls = {"si_bss_eval": lambda lens: e.si_bss_eval(ref, est, lens=lens),
             "stoi": lambda lens: e.stoi(ref, est, 8000, lens=lens),
             "composite": lambda lens: e.composite(ref, est, 8000, lens=lens)}
    for bad, msg in (((5000, 0, 4000), r"lens\[1\] = 0 outside \[1, Lmax = 5000\]"),
                     ((5000, 4000, 5001), r"lens\[2\] = 5001 outside \[1, Lmax = 5000\]"),
                     ((5000, 4000), r"one sample count per item \(B = 3\)")):
        for name, call in calls.items():
            with pytest.raises(ValueError, match=msg):
                call(bad)
    with pytest.raises(ValueError, match=r"item 2 \(lens\[2\] = 299\) is shorter than one frame "
                                         r"\(300 samples needed at fs = 8000\)"):
        e.composite(ref, est, 8000, lens=(5000, 4000, 299))
    with pytest.raises(ValueError, match=r"item 1 \(lens\[1\] = 599\) .* \(600 samples needed at fs = 16000\)"):
        e.composite(ref, est, 16000, lens=(5000, 599, 600))
    # the rule hands back the counts it accepted; one frame plus one hop is enough
    assert native.check_lens((5000, 300, 1), 3, 5000) == [5000, 300, 1]
    assert native.check_lens((5000, 300), 2, 5000, native.composite_min_samples(8000)) == [5000, 300]
    assert native.composite_min_samples(16000) == 600 and native.composite_min_samples(44100) is None


class _NoModel:
    class engine:
        device = "cpu"

    class sde:
        N = 4


@pytest.mark.parametrize("flags", [{"score_loss": True}, {"mrstft": True}, {"score_loss": True, "composite": True}])
def test_list_batches_still_refuse_score_loss_and_mrstft(flags):
    batch = ([torch.zeros(1, 4000), torch.zeros(1, 5000)], [torch.zeros(2, 4000), torch.zeros(2, 5000)])
    with pytest.raises(NotImplementedError) as err:
        evaluate.evaluate_batches(_NoModel(), [batch], 8000, **flags)
    msg = str(err.value)
    assert "score_loss / mrstft" in msg and "composite" not in msg
