"""dsn_bss_eval without a GPU: the two float64 restatements (tests/bss_eval_restatement.py) against each other and,
at one tap, against oracle.metrics.si_bss_eval; the workspace plan in C and in Python; the declaration, the export and
the binding; the refusals the Python wrapper makes itself; evaluate_batches with a stub engine."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from ditsep_amd import native
from oracle.metrics import si_bss_eval
from tests import bss_eval_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(2, 3000, 16), (2, 3000, 64), (3, 700, 7)]
# |(a) - (b)| of a dB value: both are float64 solves of one problem with cond <= 1e4, so they stay inside the bound
# R.bound gives a device value; measured here 4e-13 dB at most over CASES (values up to 33 dB)


@pytest.mark.parametrize("n,L,F", CASES)
def test_restatements_agree(n, L, F):
    ref, est = R.mixtures(1, n, L, seed=n)
    r, e = ref[0].double().numpy(), est[0].double().numpy()
    a, b = R.normal(r, e, F), R.lstsq(r, e, F)
    assert a["cond"] <= 1e4
    for k in ("sdr_pairs", "sir_pairs", "sar_j"):
        d = np.abs(a[k] - b[k])
        print(n, L, F, k, "max |a - b| = %.3g dB" % d.max(), "cond = %.3g" % a["cond"])
        assert np.all(d <= R.bound(a[k], a["cond"], L, F))
    # the assigned estimate differs from the identity for nobody here: the mixing is diagonally dominant
    assert R.choose(a)[3].tolist() == list(range(n))


@pytest.mark.parametrize("perm_by", ["sir", "sdr"])
def test_one_tap_is_si_bss_eval(perm_by):
    ref, est = R.mixtures(3, 3, 500, seed=5)
    est = est[:, [1, 2, 0]]                                  # the identity loses
    want = si_bss_eval(ref, est, perm_by=perm_by, clamp_db=100.0)
    for b in range(3):
        r, e = ref[b].double().numpy(), est[b].double().numpy()
        for tables in (R.normal(r, e, 1, clamp_db=100.0), R.lstsq(r, e, 1, clamp_db=100.0)):
            sdr, sir, sar, perm = R.choose(tables, perm_by)
            assert perm.tolist() == want[3][b].tolist() == [2, 0, 1]
            for got, w in zip((sdr, sir, sar), want):
                assert np.abs(got - w[b].numpy()).max() <= 1e-9


def test_choose_is_lexicographic_and_strict():
    t = {"sdr_pairs": np.zeros((3, 3)), "sir_pairs": np.zeros((3, 3)), "sar_j": np.arange(3.0)}
    assert R.choose(t)[3].tolist() == [0, 1, 2]              # all keys tie: the first candidate stays
    t["sdr_pairs"][0, 1] = t["sdr_pairs"][1, 0] = 1.0
    assert R.choose(t, "sdr")[3].tolist() == [1, 0, 2] and R.choose(t, "sir")[3].tolist() == [0, 1, 2]
    assert R.choose(t, perm=[2, 1, 0])[2].tolist() == [2.0, 1.0, 0.0]


def c_plan(B, n, L, F, budget):
    lib = native.load_library()
    t, M, ipc, ws = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int64()
    rc = lib.dsn_bss_eval_plan(B, n, L, F, budget, ctypes.byref(t), ctypes.byref(M), ctypes.byref(ipc), ctypes.byref(ws))
    return rc, (t.value, M.value, ipc.value, ws.value)


def test_plan_matches_library():
    for B in (1, 3, 64):
        for n in (1, 2, 4):
            for L, F in ((20, 33), (4096, 1), (4097, 64), (64000, 512)):
                one = native.bss_eval_plan(1, n, L, F)["per_item_bytes"]
                for budget in (0, one, 2 * one + 5, 1 << 40):
                    p = native.bss_eval_plan(B, n, L, F, budget)
                    rc, got = c_plan(B, n, L, F, budget)
                    assert rc == 0
                    assert got == (p["tiles"], p["M"], p["items_per_chunk"], p["workspace_bytes"])
                    assert p["M"] == n * F and p["tiles"] == -(-L // 4096)
                    if budget == one:
                        assert p["items_per_chunk"] == 1
                    if budget == 2 * one + 5:
                        assert p["items_per_chunk"] == min(2, B)
                    if budget == 0:
                        assert p["items_per_chunk"] == min(B, (512 << 20) // one)
                assert c_plan(B, n, L, F, one - 1)[0] == -1
                with pytest.raises(ValueError, match="smaller than one item"):
                    native.bss_eval_plan(B, n, L, F, one - 1)
    # the default budget holds the C2 evaluation batch (64 x 2 x 4 s, 512 taps) in one chunk and splits it at n = 4
    assert native.bss_eval_plan(64, 2, 64000, 512)["items_per_chunk"] == 64
    assert native.bss_eval_plan(64, 4, 64000, 512)["items_per_chunk"] < 64
    for bad in ((0, 2, 10, 4, 0), (1, 0, 10, 4, 0), (1, 5, 10, 4, 0), (1, 2, 0, 4, 0), (1, 2, 10, 0, 0),
                (1, 2, 10, 513, 0), (1, 2, 10, 4, -1)):
        assert c_plan(*bad)[0] == -1
        with pytest.raises(ValueError):
            native.bss_eval_plan(*bad)


def test_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "ditsep_hip.h")).read()
    lib = native.load_library()
    for name in ("dsn_bss_eval", "dsn_bss_eval_plan"):
        assert re.search(r"\bint %s\(" % name, hdr) and name in native.EXPORTS and hasattr(lib, name)
    m = re.search(r"\bint\s+dsn_bss_eval\s*\(([^)]*)\)\s*;", hdr)
    names = [re.findall(r"\w+", p)[-1] for p in m.group(1).split(",")]
    assert names == ["ctx", "ref", "est", "B", "n", "L", "lens", "perm", "opts", "out", "stream"]
    vp, ci = ctypes.c_void_p, ctypes.c_int
    assert list(lib.dsn_bss_eval.argtypes) == [vp, vp, vp, ci, ci, ci, ctypes.POINTER(ctypes.c_int32),
                                               ctypes.POINTER(ci), ctypes.POINTER(native.DsnBssEvalOpts),
                                               ctypes.POINTER(native.DsnBssEvalOut), vp]
    for struct in (native.DsnBssEvalOpts, native.DsnBssEvalOut):
        s = re.search(r"typedef\s+struct\s+%s\s*\{(.*?)\}\s*%s\s*;" % (struct.__name__, struct.__name__), hdr, re.S)
        body = re.sub(r"/\*.*?\*/", "", s.group(1), flags=re.S)
        fields = [nm for decl in body.split(";") for nm in re.findall(r"\*?\s*(\w+)\s*(?:,|$)", decl.strip())]
        assert fields == [f[0] for f in struct._fields_]
    assert "no zero_mean option" in hdr and "no conjugate-gradient solver" in hdr
    src = open(os.path.join(ROOT, "ditsep_amd", "csrc", "Makefile")).read()
    assert "bss_eval.hip" in src


def test_wrapper_refusals():
    ok = (2, 2, 100)
    chk = native.check_bss_eval
    plan, by, lens, perm = chk(ok, ok, filter_length=16, perm=[[1, 0], [0, 1]], lens=[100, 7])
    assert (plan["M"], by, lens, perm) == (32, 1, [100, 7], [1, 0, 0, 1])
    for kw, match in (({"filter_length": 0}, "filter_length = 0"), ({"filter_length": 513}, "filter_length = 513"),
                      ({"load_diag": -1e-9}, "load_diag"), ({"load_diag": float("nan")}, "load_diag"),
                      ({"lens": [100, 0]}, r"lens\[1\] = 0"), ({"lens": [101, 5]}, r"lens\[0\] = 101"),
                      ({"lens": [5]}, "one sample count per item"), ({"perm": [[0, 1], [2, 0]]}, r"perm\[2\] = 2"),
                      ({"perm": [[0, -1], [1, 0]]}, r"perm\[1\] = -1"), ({"perm": [0, 1]}, "B\\*n = 4"),
                      ({"perm_by": "sar"}, "perm_by"), ({"workspace_budget": 100}, "smaller than one item"),
                      ({"workspace_budget": -1}, "workspace_budget")):
        with pytest.raises(ValueError, match=match):
            chk(ok, ok, **kw)
    with pytest.raises(ValueError, match=r"n = 5 outside \[1, 4\]"):
        chk((1, 5, 10), (1, 5, 10))
    with pytest.raises(ValueError, match="both be"):
        chk(ok, (2, 2, 99))


def _summary(evaluate, results):
    import json
    import tempfile

    with tempfile.TemporaryDirectory() as d:
        evaluate.write_results(os.path.join(d, "r.json"), results)
        return json.load(open(os.path.join(d, "r_summary.json")))


def test_evaluate_batches_keys(monkeypatch):
    """bss_eval=True adds "sdr", "sir", "sar" last, scored on the record's SI-SIR perm, on the dense and the list
    route; without it nothing new is called and the records are what they were."""
    from ditsep_amd import evaluate

    calls = []

    class Eng:
        device = torch.device("cpu")

        def si_bss_eval(self, target, est, perm_by, clamp_db, lens=None):
            B, n = target.shape[:2]
            z = torch.zeros(B, n)
            return z, z + 1, z + 2, torch.arange(n).flip(0).expand(B, n)

        def bss_eval(self, ref, est, *, filter_length, perm, lens=None):
            calls.append((tuple(ref.shape), filter_length, perm.tolist(), lens))
            B, n = ref.shape[:2]
            t = torch.arange(B * n, dtype=torch.float64).reshape(B, n)
            return t, t + 100, t + 200, perm

        def encode_ragged(self, mixes, vae_noise, seed, codec):
            return torch.zeros(len(mixes), 2, 4), [2] * len(mixes)

        def decode_ragged(self, x, frames, lens, codec):
            return [torch.zeros(2, l) for l in lens]

    class Model:
        engine, config, sde = Eng(), {"model": {"sampler": {"N": 2}}}, type("Sde", (), {"N": 2})

        def encode(self, mix, target, seed):
            return mix, None

        def get_pc_sampler(self, *a, **k):
            return lambda: (torch.zeros(2, 2, 8), 4)

        def decode(self, x, L):
            return x

    keys = ["batch_idx", "si_sdr", "si_sir", "si_sar", "pesq", "stoi", "nfe", "runtime", "len_s", "perm"]
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: None)
    dense = [(torch.zeros(2, 1, 8), torch.zeros(2, 2, 8))]
    ragged = [([torch.zeros(1, 8), torch.zeros(1, 6)], [torch.zeros(2, 8), torch.zeros(2, 6)])]
    for batches in (dense, ragged):
        plain = evaluate.evaluate_batches(Model(), batches, fs=8000)
        assert not calls and all(list(r) == keys for r in plain.values())
        assert "bss_eval_impl" not in _summary(evaluate, plain)
    res = evaluate.evaluate_batches(Model(), dense, fs=8000, bss_eval=True)
    assert calls == [((2, 2, 8), 512, [[1, 0], [1, 0]], None)]
    assert all(list(r) == keys + ["sdr", "sir", "sar"] for r in res.values())
    assert res[1]["sdr"] == [2.0, 3.0] and res[1]["sir"] == [102.0, 103.0] and res[0]["sar"] == [200.0, 201.0]
    text = _summary(evaluate, res)["bss_eval_impl"]
    assert "native" in text and "unpinned" in text and "fast_bss_eval" in text and "mir_eval" in text
    calls.clear()
    res = evaluate.evaluate_batches(Model(), ragged, fs=8000, bss_eval=True, bss_filter_length=64)
    assert calls == [((2, 2, 8), 64, [[1, 0], [1, 0]], [8, 6])]
    assert all(list(r) == keys + ["sdr", "sir", "sar"] for r in res.values()) and res[1]["sar"] == [202.0, 203.0]
