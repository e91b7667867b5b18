"""Capture tests/golden/composite.npz from the reference's own src/evaluate/evaluate_covl.py (build container only).

Run:  python scripts/make_golden_composite.py     (exits cleanly when the reference tree is absent)

The reference module is imported as it is, with `sys.modules` stubs for what it names at import time and does not
need for the measures (librosa, pesq, tqdm, utils, evaluate_mp).  Its functions wss, llr and SSNR are called on
float32 arrays -- what librosa.load hands them -- made by tests.composite_restatement.make_items from
synthetic.synthetic_sources (the tests regenerate them by seed; the first 16 samples and the float64 sum of every
input are stored to detect generator drift).  SSNR works in place, so it gets copies.  eval_composite is called too,
with the stubbed pesq returning recorded constants; what pesq was handed (the signals after SSNR removed their means
and rescaled the estimate) is recorded by its first 16 samples and its sum.  Only arrays are stored."""
from __future__ import annotations

import importlib.util
import os
import sys
import time
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import reference_loader as rl  # noqa: E402
from tests import composite_restatement as R  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "composite.npz")
CASES = {k: R.CASES[k] for k in ("fs16k", "fs8k")}
PESQ = [1.3, 1.9, 2.4, 3.1, 3.8, 4.4]      # what the stubbed pesq returns, item by item


def load_reference_module():
    """evaluate_covl.py unmodified; pesq_calls collects what its PESQ() hands to pesq.pesq"""
    pesq_calls = []
    answers = []

    def pesq(rate, ref, deg, mode):
        pesq_calls.append((rate, np.array(ref), np.array(deg), mode))
        return answers.pop(0)

    for name, attrs in {"librosa": {}, "pesq": {"pesq": pesq}, "tqdm": {"tqdm": lambda it, *a, **k: it},
                        "utils": {}, "evaluate_mp": {"summarize": lambda out: {}}}.items():
        m = types.ModuleType(name)
        for k, v in attrs.items():
            setattr(m, k, v)
        sys.modules[name] = m
    path = os.path.join(rl.REF_SRC, "evaluate", "evaluate_covl.py")
    spec = importlib.util.spec_from_file_location("evaluate_covl", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod, pesq_calls, answers


def reference_measures(mod, x: np.ndarray, y: np.ndarray, fs: int):
    """(wss, llr, ssnr per frame as float64 arrays, overall snr) of float32 signals by the reference's functions"""
    assert x.dtype == np.float32 and y.dtype == np.float32
    w = np.array(mod.wss(x, y, fs), dtype=np.float64)
    lv = np.array(mod.llr(x, y, fs), dtype=np.float64)
    snr, seg = mod.SSNR(x.copy(), y.copy(), fs)
    return w, lv, np.array(seg, dtype=np.float64), float(snr)


def main():
    if not rl.available():
        print("reference tree not present: nothing captured")
        return 0
    mod, pesq_calls, answers = load_reference_module()
    out = {}
    for name, (fs, n, L, rows) in CASES.items():
        B = len(rows)
        ref, est = R.make_items(n, L, fs, rows)
        ref, est = ref.numpy(), est.numpy()
        out[f"{name}_shape"] = np.array([fs, B, n, L])
        out[f"{name}_rows"] = np.array(rows)
        out[f"{name}_ref_head"], out[f"{name}_est_head"] = ref[..., :16], est[..., :16]
        out[f"{name}_ref_sum"] = ref.astype(np.float64).sum(-1)
        out[f"{name}_est_sum"] = est.astype(np.float64).sum(-1)
        per = {k: [] for k in ("wss_frames", "llr_frames", "ssnr_frames", "snr", "wss", "llr", "segsnr")}
        t0 = time.perf_counter()
        for b in range(B):
            for i in range(n):
                w, lv, seg, snr = reference_measures(mod, ref[b, i], est[b, i], fs)
                k = int(round(len(w) * 0.95))
                per["wss_frames"].append(w)
                per["llr_frames"].append(lv)
                per["ssnr_frames"].append(seg)
                per["snr"].append(snr)
                per["wss"].append(np.mean(sorted(w)[:k]))
                per["llr"].append(np.mean(sorted(lv)[:k]))
                per["segsnr"].append(np.mean(seg))
        print(f"{name}: the reference took {1e3 * (time.perf_counter() - t0) / (B * n):.0f} ms per item")
        for k, v in per.items():
            out[f"{name}_{k}"] = np.array(v, dtype=np.float64).reshape(B, n, *np.shape(v[0]))
        if fs != 16000:
            continue        # eval_composite is written for 16 kHz
        comp, heads, sums = [], [], []
        for b in range(B):
            for i in range(n):
                answers.append(PESQ[b * n + i])
                res = mod.eval_composite(ref[b, i].copy(), est[b, i].copy())
                comp.append([res["csig"], res["cbak"], res["covl"]])
                rate, pr, pd, mode = pesq_calls.pop()
                assert rate == 16000 and mode == "wb"
                heads.append([pr[:16], pd[:16]])
                sums.append([pr.astype(np.float64).sum(), np.abs(pd.astype(np.float64)).sum()])
        out[f"{name}_pesq"] = np.array(PESQ, dtype=np.float64).reshape(B, n)
        out[f"{name}_composite"] = np.array(comp, dtype=np.float64).reshape(B, n, 3)       # csig, cbak, covl
        out[f"{name}_pesq_in_head"] = np.array(heads, dtype=np.float32).reshape(B, n, 2, 16)
        out[f"{name}_pesq_in_sums"] = np.array(sums, dtype=np.float64).reshape(B, n, 2)    # sum ref, sum |deg|
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT} ({os.path.getsize(OUT) / 1024:.1f} KiB, {len(out)} arrays)")
    return 0


if __name__ == "__main__":
    sys.exit(main())
