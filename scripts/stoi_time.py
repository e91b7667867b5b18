"""Time Engine.stoi (dsn_stoi) on the C2 evaluation shape (64 x 2 sources, 4 s at 16 kHz) and on 16 x 2 x 30 s,
with HIP events around whole calls after a warm-up, next to the float64 CPU restatement (tests/stoi_restatement.py,
timed on a few items and scaled to the batch).  Prints one JSON line; --out also writes it to a file."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from ditsep_amd import native, synthetic  # noqa: E402
from tests import stoi_restatement as R  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--cpu-items", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    eng = native.Engine(score_kind=native.SCORE_NONE, vae_has_encoder=False, vae_has_decoder=False)
    res = {}
    for name, (B, seconds) in {"c2_64x2x4s": (64, 4), "16x2x30s": (16, 30)}.items():
        fs = 16000
        L = seconds * fs
        ref = synthetic.synthetic_sources(B, 2, L, fs=fs, seed=7)
        est = ref + 0.3 * torch.randn(ref.shape, generator=torch.Generator().manual_seed(8)) * ref.abs().amax(-1, True)
        ref_d, est_d = ref.cuda(), est.cuda()
        for ext in (False, True):
            for _ in range(3):
                eng.stoi(ref_d, est_d, fs, extended=ext)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.iters):
                eng.stoi(ref_d, est_d, fs, extended=ext)
            e1.record()
            torch.cuda.synchronize()
            ms = e0.elapsed_time(e1) / a.iters
            t = time.perf_counter()
            for i in range(a.cpu_items):
                R.stoi(ref[i // 2, i % 2].double().numpy(), est[i // 2, i % 2].double().numpy(), fs, ext)
            cpu_ms = 1e3 * (time.perf_counter() - t) / a.cpu_items * B * 2
            res[f"{name}_{'estoi' if ext else 'stoi'}"] = {"device_ms": round(ms, 3),
                                                           "cpu_restatement_ms_scaled": round(cpu_ms, 1)}
    eng.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
