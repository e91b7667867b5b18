"""Time Engine.composite (dsn_composite) on the C2 evaluation shape (64 x 2 sources, 4 s at 16 kHz) and on one 30 s
item, with HIP events around whole calls after a warm-up, next to the reference's own wss + llr + SSNR on the CPU
(loaded as scripts/make_golden_composite.py loads them; a few items on one thread, scaled to the batch spread over 16
host threads, the reference's process pool) or, without the reference tree, next to the float64 restatement.
--cpu-only times the CPU side alone, for a host that has the reference tree and no GPU.
Prints one JSON line; --out also writes it to a file."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from ditsep_amd import native, synthetic  # noqa: E402
from tests import composite_restatement as R  # noqa: E402

HOST_THREADS = 16


def cpu_item_fn():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import make_golden_composite as G

    if G.rl.available():
        mod, _, _ = G.load_reference_module()
        return "reference", lambda x, y, fs: G.reference_measures(mod, x, y, fs)
    return "restatement", lambda x, y, fs: R.measures(x, y, fs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--cpu-items", type=int, default=2)
    ap.add_argument("--cpu-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    eng = None if a.cpu_only else native.Engine(score_kind=native.SCORE_NONE, vae_has_encoder=False,
                                                vae_has_decoder=False)
    which, cpu_item = cpu_item_fn()
    res = {"cpu": which}
    for name, (B, n, seconds) in {"c2_64x2x4s": (64, 2, 4), "1x1x30s": (1, 1, 30)}.items():
        fs = 16000
        L = seconds * fs
        ref = synthetic.synthetic_sources(B, n, L, fs=fs, seed=7)
        est = ref + 0.3 * torch.randn(ref.shape, generator=torch.Generator().manual_seed(8)) * ref.abs().amax(-1, True)
        ms = None
        if eng is not None:
            ref_d, est_d = ref.cuda(), est.cuda()
            for _ in range(3):
                eng.composite(ref_d, est_d, fs)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.iters):
                eng.composite(ref_d, est_d, fs)
            e1.record()
            torch.cuda.synchronize()
            ms = round(e0.elapsed_time(e1) / a.iters, 3)
        items = min(a.cpu_items, B * n)
        t = time.perf_counter()
        for i in range(items):
            cpu_item(ref[i // n, i % n].numpy(), est[i // n, i % n].numpy(), fs)
        per_item = 1e3 * (time.perf_counter() - t) / items
        res[name] = {"device_ms": ms, "cpu_ms_per_item": round(per_item, 1),
                     "cpu_ms_batch_16_threads": round(per_item * -(-B * n // HOST_THREADS), 1)}
    if eng is not None:
        eng.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
