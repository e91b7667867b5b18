"""Time Engine.mrstft_loss (dsn_mrstft_loss; seven resolutions, A-weighting, L1) on the C2 evaluation batch (64 x 2
sources, 4 s at 16 kHz) and on one 30 s item, with HIP events around whole calls after a warm-up.  With --reference
DIR (a checkout of the reference) the reference's own PITLoss(MultiResolutionSTFTLoss) + PITLoss(L1) is timed on the
CPU for the same shapes on 16 threads (all permutations, as it runs them); --cpu-only skips the device.
Run it under a time limit (`timeout 300 python scripts/mrstft_time.py`).  Prints one JSON line; --out writes it too."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from ditsep_amd import native, synthetic  # noqa: E402

HOST_THREADS = 16
SHAPES = {"c2_64x2x4s": (64, 2, 4), "1x2x30s": (1, 2, 30)}


def reference_fn(ref_root, fs):
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import make_golden_mrstft as G

    aura, losses = G.load(ref_root, "auraloss"), G.load(ref_root, "losses")
    base = losses.AuralossLoss(G.mrstft(aura, fs, torch.float32), input_key="decoded", target_key="reals", name="m")
    mods = [losses.PITLoss(base, input_key="decoded", target_key="reals", name="pit_mrstft_loss"),
            losses.PITLoss(losses.L1Loss(key_a="reals", key_b="decoded", weight=15.0), input_key="decoded",
                           target_key="reals", name="pit_l1_loss")]
    multi = losses.MultiLoss(mods)
    return lambda x, y: multi({"reals": x, "decoded": y})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reference", default=None)
    ap.add_argument("--cpu-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.set_num_threads(HOST_THREADS)
    fs = 16000
    eng = None if a.cpu_only else native.Engine(score_kind=native.SCORE_NONE, vae_has_encoder=False,
                                                vae_has_decoder=False)
    cpu = reference_fn(a.reference, fs) if a.reference else None
    res = {}
    for name, (B, n, seconds) in SHAPES.items():
        L = seconds * fs
        ref = synthetic.synthetic_sources(B, n, L, fs=fs, seed=7)
        est = ref.flip(1) + 0.1 * torch.randn(ref.shape, generator=torch.Generator().manual_seed(8)) * ref.abs().amax(-1, True)
        row = {"device_ms": None, "reference_cpu_ms_16_threads": None}
        if eng is not None:
            ref_d, est_d = ref.cuda(), est.cuda()
            for _ in range(3):
                out = eng.mrstft_loss(ref_d, est_d, fs, l1_weight=15.0)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.iters):
                eng.mrstft_loss(ref_d, est_d, fs, l1_weight=15.0)
            e1.record()
            torch.cuda.synchronize()
            row["device_ms"] = round(e0.elapsed_time(e1) / a.iters, 3)
            row["device_loss"] = float(out["loss"])
        if cpu is not None:
            with torch.no_grad():
                cpu(ref, est)
                t = time.perf_counter()
                total, _ = cpu(ref, est)
                row["reference_cpu_ms_16_threads"] = round(1e3 * (time.perf_counter() - t), 1)
                row["reference_loss"] = float(total)
        res[name] = row
    if eng is not None:
        eng.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
