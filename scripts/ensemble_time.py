"""Time the ensemble combine (Engine.ensemble_combine, dsn_ensemble_combine) and what `samples=K` costs a separation
call (one MI355X, inputs drawn once, seeded).
  combine   1 item x K in {4, 8, 16} x 2 sources x 4 s at 16 kHz and 64 items x K = 4, modes mean and median, with the
            mixture: milliseconds per call and the algorithmic bytes ((K n + 1) L 4 read by the Gram, K n L 4 read and
            n L 4 written by the gather) per second -- at these sizes the data fits the Infinity Cache, so these are call
            times, not HBM rates --, beside the same definition written with torch ops on the same GPU: a float64
            einsum Gram, the permutation search on the host (tests/ensemble_restatement.py's), gather, mean / median.
  samples   LatentDiffSep.separate (full-size DiT and Oobleck, fp16, graphs on) of one 4 s mixture with samples = K in
            {1, 2, 4, 8, 16} against samples=None: what K draws cost against K calls.
HIP events around whole calls; 3 warm-up runs, then the median of 5 timed runs, with the runs listed.  A combine call is
short, so a timed run is `--reps` calls back to back and the figure is per call.
Prints one JSON line; --out also writes it to a file."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from ditsep_amd import native, synthetic  # noqa: E402
from scripts.ragged_time import FS, median_ms  # noqa: E402
from scripts.resample_time import full_size_model  # noqa: E402
from tests import ensemble_restatement as er  # noqa: E402


def torch_combine(cands, mix, mode):
    """the definition with torch ops: cands [B, K, n, L], mix [B, L] -> out [B, n, L]"""
    B, K, n, L = cands.shape
    rows = torch.cat([cands.reshape(B, K * n, L), mix[:, None]], dim=1).double()
    G = torch.einsum("bpt,bqt->bpq", rows, rows).cpu().numpy()
    perm = torch.stack([torch.from_numpy(er.align(G[b], K, n)[0]) for b in range(B)]).to(cands.device)
    aligned = torch.gather(cands, 2, perm[..., None].expand(B, K, n, L))
    if mode == "mean":
        return aligned.mean(dim=1)
    s = aligned.sort(dim=1).values
    return s[:, K // 2] if K % 2 else (s[:, K // 2 - 1] + s[:, K // 2]) * 0.5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--skip-model", action="store_true", help="the combine workloads only")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ensemble_time.py measures on the GPU; none is available")
    eng = native.Engine(score_kind=native.SCORE_NONE, vae_has_encoder=False, vae_has_decoder=False)
    eng.finalize()
    dev, SECONDS, n = eng.device, 4, 2
    L = SECONDS * FS
    g = torch.Generator().manual_seed(2026)
    res = {"seconds": SECONDS, "sources": n, "warmup": a.warmup, "iters": a.iters, "reps": a.reps, "combine": {}}

    def run(fn, reps):
        def many():
            for _ in range(reps):
                fn()
        ms, times = median_ms(many, a.warmup, a.iters)
        return ms / reps, [round(t / reps, 4) for t in times]

    for B, K in ((1, 4), (1, 8), (1, 16), (64, 4)):
        src = 0.1 * torch.randn((B, 1, n, L), generator=g)
        order = torch.stack([torch.stack([torch.randperm(n, generator=g) for _ in range(K)]) for _ in range(B)])
        cands = torch.gather(src.expand(B, K, n, L) + 0.03 * torch.randn((B, K, n, L), generator=g), 2,
                             order[..., None].expand(B, K, n, L)).contiguous().to(dev)
        mix = src[:, 0].sum(dim=1).to(dev)
        for mode in ("mean", "median"):
            nbytes = 4.0 * B * L * ((K * n + 1) + K * n + n)
            ms, times = run(lambda: eng.ensemble_combine(cands, mix, mode=mode), a.reps)
            rec = dict(shape=[B, K, n, L], mode=mode, ms=round(ms, 4), runs_ms=times, algorithmic_bytes=nbytes,
                       gbytes_per_s=round(nbytes / ms * 1e-6, 1))
            try:
                got = eng.ensemble_combine(cands, mix, mode=mode)
                rec["torch_max_abs_diff"] = float((got - torch_combine(cands, mix, mode)).abs().max())
                tms, ttimes = run(lambda: torch_combine(cands, mix, mode), max(1, a.reps // 4))
                rec.update(torch_ms=round(tms, 4), torch_runs_ms=ttimes, torch_over_native=round(tms / ms, 2))
            except Exception as e:                                                  # reported only
                rec["torch_note"] = f"skipped: {type(e).__name__}: {e}"
            res["combine"][f"{B}x{K}x{n}x{SECONDS}s_{mode}"] = rec
            print(f"# combine {B} x {K} {mode}: {rec}", file=sys.stderr, flush=True)
    eng.close()

    if not a.skip_model:
        model = full_size_model()
        mix = synthetic.synthetic_sources(1, 2, L, FS, seed=1234).sum(1, keepdim=True).to(dev)
        base_ms, base_runs = median_ms(lambda: model.separate(mix, seed=7), a.warmup, a.iters)
        res["samples"] = {"none": dict(ms=round(base_ms, 2), runs_ms=[round(t, 2) for t in base_runs])}
        for K in (1, 2, 4, 8, 16):
            ms, runs = median_ms(lambda: model.separate(mix, seed=7, samples=K), a.warmup, a.iters)
            res["samples"][str(K)] = dict(ms=round(ms, 2), runs_ms=[round(t, 2) for t in runs],
                                          over_one_call=round(ms / base_ms, 2),
                                          share_of_K_calls=round(ms / (K * base_ms), 3))
            print(f"# samples {K}: {res['samples'][str(K)]}", file=sys.stderr, flush=True)
        model.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
