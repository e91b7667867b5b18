"""Time the loudness measurement (Engine.loudness, dsn_loudness) and what `loudness=True` costs a folder of files (one
MI355X, inputs drawn once, seeded; the protocol of scripts/resample_time.py).
  rows_16k        128 x 1 x 4 s at 16 kHz
  rows_44k1       128 x 2 x 4 s at 44.1 kHz
  ragged_mixed    64 items of 2 - 4 s, mono and stereo, at 8, 16, 22.05, 44.1 and 48 kHz in one call
  long_48k        one mono item of 30 min at 48 kHz (little to run side by side in the pass that carries the state)
For each, with and without the true peak: milliseconds per call and the algorithmic bytes (every sample read once for
the loudness, once more for the peaks) per second; and the same definition on the host -- the samples copied back,
scipy.signal.lfilter and numpy framing (tests/loudness_restatement.py in float64), one item per thread, 16 threads;
loudness only.  The device figures are call times on data that stays resident between the calls of a run.
  separate_files  LatentDiffSep.separate_files (full-size DiT and Oobleck, fp16, graphs on, synthetic weights) on 64
                  stereo s16 clips of 4 s at 44.1 kHz (the clips of scripts/files_time.py) with loudness=True against
                  the same call without it.
HIP events around runs of `--reps` calls; 3 warm-up runs, then the median of 5, with the runs listed.
Prints one JSON line; --out also writes it to a file."""
import argparse
import json
import os
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from ditsep_amd import native, synthetic, wavio  # noqa: E402
from scripts.ragged_time import N_STEPS, median_ms  # noqa: E402
from scripts.resample_time import full_size_model  # noqa: E402

HOST_THREADS = 16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--skip-model", action="store_true", help="the measurement calls only")
    ap.add_argument("--skip-long", action="store_true", help="without the 30 min item")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("loudness_time.py measures on the GPU; none is available")
    from tests import loudness_restatement as lr

    eng = native.Engine(score_kind=native.SCORE_NONE, vae_has_encoder=False, vae_has_decoder=False)
    eng.finalize()
    dev = eng.device
    g = torch.Generator().manual_seed(2024)
    res = {"warmup": a.warmup, "iters": a.iters, "reps": a.reps, "host_threads": HOST_THREADS}

    def timed(name, x, rates, lens=None, channels=None, reps=a.reps):
        B, Cn, L = x.shape
        rates = [rates] * B if isinstance(rates, int) else rates
        ln, ch = lens or [L] * B, channels or [Cn] * B
        samples = float(sum(v * c for v, c in zip(ln, ch)))
        rec = dict(shape=[B, Cn, L], rates=sorted(set(rates)), samples=samples)
        for key, tp in (("with_true_peak", True), ("loudness_only", False)):
            def many():
                for _ in range(reps):
                    eng.loudness(x, rates, lens, channels, true_peak=tp)
            ms, times = median_ms(many, a.warmup, a.iters)
            nbytes = 4.0 * samples * (3 if tp else 2)
            rec[key] = dict(ms=round(ms / reps, 4), runs_ms=[round(t / reps, 4) for t in times],
                            algorithmic_bytes=nbytes, gbytes_per_s=round(nbytes / (ms / reps) * 1e-6, 1))
        got = eng.loudness(x, rates, lens, channels, true_peak=False)["loudness"]

        def host_item(args):
            xb, fs = args
            return lr.measure(xb, fs, true_peak=False)["loudness"]

        def host():
            xs = x.cpu().numpy()
            with ThreadPoolExecutor(HOST_THREADS) as pool:
                return list(pool.map(host_item, [(xs[b, :ch[b], :ln[b]], rates[b]) for b in range(B)]))

        t0 = time.perf_counter()
        want = host()
        rec["host_ms"] = round(1e3 * (time.perf_counter() - t0), 2)
        rec["host_over_device"] = round(rec["host_ms"] / rec["loudness_only"]["ms"], 1)
        rec["max_abs_diff_lu"] = max(abs(p - q) for p, q in zip(got.tolist(), want) if q != float("-inf"))
        res[name] = rec
        print(f"# {name}: {rec}", file=sys.stderr, flush=True)

    timed("rows_16k", (0.1 * torch.randn((128, 1, 4 * 16000), generator=g)).to(dev), 16000)
    timed("rows_44k1", (0.1 * torch.randn((128, 2, 4 * 44100), generator=g)).to(dev), 44100)
    pool = [8000, 16000, 22050, 44100, 48000]
    rates = [pool[i % len(pool)] for i in range(64)]
    lens = [int(torch.randint(2 * r, 4 * r + 1, (1,), generator=g)) for r in rates]
    chans = [1 + (i // len(pool)) % 2 for i in range(64)]
    timed("ragged_mixed", (0.1 * torch.randn((64, 2, max(lens)), generator=g)).to(dev), rates, lens, chans)
    if not a.skip_long:
        timed("long_48k", (0.1 * torch.randn((1, 1, 30 * 60 * 48000), generator=g)).to(dev), 48000, reps=2)
    eng.close()

    if not a.skip_model:
        RATE, SECONDS, B = 44100, 4, 64
        model = full_size_model()
        src = synthetic.synthetic_sources(B, 2, SECONDS * RATE, RATE, seed=1234).sum(1)
        src = 0.5 * src / src.abs().amax()
        stereo = torch.stack([src, 0.9 * src.roll(3, dims=-1)], dim=1)
        pcm = torch.round(stereo * 2 ** 15).clamp(-2 ** 15, 2 ** 15 - 1).to(torch.int16)
        with tempfile.TemporaryDirectory() as tmp:
            paths = []
            for b in range(B):
                paths.append(os.path.join(tmp, f"clip{b:03d}.wav"))
                wavio.write_wav(paths[-1], pcm[b].T.contiguous().numpy().tobytes(), RATE, 2, "s16")
            out = os.path.join(tmp, "out")
            kw = dict(seed=7, codec="padded", batch=B)
            on_ms, on_runs = median_ms(lambda: model.separate_files(paths, out, loudness=True, **kw), a.warmup, a.iters)
            off_ms, off_runs = median_ms(lambda: model.separate_files(paths, out, **kw), a.warmup, a.iters)
            recs = model.separate_files(paths, out, loudness=True, **kw)
        res["separate_files"] = dict(items=B, seconds=SECONDS, rate=RATE, N=N_STEPS, with_loudness_ms=round(on_ms, 2),
                                     with_loudness_runs_ms=[round(t, 2) for t in on_runs], without_ms=round(off_ms, 2),
                                     without_runs_ms=[round(t, 2) for t in off_runs],
                                     feature_ms=round(on_ms - off_ms, 2),
                                     feature_share=round((on_ms - off_ms) / off_ms, 4),
                                     gain_db_range=[round(min(r["gain_db"][0] for r in recs), 2),
                                                    round(max(r["gain_db"][0] for r in recs), 2)])
        print(f"# separate_files: {res['separate_files']}", file=sys.stderr, flush=True)
        model.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
