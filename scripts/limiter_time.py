"""Time the true-peak look-ahead limiter (Engine.limiter_curve / apply_curve, dsn_limiter_curve / dsn_apply_curve) and
what `limit=True` costs a folder of files (one MI355X, inputs drawn once, seeded; the protocol of
scripts/resample_time.py).
  rows_16k        128 x 1 x 4 s at 16 kHz
  rows_44k1       128 x 2 x 4 s at 44.1 kHz
  ragged_mixed    64 items of 2 - 4 s, mono and stereo, at 8, 16, 22.05, 44.1 and 48 kHz in one call (the batch of
                  scripts/loudness_time.py)
  long_48k        one mono item of 30 min at 48 kHz
Every row is its own group; look-ahead 5 ms, ceiling -1 dBTP.  Each workload twice: "under" -- nothing exceeds the
ceiling, every tile takes the copy path -- and "reduced" -- a peak every 16 W samples, so that about a quarter of the
samples lie within 2 W of one and are reduced (the fraction the device counted is reported).  For each: milliseconds
for the curve call and for curve + apply, and the algorithmic bytes (curve: every sample read once, the curve written
once; apply: samples and curve read, output written) per second; and the same definition in torch on the same GPU --
conv1d with the four phases for the interpolation, -max_pool1d(-r) for the hold, conv1d for the smoothing, per distinct
rate on the padded rows -- with the largest difference between the two curves.  The device figures are call times on
data that stays resident between the calls of a run; the curve call includes its table uploads and its read-back of
the statistics.
  separate_files  LatentDiffSep.separate_files (full-size DiT and Oobleck, fp16, graphs on, synthetic weights) on 64
                  stereo s16 clips of 4 s at 44.1 kHz (the clips of scripts/files_time.py) with loudness=-14 and
                  limit=True against the same call with loudness=-14 alone, alternating.
HIP events around runs of `--reps` calls; 3 warm-up runs, then the median of 5, with the runs listed.
Prints one JSON line; --out also writes it to a file."""
import argparse
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from ditsep_amd import native, synthetic, wavio  # noqa: E402
from scripts.ragged_time import N_STEPS, median_ms  # noqa: E402
from scripts.resample_time import full_size_model  # noqa: E402

MS = 5.0
CEIL = float(np.float32(10.0 ** (-1.0 / 20.0)))


def torch_curve(x, W, c, taps, k0, width):
    """the definition with torch's own kernels: x [R, C, L] of one rate, every row a group -> g [R, L]"""
    R, Cn, L = x.shape
    S = taps.shape[1]
    lo = min(k0) - width
    hi = max(k0) - width + S - 1
    w = torch.zeros((4, 1, hi - lo + 1), device=x.device)
    for p in range(4):
        w[p, 0, k0[p] - width - lo:k0[p] - width - lo + S] = taps[p]
    xp = torch.nn.functional.pad(x.reshape(R * Cn, 1, L), (-lo, hi))
    u = torch.nn.functional.conv1d(xp, w)                                           # [R C, 4, L]
    p = torch.maximum(u.abs().amax(1), x.reshape(R * Cn, L).abs()).reshape(R, Cn, L).amax(1)
    r = torch.where(p > 0, (c / p).clamp(max=1.0), torch.ones_like(p))
    rp = torch.nn.functional.pad(r[:, None], (2 * W, 2 * W), value=1.0)
    m = -torch.nn.functional.max_pool1d(-rp, 2 * W + 1, stride=1)                  # [R, 1, L + 2 W]
    win = torch.from_numpy(native.limiter_window(W)).to(x.device)[None, None]
    a = torch.nn.functional.conv1d(1.0 - m, win)[:, 0]
    return torch.minimum(r, 1.0 - a).clamp(min=0.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--skip-model", action="store_true", help="the two calls only")
    ap.add_argument("--skip-long", action="store_true", help="without the 30 min item")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("limiter_time.py measures on the GPU; none is available")

    eng = native.Engine(score_kind=native.SCORE_NONE, vae_has_encoder=False, vae_has_decoder=False)
    eng.finalize()
    dev = eng.device
    g = torch.Generator().manual_seed(2025)
    plan = native.resample_plan(1, 4)
    taps = torch.from_numpy(np.asarray(plan["taps"], dtype=np.float32)).to(dev)
    k0, width = [int(v) for v in plan["k0"]], int(plan["width"])
    res = {"warmup": a.warmup, "iters": a.iters, "reps": a.reps, "lookahead_ms": MS, "ceiling": CEIL}

    def timed(name, x, rates, lens=None, channels=None, reps=a.reps):
        R, Cn, L = x.shape
        rates = [rates] * R if isinstance(rates, int) else rates
        ln, ch = lens or [L] * R, channels or [Cn] * R
        samples = float(sum(v * c for v, c in zip(ln, ch)))
        group, pre = list(range(R)), [1.0] * R
        rec = dict(shape=[R, Cn, L], rates=sorted(set(rates)), samples=samples)
        for case in ("under", "reduced"):
            y = x.clamp(-0.25, 0.25)
            for r in range(R):                                   # zero padding: torch's version reads it
                y[r, ch[r]:] = 0.0
                y[r, :, ln[r]:] = 0.0
            if case == "reduced":
                for r in range(R):
                    W = native.limiter_half_window(MS, rates[r])
                    y[r, 0, 8 * W:ln[r]:16 * W] = 1.5
            out = torch.empty_like(y)
            curve, st = eng.limiter_curve(y, rates, group, pre, CEIL, MS, lens, channels)
            frac = float(st["limited_samples"].sum()) / float(sum(ln))

            def curves():
                for _ in range(reps):
                    eng.limiter_curve(y, rates, group, pre, CEIL, MS, lens, channels)

            def pairs():
                for _ in range(reps):
                    cv, _ = eng.limiter_curve(y, rates, group, pre, CEIL, MS, lens, channels)
                    eng.apply_curve(y, group, pre, cv, lens, channels, out=out)

            def reference():
                gs = {}
                for fs in sorted(set(rates)):
                    sel = [r for r in range(R) if rates[r] == fs]
                    gs[fs] = torch_curve(y[sel], native.limiter_half_window(MS, fs), CEIL, taps, k0, width)
                return gs

            c_ms, c_runs = median_ms(curves, a.warmup, a.iters)
            p_ms, p_runs = median_ms(pairs, a.warmup, a.iters)
            t_ms, t_runs = median_ms(reference, 1, 3)
            gs = reference()
            diff = 0.0
            for fs, gt in gs.items():
                for k, r in enumerate(q for q in range(R) if rates[q] == fs):
                    # (past a shorter item's end torch's hold sees r = 1 where the definition does too: zero padding)
                    diff = max(diff, float((gt[k, :ln[r]] - curve[r, :ln[r]]).abs().max()))
            nb_c = 4.0 * (samples + float(sum(ln)))
            nb_p = nb_c + 4.0 * (2.0 * samples + float(sum(v * c for v, c in zip(ln, ch))))
            rec[case] = dict(reduced_fraction=round(frac, 4), min_gain=float(st["min_gain"].min()),
                             curve_ms=round(c_ms / reps, 4), curve_runs_ms=[round(t / reps, 4) for t in c_runs],
                             curve_gbytes_per_s=round(nb_c / (c_ms / reps) * 1e-6, 1),
                             pair_ms=round(p_ms / reps, 4), pair_runs_ms=[round(t / reps, 4) for t in p_runs],
                             pair_gbytes_per_s=round(nb_p / (p_ms / reps) * 1e-6, 1),
                             torch_curve_ms=round(t_ms, 4), torch_runs_ms=[round(t, 4) for t in t_runs],
                             torch_over_device=round(t_ms / (c_ms / reps), 1), max_abs_diff_to_torch=diff)
            del gs
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
            kw = dict(seed=7, codec="padded", batch=B, loudness=-14.0)
            on, off = [], []
            for _ in range(a.warmup):
                model.separate_files(paths, out, limit=True, **kw)
                model.separate_files(paths, out, **kw)
            for _ in range(a.iters):                                               # alternating, in the same run
                on.append(median_ms(lambda: model.separate_files(paths, out, limit=True, **kw), 0, 1)[0])
                off.append(median_ms(lambda: model.separate_files(paths, out, **kw), 0, 1)[0])
            recs = model.separate_files(paths, out, limit=True, **kw)
            plain = model.separate_files(paths, out, **kw)
        on_ms, off_ms = float(np.median(on)), float(np.median(off))
        res["separate_files"] = dict(items=B, seconds=SECONDS, rate=RATE, N=N_STEPS, target=-14.0,
                                     with_limit_ms=round(on_ms, 2), with_limit_runs_ms=[round(t, 2) for t in on],
                                     without_ms=round(off_ms, 2), without_runs_ms=[round(t, 2) for t in off],
                                     feature_ms=round(on_ms - off_ms, 2), feature_share=round((on_ms - off_ms) / off_ms, 4),
                                     files_limited=sum(1 for r in recs if r["evaluations"][0] > 0),
                                     files_reached=sum(1 for r in recs if all(r["reached"])),
                                     evaluations=sorted({r["evaluations"][0] for r in recs}),
                                     short_of_target_without_lu=round(max(-14.0 - r["loudness_out"][0] for r in plain), 2),
                                     short_of_target_with_lu=round(max(-14.0 - r["loudness_out"][0] for r in recs), 2),
                                     deepest_reduction_db=round(min(min(r["reduction_db"]) for r in recs), 2))
        print(f"# separate_files: {res['separate_files']}", file=sys.stderr, flush=True)
        model.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
