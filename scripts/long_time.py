"""Time the separation of long recordings as batched windows against the one-pass route (full-size DiT and Oobleck, fp16,
graphs on, one MI355X, inputs drawn once, 16 kHz).  Windows of 4 s sharing 1 s with their neighbour.
  one_30s      one 30 s recording:      Engine.separate_long   against one Engine.separate call on the whole length
  sixteen_30s  sixteen 30 s recordings: Engine.separate_long   against one Engine.separate call on the [16, 1, 30 s] batch
  mixed_5_15s  `--items` recordings of 5 - 15 s (lengths drawn once, seeded): Engine.separate_long on the list against
               one Engine.separate call per recording
  stitch       the sixteen window_stitch calls of sixteen_30s alone (enqueued, no host outputs): milliseconds, the bytes
               they must move -- (W n Lw + 2 (W - 1) n O) reads + n L writes, 4 bytes each, per recording -- and the
               resulting GB/s next to the 6.3 TB/s a float4 copy reaches on this part
HIP events around whole calls; 3 warm-up calls (every shape's graph is captured there), then the median of 5, with the
five runs listed.  Prints one JSON line; --out also writes it to a file."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from ditsep_amd import native, synthetic  # noqa: E402
from scripts.ragged_time import FS, N_STEPS, CORR, SNR, T_EPS, build_engine, median_ms  # noqa: E402

WINDOW, OVERLAP = 4 * FS, FS
HBM_COPY_GBS = 6300.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=64)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("long_time.py measures on the GPU; none is available")
    eng, dcfg = build_engine()
    eng.enable_graphs(True)
    dev, n = eng.device, dcfg.n_src
    kw = dict(N=N_STEPS, corrector_steps=CORR, snr=SNR, t_eps=T_EPS, seed=7)
    lkw = dict(window=WINDOW, overlap=OVERLAP, batch=a.batch, **kw)
    long30 = synthetic.synthetic_sources(16, n, 30 * FS, FS, seed=1234).sum(1, keepdim=True).to(dev)     # [16,1,30 s]
    g = torch.Generator().manual_seed(2024)
    lengths = torch.randint(5 * FS, 15 * FS + 1, (a.items,), generator=g).tolist()
    src = synthetic.synthetic_sources(a.items, n, 15 * FS, FS, seed=4321).sum(1, keepdim=True).to(dev)
    mixed = [src[i, :, :lengths[i]].contiguous() for i in range(a.items)]
    recs30 = [long30[i] for i in range(16)]

    def windows(lens):
        return sum(native.window_plan(L, WINDOW, OVERLAP)[0] for L in lens)

    res = {"fs": FS, "window_s": 4, "overlap_s": 1, "batch": a.batch, "N": N_STEPS, "warmup": a.warmup, "iters": a.iters}

    def timed(name, fn, items, seconds, **extra):
        ms, times = median_ms(fn, a.warmup, a.iters)
        res[name] = dict(ms=round(ms, 2), runs_ms=[round(t, 2) for t in times], utt_per_s=round(1e3 * items / ms, 2),
                         audio_s_per_s=round(1e3 * seconds / ms, 1), **extra)
        print(f"# {name}: {res[name]}", file=sys.stderr, flush=True)

    timed("one_30s_windowed", lambda: eng.separate_long(recs30[0], **lkw), 1, 30, windows=windows([30 * FS]))
    timed("one_30s_one_pass", lambda: eng.separate(long30[:1], **kw), 1, 30)
    timed("sixteen_30s_windowed", lambda: eng.separate_long(recs30, **lkw), 16, 480, windows=windows([30 * FS] * 16))
    timed("sixteen_30s_one_pass", lambda: eng.separate(long30, **kw), 16, 480)
    secs = sum(lengths) / FS
    timed("mixed_5_15s_windowed", lambda: eng.separate_long(mixed, **lkw), a.items, secs, windows=windows(lengths))

    def each():
        for m in mixed:
            eng.separate(m[None], **kw)

    timed("mixed_5_15s_one_call_each", each, a.items, secs)

    # the stitch calls of sixteen_30s alone, on windows of the right shape
    W, hop = native.window_plan(30 * FS, WINDOW, OVERLAP)
    sep = 0.1 * torch.randn((16 * W, n, WINDOW), device=dev)
    plans = [(W, hop, 30 * FS)] * 16
    ms, times = median_ms(lambda: eng._stitch_plans(sep, plans, OVERLAP, "hann", True, False), a.warmup, a.iters)
    nbytes = 16 * 4 * ((W * n * WINDOW + 2 * (W - 1) * n * OVERLAP) + n * 30 * FS)
    res["stitch_sixteen_30s"] = dict(ms=round(ms, 4), runs_ms=[round(t, 4) for t in times], calls=16, launches=48,
                                     bytes=nbytes, gb_per_s=round(nbytes / ms * 1e-6, 1), hbm_copy_gb_per_s=HBM_COPY_GBS)
    eng.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
