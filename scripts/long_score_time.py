"""Time the three routes for long recordings against each other in one run (full-size DiT and Oobleck, fp16, graphs on,
one MI355X, inputs drawn once, 16 kHz): Engine.separate_long(mode="score") -- every recording one latent, the DiT score
window-blended --, Engine.separate_long(mode="stitch") -- batched windows, stitched waveforms -- and one pass at full
length.  scripts/long_time.py's workloads and protocol, with the windows on the latent grid: 32 frames sharing 8, that
is 65536 samples (4.096 s) sharing 16384 (1.024 s), for both windowed routes.
  one_30s      one 30 s recording;      one pass: Engine.separate on the whole length
  sixteen_30s  sixteen 30 s recordings; one pass: Engine.separate on the [16, 1, 30 s] batch
  mixed_5_15s  `--items` recordings of 5 - 15 s (lengths drawn once, seeded); one pass: Engine.separate_ragged
               (codec="padded") on the list
For each workload and route the codec alone as well (the encoder and decoder calls the route makes, on tensors of its
shapes) and its share of the call; for mode="score" the blend launches of one call (profiled eagerly: their count and
summed kernel time).  HIP events around whole calls; 3 warm-up calls (every shape's graph is captured there), then the
median of 5, with the five runs listed.  Prints one JSON line; --out also writes it to a file."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from ditsep_amd import native, synthetic  # noqa: E402
from scripts.ragged_time import FS, N_STEPS, CORR, SNR, T_EPS, build_engine, median_ms  # noqa: E402

TW, TO = 32, 8          # latent frames


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=64)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("long_score_time.py measures on the GPU; none is available")
    eng, dcfg = build_engine()
    eng.enable_graphs(True)
    dev, n, hop = eng.device, dcfg.n_src, eng.hop_length
    window, overlap = TW * hop, TO * hop
    kw = dict(N=N_STEPS, corrector_steps=CORR, snr=SNR, t_eps=T_EPS, seed=7)
    lkw = dict(window=window, overlap=overlap, batch=a.batch, **kw)
    long30 = synthetic.synthetic_sources(16, n, 30 * FS, FS, seed=1234).sum(1, keepdim=True).to(dev)     # [16,1,30 s]
    g = torch.Generator().manual_seed(2024)
    lengths = torch.randint(5 * FS, 15 * FS + 1, (a.items,), generator=g).tolist()
    src = synthetic.synthetic_sources(a.items, n, 15 * FS, FS, seed=4321).sum(1, keepdim=True).to(dev)
    mixed = [src[i, :, :lengths[i]].contiguous() for i in range(a.items)]
    recs30 = [long30[i] for i in range(16)]
    res = {"fs": FS, "window_frames": TW, "overlap_frames": TO, "window_samples": window, "overlap_samples": overlap,
           "batch": a.batch, "N": N_STEPS, "warmup": a.warmup, "iters": a.iters}

    def timed(name, fn, items, seconds, **extra):
        ms, times = median_ms(fn, a.warmup, a.iters)
        res[name] = dict(ms=round(ms, 2), runs_ms=[round(t, 2) for t in times], utt_per_s=round(1e3 * items / ms, 2),
                         audio_s_per_s=round(1e3 * seconds / ms, 1), **extra)
        print(f"# {name}: {res[name]}", file=sys.stderr, flush=True)

    def codec_of(name, fn):
        ms, times = median_ms(fn, a.warmup, a.iters)
        res[name].update(codec_ms=round(ms, 2), codec_runs_ms=[round(t, 2) for t in times],
                         codec_share=round(ms / res[name]["ms"], 4))

    def score_codec(recs):
        """the padded encoder and decoder pass mode="score" makes"""
        frames = [native.latent_frames_of(int(m.shape[-1]), hop) for m in recs]
        lat = 0.5 * torch.randn((len(recs), n, dcfg.latent_dim, max(frames)), device=dev)
        lens = [int(m.shape[-1]) for m in recs]

        def fn():
            eng.encode_ragged(recs, None, seed=7, codec="padded")
            eng.decode_ragged(lat, frames, lens, codec="padded")
        return fn

    def stitch_codec(recs):
        """the encoder and decoder calls mode="stitch" makes: the window pool, `batch` windows at a time"""
        pool, _, _ = native.cut_windows(recs, window, overlap, dev)
        lat = 0.5 * torch.randn((pool.shape[0], n, dcfg.latent_dim, eng.latent_frames(window)), device=dev)

        def fn():
            for lo in range(0, pool.shape[0], a.batch):
                eng.encode(pool[lo:lo + a.batch], None, seed=7)
                eng.decode(lat[lo:lo + a.batch], window)
        return fn

    def blend_of(name, recs):
        """one eager, profiled call: the blend launches alone"""
        eng.profile_begin()
        eng.separate_long(recs, mode="score", **lkw)
        torch.cuda.synchronize()
        rows = {r["site"]: r for r in eng.profile_end()["rows"]}
        b = rows["score.win_blend"]
        res[name].update(blend_launches=b["launches"], blend_ms=round(b["ms"], 4), blend_bytes=b["bytes"])

    def one_pass_30(x):
        return lambda: eng.separate(x, **kw)

    work = [("one_30s", [recs30[0]], 1, 30.0, one_pass_30(long30[:1])),
            ("sixteen_30s", recs30, 16, 480.0, one_pass_30(long30)),
            ("mixed_5_15s", mixed, a.items, sum(lengths) / FS, lambda: eng.separate_ragged(mixed, codec="padded", **kw))]
    for name, recs, items, secs, one_pass in work:
        plan = native.score_window_plan([native.latent_frames_of(int(m.shape[-1]), hop) for m in recs], TW, TO)
        timed(f"{name}_score", lambda: eng.separate_long(recs, mode="score", **lkw), items, secs, windows=plan["Wtot"],
              frames_max=plan["T"])
        timed(f"{name}_stitch", lambda: eng.separate_long(recs, mode="stitch", **lkw), items, secs,
              windows=sum(native.window_plan(int(m.shape[-1]), window, overlap)[0] for m in recs))
        timed(f"{name}_one_pass", one_pass, items, secs)
        codec_of(f"{name}_score", score_codec(recs))
        codec_of(f"{name}_stitch", stitch_codec(recs))
        blend_of(f"{name}_score", recs)
    eng.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
