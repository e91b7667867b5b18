"""Time the mixture-consistent masks (Engine.mask_refine, dsn_mask_refine) and what `refine=` costs a separation call
(one MI355X, inputs drawn once, seeded; n_fft 512, hop 128, power 2).
  dense_64x2x4s    64 items x 2 sources x 4 s at 16 kHz
  ragged_64x2      64 items of 2 - 4 s in one call (lens)
  one_30s          one item of 30 s, 2 sources
For each: milliseconds per call and the algorithmic bytes ((n + 1) L 4 read, n L 4 written, over the items' own
lengths) per second -- at these sizes the data fits the Infinity Cache, so these are call times, not HBM rates --, the
largest difference from the same definition written with torch.stft / torch.istft on the same GPU, and that
formulation's time beside it (the ragged workload runs it item by item: it has no form for per-item lengths).
  separate_batch   LatentDiffSep.separate_batch(codec="padded") (full-size DiT and Oobleck, fp16, graphs on) on 64 clips
                   of 4 s with refine=True against the same call without: the difference is what the feature costs.
HIP events around whole calls; 3 warm-up runs, then the median of 5 timed runs, with the runs listed.  A refinement
call is short, so a timed run is `--reps` calls back to back and the figure is per call.
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


def torch_refine(mix, est, n_fft=512, hop=128, power=2, eps=1e-10):
    """the definition with torch.stft / torch.istft: mix [B, L], est [B, n, L] (one length) -> [B, n, L]"""
    B, n, L = est.shape
    Lp = hop * (-(-L // hop))
    x = torch.nn.functional.pad(torch.cat([mix[:, None], est], dim=1), (0, Lp - L)).reshape(B * (n + 1), Lp)
    w = torch.hann_window(n_fft, periodic=True, dtype=torch.float64, device=mix.device).float()
    Z = torch.stft(x, n_fft, hop_length=hop, window=w, center=True, pad_mode="reflect", return_complex=True)
    Z = Z.reshape(B, n + 1, *Z.shape[1:])
    X, S = Z[:, :1], Z[:, 1:]
    a = S.abs() if power == 1 else S.real ** 2 + S.imag ** 2
    M = (a + eps) / (a.sum(dim=1, keepdim=True) + n * eps)
    y = torch.istft((M * X).reshape(B * n, *Z.shape[2:]), n_fft, hop_length=hop, window=w, center=True, length=Lp)
    return y.reshape(B, n, Lp)[..., :L]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=64)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--skip-model", action="store_true", help="the kernel workloads only")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mask_refine_time.py measures on the GPU; none is available")
    eng = native.Engine(score_kind=native.SCORE_NONE, vae_has_encoder=False, vae_has_decoder=False)
    eng.finalize()
    dev, B, SECONDS, n = eng.device, a.items, 4, 2
    g = torch.Generator().manual_seed(2025)
    res = {"items": B, "seconds": SECONDS, "warmup": a.warmup, "iters": a.iters, "reps": a.reps,
           **native.MASK_REFINE_DEFAULTS}

    def run(fn):
        def many():
            for _ in range(a.reps):
                fn()
        ms, times = median_ms(many, a.warmup, a.iters)
        return ms / a.reps, [round(t / a.reps, 4) for t in times]

    def timed(name, mix, est, lens=None):
        Bx, nx, L = est.shape
        samples = sum(lens) if lens else Bx * L
        nbytes = 4.0 * (2 * nx + 1) * samples
        ms, times = run(lambda: eng.mask_refine(mix, est, lens=lens))
        rec = dict(shape=[Bx, nx, L], ms=round(ms, 4), runs_ms=times, algorithmic_bytes=nbytes,
                   gbytes_per_s=round(nbytes / ms * 1e-6, 1))
        try:
            got = eng.mask_refine(mix, est, lens=lens)
            if lens is None:
                fn = lambda: torch_refine(mix, est)                                             # noqa: E731
                rec["torch_max_abs_diff"] = float((got - fn()).abs().max())
            else:
                def fn():
                    return [torch_refine(mix[b:b + 1, :v], est[b:b + 1, :, :v]) for b, v in enumerate(lens)]
                rec["torch_max_abs_diff"] = max(float((got[b, :, :v] - w[0]).abs().max())
                                                for (b, v), w in zip(enumerate(lens), fn()))
                rec["torch_note"] = "torch.stft / istft run item by item: they have no form for per-item lengths"
            tms, ttimes = run(fn)
            rec.update(torch_ms=round(tms, 4), torch_runs_ms=ttimes, torch_over_native=round(tms / ms, 2))
        except Exception as e:                                                  # reported only
            rec["torch_note"] = f"skipped: {type(e).__name__}: {e}"
        res[name] = rec
        print(f"# {name}: {rec}", file=sys.stderr, flush=True)

    def draw(Bx, L):
        src = 0.1 * torch.randn((Bx, n, L), generator=g)
        return src.sum(dim=1).to(dev), (src + 0.03 * torch.randn((Bx, n, L), generator=g)).to(dev)

    timed("dense_64x2x4s", *draw(B, SECONDS * FS))
    lens = torch.randint(SECONDS // 2 * FS, SECONDS * FS + 1, (B,), generator=g).tolist()
    lens[0] = SECONDS * FS
    timed("ragged_64x2", *draw(B, SECONDS * FS), lens=lens)
    timed("one_30s", *draw(1, 30 * FS))
    eng.close()

    if not a.skip_model:
        model = full_size_model()
        src = synthetic.synthetic_sources(B, 2, SECONDS * FS, FS, seed=1234).sum(1, keepdim=True).to(dev)
        clips = [src[i] for i in range(B)]
        kw = dict(seed=7, codec="padded")
        with_ms, with_runs = median_ms(lambda: model.separate_batch(clips, refine=True, **kw), a.warmup, a.iters)
        base_ms, base_runs = median_ms(lambda: model.separate_batch(clips, **kw), a.warmup, a.iters)
        res["separate_batch"] = dict(items=B, seconds=SECONDS, refine_ms=round(with_ms, 2),
                                     refine_runs_ms=[round(t, 2) for t in with_runs], plain_ms=round(base_ms, 2),
                                     plain_runs_ms=[round(t, 2) for t in base_runs],
                                     feature_ms=round(with_ms - base_ms, 2),
                                     feature_share=round((with_ms - base_ms) / base_ms, 4))
        print(f"# separate_batch: {res['separate_batch']}", file=sys.stderr, flush=True)
        model.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
