"""Time the speaker-activity decision (Engine.activity, dsn_activity), the gate (Engine.activity_gate, dsn_activity_gate)
and what `activity="gate"` costs separate_files (one MI355X, inputs drawn once, seeded; the defaults at 16 kHz: n_fft 512,
hop 128, band 100 - 4000 Hz, half-width 2, 13 frames minimum on and off, fade 80 samples).
  dense_64x2x4s    64 items x 2 sources x 4 s at 16 kHz
  ragged_64x2      64 items of 2 - 4 s in one call (lens)
  one_30s          one item of 30 s, 2 sources
  one_10min        one item of 10 min, 2 sources
The sources are white noise switched on and off in stretches of 0.1 - 2 s with 10 % leakage, so the decision has runs to
work on.  For each: milliseconds per call of both calls -- at these sizes the data sits in the Infinity Cache, so these
are call times, not bandwidth measurements --, and beside the decision the same definition as far as torch has a form
for it on the same GPU: torch.stft, a band sum and avg_pool1d for the levels on the device; hysteresis and the run rules
have no torch op, so that route copies the levels to the host and does them in numpy there (the vectorised form of
tests/activity_restatement.py), and its figure includes that copy.  The ragged workload runs it item by item.
  separate_files   LatentDiffSep.separate_files (full-size DiT and Oobleck, fp16, graphs on) on the 64 clips of
                   scripts/files_time.py with activity="gate" against the same call without, in the same run.
HIP events around whole calls; 3 warm-up runs, then the median of 5 timed runs, with the runs listed.  A call is short,
so a timed run is `--reps` calls back to back and the figure is per call.
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
from scripts.ragged_time import FS, median_ms  # noqa: E402
from scripts.resample_time import full_size_model  # noqa: E402

KW = native.activity_keywords(native.ACTIVITY_DEFAULTS, FS)
FADE = native.activity_frames(native.ACTIVITY_DEFAULTS, FS)["fade"]


def _nearest(v):
    F = v.shape[-1]
    idx = np.arange(F)
    before = np.maximum.accumulate(np.where(v, idx, -1), axis=-1)
    after = np.minimum.accumulate(np.where(v, idx, F)[..., ::-1], axis=-1)[..., ::-1]
    return before, after


def host_rules(on, stay, min_on, min_off, pad):
    """hysteresis and the run rules on [rows, F] boolean arrays, with cumulative maxima and minima"""
    F = on.shape[-1]
    t = np.arange(F)
    a = _nearest(on)[0] > _nearest(~stay & ~on)[0]
    before, after = _nearest(a)
    a = a | ((before >= 0) & (after < F) & (after - before - 1 < min_off))
    before, after = _nearest(~a)
    a = a & ~(after - before - 1 < min_on)
    before, after = _nearest(a)
    return a | ((before >= 0) & (t - before <= pad)) | ((after < F) & (after - t <= pad))


def torch_activity(est):
    """the definition as far as torch has a form for it: est [B, n, L] (one length) -> act [B, n, F] numpy"""
    B, n, L = est.shape
    n_fft, hop, h = KW["n_fft"], KW["hop"], KW["half_width"]
    Lp = hop * (-(-L // hop))
    x = torch.nn.functional.pad(est, (0, Lp - L)).reshape(B * n, Lp)
    w = torch.hann_window(n_fft, periodic=True, dtype=torch.float64, device=est.device).float()
    Z = torch.stft(x, n_fft, hop_length=hop, window=w, center=True, pad_mode="reflect", return_complex=True)
    j_lo, j_hi = native.activity_band(KW["band"], FS, n_fft)
    E = (Z.real.double() ** 2 + Z.imag.double() ** 2)[:, j_lo:j_hi + 1].sum(dim=1)             # [B n, F]
    lev = torch.nn.functional.avg_pool1d(E[:, None], 2 * h + 1, stride=1, padding=h, count_include_pad=False)[:, 0]
    lev = lev.reshape(B, n, -1)
    c_r, c_d, c_rs, c_ds = native.activity_constants(KW["range_db"], KW["dominance_db"], KW["hysteresis_db"])
    P, top = lev.amax(dim=(1, 2), keepdim=True), lev.amax(dim=1, keepdim=True)
    on = (P > 0) & (lev >= P * c_r) & (lev >= top * c_d)
    stay = (P > 0) & (lev >= P * c_rs) & (lev >= top * c_ds)
    both = torch.stack([on, stay]).cpu().numpy()                                             # the copy to the host
    return host_rules(both[0], both[1], KW["min_on"], KW["min_off"], KW["pad"])


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
        raise SystemExit("activity_time.py measures on the GPU; none is available")
    eng = native.Engine(score_kind=native.SCORE_NONE, vae_has_encoder=False, vae_has_decoder=False)
    eng.finalize()
    dev, B, SECONDS, n = eng.device, a.items, 4, 2
    g = torch.Generator().manual_seed(2025)
    res = {"items": B, "seconds": SECONDS, "warmup": a.warmup, "iters": a.iters, "reps": a.reps,
           **{k: v for k, v in KW.items()}, "fade": FADE}

    def run(fn, reps):
        def many():
            for _ in range(reps):
                fn()
        ms, times = median_ms(many, a.warmup, a.iters)
        return ms / reps, [round(t / reps, 4) for t in times]

    def timed(name, est, lens=None, reps=None):
        reps = a.reps if reps is None else reps
        Bx, nx, L = est.shape
        ms, times = run(lambda: eng.activity(est, lens=lens, **KW), reps)
        got = eng.activity(est, lens=lens, **KW)
        gms, gtimes = run(lambda: eng.activity_gate(est, got["act"], lens=lens, hop=KW["hop"], fade=FADE), reps)
        rec = dict(shape=[Bx, nx, L], activity_ms=round(ms, 4), activity_runs_ms=times, gate_ms=round(gms, 4),
                   gate_runs_ms=gtimes, active_share=round(float(got["frames_on"].sum()) / sum(got["frames"]) / nx, 4))
        try:
            if lens is None:
                fn = lambda: torch_activity(est)                                               # noqa: E731
                act = got["act"].cpu().numpy() != 0
                rec["torch_frames_differing"] = int((fn() != act).sum())
            else:
                def fn():
                    return [torch_activity(est[b:b + 1, :, :v]) for b, v in enumerate(lens)]
                act = got["act"].cpu().numpy() != 0
                rec["torch_frames_differing"] = int(sum((w[0] != act[b, :, :w.shape[-1]]).sum() for b, w in enumerate(fn())))
                rec["torch_note"] = "run item by item: torch.stft has no form for per-item lengths"
            tms, ttimes = run(fn, max(1, reps // 4))
            rec.update(torch_ms=round(tms, 4), torch_runs_ms=ttimes, torch_over_native=round(tms / ms, 2),
                       torch_includes="the copy of the on / stay bits to the host and the run rules in numpy there")
        except Exception as e:                                                  # reported only
            rec["torch_note"] = f"skipped: {type(e).__name__}: {e}"
        res[name] = rec
        print(f"# {name}: {rec}", file=sys.stderr, flush=True)

    def draw(Bx, L):
        src = 0.1 * torch.randn((Bx, n, L), generator=g)
        gate = torch.zeros((Bx, n, L))
        for b in range(Bx):
            for i in range(n):
                p, on = 0, bool(torch.randint(0, 2, (1,), generator=g))
                while p < L:
                    q = p + int(torch.randint(FS // 10, 2 * FS, (1,), generator=g))
                    gate[b, i, p:q] = float(on)
                    p, on = q, not on
        src = src * gate
        return (src + 0.1 * (src.sum(dim=1, keepdim=True) - src)).to(dev)

    timed("dense_64x2x4s", draw(B, SECONDS * FS))
    lens = torch.randint(SECONDS // 2 * FS, SECONDS * FS + 1, (B,), generator=g).tolist()
    lens[0] = SECONDS * FS
    timed("ragged_64x2", draw(B, SECONDS * FS), lens=lens)
    timed("one_30s", draw(1, 30 * FS))
    timed("one_10min", draw(1, 600 * FS), reps=max(1, a.reps // 4))
    eng.close()

    if not a.skip_model:
        from scripts.files_time import RATE

        model = full_size_model()
        L = SECONDS * RATE
        src = synthetic.synthetic_sources(B, 2, L, RATE, seed=1234).sum(1)                      # [B, L]
        src = 0.5 * src / src.abs().amax()
        stereo = torch.stack([src, 0.9 * src.roll(3, dims=-1)], dim=1)                           # [B, 2, L]
        pcm = torch.round(stereo * 2 ** 15).clamp(-2 ** 15, 2 ** 15 - 1).to(torch.int16)
        with tempfile.TemporaryDirectory() as tmp:
            paths = []
            for b in range(B):
                paths.append(os.path.join(tmp, f"clip{b:03d}.wav"))
                wavio.write_wav(paths[-1], pcm[b].T.contiguous().numpy().tobytes(), RATE, 2, "s16")
            out = os.path.join(tmp, "out")
            kw = dict(seed=7, codec="padded", batch=B)
            with_ms, with_runs = median_ms(lambda: model.separate_files(paths, out, activity="gate", **kw), a.warmup,
                                           a.iters)
            base_ms, base_runs = median_ms(lambda: model.separate_files(paths, out, **kw), a.warmup, a.iters)
        res["separate_files"] = dict(items=B, seconds=SECONDS, activity_ms=round(with_ms, 2),
                                     activity_runs_ms=[round(t, 2) for t in with_runs], plain_ms=round(base_ms, 2),
                                     plain_runs_ms=[round(t, 2) for t in base_runs],
                                     feature_ms=round(with_ms - base_ms, 2),
                                     feature_share=round((with_ms - base_ms) / base_ms, 4))
        print(f"# separate_files: {res['separate_files']}", file=sys.stderr, flush=True)
        model.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
