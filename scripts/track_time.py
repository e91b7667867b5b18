"""Time the block-adaptive MVDR beamformer (Engine.beamform_track, dsn_beamform_track) against the time-invariant one
(Engine.beamform) on the same input in the same run, and what `track=True` adds to separate_files with beamform=True
(one MI355X, inputs drawn once, seeded).  The workloads of scripts/beamform_time.py and the recording the tracking is for:
  array4_4s     64 x 4 channels x 2 sources x 4 s at 16 kHz
  array8_4s     64 x 8 channels x 4 sources x 4 s
  ragged_2_4s   64 items of 2 - 4 s with 2, 4 or 8 channels each in one call (lens, channels), 2 sources
  long_30s      one 8-channel item of 30 s, 4 sources
  meeting_10min one 4-channel item of 10 minutes, 2 sources
For each: milliseconds per call of Engine.beamform, of Engine.beamform_track at the defaults (blocks of 100 frames, one
block of context each side, interpolated) and at context = 0, and what each costs over the time-invariant call; beside it
the same definition in torch on the same GPU -- torch.stft, float64 einsum statistics per block, torch.linalg.solve per
block, the frames' weights gathered and interpolated, torch.istft -- reported only (skipped with a note if it fails; it
runs the padded batch: it has no form for per-item lengths or channel counts, so its blocks are the padded item's).
  separate_files  LatentDiffSep.separate_files (full-size DiT and Oobleck, fp16, graphs on) on 64 four-channel s16 clips
                of 4 s at 44.1 kHz with beamform=True, track=True against the call with beamform=True alone, in the same
                run (--no-files skips it).
HIP events around whole calls; 3 warm-up runs, then the median of 5 timed runs, with the runs listed.  A call is short,
so a timed run is `--reps` calls back to back and the figure is per call.  These are call times with the data resident
in the Infinity Cache where it fits (the same tensors every call), not cold-HBM figures.
Prints one JSON line; --out also writes it to a file."""
import argparse
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from ditsep_amd import native, synthetic, wavio  # noqa: E402
from scripts.beamform_time import EPS, HOP, N_FFT, REG  # noqa: E402
from scripts.ragged_time import FS, median_ms  # noqa: E402
from scripts.resample_time import full_size_model  # noqa: E402

TB = 100


def torch_track(mix, est, ref, context, interpolate=True):
    """the definition of include/ditsep_hip.h (dsn_beamform_track) in torch: mix [B, C, L], est [B, n, L] -> [B, n, L]"""
    (B, Cn, L), n = mix.shape, est.shape[1]
    w = torch.hann_window(N_FFT, periodic=True, device=mix.device)
    kw = dict(hop_length=HOP, win_length=N_FFT, window=w, center=True)
    Z = torch.stft(torch.cat([mix, est], dim=1).reshape(-1, L), N_FFT, pad_mode="reflect", return_complex=True, **kw)
    Z = Z.reshape(B, Cn + n, *Z.shape[1:])
    X, S = Z[:, :Cn], Z[:, Cn:]
    a = S.real ** 2 + S.imag ** 2
    M = (a + EPS) / (a.sum(dim=1, keepdim=True) + n * EPS)
    F = X.shape[-1]
    K = (F + TB - 1) // TB
    pad = (0, K * TB - F)
    Xb = torch.nn.functional.pad(X.to(torch.complex128), pad).reshape(B, Cn, -1, K, TB)
    Mb = torch.nn.functional.pad(M, pad).reshape(B, n, -1, K, TB).to(torch.complex128)
    P = torch.stack([torch.einsum("bcfkt,bdfkt->bkfcd", Mb[:, i, None] * Xb, Xb.conj()) for i in range(n)], dim=2)
    N = torch.zeros_like(P)                                                      # [B, K, n, bins, C, C]
    for d in range(-context, context + 1):
        lo, hi = max(0, -d), min(K, K - d)
        N[:, lo:hi] += P[:, lo + d:hi + d]
    Q = N.sum(dim=2, keepdim=True) - N
    eye = torch.eye(Cn, dtype=torch.complex128, device=mix.device)
    lam = REG * torch.einsum("bkifcc->bkif", Q).real / Cn + EPS
    Zs = torch.linalg.solve(Q + lam[..., None, None] * eye, N)
    tau = torch.einsum("bkifcc->bkif", Zs).real
    wt = Zs[..., ref] / tau[..., None]                                           # [B, K, n, bins, C]
    k0, alpha = native.track_plan(F, TB, interpolate)
    k0, alpha = k0.to(mix.device), alpha.to(mix.device)
    w0 = wt[:, k0]                                                               # [B, F, n, bins, C]
    wf = w0 + alpha[None, :, None, None, None] * (wt[:, (k0 + 1).clamp(max=K - 1)] - w0)
    Y = torch.einsum("btifc,bcft->bift", wf.conj(), X.to(torch.complex128)).to(torch.complex64)
    y = torch.istft(Y.reshape(-1, *Y.shape[-2:]), N_FFT, length=L, **kw)
    return y.reshape(B, n, L)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=64)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--no-files", action="store_true")
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("track_time.py measures on the GPU; none is available")
    eng = native.Engine(score_kind=native.SCORE_NONE, vae_has_encoder=False, vae_has_decoder=False)
    eng.finalize()
    dev, B = eng.device, a.items
    g = torch.Generator().manual_seed(2026)
    res = {"items": B, "n_fft": N_FFT, "hop": HOP, "block_frames": TB, "warmup": a.warmup, "iters": a.iters,
           "reps": a.reps}

    def run(fn):
        def many():
            for _ in range(a.reps):
                fn()
        ms, times = median_ms(many, a.warmup, a.iters)
        return ms / a.reps, [round(t / a.reps, 4) for t in times]

    def draw(items, Cn, n, L, taps=8):
        """white sources through random short mixing filters plus sensor noise; the estimates are the noisy images at
        channel 0"""
        src = 0.1 * torch.randn((items, n, L), generator=g)
        h = torch.randn((items, n, Cn, taps), generator=g) * 0.3
        h[..., 0] = 1.0
        img = torch.zeros((items, n, Cn, L))
        for k in range(taps):
            img[..., k:] += h[..., k, None] * src[:, :, None, :L - k]
        mix = img.sum(dim=1) + 0.001 * torch.randn((items, Cn, L), generator=g)
        est = img[:, :, 0] + 0.03 * torch.randn((items, n, L), generator=g)
        return mix.to(dev), est.to(dev)

    def timed(name, mix, est, lens=None, channels=None):
        (items, Cn, L), n = mix.shape, est.shape[1]
        kw = dict(lens=lens, channels=channels, n_fft=N_FFT, hop=HOP, eps=EPS, reg=REG)
        rec = dict(shape=[items, Cn, n, L], blocks=-(-(1 + -(-L // HOP)) // TB),
                   workspace_item_bytes=native.track_item_bytes(N_FFT, HOP, L, Cn, n, TB))
        ms, times = run(lambda: eng.beamform(mix, est, **kw))
        rec["beamform"] = dict(ms=round(ms, 4), runs_ms=times)
        base = ms
        for tag, ctx in (("track", 1), ("track_context0", 0)):
            ms, times = run(lambda: eng.beamform_track(mix, est, block_frames=TB, context=ctx, **kw))
            rec[tag] = dict(ms=round(ms, 4), runs_ms=times, over_beamform=round(ms / base, 3))
        if not a.no_torch:
            try:
                want = torch_track(mix, est, 0, 1)
                if lens is None:
                    got = eng.beamform_track(mix, est, block_frames=TB, context=1, **kw)
                    rec["track"]["torch_max_abs_diff"] = float((got - want).abs().max())
                del want
                tms, ttimes = run(lambda: torch_track(mix, est, 0, 1))
                rec["track"].update(torch_ms=round(tms, 4), torch_runs_ms=ttimes,
                                    torch_over_native=round(tms / rec["track"]["ms"], 2))
                if lens is not None:
                    rec["track"]["torch_note"] = ("torch runs the padded batch: it has no form for per-item lengths or "
                                                  "channel counts")
            except Exception as e:                                              # reported only
                rec["track"]["torch_note"] = f"skipped: {type(e).__name__}: {e}"
            torch.cuda.empty_cache()
        res[name] = rec
        print(f"# {name}: {rec}", file=sys.stderr, flush=True)

    timed("array4_4s", *draw(B, 4, 2, 4 * FS))
    timed("array8_4s", *draw(B, 8, 4, 4 * FS))
    lens = torch.randint(2 * FS, 4 * FS + 1, (B,), generator=g).tolist()
    lens[0] = 4 * FS
    chans = [(2, 4, 8)[int(v)] for v in torch.randint(0, 3, (B,), generator=g)]
    chans[0] = 8
    timed("ragged_2_4s", *draw(B, 8, 2, 4 * FS), lens=lens, channels=chans)
    timed("long_30s", *draw(1, 8, 4, 30 * FS))
    timed("meeting_10min", *draw(1, 4, 2, 600 * FS))
    eng.close()

    if not a.no_files:
        model = full_size_model()
        src = synthetic.synthetic_sources(B, 2, 4 * 44100, 44100, seed=1234)                  # [B, 2, L]: two speakers
        pan = torch.tensor([[0.9, 0.3, 0.6, 0.2], [0.2, 0.8, 0.5, 0.7]])
        array = torch.einsum("ic,bil->blc", pan, src).clamp(-1.0, 1.0)                        # [B, L, 4] interleaved
        with tempfile.TemporaryDirectory() as tmp:
            paths = []
            for b in range(B):
                paths.append(os.path.join(tmp, f"clip{b:03d}.wav"))
                wavio.write_wav(paths[-1], (array[b] * 32767.0).round().to(torch.int16).numpy().astype("<i2").tobytes(),
                                44100, 4, "s16")
            kw = dict(batch=B, seed=7, beamform=True)
            with_ms, with_runs = median_ms(lambda: model.separate_files(paths, os.path.join(tmp, "track"), track=True,
                                                                        **kw), a.warmup, a.iters)
            base_ms, base_runs = median_ms(lambda: model.separate_files(paths, os.path.join(tmp, "beam"), **kw),
                                           a.warmup, a.iters)
        res["separate_files"] = dict(items=B, seconds=4, rate=44100, channels=4, with_track_ms=round(with_ms, 2),
                                     with_track_runs_ms=[round(t, 2) for t in with_runs],
                                     beamform_only_ms=round(base_ms, 2),
                                     beamform_only_runs_ms=[round(t, 2) for t in base_runs],
                                     feature_ms=round(with_ms - base_ms, 2),
                                     feature_share=round((with_ms - base_ms) / base_ms, 4),
                                     note="whole calls, file reads and writes included; both with beamform=True")
        print(f"# separate_files: {res['separate_files']}", file=sys.stderr, flush=True)
        model.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
