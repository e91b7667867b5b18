"""Time the WPE dereverberation (Engine.dereverb, dsn_dereverb) and what `dereverb=True` adds to separate_files (one
MI355X, inputs drawn once, seeded; the protocol of scripts/beamform_time.py).
  array4_4s     64 x 4 channels x 4 s at 16 kHz
  array8_4s     64 x 8 channels x 4 s
  ragged_2_4s   64 items of 2 - 4 s with 2, 4 or 8 channels each in one call (lens, channels)
  long_30s      one 8-channel item of 30 s
The defaults: 10 taps, delay 3, 3 iterations, 512 / 128, reg 1e-4.  For each: milliseconds per call and the algorithmic
bytes (mixture read once, output written once) per second; beside it the same definition in torch on the same GPU --
torch.stft, complex128 einsum statistics, torch.linalg.cholesky / cholesky_solve, torch.istft -- reported only (skipped
with a note if it fails; it runs the padded batch: it has no form for per-item lengths or channel counts), with the
largest absolute difference of the two outputs.
  separate_files  LatentDiffSep.separate_files (full-size DiT and Oobleck, fp16, graphs on) on 64 four-channel s16 clips
                of 4 s at 44.1 kHz with dereverb=True against the call without it, in the same run (--no-files skips it).
HIP events around whole calls; 3 warm-up runs, then the median of 5 timed runs, with the runs listed.  A timed run is
`--reps` calls back to back and the figure is per call.  These are call times with the data resident in the Infinity
Cache (the same tensors every call), not cold-HBM figures.  The script takes no kernel trace; `--only NAME` runs one
workload, which is what a trace of the call wants (`rocprofv3 --kernel-trace --stats -- python scripts/dereverb_time.py
--no-torch --only array8_4s`).
Prints one JSON line; --out also writes it to a file, after every workload."""
import argparse
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from ditsep_amd import native, synthetic, wavio  # noqa: E402
from scripts.ragged_time import FS, median_ms  # noqa: E402
from scripts.resample_time import full_size_model  # noqa: E402

OPTS = dict(native.DEREVERB_DEFAULTS)


def torch_dereverb(mix):
    """the definition of include/ditsep_hip.h (dsn_dereverb) in torch: mix [B, C, L] -> [B, C, L]"""
    B, Cn, L = mix.shape
    n_fft, hop, K, D = OPTS["n_fft"], OPTS["hop"], OPTS["taps"], OPTS["delay"]
    w = torch.hann_window(n_fft, periodic=True, device=mix.device)
    kw = dict(hop_length=hop, win_length=n_fft, window=w, center=True)
    Z = torch.stft(mix.reshape(-1, L), n_fft, pad_mode="reflect", return_complex=True, **kw)
    Y = Z.reshape(B, Cn, *Z.shape[1:]).permute(0, 2, 1, 3).to(torch.complex128)      # [B, bins, C, F]
    F = Y.shape[-1]
    Yt = torch.zeros((B, Y.shape[1], Cn * K, F), dtype=torch.complex128, device=mix.device)
    for k in range(K):
        Yt[:, :, k * Cn:(k + 1) * Cn, D + k:] = Y[..., :F - D - k]
    X = Y
    eye = torch.eye(Cn * K, dtype=torch.complex128, device=mix.device)
    for _ in range(OPTS["iterations"]):
        lam = (X.real ** 2 + X.imag ** 2).mean(dim=2)
        lam = torch.maximum(lam, 1e-10 * lam.amax(dim=-1, keepdim=True)).clamp_min(1e-300)
        Yw = Yt / lam[:, :, None, :]
        R = torch.einsum("bfit,bfjt->bfij", Yw, Yt.conj())
        P = torch.einsum("bfit,bfct->bfic", Yw, Y.conj())
        delta = OPTS["reg"] * torch.einsum("bfii->bf", R).real / (Cn * K) + OPTS["eps"]
        G = torch.cholesky_solve(P, torch.linalg.cholesky(R + delta[..., None, None] * eye))
        X = Y - torch.einsum("bfjc,bfjt->bfct", G.conj(), Yt)
    Xc = X.permute(0, 2, 1, 3).to(torch.complex64).reshape(-1, X.shape[1], F)
    return torch.istft(Xc, n_fft, length=L, **kw).reshape(B, Cn, L)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=64)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-files", action="store_true")
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--only", default=None, help="one workload by name (for a kernel trace)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("dereverb_time.py measures on the GPU; none is available")
    eng = native.Engine(score_kind=native.SCORE_NONE, vae_has_encoder=False, vae_has_decoder=False)
    eng.finalize()
    dev, B = eng.device, a.items
    g = torch.Generator().manual_seed(2026)
    res = dict(items=B, warmup=a.warmup, iters=a.iters, reps=a.reps, **OPTS)

    def save():
        if a.out:
            with open(a.out, "w") as fh:
                fh.write(json.dumps(res) + "\n")

    def run(fn):
        def many():
            for _ in range(a.reps):
                fn()
        ms, times = median_ms(many, a.warmup, a.iters)
        return ms / a.reps, [round(t / a.reps, 4) for t in times]

    def draw(items, Cn, L, taps=2400):
        """white bursts through exponentially decaying random responses of 0.15 s (an FFT convolution) plus sensor noise"""
        src = torch.randn((items, 1, L), generator=g) * ((torch.arange(L) // 2000) % 2 == 0)
        h = torch.randn((items, Cn, taps), generator=g) * torch.exp(-6.9 * torch.arange(taps) / taps)
        n = 1 << (L + taps).bit_length()
        wet = torch.fft.irfft(torch.fft.rfft(src, n) * torch.fft.rfft(h, n), n)[..., :L]
        mix = 0.5 * wet / wet.abs().amax() + 0.001 * torch.randn((items, Cn, L), generator=g)
        return mix.to(dev)

    def timed(name, mix, lens=None, channels=None):
        if a.only not in (None, name):
            return
        items, Cn, L = mix.shape
        nbytes = 8.0 * items * L * Cn if lens is None else 8.0 * sum(v * c for v, c in zip(lens, channels))
        rec = dict(shape=[items, Cn, L], algorithmic_bytes=nbytes)
        kw = dict(lens=lens, channels=channels, **OPTS)
        ms, times = run(lambda: eng.dereverb(mix, **kw))
        rec.update(ms=round(ms, 4), runs_ms=times, gbytes_per_s=round(nbytes / ms * 1e-6, 2))
        if not a.no_torch:
            try:
                want = torch_dereverb(mix)
                if lens is None:
                    rec["torch_max_abs_diff"] = float((eng.dereverb(mix, **kw) - want).abs().max())
                del want
                tms, ttimes = run(lambda: torch_dereverb(mix))
                rec.update(torch_ms=round(tms, 4), torch_runs_ms=ttimes, torch_over_native=round(tms / ms, 2))
                if lens is not None:
                    rec["torch_note"] = "torch runs the padded batch: it has no form for per-item lengths or channel counts"
            except Exception as e:                                              # reported only
                rec["torch_note"] = f"skipped: {type(e).__name__}: {e}"
            torch.cuda.empty_cache()
        res[name] = rec
        save()
        print(f"# {name}: {rec}", file=sys.stderr, flush=True)

    timed("array4_4s", draw(B, 4, 4 * FS))
    timed("array8_4s", draw(B, 8, 4 * FS))
    lens = torch.randint(2 * FS, 4 * FS + 1, (B,), generator=g).tolist()
    lens[0] = 4 * FS
    chans = [(2, 4, 8)[int(v)] for v in torch.randint(0, 3, (B,), generator=g)]
    chans[0] = 8
    timed("ragged_2_4s", draw(B, 8, 4 * FS), lens=lens, channels=chans)
    timed("long_30s", draw(1, 8, 30 * FS))
    eng.close()

    if not a.no_files and a.only is None:
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
            kw = dict(batch=B, seed=7)
            with_ms, with_runs = median_ms(lambda: model.separate_files(paths, os.path.join(tmp, "dry"),
                                                                        dereverb=True, **kw), a.warmup, a.iters)
            base_ms, base_runs = median_ms(lambda: model.separate_files(paths, os.path.join(tmp, "mono"), **kw),
                                           a.warmup, a.iters)
        res["separate_files"] = dict(items=B, seconds=4, rate=44100, channels=4, with_dereverb_ms=round(with_ms, 2),
                                     with_dereverb_runs_ms=[round(t, 2) for t in with_runs],
                                     without_ms=round(base_ms, 2), without_runs_ms=[round(t, 2) for t in base_runs],
                                     feature_ms=round(with_ms - base_ms, 2),
                                     feature_share=round((with_ms - base_ms) / base_ms, 4),
                                     note="whole calls, file reads and writes included; with dereverb the four channels "
                                          "are resampled with the channels kept, without it they are mixed down first")
        save()
        print(f"# separate_files: {res['separate_files']}", file=sys.stderr, flush=True)
        model.close()
    line = json.dumps(res)
    print(line)
    save()


if __name__ == "__main__":
    main()
