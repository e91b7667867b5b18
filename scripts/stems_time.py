"""Time the multichannel stems filter (Engine.stems, dsn_stems), the interleaving encoder (Engine.pcm_encode_frames) and
what `stems="wiener"` adds to separate_files (one MI355X, inputs drawn once, seeded).
  dense_4s      64 x stereo x 2 sources x 4 s at 16 kHz, both modes
  ragged_2_4s   64 items of 2 - 4 s in one call (lens), both modes
  long_30s      one stereo item of 30 s, both modes
For each: milliseconds per call and the algorithmic bytes (mixture and estimates read once, stems written once) per
second, and beside it the same definition in torch on the same GPU -- torch.stft, float64 einsum statistics,
torch.linalg.solve, torch.istft -- reported only (skipped with a note if it fails; it runs the padded batch: it has no
form for per-item lengths).
  encode_frames 128 stereo rows of 4 s -> interleaved s16, against transpose / round / clamp / cast in torch
  separate_files  LatentDiffSep.separate_files (full-size DiT and Oobleck, fp16, graphs on) on 64 stereo s16 clips of 4 s
                at 44.1 kHz with stems="wiener" against the call without it, in the same run (--no-files skips it).
HIP events around whole calls; 3 warm-up runs, then the median of 5 timed runs, with the runs listed.  A filter call is
short, so a timed run is `--reps` calls back to back and the figure is per call.  These are call times with the data
resident in the Infinity Cache (the same tensors every call), not cold-HBM figures.
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
from scripts.ragged_time import FS, median_ms  # noqa: E402
from scripts.resample_time import full_size_model  # noqa: E402

N_FFT, HOP, EPS, REG = 512, 128, 1e-10, 1e-3


def torch_stems(mix, est, mode):
    """the definition of include/ditsep_hip.h (dsn_stems) in torch: mix [B, C, L], est [B, n, L] -> [B, n, C, L]"""
    (B, Cn, L), n = mix.shape, est.shape[1]
    w = torch.hann_window(N_FFT, periodic=True, device=mix.device)
    kw = dict(hop_length=HOP, win_length=N_FFT, window=w, center=True)
    Z = torch.stft(torch.cat([mix, est], dim=1).reshape(-1, L), N_FFT, pad_mode="reflect", return_complex=True, **kw)
    Z = Z.reshape(B, Cn + n, *Z.shape[1:])
    X, S = Z[:, :Cn], Z[:, Cn:]
    a = S.real ** 2 + S.imag ** 2
    M = (a + EPS) / (a.sum(dim=1, keepdim=True) + n * EPS)
    if mode == "mask":
        Y = M[:, :, None] * X[:, None]
    else:
        X64, m2 = X.to(torch.complex128), M.double() ** 2
        v = m2 * (X64.real ** 2 + X64.imag ** 2).mean(dim=1, keepdim=True)
        N = torch.einsum("bift,bcft,bdft->bifcd", m2.to(torch.complex128), X64, X64.conj())
        d = v.sum(dim=-1)
        eye = torch.eye(Cn, dtype=torch.complex128, device=mix.device)
        R = torch.where((d != 0)[..., None, None], N / d[..., None, None], eye)
        Sig = torch.einsum("bift,bifcd->bftcd", v.to(torch.complex128), R)
        lam = REG * torch.einsum("bftcc->bft", Sig).real / Cn + EPS
        z = torch.linalg.solve(Sig + lam[..., None, None] * eye, X64.permute(0, 2, 3, 1)[..., None])[..., 0]
        Y = v[..., None] * torch.einsum("bifcd,bftd->biftc", R, z) + (lam / n)[:, None, ..., None] * z[:, None]
        Y = Y.permute(0, 1, 4, 2, 3).to(torch.complex64)
    y = torch.istft(Y.reshape(-1, *Y.shape[-2:]), N_FFT, length=L, **kw)
    return y.reshape(B, n, Cn, L)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=64)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no-files", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("stems_time.py measures on the GPU; none is available")
    eng = native.Engine(score_kind=native.SCORE_NONE, vae_has_encoder=False, vae_has_decoder=False)
    eng.finalize()
    dev, B, n, Cn = eng.device, a.items, 2, 2
    g = torch.Generator().manual_seed(2025)
    res = {"items": B, "n": n, "channels": Cn, "n_fft": N_FFT, "hop": HOP, "warmup": a.warmup, "iters": a.iters,
           "reps": a.reps}

    def run(fn):
        def many():
            for _ in range(a.reps):
                fn()
        ms, times = median_ms(many, a.warmup, a.iters)
        return ms / a.reps, [round(t / a.reps, 4) for t in times]

    def draw(items, L):
        src = 0.1 * torch.randn((items, n, L), generator=g)
        pan = 0.2 + 0.8 * torch.rand((items, n, Cn), generator=g)
        mix = torch.einsum("bic,bil->bcl", pan, src)
        est = pan.mean(dim=2, keepdim=True) * src + 0.03 * torch.randn((items, n, L), generator=g)
        return mix.to(dev), est.to(dev)

    def timed(name, mix, est, lens=None):
        items, _, L = mix.shape
        samples = sum(lens) if lens else items * L
        nbytes = 4.0 * samples * (Cn + n + n * Cn)
        rec = dict(shape=[items, Cn, n, L], algorithmic_bytes=nbytes)
        for mode in ("mask", "wiener"):
            ms, times = run(lambda: eng.stems(mix, est, lens=lens, mode=mode, n_fft=N_FFT, hop=HOP, eps=EPS, reg=REG))
            rec[mode] = dict(ms=round(ms, 4), runs_ms=times, gbytes_per_s=round(nbytes / ms * 1e-6, 1))
            try:
                want = torch_stems(mix, est, mode)
                if lens is None:
                    got = eng.stems(mix, est, mode=mode, n_fft=N_FFT, hop=HOP, eps=EPS, reg=REG)
                    rec[mode]["torch_max_abs_diff"] = float((got - want).abs().max())
                tms, ttimes = run(lambda: torch_stems(mix, est, mode))
                rec[mode].update(torch_ms=round(tms, 4), torch_runs_ms=ttimes, torch_over_native=round(tms / ms, 2))
                if lens is not None:
                    rec[mode]["torch_note"] = "torch runs the padded batch: it has no form for per-item lengths"
            except Exception as e:                                              # reported only
                rec[mode]["torch_note"] = f"skipped: {type(e).__name__}: {e}"
        res[name] = rec
        print(f"# {name}: {rec}", file=sys.stderr, flush=True)

    timed("dense_4s", *draw(B, 4 * FS))
    lens = torch.randint(2 * FS, 4 * FS + 1, (B,), generator=g).tolist()
    lens[0] = 4 * FS
    timed("ragged_2_4s", *draw(B, 4 * FS), lens=lens)
    timed("long_30s", *draw(1, 30 * FS))

    rows = (0.4 * torch.randn((128, Cn, 4 * FS), generator=g)).to(dev)
    buf = torch.zeros(rows.numel() * 2, dtype=torch.uint8, device=dev)
    offs = [r * Cn * 4 * FS * 2 for r in range(128)]
    i32, i64 = native.C.c_int32 * 128, native.C.c_int64 * 128
    ln, ch, of = i32(*[4 * FS] * 128), i32(*[Cn] * 128), i64(*offs)

    def encode():                                                               # the device call alone: no copy back
        eng._check(eng.lib.dsn_pcm_encode_frames(eng.ctx, native._ptr(rows), 128, Cn, 4 * FS, ln, ch,
                                                 native.PCM_ENCODINGS["s16"], native._ptr(buf), buf.numel(), of, None,
                                                 eng._stream()), "dsn_pcm_encode_frames")

    def encode_torch():
        return (rows.transpose(1, 2) * 32768.0).round().clamp(-32768.0, 32767.0).to(torch.int16).contiguous()

    ms, times = run(encode)
    tms, ttimes = run(encode_torch)
    nbytes = rows.numel() * 6.0
    same = bool(torch.equal(buf.view(torch.int16), encode_torch().reshape(-1)))
    res["encode_frames"] = dict(shape=list(rows.shape), encoding="s16", algorithmic_bytes=nbytes, ms=round(ms, 4),
                                runs_ms=times, gbytes_per_s=round(nbytes / ms * 1e-6, 1), torch_ms=round(tms, 4),
                                torch_runs_ms=ttimes, torch_over_native=round(tms / ms, 2), torch_same_bytes=same,
                                note="the native call also uploads its row table and counts clipped samples")
    print(f"# encode_frames: {res['encode_frames']}", file=sys.stderr, flush=True)
    eng.close()

    if not a.no_files:
        model = full_size_model()
        src = synthetic.synthetic_sources(B, 2, 4 * 44100, 44100, seed=1234)                  # [B, 2, L]: two speakers
        pan = torch.tensor([[0.9, 0.3], [0.2, 0.8]])
        stereo = torch.einsum("ic,bil->blc", pan, src).clamp(-1.0, 1.0)                       # [B, L, 2] interleaved
        with tempfile.TemporaryDirectory() as tmp:
            paths = []
            for b in range(B):
                paths.append(os.path.join(tmp, f"clip{b:03d}.wav"))
                wavio.write_wav(paths[-1], (stereo[b] * 32767.0).round().to(torch.int16).numpy().astype("<i2").tobytes(),
                                44100, 2, "s16")
            kw = dict(batch=B, seed=7)
            with_ms, with_runs = median_ms(lambda: model.separate_files(paths, os.path.join(tmp, "stems"),
                                                                        stems="wiener", **kw), a.warmup, a.iters)
            base_ms, base_runs = median_ms(lambda: model.separate_files(paths, os.path.join(tmp, "mono"), **kw),
                                           a.warmup, a.iters)
        res["separate_files"] = dict(items=B, seconds=4, rate=44100, channels=2, with_stems_ms=round(with_ms, 2),
                                     with_stems_runs_ms=[round(t, 2) for t in with_runs],
                                     without_ms=round(base_ms, 2), without_runs_ms=[round(t, 2) for t in base_runs],
                                     feature_ms=round(with_ms - base_ms, 2),
                                     feature_share=round((with_ms - base_ms) / base_ms, 4),
                                     note="whole calls, file reads and writes included; with stems the outputs are "
                                          "stereo: twice the bytes encoded and written")
        print(f"# separate_files: {res['separate_files']}", file=sys.stderr, flush=True)
        model.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
