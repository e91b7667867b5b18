"""Time the spatial mask refinement of the beamformer (Engine.beamform_spatial, dsn_beamform_spatial) and what
`spatial=True` adds to a separate_files call that already has beamform=True (one MI355X, inputs drawn once, seeded).
The workloads are those of scripts/beamform_time.py:
  array4_4s     64 x 4 channels x 2 sources x 4 s at 16 kHz
  array8_4s     64 x 8 channels x 4 sources x 4 s
  ragged_2_4s   64 items of 2 - 4 s with 2, 4 or 8 channels each in one call (lens, channels), 2 sources
  long_30s      one 8-channel item of 30 s, 4 sources
For each, at native.SPATIAL_DEFAULTS (one iteration) and at 10 iterations: milliseconds per call; Engine.beamform on the
same input in the same run, so the difference is what the refinement costs; and the same definition in torch on the same
GPU -- torch.stft, torch.linalg.cholesky, solve_triangular, complex128 einsum, torch.istft -- reported only (skipped with
a note if it fails; it runs the padded batch: it has no form for per-item lengths or channel counts).
  separate_files  LatentDiffSep.separate_files (full-size DiT and Oobleck, fp16, graphs on) on 64 four-channel s16 clips
                of 4 s at 44.1 kHz with beamform=True, spatial=True against beamform=True alone, in the same run
                (--no-files skips it).
HIP events around whole calls; 3 warm-up runs, then the median of 5 timed runs, with the runs listed.  A call is short,
so a timed run is `--reps` calls back to back (the torch form: `--torch-reps`) and the figure is per call.  These are
call times with the data resident in the Infinity Cache (the same tensors every call), not cold-HBM figures.
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


def torch_spatial(mix, est, ref, iterations, noise, floor, mask_reg, mask_eps):
    """the definition of include/ditsep_hip.h (dsn_beamform_spatial) in torch: mix [B, C, L], est [B, n, L] -> [B, n, L]"""
    (B, Cn, L), n = mix.shape, est.shape[1]
    w = torch.hann_window(N_FFT, periodic=True, device=mix.device)
    kw = dict(hop_length=HOP, win_length=N_FFT, window=w, center=True)
    Z = torch.stft(torch.cat([mix, est], dim=1).reshape(-1, L), N_FFT, pad_mode="reflect", return_complex=True, **kw)
    Z = Z.reshape(B, Cn + n, *Z.shape[1:])
    X, S = Z[:, :Cn], Z[:, Cn:]
    m = S.real ** 2 + S.imag ** 2
    M = ((m + EPS) / (m.sum(dim=1, keepdim=True) + n * EPS)).double()
    X64 = X.to(torch.complex128)                                                  # [B, C, bins, F]
    a = (1.0 - noise) * ((1.0 - floor) * M + floor / n)
    if noise > 0:
        a = torch.cat([a, torch.full_like(a[:, :1], noise)], dim=1)               # [B, K, bins, F]
    K = a.shape[1]
    eye = torch.eye(Cn, dtype=torch.complex128, device=mix.device)
    gamma = a
    if Cn > 1 and iterations > 0:
        p = (X64.real ** 2 + X64.imag ** 2).sum(dim=1)
        live = p > 0
        z = torch.where(live[:, None], X64 / p.sqrt().clamp_min(1e-300)[:, None], torch.zeros_like(X64))
        zc = z.permute(0, 2, 1, 3)[:, None]                                       # [B, 1, bins, C, F]
        Bk = eye.expand(B, K, Z.shape[2], Cn, Cn).contiguous()

        def e_step(Bk):
            Lc = torch.linalg.cholesky(Bk)
            y = torch.linalg.solve_triangular(Lc, zc.expand(B, K, *zc.shape[2:]), upper=False)
            q = (y.real ** 2 + y.imag ** 2).sum(dim=-2)                           # [B, K, bins, F]
            ell = 2.0 * torch.diagonal(Lc, dim1=-2, dim2=-1).real.log().sum(dim=-1)
            g = torch.softmax(a.log() - ell[..., None] - Cn * q.log(), dim=1)
            return torch.where(live[:, None], g, a), q

        for _ in range(iterations):
            g, q = e_step(Bk)
            wgt = torch.where(live[:, None], g / q, torch.zeros_like(g))
            den = torch.where(live[:, None], g, torch.zeros_like(g)).sum(dim=-1)
            Sm = torch.einsum("bkcft,bdft->bkfcd", wgt[:, :, None] * z[:, None], z.conj())
            Bk = Cn * Sm / den[..., None, None]
            tr = torch.einsum("bkfcc->bkf", Bk).real
            Bk = Bk + (mask_reg * tr / Cn + mask_eps)[..., None, None] * eye
        gamma, _ = e_step(Bk)
    N = torch.einsum("bkcft,bdft->bkfcd", gamma[:, :, None] * X64[:, None], X64.conj())   # [B, K, bins, C, C]
    Q = (N.sum(dim=1, keepdim=True) - N)[:, :n]
    lam = REG * torch.einsum("bifcc->bif", Q).real / Cn + EPS
    Zs = torch.linalg.solve(Q + lam[..., None, None] * eye, N[:, :n])
    tau = torch.einsum("bifcc->bif", Zs).real
    wt = Zs[..., ref] / tau[..., None]                                            # [B, n, bins, C]
    Y = torch.einsum("bifc,bcft->bift", wt.conj(), X64).to(torch.complex64)
    y = torch.istft(Y.reshape(-1, *Y.shape[-2:]), N_FFT, length=L, **kw)
    return y.reshape(B, n, L)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=64)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--torch-reps", type=int, default=1)
    ap.add_argument("--no-files", action="store_true")
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("spatial_time.py measures on the GPU; none is available")
    eng = native.Engine(score_kind=native.SCORE_NONE, vae_has_encoder=False, vae_has_decoder=False)
    eng.finalize()
    dev, B = eng.device, a.items
    g = torch.Generator().manual_seed(2026)
    res = {"items": B, "n_fft": N_FFT, "hop": HOP, "warmup": a.warmup, "iters": a.iters, "reps": a.reps,
           "torch_reps": a.torch_reps}

    def run(fn, reps):
        def many():
            for _ in range(reps):
                fn()
        ms, times = median_ms(many, a.warmup, a.iters)
        return ms / reps, [round(t / reps, 4) for t in times]

    def draw(items, Cn, n, L, taps=8):
        """scripts/beamform_time.py's inputs: white sources through random short mixing filters plus sensor noise; the
        estimates are the noisy images at channel 0"""
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
        bins, F = N_FFT // 2 + 1, 1 + (L + HOP - 1) // HOP
        rec = dict(shape=[items, Cn, n, L], solve_workgroups=items * bins, frames=F,
                   workspace_bytes=items * native.spatial_item_bytes(N_FFT, HOP, L, Cn, n))
        kw = dict(lens=lens, channels=channels, n_fft=N_FFT, hop=HOP, eps=EPS, reg=REG)
        ms, times = run(lambda: eng.beamform(mix, est, **kw), a.reps)
        rec["beamform"] = dict(ms=round(ms, 4), runs_ms=times)
        for tag, iterations in (("defaults", native.SPATIAL_DEFAULTS["iterations"]), ("iterations_10", 10)):
            opts = dict(native.SPATIAL_DEFAULTS, iterations=iterations)
            skw = dict(kw, iterations=iterations, noise=opts["noise"], floor=opts["floor"], mask_reg=opts["reg"],
                       mask_eps=opts["eps"])
            ms_s, times = run(lambda: eng.beamform_spatial(mix, est, **skw), a.reps)
            rec[tag] = dict(ms=round(ms_s, 4), runs_ms=times, refinement_ms=round(ms_s - ms, 4),
                            over_beamform=round(ms_s / ms, 2))
            if a.no_torch:
                continue
            try:
                targs = (mix, est, 0, iterations, opts["noise"], opts["floor"], opts["reg"], opts["eps"])
                want = torch_spatial(*targs)
                if lens is None:
                    got = eng.beamform_spatial(mix, est, **skw)
                    rec[tag]["torch_max_abs_diff"] = float((got - want).abs().max())
                del want
                tms, ttimes = run(lambda: torch_spatial(*targs), a.torch_reps)
                rec[tag].update(torch_ms=round(tms, 4), torch_runs_ms=ttimes, torch_over_native=round(tms / ms_s, 2))
                if lens is not None:
                    rec[tag]["torch_note"] = ("torch runs the padded batch: it has no form for per-item lengths or "
                                              "channel counts")
            except Exception as e:                                              # reported only
                rec[tag]["torch_note"] = f"skipped: {type(e).__name__}: {e}"
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
            with_ms, with_runs = median_ms(lambda: model.separate_files(paths, os.path.join(tmp, "spatial"),
                                                                        spatial=True, **kw), a.warmup, a.iters)
            base_ms, base_runs = median_ms(lambda: model.separate_files(paths, os.path.join(tmp, "beam"), **kw),
                                           a.warmup, a.iters)
        res["separate_files"] = dict(items=B, seconds=4, rate=44100, channels=4, with_spatial_ms=round(with_ms, 2),
                                     with_spatial_runs_ms=[round(t, 2) for t in with_runs],
                                     beamform_only_ms=round(base_ms, 2),
                                     beamform_only_runs_ms=[round(t, 2) for t in base_runs],
                                     feature_ms=round(with_ms - base_ms, 2),
                                     feature_share=round((with_ms - base_ms) / base_ms, 4),
                                     note="whole calls with beamform=True, file reads and writes included")
        print(f"# separate_files: {res['separate_files']}", file=sys.stderr, flush=True)
        model.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
