"""Time the designs of the beamforming weights (Engine.beamform(design=), dsn_beamform_design) against Souden's filter
(Engine.beamform as it was) in the same run, with the protocol and the four workloads of scripts/beamform_time.py (one
MI355X, inputs drawn once, seeded).
  array4_4s     64 x 4 channels x 2 sources x 4 s at 16 kHz
  array8_4s     64 x 8 channels x 4 sources x 4 s
  ragged_2_4s   64 items of 2 - 4 s with 2, 4 or 8 channels each in one call (lens, channels), 2 sources
  long_30s      one 8-channel item of 30 s, 4 sources
For each: milliseconds per whole call for "souden", "rank1" and "gev" (ten Jacobi sweeps) and each design's ratio to
Souden's call; and the weights launch alone (Engine.beamform_solve, dsn_beamform_solve) on float64 statistics of the
workload's shape -- items x sources x 257 bins systems of C x C, random Hermitian positive semidefinite -- for the three
designs: the eigen-solver against the one Cholesky solve it stands beside.
HIP events around whole calls; 3 warm-up runs, then the median of 5 timed runs, with the runs listed.  A call is short,
so a timed run is `--reps` calls back to back and the figure is per call.  These are call times with the data resident
in the Infinity Cache (the same tensors every call), not cold-HBM figures.
Prints one JSON line; --out also writes it to a file."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from ditsep_amd import native  # noqa: E402
from scripts.ragged_time import FS, median_ms  # noqa: E402

N_FFT, HOP, EPS, REG = 512, 128, 1e-10, 1e-3
DESIGNS = ("souden", "rank1", "gev")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=64)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--sweeps", type=int, default=native.DESIGN_DEFAULTS["sweeps"])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("beamform_design_time.py measures on the GPU; none is available")
    eng = native.Engine(score_kind=native.SCORE_NONE, vae_has_encoder=False, vae_has_decoder=False)
    eng.finalize()
    dev, B = eng.device, a.items
    g = torch.Generator().manual_seed(2026)
    res = {"items": B, "n_fft": N_FFT, "hop": HOP, "sweeps": a.sweeps, "warmup": a.warmup, "iters": a.iters,
           "reps": a.reps}

    def run(fn):
        def many():
            for _ in range(a.reps):
                fn()
        ms, times = median_ms(many, a.warmup, a.iters)
        return ms / a.reps, [round(t / a.reps, 4) for t in times]

    def draw(items, Cn, n, L, taps=8):
        """scripts/beamform_time.py's mixtures: white sources through random short mixing filters plus sensor noise;
        the estimates are the noisy images at channel 0"""
        src = 0.1 * torch.randn((items, n, L), generator=g)
        h = torch.randn((items, n, Cn, taps), generator=g) * 0.3
        h[..., 0] = 1.0
        img = torch.zeros((items, n, Cn, L))
        for k in range(taps):
            img[..., k:] += h[..., k, None] * src[:, :, None, :L - k]
        mix = img.sum(dim=1) + 0.001 * torch.randn((items, Cn, L), generator=g)
        est = img[:, :, 0] + 0.03 * torch.randn((items, n, L), generator=g)
        return mix.to(dev), est.to(dev)

    def statistics(items, Cn, n, bins):
        """random Hermitian positive semidefinite classes in the layout dsn_beamform_solve reads"""
        A = torch.randn((items, n, bins, Cn, Cn + 2), generator=g, dtype=torch.float64)
        A = torch.complex(A, torch.randn(A.shape, generator=g, dtype=torch.float64))
        N = A @ A.transpose(-1, -2).conj()
        planes = []
        for c1 in range(Cn):
            for c2 in range(c1, Cn):
                planes += [N[..., c1, c2].real, N[..., c1, c2].imag]
        return torch.stack(planes, dim=2).contiguous().to(dev)                  # [items, n, C (C + 1), bins]

    def timed(name, mix, est, lens=None, channels=None):
        (items, Cn, L), n = mix.shape, est.shape[1]
        rec = dict(shape=[items, Cn, n, L])
        kw = dict(lens=lens, channels=channels, n_fft=N_FFT, hop=HOP, eps=EPS, reg=REG)
        for kind in DESIGNS:
            design = None if kind == "souden" else dict(kind=kind, sweeps=a.sweeps)
            ms, times = run(lambda: eng.beamform(mix, est, design=design, **kw))
            rec[kind] = dict(ms=round(ms, 4), runs_ms=times)
            if kind != "souden":
                rec[kind]["over_souden"] = round(ms / rec["souden"]["ms"], 3)
        N = statistics(items, Cn, n, N_FFT // 2 + 1)
        solve = {}
        for kind in DESIGNS:
            ms, times = run(lambda: eng.beamform_solve(N, channels=channels, reg=REG, eps=EPS,
                                                       design=dict(kind=kind, sweeps=a.sweeps)))
            solve[kind] = dict(ms=round(ms, 4), runs_ms=times)
            if kind != "souden":
                solve[kind]["over_souden"] = round(ms / solve["souden"]["ms"], 2)
        rec["solve_alone"] = dict(systems=items * n * (N_FFT // 2 + 1), **solve,
                                  note="Engine.beamform_solve: the weights launch, the allocation of its output and, "
                                       "with channels, their upload")
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
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
