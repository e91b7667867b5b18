"""Time Engine.bss_eval (dsn_bss_eval) with HIP events around whole calls -- median of 5 after 3 warm-ups -- on
  c2_64x2x4s      the C2 evaluation batch: 64 mixtures of 2 sources, 4 s at 16 kHz, 512 taps
  1x2x30s         one 30 s item
  ragged_64x2     64 items of 2 .. 4 s in one call (lens=)
next to the same definition written with torch.fft (the correlations), torch.linalg.cholesky and solve_triangular in
float64 on the same GPU -- fast_bss_eval's formulation; a ragged batch is zero-padded there, which the definition
allows (every signal is zero-extended).  The largest |device - torch| of the call is reported with the times.
Prints one JSON line; --out also writes it (profiles/bss_eval_mi355x.json is such a file)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from ditsep_amd import native, synthetic  # noqa: E402

WARMUP, RUNS = 3, 5


def torch_bss_eval(ref, est, F):
    """ref, est [B,n,L] (zero past an item's end) -> sdr_pairs, sir_pairs [B,n,n], sar_j [B,n] in float64"""
    r, e = ref.double(), est.double()
    B, n, L = r.shape
    en = r.pow(2).sum(-1, keepdim=True)
    r = r * torch.where(en > 0, en.clamp_min(1e-300).rsqrt(), torch.zeros_like(en))
    N = 1 << (L + F - 1).bit_length()
    Rf, Ef = torch.fft.rfft(r, N), torch.fft.rfft(e, N)
    cc = torch.fft.irfft(Rf.conj()[:, :, None] * Rf[:, None], N)                  # [B,i,j,k]: c_ij[k], k mod N
    lag = (torch.arange(F, device=r.device)[:, None] - torch.arange(F, device=r.device)[None]) % N
    G5 = cc[..., lag].permute(0, 1, 3, 2, 4)                                      # [B,i,p,j,q] = c_ij[p - q]
    D4 = torch.fft.irfft(Rf.conj()[:, :, None] * Ef[:, None], N)[..., :F].permute(0, 1, 3, 2)   # [B,i,p,j]
    ee = e.pow(2).sum(-1)
    G, D = G5.reshape(B, n * F, n * F), D4.reshape(B, n * F, n)
    Y = torch.linalg.solve_triangular(torch.linalg.cholesky(G), D, upper=False)
    pall = Y.pow(2).sum(1)                                                        # [B,j]
    idx = torch.arange(n, device=r.device)
    Gi = G5[:, idx, :, idx].permute(1, 0, 2, 3).reshape(B * n, F, F)              # the diagonal blocks
    Yi = torch.linalg.solve_triangular(torch.linalg.cholesky(Gi), D4.reshape(B * n, F, n), upper=False)
    pt = Yi.pow(2).sum(1).reshape(B, n, n)                                        # [B,i,j]

    def db(num, den):
        return 10 * torch.log10(num.clamp_min(1e-300) / den.clamp_min(1e-300))

    return db(pt, ee[:, None] - pt), db(pt, pall[:, None] - pt), db(pall, ee - pall)


def timed(fn):
    for _ in range(WARMUP):
        out = fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(RUNS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return round(statistics.median(ms), 3), [round(v, 3) for v in ms], out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--taps", type=int, default=512)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    fs, F = 16000, a.taps
    eng = native.Engine(score_kind=native.SCORE_NONE, vae_has_encoder=False, vae_has_decoder=False)
    g = torch.Generator().manual_seed(11)
    ragged_lens = torch.randint(2 * fs, 4 * fs + 1, (64,), generator=g).tolist()
    res = {"protocol": f"HIP events around whole calls, median of {RUNS} after {WARMUP} warm-ups", "fs": fs, "taps": F,
           "device": torch.cuda.get_device_name(0)}
    for name, (B, n, L, lens) in {"c2_64x2x4s": (64, 2, 4 * fs, None), "1x2x30s": (1, 2, 30 * fs, None),
                                  "ragged_64x2": (64, 2, max(ragged_lens), ragged_lens)}.items():
        ref = synthetic.synthetic_sources(B, n, L, fs=fs, seed=7)
        mix = torch.eye(n) + 0.1 * (1 - torch.eye(n))
        est = torch.einsum("ij,bjt->bit", mix, ref) + 0.005 * torch.randn(ref.shape, generator=g)
        if lens is not None:
            for b, l in enumerate(lens):
                ref[b, :, l:] = 0.0
                est[b, :, l:] = 0.0
        ref_d, est_d = ref.cuda(), est.cuda()
        plan = native.bss_eval_plan(B, n, L, F)
        row = {"B": B, "n": n, "L": L, "ragged": lens is not None, "items_per_chunk": plan["items_per_chunk"],
               "workspace_mib": round(plan["workspace_bytes"] / 2 ** 20, 1)}
        row["device_ms"], row["device_ms_runs"], dev = timed(
            lambda: eng.bss_eval(ref_d, est_d, filter_length=F, lens=lens, return_pairs=True))
        row["device_sdr_only_ms"], _, _ = timed(
            lambda: eng.bss_eval(ref_d, est_d, filter_length=F, lens=lens, sir_sar=False))
        try:
            row["torch_ms"], row["torch_ms_runs"], tor = timed(lambda: torch_bss_eval(ref_d, est_d, F))
            sar_j = torch.gather(tor[2].cpu(), 1, dev[3])
            row["max_abs_diff_db"] = max(float((dev[4] - tor[0].cpu()).abs().max()),
                                         float((dev[5] - tor[1].cpu()).abs().max()), float((dev[2] - sar_j).abs().max()))
            row["device_over_torch"] = round(row["device_ms"] / row["torch_ms"], 3)
        except Exception as exc:   # the torch route may lack a solver or memory; the device figures stand alone
            row["torch_error"] = f"{type(exc).__name__}: {exc}"[:300]
        row["sdr_mean_db"] = round(float(dev[0].mean()), 3)
        res[name] = row
        del ref_d, est_d
        torch.cuda.empty_cache()
    eng.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
