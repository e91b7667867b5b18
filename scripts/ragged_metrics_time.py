"""Time the scoring of a mixed-length batch: `--items` two-source items with lengths drawn once (seeded, all distinct)
between 2 s and 4 s at 16 kHz, for each of Engine.si_bss_eval, Engine.stoi (extended) and Engine.composite
  one_call   one call on the padded [B, 2, Lmax] batch with lens= (dsn_*_ragged), the route evaluate_batches takes,
  per_group  one dense call per group of equal length (with distinct lengths, one call per item), the route it took
             before; stoi and composite get the permutation si_bss_eval found, as there.
  dense_4s   the dense call on as many full 4 s items: what the padded batch would cost if every item were Lmax long.
HIP events around whole calls (the stacking of a group included, as the harness paid it); the median of `--iters`
runs after `--warmup` calls.  Also checks that both routes return identical values.
Prints one JSON line; --out also writes it to a file."""
import argparse
import json
import os
import statistics
import sys
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from ditsep_amd import native, synthetic  # noqa: E402
from ditsep_amd.evaluate import _pad_items  # noqa: E402

FS, N_SRC = 16000, 2


def median_ms(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    return statistics.median(times), times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=64)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ragged_metrics_time.py measures on the GPU; none is available")
    warnings.simplefilter("ignore", RuntimeWarning)
    eng = native.Engine(score_kind=native.SCORE_NONE, vae_has_encoder=False, vae_has_decoder=False)
    dev = eng.device
    B = a.items
    g = torch.Generator().manual_seed(2024)
    lens = (2 * FS + torch.randperm(2 * FS + 1, generator=g)[:B]).tolist()           # distinct by construction
    src = synthetic.synthetic_sources(B, N_SRC, 4 * FS, FS, seed=1234)
    noisy = src + 0.3 * torch.randn(src.shape, generator=g) * src.abs().amax(-1, True) + 0.2 * src.flip(1)
    refs = [src[b, :, :L].contiguous().to(dev) for b, L in enumerate(lens)]
    ests = [noisy[b, :, :L].contiguous().to(dev) for b, L in enumerate(lens)]
    ref_p, est_p = _pad_items(refs, max(lens), dev), _pad_items(ests, max(lens), dev)
    perm = eng.si_bss_eval(ref_p, est_p, lens=lens)[3]
    groups = {}
    for i, L in enumerate(lens):
        groups.setdefault(L, []).append(i)

    def per_group(call):
        def fn():
            out = {}
            for _, members in groups.items():
                tgt = torch.stack([refs[i] for i in members])
                xr = torch.stack([ests[i] for i in members])
                got = call(tgt, xr, perm[members])
                for j, i in enumerate(members):
                    out[i] = [v[j] for v in got]
            return [torch.stack([out[i][k] for i in range(B)]) for k in range(len(out[0]))]
        return fn

    comp_keys = ("llr", "wss", "segsnr", "snr", "frames")

    def comp(res):
        return [res[k] for k in comp_keys]

    ref_d, est_d = src.to(dev), noisy.to(dev)
    dense = {"si_bss_eval": lambda: eng.si_bss_eval(ref_d, est_d),
             "stoi": lambda: eng.stoi(ref_d, est_d, FS, perm=perm),
             "composite": lambda: eng.composite(ref_d, est_d, FS, perm=perm)}
    metrics = {
        "si_bss_eval": (lambda: list(eng.si_bss_eval(ref_p, est_p, lens=lens)),
                        per_group(lambda r, e, p: list(eng.si_bss_eval(r, e)))),
        "stoi": (lambda: list(eng.stoi(ref_p, est_p, FS, perm=perm, return_frames=True, lens=lens)),
                 per_group(lambda r, e, p: list(eng.stoi(r, e, FS, perm=p, return_frames=True)))),
        "composite": (lambda: comp(eng.composite(ref_p, est_p, FS, perm=perm, lens=lens)),
                      per_group(lambda r, e, p: comp(eng.composite(r, e, FS, perm=p)))),
    }
    res = {"items": B, "n_src": N_SRC, "fs": FS, "seconds": [2, 4], "len_min": min(lens), "len_max": max(lens),
           "length_groups": len(groups), "warmup": a.warmup, "iters": a.iters}
    for name, (one_call, grouped) in metrics.items():
        same = all(torch.equal(x, y) for x, y in zip(one_call(), grouped()))
        ms1, t1 = median_ms(one_call, a.warmup, a.iters)
        msg, tg = median_ms(grouped, a.warmup, a.iters)
        msd, _ = median_ms(dense[name], a.warmup, a.iters)
        res[name] = {"one_call_ms": round(ms1, 3), "per_group_ms": round(msg, 3), "ratio": round(msg / ms1, 2),
                     "dense_4s_ms": round(msd, 3), "identical": same, "one_call_runs_ms": [round(t, 3) for t in t1],
                     "per_group_runs_ms": [round(t, 3) for t in tg]}
    eng.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
