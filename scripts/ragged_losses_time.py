"""Time the two losses on a mixed-length batch, by the protocol of scripts/ragged_metrics_time.py: `--items` two-source
items with lengths drawn once (seeded, all distinct) between 2 s and 4 s at 16 kHz.
  mrstft      Engine.mrstft_loss at its defaults (seven resolutions, A-weighting)
                one_call   one call on the padded [B, 2, Lmax] batch with lens= (dsn_mrstft_loss_ragged)
                per_group  one dense call per group of equal length (with distinct lengths, one call per item), the only
                           route before; the stacking of a group is inside the timed region, as a harness pays it
  score_loss  Engine.score_loss (DSM, reduction "none", injected t and z) on the full-size DiT in fp16; the items'
              latents are random tensors of the items' frame counts (1 + L / 2048: 16 .. 32 frames)
                one_call   one call on the padded [B, ., 64, Tmax] batch with frames= (dsn_score_loss_ragged)
                per_group  one dense call per group of equal frame count
HIP events around whole calls; the median of `--iters` runs after `--warmup` calls.  Also reports how far the two routes'
values are apart (mrstft: identical bits expected; score_loss: the score call's rounding under another batch shape).
Prints one JSON line; --out also writes it to a file."""
import argparse
import json
import os
import sys
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from ditsep_amd import native, synthetic  # noqa: E402
from ditsep_amd.evaluate import _pad_items  # noqa: E402
from scripts.ragged_metrics_time import FS, N_SRC, median_ms  # noqa: E402

HOP, D = 2048, 64
KEYS = ("sc", "log_mag", "lin_mag", "l1", "l2")


def entry(one_call, grouped, far, warmup, iters):
    ms1, t1 = median_ms(one_call, warmup, iters)
    msg, tg = median_ms(grouped, warmup, iters)
    return {"one_call_ms": round(ms1, 3), "per_group_ms": round(msg, 3), "ratio": round(msg / ms1, 2),
            "max_rel_difference": far, "one_call_runs_ms": [round(t, 3) for t in t1],
            "per_group_runs_ms": [round(t, 3) for t in tg]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=64)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ragged_losses_time.py measures on the GPU; none is available")
    warnings.simplefilter("ignore", RuntimeWarning)
    B = a.items
    g = torch.Generator().manual_seed(2024)
    lens = (2 * FS + torch.randperm(2 * FS + 1, generator=g)[:B]).tolist()           # distinct by construction
    res = {"items": B, "n_src": N_SRC, "fs": FS, "seconds": [2, 4], "len_min": min(lens), "len_max": max(lens),
           "warmup": a.warmup, "iters": a.iters}

    # ---- MR-STFT loss
    eng = native.Engine(score_kind=native.SCORE_NONE, vae_has_encoder=False, vae_has_decoder=False)
    dev = eng.device
    src = synthetic.synthetic_sources(B, N_SRC, 4 * FS, FS, seed=1234)
    noisy = src + 0.3 * torch.randn(src.shape, generator=g) * src.abs().amax(-1, True) + 0.2 * src.flip(1)
    refs = [src[b, :, :L].contiguous().to(dev) for b, L in enumerate(lens)]
    ests = [noisy[b, :, :L].contiguous().to(dev) for b, L in enumerate(lens)]
    ref_p, est_p = _pad_items(refs, max(lens), dev), _pad_items(ests, max(lens), dev)
    groups = {}
    for i, L in enumerate(lens):
        groups.setdefault(L, []).append(i)

    def mr_one():
        return eng.mrstft_loss(ref_p, est_p, FS, pit=None, lens=lens)

    def mr_grouped():
        out = {}
        for members in groups.values():
            tabs = eng.mrstft_loss(torch.stack([refs[i] for i in members]), torch.stack([ests[i] for i in members]), FS,
                                   pit=None)
            for j, i in enumerate(members):
                out[i] = {k: tabs[k][..., j, :, :] for k in KEYS}
        return {k: torch.stack([out[i][k] for i in range(B)], dim=-3) for k in KEYS}

    x, y = mr_one(), mr_grouped()
    far = max(float(((x[k] - y[k]).abs() / y[k].abs()).max()) for k in KEYS if y[k].numel() and y[k].any())
    res["mrstft"] = dict(entry(mr_one, mr_grouped, far, a.warmup, a.iters), length_groups=len(groups))
    eng.close()

    # ---- score-matching loss on the full-size DiT, fp16
    dcfg = synthetic.DiTConfig()
    eng = native.Engine(precision=native.PREC_FP16, score_kind=native.SCORE_DIT, n_src=dcfg.n_src,
                        latent_dim=dcfg.latent_dim, dit_embed_dim=dcfg.embed_dim, dit_depth=dcfg.depth,
                        dit_heads=dcfg.num_heads, vae_has_encoder=False, vae_has_decoder=False)
    eng.load_state_dict(synthetic.random_dit_weights(dcfg, 1, out_gain=0.002, skip_gain=0.02), prefix="score_model.")
    eng.finalize()
    frames = [L // HOP + 1 for L in lens]
    T, n = max(frames), dcfg.n_src
    mix, tgt, z = torch.zeros((B, 1, D, T)), torch.zeros((B, n, D, T)), torch.zeros((B, n, D, T))
    for b, f in enumerate(frames):
        mix[b, ..., :f] = torch.randn((1, D, f), generator=g)
        tgt[b, ..., :f] = 0.7 * torch.randn((n, D, f), generator=g)
        z[b, ..., :f] = torch.randn((n, D, f), generator=g)
    t = 0.03 + 0.97 * torch.rand(B, generator=g)
    mix, tgt, z, t = (v.to(dev) for v in (mix, tgt, z, t))
    fgroups = {}
    for i, f in enumerate(frames):
        fgroups.setdefault(f, []).append(i)

    def sl_one():
        return eng.score_loss(mix, tgt, time=t, noise=z, frames=frames)

    def sl_grouped():
        out = torch.empty((B, n), device=dev)
        for f, members in fgroups.items():
            out[members] = eng.score_loss(mix[members][..., :f], tgt[members][..., :f], time=t[members],
                                          noise=z[members][..., :f])
        return out

    x, y = sl_one(), sl_grouped()
    far = float(((x - y).abs() / y.abs()).max())
    res["score_loss"] = dict(entry(sl_one, sl_grouped, far, a.warmup, a.iters), frame_groups=len(fgroups),
                             frames_min=min(frames), frames_max=max(frames), precision="fp16",
                             dit=[dcfg.embed_dim, dcfg.depth, dcfg.num_heads])
    eng.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
