"""Time the separation of mixtures of different lengths (full-size DiT and Oobleck, fp16, graphs on): `--items` mixtures
with lengths drawn once (seeded) uniformly between 2 s and 4 s at 16 kHz,
  ragged_grouped / ragged_padded   Engine.separate_ragged on the whole batch in the order evaluate.length_batches
           gives, with the codec once per group of equal frame count (codec="grouped") or once on the padded batch
           (codec="padded"); for each also the codec alone (encode_ragged + decode_ragged of a latent of the same shape)
           and its share of the call,
  single   the same mixtures one Engine.separate call each,
  dense    a dense batch of as many 4 s mixtures (Engine.separate): the upper bound.
HIP events around whole calls after a warm-up that lets every shape's graph be captured; the median of the repeated
runs.  Reports utterances per second for each and the share of padded tokens of the ragged batch.
Prints one JSON line; --out also writes it to a file."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from ditsep_amd import native, synthetic  # noqa: E402
from ditsep_amd.evaluate import length_batches  # noqa: E402

FS, N_STEPS, CORR, SNR, T_EPS = 16000, 30, 1, 0.5, 0.03
DIT_OUT_GAIN, DIT_SKIP_GAIN, DEC_IN_GAIN = 0.002, 0.02, 0.08      # bench.py's synthetic checkpoint


def build_engine():
    dcfg, vcfg = synthetic.DiTConfig(), synthetic.OobleckConfig()
    dsd = synthetic.random_dit_weights(dcfg, 1, out_gain=DIT_OUT_GAIN, skip_gain=DIT_SKIP_GAIN)
    vsd = synthetic.vae_weights(vcfg, 2, dec_in_gain=DEC_IN_GAIN)
    eng = native.Engine(precision=native.PREC_FP16, n_src=dcfg.n_src, score_kind=native.SCORE_DIT,
                        dit_embed_dim=dcfg.embed_dim, dit_depth=dcfg.depth, dit_heads=dcfg.num_heads,
                        latent_dim=dcfg.latent_dim, vae_channels=vcfg.channels, vae_c_mults=vcfg.c_mults,
                        vae_strides=vcfg.strides, vae_enc_latent_dim=vcfg.enc_latent_dim, vae_use_snake=vcfg.use_snake,
                        vae_final_tanh=vcfg.final_tanh)
    eng.load_state_dict(dsd, prefix="score_model.")
    eng.load_state_dict(vsd, prefix="vae.")
    eng.finalize()
    return eng, dcfg


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
        raise SystemExit("ragged_time.py measures on the GPU; none is available")
    eng, dcfg = build_engine()
    eng.enable_graphs(True)
    dev = eng.device
    B = a.items
    g = torch.Generator().manual_seed(2024)
    lengths = torch.randint(2 * FS, 4 * FS + 1, (B,), generator=g).tolist()
    src = synthetic.synthetic_sources(B, dcfg.n_src, 4 * FS, FS, seed=1234).sum(1, keepdim=True).to(dev)   # [B,1,4 s]
    order = length_batches(lengths, B)[0]
    mixes = [src[i, :, :lengths[i]].contiguous() for i in order]
    frames = [eng.latent_frames(m.shape[-1]) for m in mixes]
    kw = dict(N=N_STEPS, corrector_steps=CORR, snr=SNR, t_eps=T_EPS, seed=7)

    lens = [int(m.shape[-1]) for m in mixes]
    lat = 0.5 * torch.randn((B, dcfg.n_src, dcfg.latent_dim, max(frames)), device=dev)     # stands in for the sampler's output

    def ragged(mode):
        return lambda: eng.separate_ragged(mixes, codec=mode, **kw)

    def codec(mode):
        def fn():
            _, fr = eng.encode_ragged(mixes, None, seed=7, codec=mode)
            eng.decode_ragged(lat, fr, lens, codec=mode)
        return fn

    def single():
        for m in mixes:
            eng.separate(m[None], **kw)

    def dense():
        eng.separate(src, **kw)

    res = {"items": B, "seconds": [2, 4], "frames_min": min(frames), "frames_max": max(frames),
           "codec_groups": len(set(frames)),
           "padded_token_share": round(1.0 - sum(1 + f for f in frames) / (B * (1 + max(frames))), 4)}
    runs = [(f"ragged_{m}", ragged(m), a.iters) for m in native.CODEC_MODES]
    runs += [("single", single, max(2, a.iters // 2)), ("dense_4s", dense, a.iters)]
    for name, fn, iters in runs:
        ms, times = median_ms(fn, a.warmup, iters)
        res[name] = {"ms": round(ms, 2), "utt_per_s": round(1e3 * B / ms, 1), "runs_ms": [round(t, 2) for t in times]}
    for m in native.CODEC_MODES:
        ms, _ = median_ms(codec(m), a.warmup, a.iters)
        res[f"ragged_{m}"].update(codec_ms=round(ms, 2), codec_share=round(ms / res[f"ragged_{m}"]["ms"], 4))
    eng.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
