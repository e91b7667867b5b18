"""Time the device resampler (Engine.resample, dsn_resample) and what the rate keywords cost a separation call (one
MI355X, inputs drawn once, seeded).
  to_16k_from_44k1   64 x 1 x 4 s at 44.1 kHz -> 16 kHz
  from_16k_to_44k1   64 x 2 x 4 s at 16 kHz -> 44.1 kHz (the way back for two sources)
  to_16k_from_48k    64 x 1 x 4 s at 48 kHz -> 16 kHz
  to_16k_from_8k     64 x 1 x 4 s at 8 kHz -> 16 kHz
  ragged_44k1        64 clips of 2 - 4 s at 44.1 kHz -> 16 kHz in one call (lens)
For each: milliseconds per call and the algorithmic bytes (input read once, output written once) per second, and beside
it the same workload as torch.nn.functional.conv1d with the dense table and stride orig on the same GPU -- the
formulation of torchaudio.transforms.Resample, reported only (skipped with a note if it fails).
  separate_batch     LatentDiffSep.separate_batch (full-size DiT and Oobleck, fp16, graphs on) on 64 clips of 4 s at
                     44.1 kHz with sample_rates=44100, against the same clips already at 16 kHz through the call without
                     rates: the difference is what the feature costs per batch.
HIP events around whole calls; 3 warm-up calls, then the median of 5 timed runs, with the runs listed.  A resampling
call is short, so a timed run is `--reps` calls back to back and the figure is per call.
Prints one JSON line; --out also writes it to a file."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from ditsep_amd import LatentDiffSep, native, synthetic  # noqa: E402
from scripts.ragged_time import CORR, DEC_IN_GAIN, DIT_OUT_GAIN, DIT_SKIP_GAIN, FS, N_STEPS, SNR, median_ms  # noqa: E402


def conv1d_resample(x, plan, dense):
    """torchaudio's formulation: x [B, C, L] -> [B, C, ceil(new L / orig)] by one strided conv1d over the dense table"""
    B, Cn, L = x.shape
    o, n, width = plan["orig"], plan["new"], plan["width"]
    xp = torch.nn.functional.pad(x.reshape(B * Cn, 1, L), (width, width + o))
    y = torch.nn.functional.conv1d(xp, dense[:, None, :], stride=o)               # [B C, new, frames]
    return y.transpose(1, 2).reshape(B, Cn, -1)[..., :native.resample_length(o, n, L)]


def dense_table(plan, device):
    h = torch.zeros((plan["new"], plan["K"]), dtype=torch.float32)
    for p, k0 in enumerate(plan["k0"].tolist()):
        m = min(plan["support"], plan["K"] - k0)
        h[p, k0:k0 + m] = torch.from_numpy(plan["taps"][p, :m].copy())
    return h.to(device)


def full_size_model():
    vcfg, dcfg = synthetic.OobleckConfig(), synthetic.DiTConfig()
    blk = {"channels": vcfg.channels, "c_mults": list(vcfg.c_mults), "strides": list(vcfg.strides)}
    cfg = {"model": {"n_speakers": dcfg.n_src, "t_eps": 0.03, "fs": FS,
                     "score_model": {"_target_": "ditsep_amd.score_models.DiTScoreModel", "embed_dim": dcfg.embed_dim,
                                     "depth": dcfg.depth, "num_heads": dcfg.num_heads},
                     "vae": {"model": {"encoder": {"type": "oobleck", "config": {"latent_dim": vcfg.enc_latent_dim, **blk}},
                                       "decoder": {"type": "oobleck", "config": {"latent_dim": vcfg.latent_dim, **blk}},
                                       "bottleneck": {"type": "vae"}, "latent_dim": vcfg.latent_dim}},
                     "sde": {"N": N_STEPS}, "sampler": {"N": N_STEPS, "snr": SNR, "corrector_steps": CORR}}}
    model = LatentDiffSep(cfg, precision="fp16")
    sd = {"score_model." + k: v for k, v in
          synthetic.random_dit_weights(dcfg, 1, out_gain=DIT_OUT_GAIN, skip_gain=DIT_SKIP_GAIN).items()}
    sd.update({"vae." + k: v for k, v in synthetic.vae_weights(vcfg, 2, dec_in_gain=DEC_IN_GAIN).items()})
    model.load_state_dict(sd)
    model.engine.enable_graphs(True)
    return model


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=64)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("resample_time.py measures on the GPU; none is available")
    eng = native.Engine(score_kind=native.SCORE_NONE, vae_has_encoder=False, vae_has_decoder=False)
    eng.finalize()
    dev, B, SECONDS = eng.device, a.items, 4
    g = torch.Generator().manual_seed(2024)
    res = {"items": B, "seconds": SECONDS, "warmup": a.warmup, "iters": a.iters, "reps": a.reps}

    def timed(name, x, fs_in, fs_out, lens=None):
        plan = native.resample_plan(fs_in, fs_out)
        Bx, Cn, L = x.shape
        ins = Cn * (sum(lens) if lens else Bx * L)
        outs = Cn * sum(native.resample_length(fs_in, fs_out, v) for v in (lens or [L] * Bx))
        nbytes = 4.0 * (ins + outs)

        def run(fn):
            def many():
                for _ in range(a.reps):
                    fn()
            ms, times = median_ms(many, a.warmup, a.iters)
            return ms / a.reps, [round(t / a.reps, 4) for t in times]

        ms, times = run(lambda: eng.resample(x, fs_in, fs_out, lens=lens))
        rec = dict(shape=[Bx, Cn, L], fs_in=fs_in, fs_out=fs_out, support=plan["support"], dense_taps=plan["K"],
                   ms=round(ms, 4), runs_ms=times, algorithmic_bytes=nbytes, gbytes_per_s=round(nbytes / ms * 1e-6, 1))
        try:
            dense = dense_table(plan, dev)
            want = conv1d_resample(x, plan, dense)
            if lens is None:
                got = eng.resample(x, fs_in, fs_out)
                rec["conv1d_max_abs_diff"] = float((got - want).abs().max())
            cms, ctimes = run(lambda: conv1d_resample(x, plan, dense))
            rec.update(conv1d_ms=round(cms, 4), conv1d_runs_ms=ctimes, conv1d_over_native=round(cms / ms, 2))
            if lens is not None:
                rec["conv1d_note"] = "conv1d runs the padded batch: it has no form for per-item lengths"
        except Exception as e:                                                  # reported only
            rec["conv1d_note"] = f"skipped: {type(e).__name__}: {e}"
        res[name] = rec
        print(f"# {name}: {rec}", file=sys.stderr, flush=True)

    def draw(Cn, fs):
        return 0.3 * torch.randn((B, Cn, SECONDS * fs), generator=g).to(dev)

    timed("to_16k_from_44k1", draw(1, 44100), 44100, FS)
    timed("from_16k_to_44k1", draw(2, FS), FS, 44100)
    timed("to_16k_from_48k", draw(1, 48000), 48000, FS)
    timed("to_16k_from_8k", draw(1, 8000), 8000, FS)
    lens = torch.randint(SECONDS // 2 * 44100, SECONDS * 44100 + 1, (B,), generator=g).tolist()
    lens[0] = SECONDS * 44100
    timed("ragged_44k1", draw(1, 44100), 44100, FS, lens=lens)
    eng.close()

    model = full_size_model()
    src = synthetic.synthetic_sources(B, 2, SECONDS * 44100, 44100, seed=1234).sum(1, keepdim=True).to(dev)
    clips44 = [src[i] for i in range(B)]
    clips16 = model.engine.to_model_rate(clips44, 44100, FS)
    kw = dict(seed=7, codec="padded")
    with_ms, with_runs = median_ms(lambda: model.separate_batch(clips44, sample_rates=44100, **kw), a.warmup, a.iters)
    base_ms, base_runs = median_ms(lambda: model.separate_batch(clips16, **kw), a.warmup, a.iters)
    res["separate_batch"] = dict(items=B, seconds=SECONDS, N=N_STEPS, at_44k1_ms=round(with_ms, 2),
                                 at_44k1_runs_ms=[round(t, 2) for t in with_runs], at_16k_ms=round(base_ms, 2),
                                 at_16k_runs_ms=[round(t, 2) for t in base_runs],
                                 feature_ms=round(with_ms - base_ms, 2),
                                 feature_share=round((with_ms - base_ms) / base_ms, 4))
    print(f"# separate_batch: {res['separate_batch']}", file=sys.stderr, flush=True)
    model.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
