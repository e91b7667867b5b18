"""Time one graph-replayed score-matching loss call (Engine.score_loss, dsn_score_loss) against one score call
(Engine.score) in the same process at the C2 shape: B = 64 mixtures, T = 32 latent frames, the full-size DiT
(bench.py's synthetic weights), in fp16 and bf16x3.  Per precision: warm-up, then `--reps` timed repetitions of each
(GPU events around single calls, interleaved), median; prints the pair and the overhead of the loss's own kernels and
copies in percent of the score call.  One JSON line; --out also writes it to a file."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from ditsep_amd import native, synthetic  # noqa: E402

DIT_OUT_GAIN, DIT_SKIP_GAIN = 0.002, 0.02   # bench.py's synthetic DiT


def _one(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=64)
    ap.add_argument("--T", type=int, default=32)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--precisions", default="fp16,bf16x3")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    cfg = synthetic.DiTConfig()
    sd = synthetic.random_dit_weights(cfg, 1, out_gain=DIT_OUT_GAIN, skip_gain=DIT_SKIP_GAIN)
    g = torch.Generator().manual_seed(2)
    y = torch.randn((a.B, 1, 64, a.T), generator=g).cuda()
    x0 = torch.randn((a.B, 2, 64, a.T), generator=g).cuda()
    res = {"B": a.B, "T": a.T, "reps": a.reps}
    precs = {"fp16": native.PREC_FP16, "bf16x3": native.PREC_BF16X3}
    for name in a.precisions.split(","):
        eng = native.Engine(precision=precs[name], score_kind=native.SCORE_DIT, vae_has_encoder=False,
                            vae_has_decoder=False)
        eng.load_state_dict(sd, prefix="score_model.")
        eng.finalize()
        eng.enable_graphs(True)
        tt = torch.full((a.B,), 0.5, device="cuda")
        xt = (y + 3.0 * x0).contiguous()
        loss = lambda: eng.score_loss(y, x0, seed=1)          # noqa: E731
        pit = lambda: eng.score_loss(y, x0, seed=1, mode="init_pit")   # noqa: E731
        score = lambda: eng.score(xt, tt, y)                  # noqa: E731
        for _ in range(5):                                    # eager warm-up, graph capture, replays
            loss(), pit(), score()
        torch.cuda.synchronize()
        tl, tp, ts = [], [], []
        for _ in range(a.reps):
            ts.append(_one(score))
            tl.append(_one(loss))
            tp.append(_one(pit))
        ms_s, ms_l, ms_p = statistics.median(ts), statistics.median(tl), statistics.median(tp)
        res[name] = {"score_call_ms": round(ms_s, 4), "score_loss_ms": round(ms_l, 4),
                     "score_loss_pit_ms": round(ms_p, 4),
                     "overhead_pct": round(100 * (ms_l - ms_s) / ms_s, 2),
                     "overhead_pit_pct": round(100 * (ms_p - ms_s) / ms_s, 2),
                     "min_ms": [round(min(ts), 4), round(min(tl), 4), round(min(tp), 4)]}
        eng.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
