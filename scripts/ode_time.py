"""Time the probability-flow ODE sampler (Engine.ode_sample, dsn_ode_sample) at the C2 shape: B = 64 mixtures,
T = 32 latent frames, the full-size DiT (bench.py's synthetic weights), in fp16 and bf16x3, RK45 at the reference's
default tolerances (rtol = atol = 1e-5), hipGraph replay on.  Prints per precision: nfev, accepted / rejected steps,
ms per call, ms per step attempt, and 6x the ms of one score call (eager dsn_score) so that the solver's own overhead
per attempt is visible.  One JSON line; --out also writes it to a file."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from ditsep_amd import native, synthetic  # noqa: E402

DIT_OUT_GAIN, DIT_SKIP_GAIN = 0.002, 0.02   # bench.py's synthetic DiT


def _ms(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=64)
    ap.add_argument("--T", type=int, default=32)
    ap.add_argument("--iters", type=int, default=2)
    ap.add_argument("--precisions", default="fp16,bf16x3")
    ap.add_argument("--rtol", type=float, default=1e-5)
    ap.add_argument("--atol", type=float, default=1e-5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    cfg = synthetic.DiTConfig()
    sd = synthetic.random_dit_weights(cfg, 1, out_gain=DIT_OUT_GAIN, skip_gain=DIT_SKIP_GAIN)
    g = torch.Generator().manual_seed(2)
    y = torch.randn((a.B, 1, 64, a.T), generator=g).cuda()
    z = torch.randn((a.B, 2, 64, a.T), generator=g).cuda()
    res = {"B": a.B, "T": a.T, "rtol": a.rtol, "atol": a.atol}
    precs = {"fp16": native.PREC_FP16, "bf16x3": native.PREC_BF16X3}
    for name in a.precisions.split(","):
        eng = native.Engine(precision=precs[name], score_kind=native.SCORE_DIT, vae_has_encoder=False,
                            vae_has_decoder=False)
        eng.load_state_dict(sd, prefix="score_model.")
        eng.finalize()
        eng.enable_graphs(True)
        run = lambda: eng.ode_sample(y, z, rtol=a.rtol, atol=a.atol, return_stats=True)  # noqa: E731
        for _ in range(2):          # eager warm-up, graph capture
            run()
        torch.cuda.synchronize()
        ms, (_, nfev, st) = _ms(run, a.iters)
        attempts = st["n_accepted"] + st["n_rejected"]
        xt = (y + 3.0 * z).contiguous()
        tt = torch.full((a.B,), 0.5, device="cuda")
        eng.score(xt, tt, y)
        torch.cuda.synchronize()
        score_ms, _ = _ms(lambda: eng.score(xt, tt, y), 5)
        res[name] = {"nfev": nfev, "accepted": st["n_accepted"], "rejected": st["n_rejected"],
                     "ms_per_call": round(ms, 2), "ms_per_attempt": round(ms / max(attempts, 1), 3),
                     "six_score_calls_ms": round(6 * score_ms, 3), "score_call_ms": round(score_ms, 3)}
        eng.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
