"""Time the file layer (one MI355X, inputs drawn once, seeded): the device sample conversions against the same
conversions written with torch ops on the same GPU and with numpy on the host, and what reading and writing WAV files
costs a separation batch.  Two workloads: `--items` stereo s16 clips of 4 s at 44.1 kHz, and as many mono s24 clips.
  decode_*   Engine.pcm_decode(downmix=True) of the payloads already on the device ("native_ms"), the torch formulation
             on the device ("torch_ms", checked to give the same bits), and the two whole routes from host bytes to a
             device tensor: the payload bytes copied from pinned memory and decoded there ("native_from_host_ms") against
             numpy on one host thread plus the copy of its float32 result ("numpy_from_host_ms")
  encode_*   dsn_pcm_encode of 2 x items mono rows into a device buffer ("native_ms"), the torch formulation
             ("torch_ms", same bytes), and the two whole routes to host bytes: Engine.pcm_encode ("native_to_host_ms")
             against the float32 copy plus numpy ("numpy_to_host_ms")
  separate_files   LatentDiffSep.separate_files (full-size DiT and Oobleck, fp16, graphs on, synthetic weights) on a
             temporary folder of the stereo clips, against separate_batch(sample_rates=44100) on the same clips already
             in device memory as float32: the difference is what the file layer costs a batch.
HIP events around whole calls; 3 warm-up calls, then the median of 5 timed runs, with the runs listed.  A conversion is
short, so a timed run is `--reps` calls back to back and the figure is per call.
Prints one JSON line; --out also writes it to a file."""
import argparse
import ctypes as C
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from ditsep_amd import native, synthetic, wavio  # noqa: E402
from scripts.ragged_time import FS, N_STEPS, median_ms  # noqa: E402
from scripts.resample_time import full_size_model  # noqa: E402

RATE, SECONDS = 44100, 4


def torch_decode(raw, B, L, channels, enc):
    """the payload bytes on the device -> [B, 1, L] float32 with torch ops"""
    if enc == "s16":
        x = raw.view(torch.int16).view(B, L, channels).to(torch.float32) * 2.0 ** -15
    else:
        b = raw.view(B, L, channels, 3).to(torch.int32)
        v = b[..., 0] | (b[..., 1] << 8) | (b[..., 2] << 16)
        x = ((v << 8) >> 8).to(torch.float32) * 2.0 ** -23
    if channels == 1:
        return x.transpose(1, 2).contiguous()
    s = x[..., 0]
    for c in range(1, channels):
        s = s + x[..., c]
    return (s / channels)[:, None].contiguous()


def numpy_decode(raw, B, L, channels, enc):
    if enc == "s16":
        x = raw.view("<i2").reshape(B, L, channels).astype(np.float32) / np.float32(2 ** 15)
    else:
        b = raw.reshape(B, L, channels, 3).astype(np.int32)
        v = b[..., 0] | (b[..., 1] << 8) | (b[..., 2] << 16)
        x = ((v << 8) >> 8).astype(np.float32) / np.float32(2 ** 23)
    if channels == 1:
        return np.ascontiguousarray(x.transpose(0, 2, 1))
    s = x[..., 0]
    for c in range(1, channels):
        s = s + x[..., c]
    return (s / np.float32(channels))[:, None]


def torch_encode(x, enc):
    """[R, L] float32 on the device -> (payload bytes [R, L w] uint8, clipped [R]) with torch ops"""
    scale = 2.0 ** (15 if enc == "s16" else 23)
    y = torch.round(x * scale)
    bad = ~((y >= -scale) & (y <= scale - 1))
    q = torch.nan_to_num(y, nan=0.0).clamp(-scale, scale - 1)
    if enc == "s16":
        return q.to(torch.int16).view(torch.uint8), bad.sum(dim=1)
    q = q.to(torch.int32)
    return torch.stack([q & 0xFF, (q >> 8) & 0xFF, (q >> 16) & 0xFF], dim=-1).to(torch.uint8).reshape(x.shape[0], -1), \
        bad.sum(dim=1)


def numpy_encode(x, enc):
    scale = np.float32(2.0 ** (15 if enc == "s16" else 23))
    y = np.rint(x * scale)
    bad = ~((y >= -scale) & (y <= scale - 1))
    q = np.where(np.isnan(y), np.float32(0), np.clip(y, -scale, scale - 1))
    if enc == "s16":
        return [r.tobytes() for r in q.astype("<i2")], bad.sum(axis=1)
    u = q.astype(np.int32)
    out = np.stack([u & 0xFF, (u >> 8) & 0xFF, (u >> 16) & 0xFF], axis=-1).astype(np.uint8)
    return [r.tobytes() for r in out], bad.sum(axis=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=64)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--skip-model", action="store_true", help="the conversions only")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("files_time.py measures on the GPU; none is available")
    eng = native.Engine(score_kind=native.SCORE_NONE, vae_has_encoder=False, vae_has_decoder=False)
    eng.finalize()
    dev, B, L = eng.device, a.items, SECONDS * RATE
    rng = np.random.default_rng(2024)
    res = {"items": B, "seconds": SECONDS, "rate": RATE, "warmup": a.warmup, "iters": a.iters, "reps": a.reps}

    def per_call(fn, reps=a.reps):
        def many():
            for _ in range(reps):
                fn()
        ms, times = median_ms(many, a.warmup, a.iters)
        return round(ms / reps, 4), [round(t / reps, 4) for t in times]

    def put(rec, key, fn, reps=a.reps):
        rec[key + "_ms"], rec[key + "_runs_ms"] = per_call(fn, reps)

    payloads = {}
    for name, channels, enc in (("stereo_s16", 2, "s16"), ("mono_s24", 1, "s24")):
        w = native.PCM_SAMPLE_BYTES[enc]
        if enc == "s16":
            host = (0.3 * rng.standard_normal((B, L, channels), dtype=np.float32) * 2 ** 15).astype("<i2").view(np.uint8)
        else:
            v = (0.3 * rng.standard_normal((B, L, channels), dtype=np.float32) * 2 ** 23).astype(np.int32)
            host = np.stack([v & 0xFF, (v >> 8) & 0xFF, (v >> 16) & 0xFF], axis=-1).astype(np.uint8)
        host = np.ascontiguousarray(host).reshape(-1)
        payloads[name] = (host, channels, enc)
        pinned = torch.from_numpy(host).pin_memory()
        raw = pinned.to(dev)
        per = L * channels * w
        items = [(b * per, L, channels, enc) for b in range(B)]
        got, _ = eng.pcm_decode(raw, items)
        same = bool(torch.equal(got.view(torch.int32), torch_decode(raw, B, L, channels, enc).view(torch.int32)))
        same_np = bool(np.array_equal(got.cpu().numpy(), numpy_decode(host, B, L, channels, enc)))
        rec = dict(shape=[B, channels, L], encoding=enc, payload_bytes=int(host.size), float32_bytes=4 * B * L,
                   torch_same_bits=same, numpy_same_bits=same_np)
        put(rec, "native", lambda: eng.pcm_decode(raw, items))
        put(rec, "torch", lambda: torch_decode(raw, B, L, channels, enc))
        put(rec, "native_from_host", lambda: eng.pcm_decode(pinned, items))
        put(rec, "numpy_from_host", lambda: torch.from_numpy(numpy_decode(host, B, L, channels, enc)).to(dev), reps=1)
        rec["gbytes_per_s"] = round((host.size + 4.0 * B * L) / rec["native_ms"] * 1e-6, 1)
        rec["torch_over_native"] = round(rec["torch_ms"] / rec["native_ms"], 2)
        rec["numpy_over_native_from_host"] = round(rec["numpy_from_host_ms"] / rec["native_from_host_ms"], 2)
        res["decode_" + name] = rec
        print(f"# decode_{name}: {rec}", file=sys.stderr, flush=True)

    R = 2 * B
    x = (0.3 * torch.randn((R, L), generator=torch.Generator().manual_seed(2025))).to(dev)
    x[0, :4] = torch.tensor([1.0, -1.0, float("nan"), 3.0])
    for enc in ("s16", "s24"):
        w = native.PCM_SAMPLE_BYTES[enc]
        buf = torch.zeros(R * L * w, dtype=torch.uint8, device=dev)
        lens, offs = (C.c_int32 * R)(*([L] * R)), (C.c_int64 * R)(*[r * L * w for r in range(R)])
        clipped = (C.c_int64 * R)()

        def native_encode(counts=None):
            rc = eng.lib.dsn_pcm_encode(eng.ctx, native._ptr(x), R, L, lens, native.PCM_ENCODINGS[enc], native._ptr(buf),
                                        buf.numel(), offs, counts, eng._stream())
            assert rc == 0, eng.lib.dsn_last_error(eng.ctx).decode()

        native_encode(clipped)
        tb, tc = torch_encode(x, enc)
        same = bool(torch.equal(buf, tb.reshape(-1))) and list(clipped) == tc.tolist()
        nb, nc = numpy_encode(x.cpu().numpy(), enc)
        hb, hc = eng.pcm_encode(x, None, enc)
        same_np = hb == nb and hc == nc.tolist()
        rec = dict(shape=[R, L], encoding=enc, payload_bytes=R * L * w, float32_bytes=4 * R * L, clipped=int(sum(hc)),
                   torch_same_bytes=same, numpy_same_bytes=same_np)
        put(rec, "native", native_encode)
        put(rec, "torch", lambda: torch_encode(x, enc))
        put(rec, "native_to_host", lambda: eng.pcm_encode(x, None, enc), reps=1)
        put(rec, "numpy_to_host", lambda: numpy_encode(x.cpu().numpy(), enc), reps=1)
        rec["gbytes_per_s"] = round((4.0 + w) * R * L / rec["native_ms"] * 1e-6, 1)
        rec["torch_over_native"] = round(rec["torch_ms"] / rec["native_ms"], 2)
        rec["numpy_over_native_to_host"] = round(rec["numpy_to_host_ms"] / rec["native_to_host_ms"], 2)
        res["encode_" + enc] = rec
        print(f"# encode_{enc}: {rec}", file=sys.stderr, flush=True)
    eng.close()

    if not a.skip_model:
        model = full_size_model()
        src = synthetic.synthetic_sources(B, 2, L, RATE, seed=1234).sum(1)                      # [B, L]
        src = 0.5 * src / src.abs().amax()
        stereo = torch.stack([src, 0.9 * src.roll(3, dims=-1)], dim=1)                           # [B, 2, L]
        pcm = torch.round(stereo * 2 ** 15).clamp(-2 ** 15, 2 ** 15 - 1).to(torch.int16)
        clips = [(pcm[b].to(torch.float32) / 2 ** 15).to(model.engine.device) for b in range(B)]
        with tempfile.TemporaryDirectory() as tmp:
            paths = []
            for b in range(B):
                paths.append(os.path.join(tmp, f"clip{b:03d}.wav"))
                wavio.write_wav(paths[-1], pcm[b].T.contiguous().numpy().tobytes(), RATE, 2, "s16")
            out = os.path.join(tmp, "out")
            kw = dict(seed=7, codec="padded")
            files_ms, files_runs = median_ms(lambda: model.separate_files(paths, out, batch=B, **kw), a.warmup, a.iters)
            base_ms, base_runs = median_ms(lambda: model.separate_batch(clips, sample_rates=RATE, **kw), a.warmup,
                                           a.iters)
        res["separate_files"] = dict(items=B, seconds=SECONDS, N=N_STEPS, files_ms=round(files_ms, 2),
                                     files_runs_ms=[round(t, 2) for t in files_runs], in_memory_ms=round(base_ms, 2),
                                     in_memory_runs_ms=[round(t, 2) for t in base_runs],
                                     file_layer_ms=round(files_ms - base_ms, 2),
                                     file_layer_share=round((files_ms - base_ms) / base_ms, 4),
                                     utt_per_s=round(1e3 * B / files_ms, 1))
        print(f"# separate_files: {res['separate_files']}", file=sys.stderr, flush=True)
        model.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
