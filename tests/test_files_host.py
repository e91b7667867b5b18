"""The GPU-free side of the file layer: files.plan_files, the command line's parser, the refusals raised before any
device work, and the three new C-ABI symbols declared and exported."""
import os
import re

import numpy as np
import pytest

from ditsep_amd import files, native, wavio
from ditsep_amd import separate as cli
from tests import pcm_restatement as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FS, HOP = 16000, 8


def header(rate, frames, channels=1, encoding="s16"):
    return wavio.WavHeader(rate, channels, frames, encoding, 44, frames * channels * wavio.SAMPLE_BYTES[encoding])


def test_plan_files():
    hs = [header(16000, 203), header(44100, 611, 2, "s24"), header(32000, 417, 1, "f32"), header(8000, 90, 2, "u8"),
          header(16000, 1500), header(48000, 1), header(16000, 203)]
    plan = files.plan_files(hs, FS, HOP, batch=3)
    assert plan["lengths"] == [203, 222, 209, 180, 1500, 1, 203]
    assert plan["lengths"] == [-(-h.frames * FS // h.rate) for h in hs]
    assert plan["frames"] == [native.latent_frames_of(v, HOP) for v in plan["lengths"]]
    assert plan["long"] == []
    assert plan["batches"] == [[5, 3, 0], [6, 2, 1], [4]]               # sorted by length, ties by index, cut in order
    assert sorted(i for b in plan["batches"] for i in b) == list(range(len(hs)))
    flat = [plan["lengths"][i] for b in plan["batches"] for i in b]
    assert flat == sorted(flat)
    # long_after is seconds at the file's own rate: the files last 12.7, 13.9, 13.0, 11.3, 93.8, 0.02 and 12.7 ms
    plan = files.plan_files(hs, FS, HOP, batch=2, long_after=0.0135)
    assert plan["long"] == [1, 4]
    assert plan["batches"] == [[5, 3], [0, 6], [2]]
    assert sorted(plan["long"] + [i for b in plan["batches"] for i in b]) == list(range(len(hs)))
    assert files.plan_files(hs, FS, HOP, batch=64, long_after=1e-6)["batches"] == []
    with pytest.raises(ValueError, match="batch"):
        files.plan_files(hs, FS, HOP, batch=0)
    with pytest.raises(ValueError, match="long_after"):
        files.plan_files(hs, FS, HOP, long_after=0)


def test_parse_inputs_refuses_before_any_device_work(tmp_path):
    (tmp_path / "a").mkdir()
    good = tmp_path / "x.wav"
    wavio.write_wav(good, b"\0\0" * 4, 16000, 1, "s16")
    same = tmp_path / "a" / "x.wav"
    wavio.write_wav(same, b"\0\0" * 4, 16000, 1, "s16")
    bad = tmp_path / "bad.wav"
    bad.write_bytes(b"RIFX" + b"\0" * 40)
    assert [h.frames for h in files.parse_inputs([good])] == [4]
    with pytest.raises(ValueError, match="same stem"):
        files.parse_inputs([good, same])
    with pytest.raises(ValueError, match="RIFX"):
        files.parse_inputs([good, bad])
    with pytest.raises(ValueError, match="no input files"):
        files.parse_inputs([])


def test_parser_defaults_and_reference_flags():
    p = cli.build_parser()
    a = p.parse_args(["in", "out", "--config", "c.json"])
    assert (str(a.input_dir), str(a.output_dir), str(a.config)) == ("in", "out", "c.json")
    assert (a.N, a.snr, a.corrector_steps, a.denoise, a.schedule, a.device) == (None, None, None, True, None, "cuda:0")
    assert (a.checkpoint, a.ema, a.precision, a.batch, a.encoding, a.rescale) == (None, False, "fp16", 64, "s16", False)
    assert (a.long_after, a.window, a.overlap, a.long_mode, a.seed) == (None, None, None, "stitch", None)
    a = p.parse_args(["in", "out", "--config", "c.yaml", "-N", "12", "--snr", "0.4", "--corrector-steps", "2",
                      "--denoise", "false", "-s", "cosine", "-d", "1", "--checkpoint", "m.pt", "--ema", "--precision",
                      "bf16x3", "--batch", "8", "--encoding", "s24", "--rescale", "--long-after", "30", "--window",
                      "65536", "--overlap", "8192", "--long-mode", "score", "--seed", "5"])
    assert (a.N, a.snr, a.corrector_steps, a.denoise, a.schedule, a.device) == (12, 0.4, 2, False, "cosine", 1)
    assert (str(a.checkpoint), a.ema, a.precision, a.batch, a.encoding, a.rescale) == ("m.pt", True, "bf16x3", 8, "s24",
                                                                                      True)
    assert (a.long_after, a.window, a.overlap, a.long_mode, a.seed) == (30.0, 65536, 8192, "score", 5)
    assert p.parse_args(["in", "out", "--config", "c", "--schedule", "x", "--device", "cuda:2"]).device == "cuda:2"
    assert cli.device_index("cuda:2") == 2 and cli.device_index(1) == 1 and cli.device_index("cuda") == 0
    with pytest.raises(ValueError, match="GPU"):
        cli.device_index("cpu")
    with pytest.raises(SystemExit):
        p.parse_args(["in", "out", "--config", "c", "--encoding", "u8"])


def test_main_refuses_an_empty_folder(tmp_path, capsys):
    (tmp_path / "in").mkdir()
    (tmp_path / "c.json").write_text("{}")
    assert cli.main([str(tmp_path / "in"), str(tmp_path / "out"), "--config", str(tmp_path / "c.json")]) == 2
    assert "no .wav files" in capsys.readouterr().err
    assert not (tmp_path / "out").exists()


def test_check_pcm_items():
    items = [(0, 4, 2, "s16"), (16, 3, 3, "s24"), (43, 1, 1, "f64")]
    assert native.check_pcm_items(items, 51) == ([0, 16, 43], [4, 3, 1], [2, 3, 1], [1, 2, 5], 1, 4)
    assert native.check_pcm_items(items, 51, downmix=False)[4:] == (3, 4)
    for bad, why in (([(0, 4, 2, "s12")], "encoding"), ([(0, 0, 2, "s16")], "at least 1"),
                     ([(0, 4, 0, "s16")], "at least 1"), ([(0, 1, 7, "f64")], "PCM_MAX_FRAME_BYTES"),
                     ([(44, 1, 1, "f64")], "outside"), ([(-1, 1, 1, "u8")], "outside"), ([], "at least one")):
        with pytest.raises(ValueError, match=why):
            native.check_pcm_items(bad, 51)
    assert native.PCM_SAMPLE_BYTES == pr.SAMPLE_BYTES == wavio.SAMPLE_BYTES


def test_pcm_symbols_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "ditsep_hip.h")).read()
    assert re.search(r"\bint dsn_pcm_decode\(dsn_ctx\* ctx, const void\* bytes, int64_t nbytes, int B, "
                     r"const int64_t\* offset, const int32_t\* frames,\s+const int32_t\* channels, "
                     r"const int32_t\* encoding, int downmix, float\* out, int Cout, int Lmax,\s+void\* stream\);", hdr)
    assert re.search(r"\bint dsn_pcm_encode\(dsn_ctx\* ctx, const float\* x, int R, int Lmax, const int32_t\* lens, "
                     r"int encoding, void\* bytes,\s+int64_t nbytes, const int64_t\* offset, int64_t\* clipped, "
                     r"void\* stream\);", hdr)
    assert re.search(r"\bint dsn_scale_output\(dsn_ctx\* ctx, const float\* mix, const float\* sep, int B, int n, "
                     r"int Lmax, const int32_t\* lens,\s+float\* out, float\* alpha_out, void\* stream\);", hdr)
    m = re.search(r"enum \{ DSN_PCM_U8 = 0, DSN_PCM_S16 = 1, DSN_PCM_S24 = 2, DSN_PCM_S32 = 3, DSN_PCM_F32 = 4, "
                  r"DSN_PCM_F64 = 5 \};", hdr)
    assert m and native.PCM_ENCODINGS == {"u8": 0, "s16": 1, "s24": 2, "s32": 3, "f32": 4, "f64": 5}
    assert int(re.search(r"#define DSN_PCM_MAX_FRAME_BYTES (\d+)", hdr).group(1)) == native.PCM_MAX_FRAME_BYTES
    lib = native.load_library()
    for name in ("dsn_pcm_decode", "dsn_pcm_encode", "dsn_scale_output"):
        assert name in native.EXPORTS and hasattr(lib, name)
    for name in ("pcm_decode", "pcm_encode", "scale_output"):
        assert callable(getattr(native.Engine, name))
    src = open(os.path.join(ROOT, "ditsep_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS = .*\bpcm\.hip\b", src, flags=re.M)


def test_restatement_is_self_consistent():
    """quantise then decode is the identity on the s16 grid; the ties go to even; the clipped count"""
    v = np.arange(-2 ** 15, 2 ** 15, dtype=np.int32)
    x = v.astype(np.float32) / np.float32(2 ** 15)
    payload, clipped = pr.quantise(x, "s16")
    assert clipped == 0 and payload == v.astype("<i2").tobytes()
    assert np.array_equal(pr.decode(payload, x.size, 1, "s16")[0], x)
    lsb = np.float32(2.0 ** -15)
    ties = np.array([0.5, -0.5, 1.5, -1.5, 2.5, -2.5], dtype=np.float32) * lsb
    assert np.frombuffer(pr.quantise(ties, "s16")[0], dtype="<i2").tolist() == [0, 0, 2, -2, 2, -2]
    x = np.array([1.0, -1.0, 1 - 2.0 ** -16, np.inf, -np.inf, np.nan, 0.25], dtype=np.float32)
    payload, clipped = pr.quantise(x, "s16")
    assert np.frombuffer(payload, dtype="<i2").tolist() == [32767, -32768, 32767, 32767, -32768, 0, 8192]
    assert clipped == 5            # 1.0, 1 - 2^-16 (rounds to 32768), +inf, -inf, NaN
    payload, clipped = pr.quantise(x, "s24")
    assert clipped == 4 and payload[:3] == b"\xff\xff\x7f" and payload[3:6] == b"\x00\x00\x80"
    assert pr.decode(payload, 7, 1, "s24")[0, 2] == np.float32(1 - 2.0 ** -16)
