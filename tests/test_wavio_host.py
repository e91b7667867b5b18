"""ditsep_amd/wavio.py on the host: files written by Python's `wave` and files built with `struct` parse to the
expected header and payload, every refused form raises ValueError naming the file, write_wav round-trips, and -- where
scipy is installed -- scipy.io.wavfile as a second, independent reader agrees with the restatement's decode."""
import struct
import wave

import numpy as np
import pytest

from ditsep_amd import wavio
from tests import pcm_restatement as pr


def chunk(cid, body):
    return cid + struct.pack("<I", len(body)) + body + (b"\0" if len(body) & 1 else b"")


def fmt_body(tag, channels, rate, bits, block_align=None, extensible_sub=None, valid_bits=None):
    ba = channels * bits // 8 if block_align is None else block_align
    body = struct.pack("<HHIIHH", 0xFFFE if extensible_sub is not None else tag, channels, rate, rate * ba, ba, bits)
    if extensible_sub is not None:
        guid = struct.pack("<H", extensible_sub) + bytes.fromhex("000000001000800000aa00389b71")
        body += struct.pack("<HHI", 22, bits if valid_bits is None else valid_bits, 0) + guid
    return body


def riff(chunks, magic=b"RIFF", data=None, data_size=None):
    """a file image: the chunks, then (optionally) a data chunk whose size field may lie"""
    body = b"WAVE" + b"".join(chunks)
    if data is not None:
        body += b"data" + struct.pack("<I", len(data) if data_size is None else data_size) + data
    return magic + struct.pack("<I", len(body) & 0xFFFFFFFF) + body


def put(tmp_path, name, image):
    p = tmp_path / name
    p.write_bytes(image)
    return p


@pytest.mark.parametrize("width,enc", [(1, "u8"), (2, "s16"), (3, "s24"), (4, "s32")])
@pytest.mark.parametrize("channels", [1, 2, 3])
def test_files_written_by_wave(tmp_path, width, enc, channels):
    frames = 37
    payload = np.random.default_rng(width * 10 + channels).integers(0, 256, frames * channels * width,
                                                                    dtype=np.uint8).tobytes()
    p = tmp_path / "w.wav"
    with wave.open(str(p), "wb") as w:
        w.setnchannels(channels), w.setsampwidth(width), w.setframerate(22050)
        w.writeframes(payload)
    h = wavio.read_header(p)
    assert h == wavio.WavHeader(22050, channels, frames, enc, 44, len(payload))
    assert wavio.read_payload(p, h) == payload
    buf = np.zeros(len(payload) + 5, dtype=np.uint8)
    assert wavio.read_payload(p, h, out=buf[2:2 + len(payload)]) == len(payload)
    assert buf[2:-3].tobytes() == payload and not buf[:2].any() and not buf[-3:].any()


def test_struct_built_files(tmp_path):
    f32 = np.arange(10, dtype="<f4").tobytes()
    f64 = np.arange(6, dtype="<f8").tobytes()
    # IEEE float, 18-byte fmt and a fact chunk
    p = put(tmp_path, "f32.wav", riff([chunk(b"fmt ", fmt_body(3, 2, 32000, 32) + b"\0\0"),
                                       chunk(b"fact", struct.pack("<I", 5))], data=f32))
    assert wavio.read_header(p)[:4] == (32000, 2, 5, "f32") and wavio.read_payload(p, wavio.read_header(p)) == f32
    p = put(tmp_path, "f64.wav", riff([chunk(b"fmt ", fmt_body(3, 3, 8000, 64))], data=f64))
    assert wavio.read_header(p)[:4] == (8000, 3, 2, "f64")
    # extensible: the sub-format decides, the container size governs (24 valid bits in a 32-bit container is s32)
    s32 = bytes(range(32))
    p = put(tmp_path, "ext.wav", riff([chunk(b"fmt ", fmt_body(1, 2, 48000, 32, extensible_sub=1, valid_bits=24))],
                                      data=s32))
    assert wavio.read_header(p)[:4] == (48000, 2, 4, "s32")
    p = put(tmp_path, "extf.wav", riff([chunk(b"fmt ", fmt_body(3, 1, 44100, 32, extensible_sub=3))], data=f32))
    assert wavio.read_header(p)[:4] == (44100, 1, 10, "f32")
    # an odd-sized LIST chunk (with its pad byte) and an unknown chunk before data
    s16 = bytes(range(24))
    chunks = [chunk(b"fmt ", fmt_body(1, 2, 16000, 16)), chunk(b"LIST", b"INFOabc"), chunk(b"bext", b"x" * 10)]
    p = put(tmp_path, "list.wav", riff(chunks, data=s16))
    h = wavio.read_header(p)
    assert h == wavio.WavHeader(16000, 2, 6, "s16", 12 + 24 + 16 + 18 + 8, 24) and wavio.read_payload(p, h) == s16
    # a data size of 0xFFFFFFFF or 0: until the end of the file
    for k, size in enumerate((0xFFFFFFFF, 0)):
        p = put(tmp_path, f"stream{k}.wav", riff([chunk(b"fmt ", fmt_body(1, 1, 16000, 16))], data=s16, data_size=size))
        h = wavio.read_header(p)
        assert (h.frames, h.data_bytes) == (12, 24) and wavio.read_payload(p, h) == s16
    # cut mid-frame: 3-channel s24 frames of 9 bytes, the size field promises 10 frames, 31 bytes are there
    cut = bytes(range(31))
    p = put(tmp_path, "cut.wav", riff([chunk(b"fmt ", fmt_body(1, 3, 44100, 24))], data=cut, data_size=90))
    h = wavio.read_header(p)
    assert (h.frames, h.data_bytes, h.encoding) == (3, 27, "s24") and wavio.read_payload(p, h) == cut[:27]
    # .. and the size field wins when the file goes on after the chunk
    p = put(tmp_path, "more.wav", riff([chunk(b"fmt ", fmt_body(1, 1, 8000, 8))], data=b"abcdef", data_size=4))
    assert wavio.read_header(p).frames == 4


REFUSED = {
    "rifx": riff([chunk(b"fmt ", fmt_body(1, 1, 8000, 16))], magic=b"RIFX", data=b"\0\0"),
    "rf64": riff([chunk(b"fmt ", fmt_body(1, 1, 8000, 16))], magic=b"RF64", data=b"\0\0"),
    "alaw": riff([chunk(b"fmt ", fmt_body(6, 1, 8000, 8))], data=b"\0\0"),
    "mulaw": riff([chunk(b"fmt ", fmt_body(7, 1, 8000, 8))], data=b"\0\0"),
    "adpcm": riff([chunk(b"fmt ", fmt_body(2, 1, 8000, 4, block_align=256))], data=b"\0" * 256),
    "ima": riff([chunk(b"fmt ", fmt_body(17, 1, 8000, 4, block_align=256))], data=b"\0" * 256),
    "ext_alaw": riff([chunk(b"fmt ", fmt_body(1, 1, 8000, 8, extensible_sub=6))], data=b"\0\0"),
    "block_align": riff([chunk(b"fmt ", fmt_body(1, 2, 8000, 16, block_align=6))], data=b"\0" * 12),
    "zero_frames": riff([chunk(b"fmt ", fmt_body(1, 2, 8000, 16))], data=b"\0\0\0"),
    "zero_channels": riff([chunk(b"fmt ", fmt_body(1, 0, 8000, 16))], data=b"\0\0"),
    "pcm12": riff([chunk(b"fmt ", fmt_body(1, 1, 8000, 12, block_align=2))], data=b"\0\0"),
    "no_data": riff([chunk(b"fmt ", fmt_body(1, 1, 8000, 16))]),
    "not_wave": b"RIFF\x04\0\0\0AVI ",
    "short": b"RIF",
}


@pytest.mark.parametrize("name", sorted(REFUSED))
def test_refused_forms_name_the_file(tmp_path, name):
    p = put(tmp_path, name + ".wav", REFUSED[name])
    with pytest.raises(ValueError) as e:
        wavio.read_header(p)
    assert str(p) in str(e.value)
    reason = {"rifx": "RIFX", "rf64": "RF64", "alaw": "A-law", "mulaw": "mu-law", "adpcm": "ADPCM", "ima": "ADPCM",
              "ext_alaw": "A-law", "block_align": "block_align", "zero_frames": "zero frames",
              "zero_channels": "zero channels"}.get(name)
    if reason:
        assert reason in str(e.value)


@pytest.mark.parametrize("enc,width", [("s16", 2), ("s24", 3), ("f32", 4)])
def test_write_wav_round_trips(tmp_path, enc, width):
    for channels, frames in ((1, 7), (2, 5)):         # (an odd payload: 24-bit mono with 7 frames carries a pad byte)
        payload = np.random.default_rng(frames).integers(0, 256, frames * channels * width, dtype=np.uint8).tobytes()
        p = tmp_path / f"{enc}_{channels}.wav"
        wavio.write_wav(p, payload, 44100, channels, enc)
        h = wavio.read_header(p)
        assert h[:4] == (44100, channels, frames, enc) and wavio.read_payload(p, h) == payload
        image = p.read_bytes()
        assert struct.unpack("<I", image[4:8])[0] == len(image) - 8 and len(image) % 2 == 0
        if enc == "f32":
            assert struct.unpack("<H", image[20:22])[0] == 3 and image[38:42] == b"fact"
            assert struct.unpack("<I", image[46:50])[0] == frames
        else:
            with wave.open(str(p), "rb") as w:          # Python's own reader takes the PCM files
                assert (w.getnchannels(), w.getsampwidth(), w.getframerate(), w.getnframes()) == (
                    channels, width, 44100, frames)
                assert w.readframes(frames) == payload
    with pytest.raises(ValueError, match="encoding"):
        wavio.write_wav(tmp_path / "x.wav", b"\0\0", 8000, 1, "u8")
    with pytest.raises(ValueError, match="frames"):
        wavio.write_wav(tmp_path / "x.wav", b"\0\0\0", 8000, 1, "s16")


def test_scipy_reads_the_same_samples(tmp_path):
    """a second, independent reader: scipy's integer and float arrays through the restatement's scaling equal the
    restatement's decode of the raw payload"""
    wavfile = pytest.importorskip("scipy.io.wavfile")
    rng = np.random.default_rng(3)
    cases = [("u8", 1, 2, rng.integers(0, 256, 40, dtype=np.uint8).tobytes()),
             ("s16", 1, 2, rng.integers(-2 ** 15, 2 ** 15, 40).astype("<i2").tobytes()),
             ("s32", 1, 1, rng.integers(-2 ** 31, 2 ** 31, 20).astype("<i4").tobytes()),
             ("f32", 3, 2, rng.standard_normal(40).astype("<f4").tobytes()),
             ("f64", 3, 1, rng.standard_normal(20).astype("<f8").tobytes())]
    for enc, tag, channels, payload in cases:
        bits = 8 * pr.SAMPLE_BYTES[enc]
        p = put(tmp_path, enc + ".wav", riff([chunk(b"fmt ", fmt_body(tag, channels, 16000, bits))], data=payload))
        h = wavio.read_header(p)
        want = pr.decode(wavio.read_payload(p, h), h.frames, h.channels, h.encoding)
        rate, a = wavfile.read(str(p))
        a = a.reshape(h.frames, channels).T
        assert rate == 16000
        if enc == "u8":
            got = (a.astype(np.int32) - 128).astype(np.float32) / np.float32(128)
        elif enc == "s16":
            got = a.astype(np.float32) / np.float32(2 ** 15)
        elif enc == "s32":
            got = a.astype(np.float32) * np.float32(2.0 ** -31)
        else:
            got = a.astype(np.float32)
        assert np.array_equal(got.view(np.int32), want.view(np.int32)), enc
    # 24-bit: scipy hands back int32 with the sample in the upper three bytes
    v = rng.integers(-2 ** 23, 2 ** 23, 30)
    payload = b"".join(int(x & 0xFFFFFF).to_bytes(3, "little") for x in v)
    p = put(tmp_path, "s24.wav", riff([chunk(b"fmt ", fmt_body(1, 1, 16000, 24))], data=payload))
    h = wavio.read_header(p)
    _, a = wavfile.read(str(p))
    got = (a.astype(np.int64) >> 8).astype(np.float32) / np.float32(2 ** 23)
    assert np.array_equal(got, pr.decode(wavio.read_payload(p, h), 30, 1, "s24")[0])
