"""RIFF/WAVE containers on the host: headers in, raw `data` payloads in and out.  No sample is touched here -- the
payload bytes go to the device as they are (Engine.pcm_decode) and come back as they will be written
(Engine.pcm_encode).  Pure Python: the standard `wave` module refuses IEEE float and, before Python 3.12,
WAVE_FORMAT_EXTENSIBLE.

Read, little-endian only: format tag 1 (PCM) with 8, 16, 24 or 32 bits per sample, tag 3 (IEEE float) with 32 or 64,
and tag 0xFFFE (extensible) whose sub-format -- the first two bytes of its GUID -- is one of those two; the container
size (wBitsPerSample) governs, not wValidBitsPerSample.  Unknown chunks are skipped, odd chunk sizes carry their pad
byte, a `data` size of 0 or 0xFFFFFFFF means "until the end of the file", and a truncated `data` chunk is cut down to
whole frames.  Everything else raises ValueError naming the file and the reason."""
from __future__ import annotations

import os
import struct
from typing import NamedTuple

TAG_PCM, TAG_ADPCM, TAG_FLOAT, TAG_ALAW, TAG_MULAW, TAG_IMA_ADPCM, TAG_EXTENSIBLE = 1, 2, 3, 6, 7, 17, 0xFFFE
REFUSED_TAGS = {TAG_ADPCM: "Microsoft ADPCM", TAG_ALAW: "A-law", TAG_MULAW: "mu-law", TAG_IMA_ADPCM: "IMA ADPCM"}
ENCODING_OF = {(TAG_PCM, 8): "u8", (TAG_PCM, 16): "s16", (TAG_PCM, 24): "s24", (TAG_PCM, 32): "s32",
               (TAG_FLOAT, 32): "f32", (TAG_FLOAT, 64): "f64"}
SAMPLE_BYTES = {"u8": 1, "s16": 2, "s24": 3, "s32": 4, "f32": 4, "f64": 8}
WRITE_TAGS = {"s16": TAG_PCM, "s24": TAG_PCM, "f32": TAG_FLOAT}


class WavHeader(NamedTuple):
    rate: int           # frames per second
    channels: int
    frames: int         # whole frames the file really holds
    encoding: str       # "u8" | "s16" | "s24" | "s32" | "f32" | "f64"
    data_offset: int    # the payload's first byte in the file
    data_bytes: int     # frames * channels * SAMPLE_BYTES[encoding]


def _parse_fmt(path: str, body: bytes) -> tuple:
    if len(body) < 16:
        raise ValueError(f"{path}: fmt chunk of {len(body)} bytes (at least 16 are needed)")
    tag, channels, rate, _, block_align, bits = struct.unpack("<HHIIHH", body[:16])
    if tag == TAG_EXTENSIBLE:
        if len(body) < 40:
            raise ValueError(f"{path}: WAVE_FORMAT_EXTENSIBLE fmt chunk of {len(body)} bytes (40 are needed)")
        tag = struct.unpack("<H", body[24:26])[0]      # the sub-format GUID's first two bytes
    if tag in REFUSED_TAGS:
        raise ValueError(f"{path}: {REFUSED_TAGS[tag]} (format tag {tag}) is not supported: only PCM and IEEE float")
    if (tag, bits) not in ENCODING_OF:
        raise ValueError(f"{path}: format tag {tag} with {bits} bits per sample is not supported (PCM 8/16/24/32, "
                         f"IEEE float 32/64)")
    encoding = ENCODING_OF[(tag, bits)]
    if channels < 1:
        raise ValueError(f"{path}: zero channels")
    if rate < 1:
        raise ValueError(f"{path}: sample rate 0")
    if block_align != channels * SAMPLE_BYTES[encoding]:
        raise ValueError(f"{path}: block_align = {block_align} is not channels * bytes_per_sample = "
                         f"{channels} * {SAMPLE_BYTES[encoding]}")
    return rate, channels, encoding


def read_header(path) -> WavHeader:
    """Parse the chunks of `path` up to its `data` chunk -> WavHeader.  Raises ValueError (naming the file) for RIFX,
    RF64, a compressed format, an inconsistent block_align, zero channels or zero frames, and anything that is not a
    RIFF/WAVE file."""
    path = os.fspath(path)
    size = os.path.getsize(path)
    with open(path, "rb") as fh:
        head = fh.read(12)
        if len(head) < 12:
            raise ValueError(f"{path}: {len(head)} bytes, too short for a RIFF header")
        if head[:4] in (b"RIFX", b"RF64", b"BW64"):
            raise ValueError(f"{path}: {head[:4].decode()} containers are not supported (little-endian RIFF only)")
        if head[:4] != b"RIFF" or head[8:12] != b"WAVE":
            raise ValueError(f"{path}: not a RIFF/WAVE file")
        fmt, pos = None, 12
        while True:
            fh.seek(pos)
            ck = fh.read(8)
            if len(ck) < 8:
                raise ValueError(f"{path}: no data chunk")
            cid, csize = ck[:4], struct.unpack("<I", ck[4:])[0]
            if cid == b"fmt ":
                fmt = _parse_fmt(path, fh.read(csize))
            elif cid == b"data":
                if fmt is None:
                    raise ValueError(f"{path}: the data chunk comes before any fmt chunk")
                rate, channels, encoding = fmt
                offset = pos + 8
                have = size - offset
                nbytes = have if csize in (0, 0xFFFFFFFF) else min(csize, have)
                fb = channels * SAMPLE_BYTES[encoding]
                frames = max(nbytes, 0) // fb
                if frames < 1:
                    raise ValueError(f"{path}: zero frames")
                return WavHeader(rate, channels, frames, encoding, offset, frames * fb)
            pos += 8 + csize + (csize & 1)


def read_payload(path, header: WavHeader, out=None):
    """The raw `data` bytes of `path` (header.data_bytes of them).  With `out` -- a writable buffer of at least that
    size, e.g. a slice of a pinned uint8 tensor's numpy view -- they are read straight into it and the count comes
    back; otherwise a `bytes` object does."""
    with open(os.fspath(path), "rb") as fh:
        fh.seek(header.data_offset)
        if out is None:
            data = fh.read(header.data_bytes)
            got = len(data)
        else:
            view = memoryview(out).cast("B")[:header.data_bytes]
            got = fh.readinto(view)
            data = got
    if got != header.data_bytes:
        raise ValueError(f"{os.fspath(path)}: {got} payload bytes where the header promised {header.data_bytes}")
    return data


def write_wav(path, payload, rate: int, channels: int, encoding: str) -> None:
    """Write `payload` (the interleaved little-endian samples, whole frames) as a WAV file: format tag 1 for "s16" and
    "s24", tag 3 with a `fact` chunk for "f32"."""
    path = os.fspath(path)
    if encoding not in WRITE_TAGS:
        raise ValueError(f"{path}: encoding must be one of {sorted(WRITE_TAGS)} (got {encoding!r})")
    rate, channels = int(rate), int(channels)
    if rate < 1 or channels < 1:
        raise ValueError(f"{path}: rate = {rate} and channels = {channels} must be at least 1")
    payload = bytes(payload)
    w = SAMPLE_BYTES[encoding]
    fb = channels * w
    if not payload or len(payload) % fb:
        raise ValueError(f"{path}: a payload of {len(payload)} bytes is not a positive number of {fb}-byte frames")
    tag = WRITE_TAGS[encoding]
    fmt = struct.pack("<HHIIHH", tag, channels, rate, rate * fb, fb, 8 * w)
    chunks = []
    if tag == TAG_FLOAT:
        chunks.append(b"fmt " + struct.pack("<I", 18) + fmt + struct.pack("<H", 0))
        chunks.append(b"fact" + struct.pack("<II", 4, len(payload) // fb))
    else:
        chunks.append(b"fmt " + struct.pack("<I", 16) + fmt)
    chunks.append(b"data" + struct.pack("<I", len(payload)) + payload + (b"\0" if len(payload) & 1 else b""))
    body = b"WAVE" + b"".join(chunks)
    if len(body) > 0xFFFFFFFF:
        raise ValueError(f"{path}: {len(body)} bytes do not fit a RIFF container (RF64 is not written)")
    with open(path, "wb") as fh:
        fh.write(b"RIFF" + struct.pack("<I", len(body)) + body)
