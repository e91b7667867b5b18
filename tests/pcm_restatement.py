"""numpy restatement of dsn_pcm_decode, dsn_pcm_encode and dsn_scale_output (include/ditsep_hip.h; csrc/pcm.hip).
Imports nothing from the package.  decode and quantise are float32 and defined to the bit; scale_output is float64."""
import numpy as np

SAMPLE_BYTES = {"u8": 1, "s16": 2, "s24": 3, "s32": 4, "f32": 4, "f64": 8}
QNAN = np.uint32(0x7FC00000)


def decode(payload, frames, channels, encoding):
    """the interleaved little-endian payload -> float32 [channels, frames], torchaudio.load(normalize=True)'s scaling"""
    w = SAMPLE_BYTES[encoding]
    raw = np.frombuffer(bytes(payload), dtype=np.uint8)
    assert raw.size == frames * channels * w, (raw.size, frames, channels, encoding)
    if encoding == "u8":
        x = (raw.astype(np.int32) - 128).astype(np.float32) / np.float32(128)
    elif encoding == "s16":
        x = raw.view("<i2").astype(np.float32) / np.float32(2 ** 15)
    elif encoding == "s24":
        b = raw.reshape(-1, 3).astype(np.int32)
        v = b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16)
        v = np.where(v >= 1 << 23, v - (1 << 24), v)
        x = v.astype(np.float32) / np.float32(2 ** 23)
    elif encoding == "s32":
        x = raw.view("<i4").astype(np.float32) * np.float32(2.0 ** -31)      # one rounding (nearest even), exact scaling
    elif encoding == "f32":
        x = raw.view("<f4").copy()
    elif encoding == "f64":
        d = raw.view("<f8")
        with np.errstate(over="ignore", invalid="ignore"):
            x = d.astype(np.float32)
        x.view(np.uint32)[np.isnan(d)] = QNAN
    else:
        raise ValueError(encoding)
    return np.ascontiguousarray(x.reshape(frames, channels).T)


def downmix(x):
    """[C, L] float32 -> [L]: (x_0 + .. + x_{C-1}) / C in float32 in that order; one channel passes as it is"""
    if x.shape[0] == 1:
        return x[0].copy()
    with np.errstate(over="ignore", invalid="ignore"):
        s = x[0].copy()
        for c in range(1, x.shape[0]):
            s = (s + x[c]).astype(np.float32)
        return (s / np.float32(x.shape[0])).astype(np.float32)


def quantise(x, encoding):
    """float32 [L] -> (payload bytes, clipped count).  s16 / s24: rint(x 2^(b-1)) ties to even, clamped, NaN -> 0;
    clipped counts the samples whose rounded value lay outside the range or was not finite.  f32: the bits, count 0."""
    x = np.asarray(x, dtype=np.float32)
    if encoding == "f32":
        return x.astype("<f4").tobytes(), 0
    bits = {"s16": 16, "s24": 24}[encoding]
    scale = np.float32(2.0 ** (bits - 1))
    with np.errstate(over="ignore", invalid="ignore"):
        y = np.rint(x * scale).astype(np.float32)
        bad = ~((y >= -scale) & (y <= scale - 1))
        y = np.where(np.isnan(y), np.float32(0), np.clip(y, -scale, scale - 1))
    q = y.astype(np.int64)
    if encoding == "s16":
        return q.astype("<i2").tobytes(), int(bad.sum())
    u = (q & 0xFFFFFF).astype(np.uint32)
    out = np.stack([u & 0xFF, (u >> 8) & 0xFF, (u >> 16) & 0xFF], axis=1).astype(np.uint8)
    return out.tobytes(), int(bad.sum())


def scale_output(mix, sep):
    """mix [L], sep [n, L] -> (alpha [n], kappa [n]) in float64: alpha = sum m s / sum (s^2 + 1e-10), and
    kappa = sum |m s| / |sum m s|, the condition number of the numerator's sum"""
    m, s = np.asarray(mix, dtype=np.float64), np.asarray(sep, dtype=np.float64)
    num = (m[None] * s).sum(axis=-1)
    den = (s * s + 1e-10).sum(axis=-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        kappa = np.abs(m[None] * s).sum(axis=-1) / np.abs(num)
    return num / den, kappa
