"""dsn_pcm_decode, dsn_pcm_encode and dsn_scale_output (ditsep_amd/csrc/pcm.hip) through the Engine methods on an
engine with no score network and no codec, against tests/pcm_restatement.py.

decode and encode are compared bit for bit (float32 as int32 views, payloads as bytes): every conversion is exact or
one defined rounding.  scale_output's gain is compared with the float64 restatement within bounds that follow from the
arithmetic (u = 2^-24, L the row's samples, kappa = sum |m s| / |sum m s| the condition number of the numerator):
* the device's sums are float64 over exact products, any order: each is within L 2^-53 (kappa, resp. 1) of the exact
  sum, the restatement's own sums likewise, and alpha is rounded once to float32:
  |alpha_dev - alpha| <= (u + L 2^-52 kappa) |alpha|;
* out = fl(alpha_dev sep) adds one more float32 rounding: |out - alpha sep| <= (2 u + L 2^-52 kappa) |alpha sep| (the
  cross term u^2 is below the slack the first bound leaves).
Everything else -- a row against the row alone, reruns -- is bit for bit."""
import os
import re

import numpy as np
import pytest
import torch

from ditsep_amd import native
from tests import pcm_restatement as pr
from tests.util import make_engine

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = open(os.path.join(ROOT, "ditsep_amd", "csrc", "pcm.hip")).read()
TILE = int(re.search(r"constexpr int PCM_TILE = (\d+);", SRC).group(1))        # frames / samples per workgroup
STILE = int(re.search(r"constexpr int SCALE_TILE = (\d+);", SRC).group(1))     # samples per workgroup of the gain's sums
U = 2.0 ** -24


@pytest.fixture(scope="module")
def eng():
    e = make_engine()
    assert e.cfg.score_kind == native.SCORE_NONE
    yield e
    e.close()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


# ------------------------------------------------------------------ decode
# (encoding, channels, frames, byte offset mod 16; None: wherever the previous item ended)
ITEMS = [("u8", 1, 1, 0), ("s16", 2, 2, 13), ("s24", 3, TILE - 1, 1), ("s32", 1, TILE, 3), ("f32", 2, TILE + 1, 13),
         ("f64", 1, 3 * TILE + 37, 1), ("s24", 1, TILE + 1, None), ("s16", 1, 3 * TILE + 37, 3), ("u8", 3, 5, 0),
         ("f64", 2, 7, 13), ("s32", 2, 2 * TILE + 3, None), ("f32", 1, 9, 3)]


def payload_of(enc, channels, frames, rng):
    """random samples with the extreme codes of the format first (as far as the item has room)"""
    n = frames * channels
    if enc == "u8":
        v = rng.integers(0, 256, n).astype(np.uint8)
        v[:3] = [0, 128, 255][:n]
        return v.tobytes()
    if enc == "s16":
        v = rng.integers(-2 ** 15, 2 ** 15, n).astype("<i2")
        v[:2] = [-2 ** 15, 2 ** 15 - 1][:n]
        return v.tobytes()
    if enc == "s24":
        v = rng.integers(-2 ** 23, 2 ** 23, n)
        v[:4] = [-2 ** 23, 2 ** 23 - 1, -1, 1][:n]
        return b"".join(int(x & 0xFFFFFF).to_bytes(3, "little") for x in v)
    if enc == "s32":
        v = rng.integers(-2 ** 31, 2 ** 31, n).astype("<i4")
        # the extremes, and values that need the rounding to 24 bits: ties both ways, just above and below a tie
        special = [-2 ** 31, 2 ** 31 - 1, 2 ** 24 + 1, 2 ** 24 + 3, -(2 ** 24 + 1), 2 ** 31 - 65, 2 ** 31 - 64,
                   0x7FFFFF81, 2 ** 25 + 2, 2 ** 25 + 6, 2 ** 25 + 3]
        v[:len(special)] = special[:n]
        return v.tobytes()
    if enc == "f32":
        v = rng.standard_normal(n).astype("<f4")
        if channels == 1:            # NaN payloads (quiet and signalling), infinities, a subnormal, -0.0: the bits pass
            v.view(np.uint32)[:8] = [0x7FC12345, 0xFFC00001, 0x7F800001, 0x7F800000, 0xFF800000, 0x00000001,
                                     0x80000000, 0x7FFFFFFF][:n]
        return v.tobytes()
    v = rng.standard_normal(n).astype("<f8")
    if channels == 1:                # overflow both ways, subnormals of both formats, a tie, NaN with a payload
        special = [1e300, -1e300, 5e-324, 1e-40, -1e-46, 1.0 + 2.0 ** -24, 1.0 + 3 * 2.0 ** -24, float("nan"),
                   3.4028235677973366e38, float("inf")]
        v[:len(special)] = special[:n]
        v.view(np.uint64)[len(special)] = 0xFFF8000000012345
    return v.tobytes()


@pytest.fixture(scope="module")
def batch():
    """the payloads back to back at the prescribed offsets; the last item ends on the buffer's last byte"""
    rng = np.random.default_rng(41)
    payloads = [payload_of(e, c, f, rng) for e, c, f, _ in ITEMS]
    offs, cur = [], 0
    for (e, c, f, mod), p in zip(ITEMS, payloads):
        if mod is not None:
            cur += (mod - cur) % 16 + (32 if offs else 0)
        offs.append(cur)
        cur += len(p)
    offs[1] = 45                                        # (13 mod 16; item 0 is one byte at 0)
    assert offs[2] > 45 + len(payloads[1]) and cur % 16 != 0
    assert {o % 16 for o in offs} >= {0, 1, 3, 13}

    def image(fill):
        raw = np.full(cur, fill, dtype=np.uint8)
        for o, p in zip(offs, payloads):
            raw[o:o + len(p)] = np.frombuffer(p, dtype=np.uint8)
        return torch.from_numpy(raw)

    items = [(o, f, c, e) for o, (e, c, f, _) in zip(offs, ITEMS)]
    want = [pr.decode(p, f, c, e) for p, (e, c, f, _) in zip(payloads, ITEMS)]
    assert np.isnan(np.frombuffer(bytes([0xFF] * 4), dtype="<f4"))[0]
    return {"items": items, "payloads": payloads, "want": want, "raw_nan": image(0xFF), "raw_zero": image(0)}


def test_decode_mixed_batch_downmix(eng, batch):
    out, frames = eng.pcm_decode(batch["raw_nan"], batch["items"], downmix=True)
    Lmax = max(f for _, _, f, _ in ITEMS)
    assert tuple(out.shape) == (len(ITEMS), 1, Lmax) and frames == [f for _, _, f, _ in ITEMS] and Lmax % 4 != 0
    got = out.cpu().numpy()
    for b, (want, (e, c, f, _)) in enumerate(zip(batch["want"], ITEMS)):
        assert np.array_equal(bits(got[b, 0, :f]), bits(pr.downmix(want))), f"item {b} ({e} x {c}, {f} frames)"
        assert not bits(got[b, 0, f:]).any(), f"item {b}: not zero past its end"
    # the gaps between the items hold 0xFF (NaN as float32): with zeros there nothing changes
    again, _ = eng.pcm_decode(batch["raw_zero"], batch["items"], downmix=True)
    assert torch.equal(out.view(torch.int32), again.view(torch.int32))
    # a buffer that is not 16-byte aligned takes the byte loads: the same bits
    dev = torch.cat([torch.zeros(1, dtype=torch.uint8), batch["raw_nan"]]).to(eng.device)
    assert dev[1:].data_ptr() % 16 == 1
    shifted, _ = eng.pcm_decode(dev[1:], batch["items"], downmix=True)
    assert torch.equal(out.view(torch.int32), shifted.view(torch.int32))


def test_decode_mixed_batch_channels(eng, batch):
    out, _ = eng.pcm_decode(batch["raw_nan"], batch["items"], downmix=False)
    assert tuple(out.shape) == (len(ITEMS), 3, max(f for _, _, f, _ in ITEMS))
    got = out.cpu().numpy()
    for b, (want, (e, c, f, _)) in enumerate(zip(batch["want"], ITEMS)):
        assert np.array_equal(bits(got[b, :c, :f]), bits(want)), f"item {b} ({e} x {c}, {f} frames)"
        assert not bits(got[b, c:]).any() and not bits(got[b, :, f:]).any(), f"item {b}: unused channels / tail not zero"


def test_decode_item_alone(eng, batch):
    """every item of the batch is the item decoded alone (its payload at offset 0 of its own buffer; frame counts that
    are multiples of 4 take the 16-byte stores there)"""
    out, _ = eng.pcm_decode(batch["raw_nan"], batch["items"], downmix=True)
    full, _ = eng.pcm_decode(batch["raw_nan"], batch["items"], downmix=False)
    for b, (p, (e, c, f, _)) in enumerate(zip(batch["payloads"], ITEMS)):
        alone, fr = eng.pcm_decode(p, [(0, f, c, e)], downmix=True)
        assert fr == [f] and tuple(alone.shape) == (1, 1, f)
        assert torch.equal(alone[0].view(torch.int32), out[b, :, :f].view(torch.int32)), f"item {b}"
        alone, _ = eng.pcm_decode(p, [(0, f, c, e)], downmix=False)
        assert torch.equal(alone[0].view(torch.int32), full[b, :c, :f].view(torch.int32)), f"item {b}"


def test_decode_refusals_launch_nothing(eng):
    raw = torch.zeros(64, dtype=torch.uint8, device=eng.device)
    out = torch.full((1, 1, 8), 7.0, device=eng.device)

    def call(off, frames, ch, enc, nbytes=64, Cout=1, downmix=1, Lmax=8):
        i32 = native.C.c_int32
        return eng.lib.dsn_pcm_decode(eng.ctx, native._ptr(raw), nbytes, 1, (native.C.c_int64 * 1)(off),
                                      (i32 * 1)(frames), (i32 * 1)(ch), (i32 * 1)(enc), downmix, native._ptr(out), Cout,
                                      Lmax, eng._stream())

    err = lambda: eng.lib.dsn_last_error(eng.ctx).decode()
    assert call(0, 8, 1, 6) != 0 and "encoding[0] = 6" in err()
    assert call(0, 9, 1, 0) != 0 and "frames[0] = 9 outside [1, Lmax = 8]" in err()
    assert call(0, 0, 1, 0) != 0 and "frames[0] = 0" in err()
    assert call(0, 8, 0, 0) != 0 and "channels[0] = 0 < 1" in err()
    assert call(49, 8, 1, 1) != 0 and "outside [0, nbytes = 64)" in err()
    assert call(-1, 8, 1, 0) != 0 and "outside [0, nbytes = 64)" in err()
    assert call(0, 1, 7, 5) != 0 and "DSN_PCM_MAX_FRAME_BYTES" in err()
    assert call(0, 8, 2, 0, Cout=1, downmix=0) != 0 and "channels[0] = 2 > Cout = 1" in err()
    assert call(0, 8, 2, 0, Cout=2, downmix=1) != 0 and "downmix gives one channel" in err()
    with pytest.raises(ValueError, match="outside"):
        eng.pcm_decode(raw, [(60, 8, 1, "u8")])
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    assert call(48, 8, 1, 1) == 0                       # the last item may end on the buffer's last byte
    torch.cuda.synchronize()
    assert bool((out == 0.0).all())


# ------------------------------------------------------------------ encode
LENS = [1, 7, TILE - 1, TILE + 1, 2 * TILE + 37]


def rows_for(encoding):
    """odd row lengths (so s16 and s24 rows start unaligned); ties, full scale and the non-finite values first; NaN in
    the padding"""
    g = np.random.default_rng(43)
    lsb = 2.0 ** -(15 if encoding != "s24" else 23)
    special = np.array([0.5 * lsb, -0.5 * lsb, 1.5 * lsb, -1.5 * lsb, 2.5 * lsb, -2.5 * lsb, 1.0, -1.0, 1 - 2.0 ** -16,
                        np.inf, -np.inf, np.nan, -1 - lsb, 3e38, -0.0], dtype=np.float32)
    x = np.full((len(LENS), max(LENS)), np.nan, dtype=np.float32)
    for r, L in enumerate(LENS):
        x[r, :L] = (0.4 * g.standard_normal(L)).astype(np.float32)
        k = min(L, special.size)
        x[r, :k] = np.roll(special, -r)[:k]
    return x


@pytest.mark.parametrize("encoding", ["s16", "s24", "f32"])
def test_encode(eng, encoding):
    x = rows_for(encoding)
    want = [pr.quantise(x[r, :L], encoding) for r, L in enumerate(LENS)]
    payloads, clipped = eng.pcm_encode(torch.from_numpy(x), LENS, encoding)
    for r in range(len(LENS)):
        assert payloads[r] == want[r][0], f"row {r}"
    assert clipped == [w[1] for w in want]
    if encoding != "f32":
        # 1.0, +-inf, NaN, -1 - lsb, 3e38 -- and 1 - 2^-16 as s16, where it rounds to 2^15; half an lsb is not clipped
        assert clipped[-1] >= (7 if encoding == "s16" else 6) and clipped[0] == 0
    # rows placed with gaps in a buffer filled with 0xA5: only each row's own bytes change, and a rerun gives the same
    w = native.PCM_SAMPLE_BYTES[encoding]
    offs, cur = [], 5
    for L in LENS:
        offs.append(cur)
        cur += L * w + 7
    buf = torch.full((cur + 33,), 0xA5, dtype=torch.uint8, device=eng.device)
    placed, clipped2 = eng.pcm_encode(torch.from_numpy(x), LENS, encoding, offsets=offs, out=buf)
    assert placed == payloads and clipped2 == clipped
    host = buf.cpu().numpy()
    keep = np.ones(host.size, dtype=bool)
    for o, L in zip(offs, LENS):
        keep[o:o + L * w] = False
        assert host[o:o + L * w].tobytes() == pr.quantise(x[offs.index(o), :L], encoding)[0]
    assert bool((host[keep] == 0xA5).all()), "bytes outside the rows were written"
    first = host.copy()
    eng.pcm_encode(torch.from_numpy(x), LENS, encoding, offsets=offs, out=buf)
    assert np.array_equal(buf.cpu().numpy(), first)


def test_encode_then_decode_on_the_grid(eng):
    g = np.random.default_rng(47)
    v = g.integers(-2 ** 15, 2 ** 15, (3, TILE + 5))
    v[0, :2] = [-2 ** 15, 2 ** 15 - 1]
    x = torch.from_numpy((v / 2.0 ** 15).astype(np.float32))
    lens = [TILE + 5, 3, TILE - 1]
    payloads, clipped = eng.pcm_encode(x, lens, "s16")
    assert clipped == [0, 0, 0]
    offs = np.cumsum([0] + [len(p) for p in payloads[:-1]]).tolist()
    back, _ = eng.pcm_decode(b"".join(payloads), [(o, L, 1, "s16") for o, L in zip(offs, lens)])
    for r, L in enumerate(lens):
        assert torch.equal(back[r, 0, :L].cpu(), x[r, :L])


def test_encode_refusals(eng):
    x = torch.zeros((2, 8), device=eng.device)
    buf = torch.full((40,), 0xA5, dtype=torch.uint8, device=eng.device)

    def call(lens, offs, enc=1, nbytes=40):
        return eng.lib.dsn_pcm_encode(eng.ctx, native._ptr(x), 2, 8, (native.C.c_int32 * 2)(*lens), enc,
                                      native._ptr(buf), nbytes, (native.C.c_int64 * 2)(*offs), None, eng._stream())

    err = lambda: eng.lib.dsn_last_error(eng.ctx).decode()
    assert call([8, 8], [0, 15]) != 0 and "rows 0 and 1 overlap" in err()
    assert call([8, 8], [16, 0]) == 0
    assert call([8, 8], [0, 25]) != 0 and "outside [0, nbytes = 40)" in err()
    assert call([8, 9], [0, 16]) != 0 and "lens[1] = 9 outside [1, Lmax = 8]" in err()
    assert call([8, 8], [0, 16], enc=0) != 0 and "encoding = 0" in err()
    with pytest.raises(ValueError, match="encoding"):
        eng.pcm_encode(x, None, "u8")
    torch.cuda.synchronize()
    assert bool((buf[32:] == 0xA5).all()) and bool((buf[:32] == 0).all())


# ------------------------------------------------------------------ scale_output
SLENS = [1, 7, 1000, 2 * STILE + 123]


@pytest.fixture(scope="module")
def scale_inputs():
    g = torch.Generator().manual_seed(53)
    Lmax = max(SLENS)
    mix = 0.3 * torch.randn((len(SLENS), Lmax), generator=g)
    sep = 0.7 * mix[:, None] + 0.05 * torch.randn((len(SLENS), 2, Lmax), generator=g)
    for b, L in enumerate(SLENS):
        mix[b, L:] = float("nan")
        sep[b, :, L:] = float("nan")
    return mix, sep


def test_scale_output(eng, scale_inputs):
    mix, sep = scale_inputs
    out, alpha = eng.scale_output(mix, sep, SLENS)
    assert tuple(out.shape) == tuple(sep.shape) and tuple(alpha.shape) == (len(SLENS), 2)
    assert not bool(torch.isnan(out).any())
    again, alpha2 = eng.scale_output(mix[:, None], sep, SLENS)                  # [B, 1, Lmax] is the same mixture
    assert torch.equal(out, again) and torch.equal(alpha, alpha2)
    for b, L in enumerate(SLENS):
        alone, a1 = eng.scale_output(mix[b:b + 1, :L], sep[b:b + 1, :, :L])
        assert torch.equal(alone[0], out[b, :, :L]) and torch.equal(a1[0], alpha[b]), f"item {b} differs from it alone"
        assert bool((out[b, :, L:] == 0).all())
        want, kappa = pr.scale_output(mix[b, :L].numpy(), sep[b, :, :L].numpy())
        assert float(kappa.max()) < 1e3
        a = alpha[b].double().numpy()
        rel = U + L * 2.0 ** -52 * kappa
        print(f"item {b} L {L}: kappa {kappa}, |alpha_dev - alpha| / bound {np.abs(a - want) / (rel * np.abs(want))}")
        assert np.all(np.abs(a - want) <= rel * np.abs(want))
        exact = want[:, None] * sep[b, :, :L].double().numpy()
        err = np.abs(out[b, :, :L].cpu().double().numpy() - exact)
        assert np.all(err <= (2 * U + L * 2.0 ** -52 * kappa)[:, None] * np.abs(exact))


def test_scale_output_zero_estimate_and_refusals(eng, scale_inputs):
    mix, sep = scale_inputs
    sep = sep.clone()
    sep[2, 0, :SLENS[2]] = 0.0
    out, alpha = eng.scale_output(mix, sep, SLENS)
    assert float(alpha[2, 0]) == 0.0 and bool((out[2, 0] == 0).all()) and float(alpha[2, 1]) > 0.5
    assert not bool(torch.isnan(out).any())
    with pytest.raises(ValueError, match="outside"):
        eng.scale_output(mix, sep, [1, 7, 1000, max(SLENS) + 1])
    with pytest.raises(ValueError, match="mix must be"):
        eng.scale_output(mix[:2], sep)
    rc = eng.lib.dsn_scale_output(eng.ctx, None, native._ptr(out), 1, 2, 8, None, native._ptr(out), None, eng._stream())
    assert rc != 0 and "mix, sep or out is null" in eng.lib.dsn_last_error(eng.ctx).decode()
