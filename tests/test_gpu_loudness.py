"""dsn_loudness / dsn_apply_gain (csrc/loudness.hip) against the float64 restatement (tests/loudness_restatement.py).

Shapes are the smallest at which the kernels can go wrong: no block, exactly one, a block boundary inside a chunk of
the recursion, more chunks than the carry pass has threads (its runs of 2 and of 4 chunks), more than one peak tile,
lengths that are no multiple of 4, h = 1103 (a segment that is no multiple of anything).
  I            no further from the float64 restatement than the restatement's own float32 run on the same input
  blocks       J and the gated count equal, after the restatement shows every block 1e-6 LU clear of both gates
  true peak    within (S + 1) 2^-24 max_j sum |h| |x|: every interpolated value is one product and S - 1 fused
               multiply-adds (test_gpu_resample.py's bound), and |max a - max b| <= max |a - b|
  sample peak  exact
and bit for bit: an item in a NaN-padded ragged mixed-rate batch against the item alone, a permuted batch, a second
call, a base pointer one float off 16-byte alignment; apply_gain against x * g in torch, and in place."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

from ditsep_amd import native
from tests import loudness_restatement as lr
from tests import resample_restatement as rr
from tests.util import make_engine

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = open(os.path.join(ROOT, "ditsep_amd", "csrc", "kernels.h")).read()
SRC = open(os.path.join(ROOT, "ditsep_amd", "csrc", "loudness.hip")).read()
CHUNK = int(re.search(r"#define LOUD_CHUNK (\d+)", HDR).group(1))
PEAK_TILE = int(re.search(r"#define LOUD_PEAK_TILE (\d+)", HDR).group(1))
LPB = int(re.search(r"constexpr int LPB = (\d+);", SRC).group(1))
SPAN = CHUNK * LPB            # samples the carry pass covers with one chunk per thread
U = 2.0 ** -24

# (fs, L): see the module docstring
LENGTHS = [(8000, 1), (8000, 3199), (8000, 3200), (8000, 3999), (8000, 4000), (8000, 32000), (8000, SPAN + 4465),
           (8000, 3 * SPAN + 4321), (11025, 4411), (11025, 4412), (11025, 9000), (48000, 48000)]


@pytest.fixture(scope="module")
def eng():
    e = make_engine()
    assert e.cfg.score_kind == native.SCORE_NONE
    yield e
    e.close()


@pytest.fixture(scope="module")
def taps():
    p = native.resample_plan(1, 4)
    assert (p["new"], p["support"]) == (4, 13)
    return p, rr.dense_from_compact(p["k0"], p["taps"], p["K"])


def noise(seed, Cn, L, amp=0.1):
    g = torch.Generator().manual_seed(seed)
    return amp * torch.randn((Cn, L), generator=g)


def burst(seed, Cn, L, fs):
    """a loud second inside a quiet bed: the bed passes the absolute gate and falls to the relative one"""
    x = noise(seed, Cn, L, 1e-3)
    lo = (L // 2 // fs) * fs
    x[:, lo:lo + fs] += noise(seed + 1, Cn, min(fs, L - lo), 0.3)
    return x


_worst = {"ratio": 0.0}


def check(eng, taps, x, fs, what):
    """one item x [C, L] float32 through the device against the restatement"""
    plan, h = taps
    got = eng.loudness(x, fs)
    x64 = x.double().numpy()
    m64 = lr.measure(x64, fs, taps=h)
    m32 = lr.measure(x.numpy(), fs, dtype=np.float32, true_peak=False)
    margin = lr.gate_margin(m64)
    assert margin >= 1e-6, f"{what}: a block lies {margin:.2e} LU from a gate; choose another input"
    I = float(got["loudness"][0])
    assert int(got["blocks"][0]) == m64["blocks"], what
    assert int(got["gated_blocks"][0]) == m64["gated_blocks"], what
    assert int(got["nonfinite"][0]) == 0
    if m64["loudness"] == -math.inf:
        assert I == -math.inf, (what, I)
    else:
        err, err32 = abs(I - m64["loudness"]), abs(m32["loudness"] - m64["loudness"])
        print(f"{what}: I = {I:.6f} LUFS, |device - float64| = {err:.2e} LU, |float32 - float64| = {err32:.2e} LU")
        assert err <= err32, f"{what}: {err:.3e} LU from the float64 restatement, its float32 run is {err32:.3e} away"
        if err32 > 0:
            _worst["ratio"] = max(_worst["ratio"], err / err32)
    assert float(got["sample_peak"][0]) == float(x.abs().max()), what
    bound = (plan["support"] + 1) * U * m64["true_peak_scale"]
    tp_err = abs(float(got["true_peak"][0]) - m64["true_peak"])
    print(f"{what}: true peak {float(got['true_peak'][0]):.6f}, error / bound {tp_err / max(bound, 1e-300):.3f}")
    assert tp_err <= bound, f"{what}: true peak off by {tp_err:.3e}, bound {bound:.3e}"
    return got, m64


@pytest.mark.parametrize("Cn", [1, 2])
@pytest.mark.parametrize("fs,L", LENGTHS, ids=lambda v: str(v))
def test_white_noise_against_the_restatement(eng, taps, fs, L, Cn):
    got, m64 = check(eng, taps, noise(fs + L + Cn, Cn, L), fs, f"noise fs={fs} L={L} C={Cn}")
    h = lr.block_step(fs)
    assert m64["blocks"] == ((L - 4 * h) // h + 1 if L >= 4 * h else 0)
    if L == 3199:
        assert float(got["loudness"][0]) == -math.inf and int(got["blocks"][0]) == 0
    if L == 3200:
        assert int(got["blocks"][0]) == 1 and math.isfinite(float(got["loudness"][0]))


def test_worst_ratio_is_reported(eng):
    print(f"worst |device - float64| / |float32 - float64| over the cases above: {_worst['ratio']:.3e}")


@pytest.mark.parametrize("fs,L,Cn", [(8000, 32000, 1), (8000, 32000, 2), (11025, 44100, 2), (48000, 144000, 1)])
def test_relative_gate_removes_the_quiet_bed(eng, taps, fs, L, Cn):
    got, m64 = check(eng, taps, burst(fs + Cn, Cn, L, fs), fs, f"burst fs={fs} L={L} C={Cn}")
    assert 0 < m64["gated_blocks"] < m64["blocks"]            # the relative gate did remove blocks
    assert (m64["l"] > -70.0).all()                           # .. and they had all passed the absolute one


@pytest.mark.parametrize("fs,L,Cn", [(8000, 1, 1), (8000, 4000, 2), (11025, 9000, 1)])
def test_all_zero_items(eng, fs, L, Cn):
    got = eng.loudness(torch.zeros((Cn, L)), fs)
    h = lr.block_step(fs)
    assert float(got["loudness"][0]) == -math.inf and int(got["gated_blocks"][0]) == 0
    assert int(got["blocks"][0]) == ((L - 4 * h) // h + 1 if L >= 4 * h else 0)
    assert float(got["true_peak"][0]) == 0.0 and float(got["sample_peak"][0]) == 0.0


def test_without_true_peak(eng):
    x = noise(5, 2, 9000)
    a, b = eng.loudness(x, 11025), eng.loudness(x, 11025, true_peak=False)
    assert math.isnan(float(b["true_peak"][0]))
    for k in ("loudness", "sample_peak", "blocks", "gated_blocks", "nonfinite"):
        assert torch.equal(a[k], b[k]), k


# ---------------------------------------------------------------------------------------------- bit for bit
ITEMS = [(8000, 32000, 1), (48000, 48000, 2), (11025, 9000, 2), (8000, 3199, 1), (8000, SPAN + 4465, 2),
         (11025, 4412, 1), (44100, 30001, 2), (8000, 1, 1)]
KEYS = ("loudness", "true_peak", "sample_peak", "blocks", "gated_blocks", "nonfinite")


@pytest.fixture(scope="module")
def ragged(eng):
    """the mixed-rate batch, padded with NaN past every item's end and in the channels it does not have; and every
    item's statistics alone"""
    clips = [burst(70 + b, Cn, L, fs) if L >= 4 * fs else noise(70 + b, Cn, L) for b, (fs, L, Cn) in enumerate(ITEMS)]
    Lmax = max(L for _, L, _ in ITEMS) + 37
    x = torch.full((len(ITEMS), 2, Lmax), float("nan"))
    for b, c in enumerate(clips):
        x[b, :c.shape[0], :c.shape[1]] = c
    alone = [eng.loudness(c, fs) for c, (fs, _, _) in zip(clips, ITEMS)]
    return clips, x, alone


def _same(got, b, alone, what):
    for k in KEYS:
        assert torch.equal(got[k][b:b + 1], alone[k]), (what, k, got[k][b], alone[k])


def test_ragged_mixed_rate_batch_gives_each_item_its_own_bits(eng, ragged):
    clips, x, alone = ragged
    got = eng.loudness(x, [fs for fs, _, _ in ITEMS], [L for _, L, _ in ITEMS], [c for _, _, c in ITEMS])
    assert not torch.isnan(got["loudness"]).any() and int(got["nonfinite"].sum()) == 0     # no NaN was read
    for b in range(len(ITEMS)):
        _same(got, b, alone[b], f"item {b}")
    again = eng.loudness(x, [fs for fs, _, _ in ITEMS], [L for _, L, _ in ITEMS], [c for _, _, c in ITEMS])
    for k in KEYS:
        assert torch.equal(got[k], again[k]), f"second call: {k}"


def test_permuted_batch(eng, ragged):
    clips, x, alone = ragged
    perm = [5, 2, 7, 0, 3, 6, 1, 4]
    got = eng.loudness(x[perm], [ITEMS[p][0] for p in perm], [ITEMS[p][1] for p in perm], [ITEMS[p][2] for p in perm])
    for b, p in enumerate(perm):
        _same(got, b, alone[p], f"item {p} at position {b}")


def test_base_pointer_one_float_off(eng, ragged):
    clips, x, alone = ragged
    for b in (0, 1, 6):
        c = clips[b]
        flat = torch.full((c.numel() + 5,), float("nan"), device="cuda")
        for off in (1, 2, 3):
            v = flat[off:off + c.numel()].view(c.shape)
            v.copy_(c)
            assert v.data_ptr() % 16 == (flat.data_ptr() + 4 * off) % 16 and v.is_contiguous()
            _same(eng.loudness(v, ITEMS[b][0]), 0, alone[b], f"item {b}, {off} floats off")


def test_nan_sample_is_counted_and_the_peaks_are_nan(eng):
    x = noise(9, 2, 9000)
    x[1, 4500] = float("nan")
    x[0, 17] = float("inf")
    got = eng.loudness(x, 8000)
    assert int(got["nonfinite"][0]) == 2
    assert math.isnan(float(got["true_peak"][0])) and math.isnan(float(got["sample_peak"][0]))
    torch.cuda.synchronize()
    clean = eng.loudness(noise(9, 2, 9000), 8000)                  # .. and the next call is unharmed
    assert int(clean["nonfinite"][0]) == 0 and math.isfinite(float(clean["true_peak"][0]))


# ---------------------------------------------------------------------------------------------- the gain
@pytest.mark.parametrize("L", [1, 1003, 4096, 2 * 4096 + 6])
def test_apply_gain_is_one_float32_product(eng, L):
    R, Cn = 5, 2
    x = torch.randn((R, Cn, L), generator=torch.Generator().manual_seed(L)).cuda()
    lens = [L, max(1, L - 1), max(1, L // 2 + 1), 1, max(1, L - 5)]
    chans = [2, 1, 2, 1, 2]
    g = torch.tensor([0.5, 1.2345678, 3.0e-3, 1.0, 7.7], dtype=torch.float32)
    want = x * g.cuda()[:, None, None]
    for r in range(R):
        want[r, :, lens[r]:] = 0.0
        want[r, chans[r]:] = 0.0
    xn = x.clone()
    for r in range(R):                                             # nothing there may be read
        xn[r, :, lens[r]:] = float("nan")
        xn[r, chans[r]:] = float("nan")
    out = eng.apply_gain(xn, g, lens, chans)
    assert torch.equal(out, want)
    flat = torch.zeros(xn.numel() + 3, device="cuda")               # a base pointer one float off, in and out
    v = flat[1:1 + xn.numel()].view(xn.shape)
    v.copy_(xn)
    assert torch.equal(eng.apply_gain(v, g, lens, chans), want)
    inplace = xn.clone()
    assert eng.apply_gain(inplace, g, lens, chans, out=inplace) is inplace
    assert torch.equal(inplace, want)
    assert torch.equal(eng.apply_gain(x, g), x * g.cuda()[:, None, None])


def test_gain_reaches_the_target(eng):
    """measure, form the gain on the host, apply, measure again: the target within the float32 rounding of the gain"""
    x = noise(3, 2, 32000, 0.05)
    a = eng.loudness(x, 16000)
    g = native.loudness_gain(a["loudness"].tolist(), a["true_peak"].tolist(), None, -23.0, None)
    y = eng.apply_gain(x[None], g["gain"])
    b = eng.loudness(y, 16000)
    assert abs(float(b["loudness"][0]) - (-23.0)) <= 20.0 * math.log10(1.0 + 2.0 ** -23) + 1e-6
    lim = native.loudness_gain(a["loudness"].tolist(), a["true_peak"].tolist(), None, 0.0, -1.0)
    assert lim["limited"] == [True]
    c = eng.loudness(eng.apply_gain(x[None], lim["gain"]), 16000)
    assert abs(20.0 * math.log10(float(c["true_peak"][0])) - (-1.0)) <= 1e-4


# ---------------------------------------------------------------------------------------------- refusals, by name
def test_library_refusals(eng):
    lib = eng.lib
    x = torch.zeros((2, 2, 100), device="cuda")
    stats = (C.c_double * 12)()
    i32 = C.c_int32 * 2
    ok = dict(x=C.c_void_p(x.data_ptr()), B=2, Cn=2, L=100, lens=i32(100, 50), ch=i32(2, 1), rates=i32(8000, 48000))

    def call(**kw):
        a = dict(ok, **kw)
        rc = lib.dsn_loudness(eng.ctx, a["x"], a["B"], a["Cn"], a["L"], a["lens"], a["ch"], a["rates"], 1, stats, None)
        return rc, lib.dsn_last_error(eng.ctx).decode()

    before = eng.workspace_bytes()
    for kw, msg in [(dict(x=None), "null"), (dict(rates=None), "null"), (dict(B=0), "outside [1, 65535]"),
                    (dict(B=65536), "outside [1, 65535]"), (dict(Cn=3), "C = 3"), (dict(Cn=0), "C = 0"),
                    (dict(ch=i32(2, 3)), "channels[1] = 3"), (dict(ch=i32(0, 1)), "channels[0] = 0"),
                    (dict(lens=i32(100, 101)), "lens[1] = 101"), (dict(lens=i32(0, 1)), "lens[0] = 0"),
                    (dict(rates=i32(7999, 8000)), "rates[0] = 7999"), (dict(rates=i32(8000, 192001)), "rates[1] = 192001"),
                    (dict(L=2 ** 30 + 1), "Lmax")]:
        rc, err = call(**kw)
        assert rc == -1 and "dsn_loudness" in err and msg in err, (kw, rc, err)
    assert eng.workspace_bytes() == before                       # nothing was allocated
    rc, _ = call(lens=None, ch=None)                              # NULL lens / channels: Lmax and C for every item
    assert rc == 0
    g = (C.c_float * 2)(1.0, 2.0)
    rc = lib.dsn_apply_gain(eng.ctx, C.c_void_p(x.data_ptr()), 2, 2, 100, None, None, g, C.c_void_p(x.data_ptr() + 4), None)
    assert rc == -1 and "overlaps" in lib.dsn_last_error(eng.ctx).decode()
    rc = lib.dsn_apply_gain(eng.ctx, C.c_void_p(x.data_ptr()), 2, 2, 100, None, None, None, C.c_void_p(x.data_ptr()), None)
    assert rc == -1 and "null" in lib.dsn_last_error(eng.ctx).decode()
