"""The load-time weight preparation, the per-call movers and the feature kernels (ditsep_amd/csrc/kernels.hip,
ncsn_kernels.hip, codec_ragged.hip), one launch wrapper at a time through dsn_test_kernel on caller-owned tensors, against
tests/prep_kernels_ref.py.  tests/test_prep_kernels_host.py shows on the CPU that each check refuses its mutation.

Every output buffer carries a sentinel tail -- NaN (fp32), 0x7fff (planes), 0xA5 (fp8 and scale bytes) -- that must
survive, every input must come back bit-identical (Keep), and every case prints its worst error over its bound.

Bit-exact (no element excused): pack_weight in its six modes (both planes equal dsn_split of the float32 product),
pack_bias_swiglu, pack_tokens, unpack_tokens, copy_rows, to_planes, zero_tail, ncsn_pack, the zero tail of
vae_sample_ragged, and pack_weight_fp8 (bytes and scale bytes equal mx_exponent + e4m3 round-to-nearest-even of the value
times the exact power of two), whose float64 properties are checked independently (check_fp8_properties).

Bounded: (R + 1) 2^-24 A with R the float32 roundings on the longest path of the kernel's expression order, nothing
contracted, and A the sum of the magnitudes of the terms in float64 (derivations in tests/prep_kernels_ref.py):
  wn_scale         R = ceil(inner / 64) + 8, relative       packed_row_sum   R = ceil(K / 64) + 5 (one plane), + 7 (two)
  fp8_row_sum      R = ceil(K / 256) + 5                    bias_plus_wbeta  R = ceil(K / 64) + 7
  snake_params     R = 2 (a), 4 (1 / b): expf at 2 units    ncsn_output      R = cin + 3
  vae_sample_ragged  R = 7 (tests/sampler_kernels_ref.py::vae_sample) on the valid frames
  timestep_features, ncsn_fourier, rope_tables: an argument term (R_arg + 1) 2^-24 |phase| with R_arg = 3,
    log units + 3 and pow units + 2, plus a function term for sinf / cosf.  The toolchain ships no accuracy table of the
    device's math library, so every function term is MEASURED on the reference alone (prep_kernels_ref.function_units:
    numpy's float32 call against float64 at the float32 argument, times 4, at least 2 units of 2^-24; each case prints
    its figures).  They depend on the host's numpy: sin / cos 2.0 .. 4.1 units, logf 2.0 .. 4.9, powf 3.2 over the cases
    on the two hosts tried.  Plane outputs: one unit of the operand format on top (check_planes_abs).

Composition (float64 on the CPU from the device's packed output, weights exact in every format, 1e-12 relative):
CONVT under the decoder's phase-GEMM descriptor equals conv_transpose1d; CONV equals conv1d at dilation 1, 3, 9; the
SwiGLU row order under swiglu64 equals a silu(g); the folded LayerNorm equals LN(x) W^T + b to the two float32 kernels'
own bounds, with 16-bit planes and with the fp8 pair.

Worst error over bound measured on an MI355X (0 of all elements differ in every bit-exact case, 1,054,720-element
PACK_LINEAR, 1,049,600-element pack_tokens / unpack_tokens and 4,198,400-element to_planes included):
  pack_weight_fp8 1.000 of half an e4m3 step (the planted ties)      fp8_row_sum 0.000 (its sums are exact)
  wn_scale 0.187    packed_row_sum 0.132    bias_plus_wbeta 0.159    snake_params 0.358    ncsn_output 0.307
  vae_sample_ragged 0.204    timestep_features 0.363    ncsn_fourier 0.884 (fp16, nf 130; 0.59 and below in the other
  formats)    rope_tables 0.392    folded LayerNorm 0.033 (0.012 through the fp8 pair)
  composition: 4.6e-16 and below against conv1d / conv_transpose1d, 0 for the SwiGLU row order
The module runs in about 3 s.
"""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from ditsep_amd.native import PACK_MODES
from tests import prep_kernels_ref as R
from tests import sampler_kernels_ref as K
from tests.prep_kernels_ref import ALL, NAME
from tests.test_gpu_gemm_kernels import (DEV, IS_F16, PLANES, SENT16, TAIL, conv_ref, nan_f32, nan_planes,
                                         scatter_positions, silu, swiglu64)
from tests.util import make_engine

pytestmark = pytest.mark.gpu

SENT8 = 0xA5
SEED0 = 2468
F32 = R.FP16            # the engine that runs the fp32-only kernels


@pytest.fixture(scope="module")
def eng():
    engs = {p: make_engine(precision=p) for p in ALL}
    yield engs
    for e in engs.values():
        e.close()


def gen(i=0):
    return torch.Generator().manual_seed(SEED0 + i)


def same_bits(a, b):
    a, b = a.contiguous(), b.contiguous()
    it = {4: torch.int32, 2: torch.int16, 1: torch.uint8}[a.element_size()]
    return torch.equal(a.view(it), b.view(it))


class Keep:
    """device copies of a case's inputs; check() asserts that every one came back bit-identical"""

    def __init__(self):
        self.items = []

    def __call__(self, t, dtype=torch.float32):
        d = t.detach().to(device=DEV, dtype=dtype).contiguous()
        self.items.append((d, d.cpu().clone()))
        return d

    def check(self, what):
        for i, (d, c) in enumerate(self.items):
            assert same_bits(d.cpu(), c), f"{what}: input {i} was modified"


def nan_bytes(n):
    return torch.full((n + TAIL,), SENT8, device=DEV, dtype=torch.uint8)


def planes_out(pl, n, what):
    raw = pl.cpu()
    assert (raw[:, n:] == SENT16).all(), f"{what}: planes written past the output"
    return raw[:, :n]


def f32_out(buf, n, what):
    b = buf.cpu()
    assert torch.isnan(b[n:]).all(), f"{what}: fp32 output written past its end"
    return b[:n]


def bytes_out(buf, n, what):
    b = buf.cpu()
    assert (b[n:] == SENT8).all(), f"{what}: bytes written past the output"
    return b[:n]


def split_planes(raw, prec):
    """raw int16 [P][n] -> (hi, lo) float64, lo None with one plane"""
    dt = torch.float16 if IS_F16[prec] else torch.bfloat16
    v = [raw[p].contiguous().view(dt).double() for p in range(raw.shape[0])]
    return v[0], (v[1] if len(v) == 2 else None)


# ================================================================================================ pack_weight
def pw_cases():
    c = []
    for N, Kk in [(5, 7), (33, 130), (1030, 1024)]:
        c += [("linear", (N, Kk), s) for s in (False, True)]
    for N in (32, 96):
        c += [("linear_swiglu", (N, 40), s) for s in (False, True)]
    for d in [(6, 5, 7), (16, 8, 1), (130, 12, 7)]:
        c += [("conv", d, s) for s in (False, True)]
    for d in [(8, 12, 2), (5, 3, 4), (16, 4, 8)]:
        c += [("convt", d, s) for s in (False, True)]
    c += [("conv2d", d, False) for d in [(3, 4, 3, 32, 9), (10, 12, 40, 64, 9), (8, 8, 32, 32, 1)]]
    c += [("nin", d, False) for d in [(12, 12), (8, 20)]]
    return c


def pw_id(c):
    return f"{c[0]}-{'x'.join(map(str, c[1]))}{'-scaled' if c[2] else ''}"


def run_pack_weight(e, prec, mode, dims, scaled, src=None, scale=None, seed=0):
    """-> (raw planes [P][N K] on the CPU, the float32 [N][K] they must hold, N, K)"""
    g = gen(seed)
    keep = Keep()
    kw = dict(mode=PACK_MODES[mode])
    sc = cs = None
    pos = lambda n: (torch.rand(n, generator=g) + 0.5).float()
    if mode in ("linear", "linear_swiglu", "nin"):
        N, Kk = dims
        src = R.weight(g, *((Kk, N) if mode == "nin" else (N, Kk))) if src is None else src
        cs = (pos(Kk) if scale is None else scale) if scaled else None
        want = R.pack_weight_ref(mode, src, colscale=cs)
    elif mode == "conv":
        Cout, Cin, kw_ = dims
        src = R.weight(g, Cout, Cin, kw_) if src is None else src
        sc = (pos(Cout) if scale is None else scale) if scaled else None
        want = R.pack_weight_ref(mode, src, scale=sc)
        N, Kk = Cout, kw_ * Cin
        kw.update(Cin=Cin, Cout=Cout, kw=kw_, stride=1)
    elif mode == "convt":
        Cin, Cout, s = dims
        src = R.weight(g, Cin, Cout, 2 * s) if src is None else src
        sc = (pos(Cin) if scale is None else scale) if scaled else None
        want = R.pack_weight_ref(mode, src, scale=sc)
        N, Kk = s * Cout, 2 * Cin
        kw.update(Cin=Cin, Cout=Cout, kw=2 * s, stride=s)
    else:
        Cout, N, Cin, cpad, taps = dims
        src = R.weight(g, Cout, Cin, taps) if src is None else src
        want = R.pack_weight_ref(mode, src, N=N, cin_pad=cpad)
        Kk = taps * cpad
        kw.update(Cin=Cin, Cout=Cout, kw=taps, stride=cpad)
    assert tuple(want.shape) == (N, Kk)
    pl = nan_planes(PLANES[prec], N * Kk)
    what = f"pack_weight {NAME[prec]} {mode} {dims}{' scaled' if scaled else ''}"
    e.test_kernel("pack_weight", x=keep(src), count=src.numel(), N=N, K=Kk, out_planes=pl,
                  scale=None if sc is None else keep(sc), colscale=None if cs is None else keep(cs), **kw)
    torch.cuda.synchronize()
    keep.check(what)
    return planes_out(pl, N * Kk, what), want, what


@pytest.mark.parametrize("case", pw_cases(), ids=pw_id)
@pytest.mark.parametrize("prec", ALL, ids=lambda p: NAME[p])
def test_pack_weight(eng, prec, case):
    mode, dims, scaled = case
    raw, want, what = run_pack_weight(eng[prec], prec, mode, dims, scaled, seed=len(pw_id(case)))
    R.check_bits(raw, R.plane_bits(want, prec), what)
    if mode == "conv2d":                      # the padding is +0 bits in every plane
        Cout, N, Cin, cpad, taps = dims
        pad = torch.ones(N, taps, cpad, dtype=torch.bool)
        pad[:Cout, :, :Cin] = False
        assert (raw[:, pad.reshape(-1)] == 0).all(), f"{what}: padding not +0"


@pytest.mark.parametrize("N", [32, 96, 2080])
def test_pack_bias_swiglu(eng, N):
    keep = Keep()
    b = R.weight(gen(N), N, zero_row=False)
    out = nan_f32(N)
    eng[F32].test_kernel("pack_bias_swiglu", x=keep(b), N=N, out_f32=out)
    torch.cuda.synchronize()
    keep.check("pack_bias_swiglu")
    R.check_f32_exact(f32_out(out, N, "pack_bias_swiglu"), R.swiglu_rows(b), f"pack_bias_swiglu N {N}")


# ================================================================================================ movers
TOKEN_SHAPES = [(2, 5, 3, 7), (1, 8, 0, 1), (2, 96, 32, 4100)]


@pytest.mark.parametrize("shape", TOKEN_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("prec", ALL, ids=lambda p: NAME[p])
def test_pack_tokens(eng, prec, shape):
    B, C0, C1, T = shape
    g = gen(T)
    s0 = R.weight(g, B, C0, T, zero_row=False)
    s1 = R.weight(g, B, C1, T, zero_row=False) if C1 else None
    want = R.pack_tokens_ref(s0, s1).reshape(-1)
    n = want.numel()
    assert (n > R.CAP) == (T == 4100)
    for f32o, plo in ((True, False), (False, True), (True, True)):
        keep = Keep()
        of = nan_f32(n) if f32o else None
        pl = nan_planes(PLANES[prec], n) if plo else None
        what = f"pack_tokens {NAME[prec]} {shape} f32 {f32o} planes {plo}"
        eng[prec].test_kernel("pack_tokens", x=keep(s0), y=None if s1 is None else keep(s1), B=B, C0=C0, C1=C1, T=T,
                              out_f32=of, out_planes=pl)
        torch.cuda.synchronize()
        keep.check(what)
        if f32o:
            R.check_f32_exact(f32_out(of, n, what), want, what + " fp32")
        if plo:
            R.check_bits(planes_out(pl, n, what), R.plane_bits(want, prec), what + " planes")


@pytest.mark.parametrize("shape", [(2, 6, 5), (1, 1, 1), (2, 128, 4100)], ids=lambda s: "x".join(map(str, s)))
def test_unpack_tokens_and_round_trip(eng, shape):
    B, C, T = shape
    n = B * C * T
    keep = Keep()
    x = R.weight(gen(C), B * T, C, zero_row=False)
    out = nan_f32(n)
    e = eng[F32]
    e.test_kernel("unpack_tokens", x=keep(x), B=B, C=C, T=T, out_f32=out)
    torch.cuda.synchronize()
    what = f"unpack_tokens {shape}"
    got = f32_out(out, n, what)
    R.check_f32_exact(got, R.unpack_tokens_ref(x, B, C, T).reshape(-1), what)
    back = nan_f32(n)
    e.test_kernel("pack_tokens", x=out[:n], B=B, C0=C, C1=0, T=T, out_f32=back)      # [B][C][T] -> [B T][C] again
    torch.cuda.synchronize()
    keep.check(what)
    R.check_f32_exact(f32_out(back, n, what), x.reshape(-1), what + " round trip")


def test_copy_rows(eng):
    for rows in (1, 3, 9):
        for width in (4, 64, 1024):
            for stride in (width, 3 * width):
                keep = Keep()
                src = R.weight(gen(rows + width), rows, width, zero_row=False)
                n = (rows - 1) * stride + width
                out = nan_f32(n)
                what = f"copy_rows rows {rows} width {width} stride {stride}"
                eng[F32].test_kernel("copy_rows", x=keep(src), rows=rows, C=width, dst_stride=stride, out_f32=out)
                torch.cuda.synchronize()
                keep.check(what)
                want = torch.full((rows, stride), float("nan"))
                want[:, :width] = src                           # the gaps keep their NaN, bit for bit
                R.check_bits(R.f32_bits(f32_out(out, n, what)), R.f32_bits(want.reshape(-1)[:n]), what)


@pytest.mark.parametrize("n", [4, 252, 4198400])
@pytest.mark.parametrize("prec", ALL, ids=lambda p: NAME[p])
def test_to_planes(eng, prec, n):
    keep = Keep()
    x = R.weight(gen(n % 1000), n, zero_row=False)
    pl = nan_planes(PLANES[prec], n)
    what = f"to_planes {NAME[prec]} n {n}"
    eng[prec].test_kernel("to_planes", x=keep(x), count=n, out_planes=pl)
    torch.cuda.synchronize()
    keep.check(what)
    R.check_bits(planes_out(pl, n, what), R.plane_bits(x, prec), what)


@pytest.mark.parametrize("lens", [[1, 5, 10], [2, 2, 2]], ids=str)
def test_zero_tail(eng, lens):
    B, n, D, T = 3, 2, 4, 9
    keep = Keep()
    x = torch.randn(B, n, D, T, generator=gen(lens[0]))
    x[1, 0, 0, :] = -0.0                                   # (a -0 in the kept part stays -0, in the tail becomes +0)
    tot = x.numel()
    buf = nan_f32(tot)
    buf[:tot] = x.reshape(-1).to(DEV)
    what = f"zero_tail lens {lens}"
    eng[F32].test_kernel("zero_tail", x=buf, lens=keep(torch.tensor(lens), torch.int32), B=B, n=n, D=D, T=T)
    torch.cuda.synchronize()
    keep.check(what)
    R.check_f32_exact(f32_out(buf, tot, what), R.zero_tail_ref(x, lens).reshape(-1), what)


def test_vae_sample_ragged(eng):
    S, D, T = 3, 32, 5
    frames = [0, 3, T]
    enc, noise = K.vae_inputs(S, D, T, SEED0)
    want, A, Rn = K.vae_sample(enc, noise)
    keep = Keep()
    out = nan_f32(S * D * T)
    eng[F32].test_kernel("vae_sample_ragged", x=keep(torch.from_numpy(enc)), z=keep(torch.from_numpy(noise)),
                         lens=keep(torch.tensor(frames), torch.int32), B=S, D=D, T=T, out_f32=out)
    torch.cuda.synchronize()
    keep.check("vae_sample_ragged")
    got = f32_out(out, S * D * T, "vae_sample_ragged").reshape(S, D, T)
    valid = (torch.arange(T).view(1, 1, T) < torch.tensor(frames).view(S, 1, 1)).expand(S, D, T)
    v = valid.numpy()
    K.check(got.numpy()[v], want[v], np.broadcast_to(A, want.shape)[v], Rn, "vae_sample_ragged valid frames")
    R.check_bits(R.f32_bits(got)[~valid], torch.zeros(int((~valid).sum()), dtype=torch.int32), "vae_sample_ragged tail +0")


@pytest.mark.parametrize("shape", [(2, 2, 4, 5, 8, 32), (1, 3, 3, 7, 7, 8)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("prec", ALL, ids=lambda p: NAME[p])
def test_ncsn_pack(eng, prec, shape):
    B, n, H, T, Wp, Cp = shape
    g = gen(T)
    keep = Keep()
    xt, mix = R.weight(g, B, n, H, T, zero_row=False), R.weight(g, B, 1, H, T, zero_row=False)
    want = R.ncsn_pack_ref(xt, mix, Wp, Cp).reshape(-1)
    tot = want.numel()
    of, pl = nan_f32(tot), nan_planes(PLANES[prec], tot)
    what = f"ncsn_pack {NAME[prec]} {shape}"
    eng[prec].test_kernel("ncsn_pack", x=keep(xt), y=keep(mix), B=B, n=n, H=H, T=T, Wp=Wp, Cp=Cp, out_f32=of, out_planes=pl)
    torch.cuda.synchronize()
    keep.check(what)
    R.check_f32_exact(f32_out(of, tot, what), want, what + " fp32")
    R.check_bits(planes_out(pl, tot, what), R.plane_bits(want, prec), what + " planes")
    pad = torch.ones(B, H, Wp, Cp, dtype=torch.bool)
    pad[:, :, :T, :n + 1] = False
    assert (R.f32_bits(of.cpu()[:tot])[pad.reshape(-1)] == 0).all(), f"{what}: padding not +0"


# ================================================================================================ MX fp8 weights
def run_pack_fp8(e, x, swiglu, colscale):
    """x float32 [N][K] -> (bytes [N][K], scale bytes [N][K/32] on the CPU, the float32 [N][K] that was quantised)"""
    N, Kk = x.shape
    keep = Keep()
    b8, s8 = nan_bytes(N * Kk), nan_bytes(N * Kk // 32)
    e.test_kernel("pack_weight_fp8", x=keep(x), N=N, K=Kk, mode=1 if swiglu else 0, out_fp8=b8, out_fp8_scale=s8,
                  colscale=None if colscale is None else keep(colscale))
    torch.cuda.synchronize()
    keep.check("pack_weight_fp8")
    src = R.pack_weight_ref("linear_swiglu" if swiglu else "linear", x, colscale=colscale)
    return bytes_out(b8, N * Kk, "fp8 bytes").reshape(N, Kk), bytes_out(s8, N * Kk // 32, "fp8 scales").reshape(N, Kk // 32), src


FP8_CASES = [(1, 32, False), (5, 160, False), (64, 128, True), (96, 160, True)]


@pytest.mark.parametrize("scaled", [False, True], ids=["plain", "colscale"])
@pytest.mark.parametrize("case", FP8_CASES, ids=lambda c: f"{c[0]}x{c[1]}{'-swiglu' if c[2] else ''}")
def test_pack_weight_fp8(eng, case, scaled):
    N, Kk, swiglu = case
    what = f"pack_weight_fp8 {N}x{Kk}{' swiglu' if swiglu else ''}{' colscale' if scaled else ''}"
    cs = (torch.rand(Kk, generator=gen(Kk)) + 0.5).float() if scaled else None
    # (1, 32) is one block: every edge block of the list is its own launch there
    sources = [b.reshape(1, 32) for b in R.fp8_edge_blocks()] if N * Kk == 32 else [R.fp8_source(N, Kk, SEED0 + N)]
    for i, x in enumerate(sources):
        b8, s8, src = run_pack_fp8(eng[F32], x, swiglu, cs)
        wb, ws = R.mx_pack_ref(src)
        R.check_bits(s8, ws, f"{what} [{i}] scale bytes")
        R.check_bits(b8, wb, f"{what} [{i}] e4m3 bytes")
        R.check_fp8_properties(src, b8, s8, f"{what} [{i}]")


# ================================================================================================ bounded: reductions
@pytest.mark.parametrize("inner", [1, 7, 63, 64, 65, 896])
def test_wn_scale(eng, inner):
    for rows in (1, 3, 4, 5, 130):
        g = gen(inner + rows)
        keep = Keep()
        v = torch.randn(rows, inner, generator=g) * torch.exp2(torch.randint(-20, 21, (rows, 1), generator=g).float())
        gg = torch.randn(rows, generator=g)
        want, A, Rn = R.wn_scale(v.float(), gg)
        assert Rn + 1 <= -(-inner // 64) + 10
        out = nan_f32(rows)
        what = f"wn_scale rows {rows} inner {inner}"
        eng[F32].test_kernel("wn_scale", x=keep(v), gamma=keep(gg), rows=rows, count=inner, out_f32=out)
        torch.cuda.synchronize()
        keep.check(what)
        K.check(f32_out(out, rows, what).numpy(), want, A, Rn, what)


def device_planes(e, prec, W, mode="linear", colscale=None):
    """pack_weight on the device -> the int16 plane tensor (with its tail) and its decoded (hi, lo)"""
    N, Kk = W.shape
    pl = nan_planes(PLANES[prec], N * Kk)
    e.test_kernel("pack_weight", x=W.to(DEV).contiguous(), count=W.numel(), N=N, K=Kk, mode=PACK_MODES[mode],
                  out_planes=pl, colscale=None if colscale is None else colscale.to(DEV).contiguous())
    torch.cuda.synchronize()
    hi, lo = split_planes(planes_out(pl, N * Kk, "pack_weight"), prec)
    return pl, hi.reshape(N, Kk), (None if lo is None else lo.reshape(N, Kk))


def run_row_sum(e, pl, N, Kk, what):
    before = pl.cpu().clone()
    outs = []
    for _ in range(2):
        out = nan_f32(N)
        e.test_kernel("packed_row_sum", in_planes=pl, N=N, K=Kk, out_f32=out)
        torch.cuda.synchronize()
        outs.append(f32_out(out, N, what))
    assert same_bits(pl.cpu(), before), f"{what}: the planes were modified"
    assert same_bits(outs[0], outs[1]), f"{what}: two calls returned different bits"
    return outs[0]


@pytest.mark.parametrize("Kk", [4, 63, 64, 65, 200, 1024])
@pytest.mark.parametrize("prec", ALL, ids=lambda p: NAME[p])
def test_packed_row_sum(eng, prec, Kk):
    for N in (1, 5, 33):
        W = torch.randn(N, Kk, generator=gen(N + Kk))
        W[N - 1, Kk // 2:2 * (Kk // 2)] = -W[N - 1, :Kk // 2]          # a row that cancels to about 0
        pl, hi, lo = device_planes(eng[prec], prec, W)
        want, A, Rn = R.packed_row_sum(hi, lo)
        assert Rn + 1 <= -(-Kk // 64) + 8
        what = f"packed_row_sum {NAME[prec]} N {N} K {Kk}"
        K.check(run_row_sum(eng[prec], pl, N, Kk, what).numpy(), want, A, Rn, what)


def run_fp8_row_sum(e, b8, s8, what):
    N, Kk = b8.shape
    db, ds = b8.to(DEV).contiguous(), s8.to(DEV).contiguous()
    outs = []
    for _ in range(2):
        out = nan_f32(N)
        e.test_kernel("fp8_row_sum", in_fp8=db, in_fp8_scale=ds, N=N, K=Kk, out_f32=out)
        torch.cuda.synchronize()
        outs.append(f32_out(out, N, what))
    assert torch.equal(db.cpu(), b8) and torch.equal(ds.cpu(), s8), f"{what}: an input was modified"
    assert same_bits(outs[0], outs[1]), f"{what}: two calls returned different bits"
    return outs[0]


@pytest.mark.parametrize("Kk", [32, 128, 160, 1024])
def test_fp8_row_sum(eng, Kk):
    N = 5
    x = torch.randn(N, Kk, generator=gen(Kk))
    x[N - 1, Kk // 2:] = -x[N - 1, :Kk // 2]
    b8, s8, _ = run_pack_fp8(eng[F32], x, False, None)
    want, A, Rn = R.fp8_row_sum(R.mx_decode(b8, s8))
    assert Rn + 1 <= -(-Kk // 256) + 9
    what = f"fp8_row_sum K {Kk}"
    K.check(run_fp8_row_sum(eng[F32], b8, s8, what).numpy(), want, A, Rn, what)


@pytest.mark.parametrize("Kk", [4, 65, 512])
def test_bias_plus_wbeta(eng, Kk):
    for N in (1, 5, 33):
        for with_bias in (False, True):
            g = gen(N + Kk)
            keep = Keep()
            W, beta, bias = torch.randn(N, Kk, generator=g), torch.randn(Kk, generator=g), torch.randn(N, generator=g)
            want, A, Rn = R.bias_plus_wbeta(W, beta, bias if with_bias else None)
            out = nan_f32(N)
            what = f"bias_plus_wbeta N {N} K {Kk} bias {with_bias}"
            eng[F32].test_kernel("bias_plus_wbeta", x=keep(W), beta=keep(beta), bias=keep(bias) if with_bias else None,
                                 N=N, K=Kk, out_f32=out)
            torch.cuda.synchronize()
            keep.check(what)
            K.check(f32_out(out, N, what).numpy(), want, A, Rn, what)


@pytest.mark.parametrize("C", [1, 7, 300])
def test_snake_params(eng, C):
    g = gen(C)
    keep = Keep()
    alpha, beta = torch.rand(C, generator=g) * 8 - 4, torch.rand(C, generator=g) * 8 - 4
    alpha[0], beta[0] = 4.0, -4.0
    beta[C - 1] = -30.0                                     # the 1e-9 term dominates
    a, ib = nan_f32(C), nan_f32(C)
    eng[F32].test_kernel("snake_params", act_a=keep(alpha), act_b=keep(beta), C=C, out_f32=a, out2_f32=ib)
    torch.cuda.synchronize()
    keep.check("snake_params")
    outs = R.snake_params(alpha, beta)
    K.check_formula({"a": f32_out(a, C, "snake a").numpy(), "ib": f32_out(ib, C, "snake ib").numpy()}, outs, f"snake_params C {C}")


def test_ncsn_output(eng):
    B, n, H, T, Wp, Cp, cin = 2, 2, 4, 5, 8, 32, 3
    g = gen(5)
    keep = Keep()
    pyr = torch.full((B, H, Wp, Cp), float("nan"))           # the padding must not reach the output
    pyr[:, :, :T, :cin] = torch.randn(B, H, T, cin, generator=g)
    t = torch.rand(B, generator=g) * 0.97 + 0.03
    w, bias = torch.randn(n, cin, generator=g), torch.randn(n, generator=g)
    want, A, Rn = R.ncsn_output(torch.nan_to_num(pyr), t, w, bias, cin, n, T)
    tot = B * T * n * H
    out = nan_f32(tot)
    eng[F32].test_kernel("ncsn_output", x=keep(pyr), y=keep(t), w=keep(w), bias=keep(bias), B=B, n=n, H=H, T=T, Wp=Wp,
                         Cp=Cp, cin=cin, out_f32=out)
    torch.cuda.synchronize()
    keep.check("ncsn_output")
    K.check(f32_out(out, tot, "ncsn_output").numpy(), want, A, Rn, "ncsn_output")


# ================================================================================================ bounded: features
@pytest.mark.parametrize("half", [4, 128])
@pytest.mark.parametrize("prec", ALL, ids=lambda p: NAME[p])
def test_timestep_features(eng, prec, half):
    for B in (1, 3):
        g = gen(B + half)
        keep = Keep()
        t, w = torch.rand(B, generator=g), torch.randn(half, generator=g)
        t[0] = 1.0
        if B > 1:
            t[1] = 0.0
        want, bound, fu = R.timestep_features(t, w)
        pl = nan_planes(PLANES[prec], B * 2 * half)
        what = f"timestep_features {NAME[prec]} B {B} half {half} (sin / cos at {fu:.1f} units)"
        eng[prec].test_kernel("timestep_features", x=keep(t), w=keep(w), B=B, half=half, out_planes=pl)
        torch.cuda.synchronize()
        keep.check(what)
        R.check_planes_abs(planes_out(pl, B * 2 * half, what), want, bound, prec, what)


@pytest.mark.parametrize("nf", [4, 130])
@pytest.mark.parametrize("prec", ALL, ids=lambda p: NAME[p])
def test_ncsn_fourier(eng, prec, nf):
    B = 3
    g = gen(nf)
    keep = Keep()
    t, w = torch.rand(B, generator=g) * 0.97 + 0.03, 16 * torch.randn(nf, generator=g)
    t[0], t[1] = 0.03, 1.0
    want, bound, (lu, fu) = R.ncsn_fourier(t, w)
    pl = nan_planes(PLANES[prec], B * 2 * nf)
    what = f"ncsn_fourier {NAME[prec]} nf {nf} (log at {lu:.1f}, sin / cos at {fu:.1f} units)"
    eng[prec].test_kernel("ncsn_fourier", x=keep(t), w=keep(w), B=B, half=nf, out_planes=pl)
    torch.cuda.synchronize()
    keep.check(what)
    R.check_planes_abs(planes_out(pl, B * 2 * nf, what), want, bound, prec, what)


@pytest.mark.parametrize("S", [1, 33, 385])
def test_rope_tables(eng, S):
    rot = 32
    c, s = nan_f32(S * rot), nan_f32(S * rot)
    eng[F32].test_kernel("rope_tables", S=S, dh=rot, rope_cos=c, rope_sin=s)
    torch.cuda.synchronize()
    wc, ws, bound, (pu, fu) = R.rope_tables(S, rot)
    what = f"rope_tables S {S} (pow at {pu:.1f}, sin / cos at {fu:.1f} units)"
    R.check_abs(f32_out(c, S * rot, what).numpy(), wc, bound, what + " cos")
    R.check_abs(f32_out(s, S * rot, what).numpy(), ws, bound, what + " sin")


# ================================================================================================ composition
def exact_weight(g, *shape):
    """multiples of 1 / 64 in [-1, 1]: exact in every operand format, also times a power of two"""
    return torch.randint(-64, 65, shape, generator=g).float() / 64


def close64(got, want, what, tol=1e-12):
    err = float((got - want).abs().max()) / float(want.abs().max())
    print(f"{what}: float64 error {err:.2e} relative to the largest value (tolerance {tol:.0e})")
    assert err <= tol, f"{what}: {err:.3e} > {tol:.0e}"


def pow2(g, n):
    return torch.exp2(torch.randint(-3, 4, (n,), generator=g).float())


@pytest.mark.parametrize("dims", [(8, 12, 2), (5, 3, 4), (16, 4, 8)], ids=lambda d: "x".join(map(str, d)))
@pytest.mark.parametrize("prec", ALL, ids=lambda p: NAME[p])
def test_convt_layout_is_the_decoders_phase_gemm(eng, prec, dims):
    Cin, Cout, s = dims
    B, L = 2, 6
    g = gen(s)
    v, sc = exact_weight(g, Cin, Cout, 2 * s), pow2(g, Cin)
    raw, want, what = run_pack_weight(eng[prec], prec, "convt", dims, True, src=v, scale=sc)
    Wd = R.decode_bits(raw, prec).reshape(s * Cout, 2, Cin)
    assert torch.equal(Wd.reshape(-1), want.double().reshape(-1)), f"{what}: the exact weights were rounded"
    x = torch.randn(B, L, Cin, generator=g, dtype=torch.float64)
    rows = L + 1                                             # the decoder's descriptor: 2 taps, tap_dil = -1, no padding
    j = torch.arange(rows).view(rows, 1) - torch.arange(2).view(1, 2)
    ok = (j >= 0) & (j < L)
    y = torch.einsum("bjtc,ntc->bjn", x[:, j.clamp(0, L - 1), :] * ok.view(1, rows, 2, 1), Wd)
    flat, keep = scatter_positions(B, rows, s * Cout, L * s * Cout, s * Cout, -((s + 1) // 2) * Cout, L * s * Cout)
    assert torch.equal(flat.sort().values, torch.arange(B * L * s * Cout)), f"{what}: the scatter is not a bijection"
    out = torch.zeros(B * L * s * Cout, dtype=torch.float64)
    out[flat] = y[keep]
    ref = F.conv_transpose1d(x.transpose(1, 2), v.double() * sc.double()[:, None, None], stride=s, padding=(s + 1) // 2)
    close64(out.reshape(B, L * s, Cout), ref.transpose(1, 2), what + " vs conv_transpose1d")


@pytest.mark.parametrize("d", [1, 3, 9])
@pytest.mark.parametrize("prec", ALL, ids=lambda p: NAME[p])
def test_conv_layout_is_the_dilated_conv(eng, prec, d):
    Cout, Cin, kw = 6, 5, 7
    B, L = 2, 40
    g = gen(d)
    v, sc = exact_weight(g, Cout, Cin, kw), pow2(g, Cout)
    raw, want, what = run_pack_weight(eng[prec], prec, "conv", (Cout, Cin, kw), True, src=v, scale=sc)
    Wd = R.decode_bits(raw, prec)
    assert torch.equal(Wd, want.double().reshape(-1)), f"{what}: the exact weights were rounded"
    x = torch.randn(B * L * Cin, generator=g, dtype=torch.float64)
    pad = d * (kw - 1) // 2
    y = conv_ref(x, Wd, B=B, Lin=L, Cin=Cin, N=Cout, taps=kw, rows=L, tap_dil=d, in_pad=pad)
    ref = F.conv1d(x.reshape(B, L, Cin).transpose(1, 2), v.double() * sc.double()[:, None, None], dilation=d, padding=pad)
    close64(y, ref.transpose(1, 2), what + f" vs conv1d dilation {d}")


@pytest.mark.parametrize("prec", ALL, ids=lambda p: NAME[p])
def test_swiglu_layout_is_a_silu_g(eng, prec):
    N, Kk, M = 96, 40, 7
    g = gen(3)
    W, b = exact_weight(g, N, Kk), torch.randn(N, generator=g)
    raw, want, what = run_pack_weight(eng[prec], prec, "linear_swiglu", (N, Kk), False, src=W)
    Wp = R.decode_bits(raw, prec).reshape(N, Kk)
    bp = nan_f32(N)
    eng[prec].test_kernel("pack_bias_swiglu", x=b.to(DEV), N=N, out_f32=bp)
    torch.cuda.synchronize()
    x = torch.randn(M, Kk, generator=g, dtype=torch.float64)
    a, gate = (x @ W.double().t() + b.double()).chunk(2, -1)
    close64(swiglu64(x @ Wp.t() + f32_out(bp, N, what).double()), a * silu(gate), what + " under swiglu64")


def folded_ln_case(seed, N=64, Kk=128, M=9):
    g = gen(seed)
    W = torch.randn(N, Kk, generator=g) / math.sqrt(Kk)
    gamma, beta, b = torch.rand(Kk, generator=g) + 0.5, 0.3 * torch.randn(Kk, generator=g), torch.randn(N, generator=g)
    x = torch.randn(M, Kk, generator=g, dtype=torch.float64) + 1.5          # a mean that matters
    return W, gamma, beta, b, x


def folded_ln_check(e, W, gamma, beta, b, x, Wgd, colsum, cs_bound, what):
    """rstd (x Wg^T - mean colsum) + b' against LN(x) W^T + b in packed row order, decoded Wg on both sides"""
    N, Kk = W.shape
    bw, bp = nan_f32(N), nan_f32(N)
    e.test_kernel("bias_plus_wbeta", x=W.to(DEV), beta=beta.to(DEV), bias=b.to(DEV), N=N, K=Kk, out_f32=bw)
    e.test_kernel("pack_bias_swiglu", x=bw[:N], N=N, out_f32=bp)
    torch.cuda.synchronize()
    bprime = f32_out(bp, N, what).double()
    want_b, A_b, R_b = R.bias_plus_wbeta(W, beta, b)
    mean = x.mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(x.var(1, unbiased=False, keepdim=True) + 1e-5)
    lhs = rstd * (x @ Wgd.t() - mean * colsum.double()[None, :]) + bprime[None, :]
    rhs = rstd * ((x - mean) @ Wgd.t()) + R.swiglu_rows(torch.from_numpy(want_b))[None, :]
    tol = (mean.abs() * rstd) * cs_bound[None, :] + R.swiglu_rows(torch.from_numpy((R_b + 1) * R.U * A_b))[None, :] + \
        1e-12 * rhs.abs().max()
    ratio = float(((lhs - rhs).abs() / tol).max())
    print(f"{what}: worst error / bound {ratio:.3f}")
    assert ratio <= 1.0, f"{what}: the folded LayerNorm is off by {ratio:.3g} x the two kernels' bounds"


@pytest.mark.parametrize("prec", ALL, ids=lambda p: NAME[p])
def test_folded_layernorm(eng, prec):
    W, gamma, beta, b, x = folded_ln_case(11)
    N, Kk = W.shape
    pl, hi, lo = device_planes(eng[prec], prec, W, "linear_swiglu", gamma)
    what = f"folded LayerNorm {NAME[prec]}"
    colsum = run_row_sum(eng[prec], pl, N, Kk, what)
    want, A, Rn = R.packed_row_sum(hi, lo)
    folded_ln_check(eng[prec], W, gamma, beta, b, x, hi if lo is None else hi + lo, colsum,
                    torch.from_numpy((Rn + 1) * R.U * A), what)


def test_folded_layernorm_fp8(eng):
    W, gamma, beta, b, x = folded_ln_case(12)
    b8, s8, _ = run_pack_fp8(eng[F32], W, True, gamma)
    deq = R.mx_decode(b8, s8)
    colsum = run_fp8_row_sum(eng[F32], b8, s8, "folded LayerNorm fp8")
    want, A, Rn = R.fp8_row_sum(deq)
    folded_ln_check(eng[F32], W, gamma, beta, b, x, deq, colsum, torch.from_numpy((Rn + 1) * R.U * A), "folded LayerNorm fp8")


# ================================================================================================ refusals
def test_refusals(eng):
    """every refusal of the hook fails by name before any launch: the sentinel-filled outputs are intact afterwards"""
    e = eng[R.FP16X3]
    P = PLANES[R.FP16X3]
    n = 4096
    x = torch.zeros(n, device=DEV)
    i32 = torch.ones(4, device=DEV, dtype=torch.int32)
    of, of2, pl, b8, s8 = nan_f32(n), nan_f32(n), nan_planes(P, n), nan_bytes(n), nan_bytes(n)
    pw = dict(x=x, out_planes=pl)
    cases = [
        ("pack_weight", dict(pw, mode=1, N=48, K=8, count=384), "N % 32 != 0"),
        ("pack_bias_swiglu", dict(x=x, N=48, out_f32=of), "N % 32 != 0"),
        ("pack_weight_fp8", dict(x=x, mode=1, N=48, K=32, out_fp8=b8, out_fp8_scale=s8), "N % 32 != 0"),
        ("pack_weight_fp8", dict(x=x, mode=0, N=4, K=40, out_fp8=b8, out_fp8_scale=s8), "K % 32 != 0"),
        ("fp8_row_sum", dict(in_fp8=b8, in_fp8_scale=s8, N=4, K=40, out_f32=of), "K % 32 != 0"),
        ("pack_weight", dict(pw, mode=3, N=16, K=8, Cin=4, Cout=4, kw=6, stride=4, count=96), "kw != 2\\*stride"),
        ("pack_weight", dict(pw, mode=2, N=4, K=12, Cin=4, Cout=4, kw=3, stride=1, count=47), "count 47 !="),
        ("pack_weight", dict(pw, mode=0, N=4, K=8, count=32, scale=x), "scale is read by conv and convt only"),
        ("pack_weight", dict(pw, mode=5, N=4, K=8, count=32, colscale=x), "colscale is read by the linear modes only"),
        ("pack_weight", dict(pw, mode=4, N=4, K=36, Cin=8, Cout=4, kw=9, stride=4, count=288), "conv2d: needs stride"),
        ("pack_weight", dict(pw, mode=7, N=4, K=8, count=32), "unknown mode 7"),
        ("pack_weight", dict(pw, mode=0, N=0, K=8, count=0), "N and K must be positive"),
        ("pack_weight", dict(out_planes=pl, mode=0, N=4, K=8, count=32), "out_planes missing"),
        ("to_planes", dict(x=x, count=6, out_planes=pl), "count % 4 != 0"),
        ("to_planes", dict(x=x, count=0, out_planes=pl), "count % 4 != 0 or count < 1"),
        ("copy_rows", dict(x=x, rows=2, C=6, dst_stride=8, out_f32=of), "C % 4 != 0"),
        ("copy_rows", dict(x=x, rows=2, C=8, dst_stride=10, out_f32=of), "dst_stride % 4 != 0"),
        ("copy_rows", dict(x=x, rows=2, C=8, dst_stride=4, out_f32=of), "dst_stride < C"),
        ("copy_rows", dict(x=x, rows=0, C=8, dst_stride=8, out_f32=of), "rows and C must be positive"),
        ("ncsn_pack", dict(x=x, y=x, B=1, n=2, H=2, T=5, Wp=4, Cp=8, out_f32=of), "Wp 4 < T 5"),
        ("ncsn_pack", dict(x=x, y=x, B=1, n=2, H=2, T=4, Wp=4, Cp=2, out_f32=of), "Cp 2 < n \\+ 1"),
        ("ncsn_output", dict(x=x, y=x, w=x, bias=x, B=1, n=2, H=2, T=5, Wp=4, Cp=8, cin=3, out_f32=of), "Wp 4 < T 5"),
        ("ncsn_output", dict(x=x, y=x, w=x, bias=x, B=1, n=2, H=2, T=4, Wp=4, Cp=2, cin=3, out_f32=of), "Cp 2 < cin 3"),
        ("ncsn_output", dict(x=x, y=x, w=x, B=1, n=2, H=2, T=4, Wp=4, Cp=4, cin=3, out_f32=of), "bias or out_f32 missing"),
        ("wn_scale", dict(x=x, gamma=x, rows=0, count=4, out_f32=of), "rows and count must be positive"),
        ("wn_scale", dict(x=x, rows=2, count=4, out_f32=of), "gamma \\(g\\) or out_f32 missing"),
        ("packed_row_sum", dict(N=2, K=4, out_f32=of), "in_planes or out_f32 missing"),
        ("packed_row_sum", dict(in_planes=pl, in_ps=4, N=2, K=4, out_f32=of), "in_ps 4 < N\\*K"),
        ("bias_plus_wbeta", dict(x=x, N=2, K=4, out_f32=of), "beta or out_f32 missing"),
        ("snake_params", dict(act_a=x, act_b=x, C=4, out_f32=of), "out2_f32 missing"),
        ("snake_params", dict(act_a=x, act_b=x, C=0, out_f32=of, out2_f32=of2), "C must be positive"),
        ("pack_tokens", dict(x=x, B=1, C0=4, C1=2, T=3, out_f32=of), "does not go with C1 = 2"),
        ("pack_tokens", dict(x=x, y=x, B=1, C0=4, C1=0, T=3, out_f32=of), "does not go with C1 = 0"),
        ("pack_tokens", dict(x=x, B=1, C0=4, C1=0, T=3), "out_f32 and out_planes both missing"),
        ("unpack_tokens", dict(x=x, B=1, C=4, T=0, out_f32=of), "B, C, T must be positive"),
        ("zero_tail", dict(x=of, B=1, n=1, D=2, T=4), "x or lens missing"),
        ("vae_sample_ragged", dict(x=x, z=x, B=1, D=2, T=4, out_f32=of), "lens \\(frames\\) or out_f32 missing"),
        ("timestep_features", dict(x=x, w=x, B=1, half=0, out_planes=pl), "B and half must be positive"),
        ("ncsn_fourier", dict(x=x, B=1, half=4, out_planes=pl), "w or out_planes missing"),
        ("rope_tables", dict(S=4, dh=31, rope_cos=of, rope_sin=of2), "rotary width\\) even"),
        ("rope_tables", dict(S=4, dh=32, rope_cos=of), "rope_cos or rope_sin missing"),
    ]
    for kind, kw, match in cases:
        with pytest.raises(RuntimeError, match=match):
            e.test_kernel(kind, **kw)
    torch.cuda.synchronize()
    assert torch.isnan(of.cpu()).all() and torch.isnan(of2.cpu()).all(), "a refused call wrote fp32 output"
    assert (pl.cpu() == SENT16).all(), "a refused call wrote planes"
    assert (b8.cpu() == SENT8).all() and (s8.cpu() == SENT8).all(), "a refused call wrote fp8 output"
    assert (x.cpu() == 0).all() and (i32.cpu() == 1).all()


def test_engine_refuses_a_ragged_swiglu_weight():
    """pack_linear / pack_linear_fp8 (finalize) refuse a SwiGLU weight whose N is no multiple of 32 by name: its row map
    would read rows past the source"""
    from oracle import dit as odit

    for prec in (R.FP16, 5):
        dcfg = odit.DiTConfig(n_src=2, embed_dim=128, depth=1, num_heads=2)
        dsd = odit.random_dit_weights(dcfg, 32, out_gain=0.005)
        key = next(k for k in dsd if k.endswith("ff.ff.0.proj.weight"))
        dsd[key] = dsd[key][:1008].clone()                                         # N = 8 D - 16
        dsd[key.replace("weight", "bias")] = dsd[key.replace("weight", "bias")][:1008].clone()
        with pytest.raises(RuntimeError, match="SwiGLU weight needs N % 32 == 0"):
            make_engine(dcfg, dsd, precision=prec)
