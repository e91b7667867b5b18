"""Expected outputs, rounding counts and check functions for the load-time weight preparation, the per-call movers and
the feature kernels (ditsep_amd/csrc/kernels.hip, ncsn_kernels.hip, codec_ragged.hip), shared by
tests/test_gpu_prep_kernels.py (the device against them) and tests/test_prep_kernels_host.py (the checks against one
mutated output each).  No GPU is needed to import it.

Layouts are written in tensor terms (permute / reshape / stack of the checkpoint's own tensors), never as the kernels'
index arithmetic.  A multiply by `scale` / `colscale` is one float32 product, as on the device; what lands in operand
planes is dsn_split of that float32 value, restated by plane_bits (whose decoded sum is emulate_split of
tests/test_gpu_gemm_kernels.py, asserted by the host test).  The MX format is mx_exponent of tests/util.py plus e4m3
round-to-nearest-even of the value scaled by the exact power of two.

Bounded checks follow tests/sampler_kernels_ref.py: a formula returns (want, A, R) and check() holds every element to
(R + 1) 2^-24 A.  R is counted in each docstring on the kernel's expression order with nothing contracted.
"""
import math

import numpy as np
import torch

from tests.sampler_kernels_ref import CAP, U, check, f32  # noqa: F401  (re-exported)
from tests.test_gpu_gemm_kernels import BF16, FP16, FP16X3, IS_F16, MANT, PLANES, X3, emulate_split
from tests.util import mx_exponent

ALL = (BF16, FP16, X3, FP16X3)
NAME = {BF16: "bf16", FP16: "fp16", X3: "bf16x3", FP16X3: "fp16x3"}

# fp16 saturation (the largest finite value, the first value that rounds past it, far beyond it), fp16-subnormal
# magnitudes (below 2^-14: the smallest subnormal, half of it -- a tie to zero --, an odd multiple, the largest), zeros
EDGES = [65504.0, -65504.0, 65520.0, -65520.0, 1e5, -1e5, 2.0 ** -24, -2.0 ** -24, 2.0 ** -25, 3 * 2.0 ** -25,
         1023 * 2.0 ** -24, -1e-6, 3.1e-5, 0.0, -0.0, 1.0]


# ================================================================================================ bit-exact outputs
def plane_bits(v, prec):
    """dsn_split of float32 v -> raw int16 [P][n]: hi = fmt(sat(v)), lo = fmt(sat(v - hi)); fp16 saturates at +-65504"""
    f16 = IS_F16[prec]
    dt = torch.float16 if f16 else torch.bfloat16
    sat = (lambda t: t.clamp(-65504.0, 65504.0)) if f16 else (lambda t: t)
    v = v.float().reshape(-1)
    hi = sat(v).to(dt)
    out = [hi.view(torch.int16)]
    if PLANES[prec] == 2:
        out.append(sat(v - hi.float()).to(dt).view(torch.int16))
    return torch.stack(out)


def decode_bits(raw, prec):
    """raw int16 [P][n] -> the float64 value the planes hold"""
    dt = torch.float16 if IS_F16[prec] else torch.bfloat16
    return sum(raw[p].contiguous().view(dt).double() for p in range(raw.shape[0]))


def check_bits(got, want, what):
    """integer tensors of raw bits (planes, fp8 bytes, scale bytes, float32 viewed as int32): every element equal"""
    assert got.shape == want.shape, f"{what}: shape {tuple(got.shape)}, expected {tuple(want.shape)}"
    bad = got != want
    nbad = int(bad.sum())
    print(f"{what}: {nbad} of {got.numel()} elements differ in their bits")
    if nbad:
        i = int(bad.reshape(-1).nonzero()[0])
        raise AssertionError(f"{what}: {nbad} of {got.numel()} elements differ in their bits, first at flat index {i}: "
                             f"got {int(got.reshape(-1)[i]) & 0xffffffff:#x}, expected {int(want.reshape(-1)[i]) & 0xffffffff:#x}")
    return 0.0


def f32_bits(t):
    return t.detach().cpu().float().contiguous().view(torch.int32)


def check_f32_exact(got, want, what):
    return check_bits(f32_bits(got), f32_bits(want), what)


def weight(g, *shape, zero_row=True):
    """float32 test weight: N(0, 1) with EDGES planted at the front, spread over the tensor's tail and a row of zeros"""
    w = torch.randn(shape, generator=g, dtype=torch.float32)
    flat = w.reshape(-1)
    n = flat.numel()
    e = torch.tensor(EDGES, dtype=torch.float32)
    if n >= 2 * e.numel():
        flat[:e.numel()] = e
        flat[n - e.numel():] = e.flip(0)
    else:
        flat[:] = e[torch.arange(n) % e.numel()]
    if zero_row and shape[0] > 2:
        w[shape[0] // 2] = 0.0
    return w


def swiglu_rows(W, group=16):
    """[N][..] value rows then gate rows -> groups of `group` value rows followed by their `group` gate rows"""
    N = W.shape[0]
    F_ = N // 2
    rest = W.shape[1:]
    return torch.stack([W[:F_].reshape(-1, group, *rest), W[F_:].reshape(-1, group, *rest)], 1).reshape(N, *rest)


def pack_weight_ref(mode, src, scale=None, colscale=None, N=None, cin_pad=None, mut=None):
    """float32 [N][K] that launch_pack_weight rounds into planes.  src as the checkpoint stores it: linear [N][K];
    conv [Cout][Cin][kw]; convt [Cin][Cout][2 s]; conv2d [Cout][Cin][taps] (N >= Cout rows, cin_pad >= Cin); nin [K][N]"""
    src = src.float()
    if mode in ("linear", "linear_swiglu"):
        W = src
        if colscale is not None:
            if mut == "colscale_by_row":
                W = W * colscale.float()[torch.arange(W.shape[0]) % colscale.numel()][:, None]
            else:
                W = W * colscale.float()[None, :]
        if mode == "linear_swiglu":
            W = swiglu_rows(W, 32 if mut == "swiglu_groups_of_32" else 16)
        return W
    if mode == "conv":
        Cout, Cin, kw = src.shape
        v = src if scale is None else src * scale.float()[:, None, None]
        if mut == "conv_tap_channel_swapped":
            return v.reshape(Cout, Cin * kw)
        return v.permute(0, 2, 1).reshape(Cout, kw * Cin)
    if mode == "convt":
        Cin, Cout, kw = src.shape
        s = kw // 2
        v = src if scale is None else src * scale.float()[:, None, None]
        if mut == "convt_phase_major_taps":                       # kernel index read as p * 2 + tap
            return v.reshape(Cin, Cout, s, 2).permute(2, 1, 3, 0).reshape(s * Cout, 2 * Cin)
        t = v.reshape(Cin, Cout, 2, s).permute(3, 1, 2, 0)
        if mut == "convt_phases_reversed":
            t = t.flip(0)
        return t.reshape(s * Cout, 2 * Cin)
    if mode == "conv2d":
        Cout, Cin, taps = src.shape
        out = torch.zeros(N, taps, cin_pad, dtype=torch.float32)
        if mut == "padding_negative_zero":
            out = -out
        out[:Cout, :, :Cin] = src.permute(0, 2, 1)
        return out.reshape(N, taps * cin_pad)
    if mode == "nin":
        return src.t().contiguous()
    raise ValueError(mode)


def pack_tokens_ref(s0, s1):
    """[B][C0][T] (+ [B][C1][T]) -> [B T][C0 + C1]"""
    x = s0 if s1 is None else torch.cat([s0, s1], 1)
    return x.permute(0, 2, 1).reshape(-1, x.shape[1])


def unpack_tokens_ref(x, B, C, T):
    return x.reshape(B, T, C).permute(0, 2, 1).contiguous()


def zero_tail_ref(x, lens, mut=None):
    """x [B,n,D,T]: frames t >= lens[b] - 1 become +0 (lens counts the timestep token), the rest is untouched"""
    T = x.shape[-1]
    cut = torch.as_tensor(lens).view(-1, 1, 1, 1) - (0 if mut == "cut_at_lens" else 1)
    return torch.where(torch.arange(T).view(1, 1, 1, T) >= cut, torch.zeros_like(x), x)


def ncsn_pack_ref(xt, mix, Wp, Cp):
    """xt [B,n,H,T], mix [B,1,H,T] -> [B][H][Wp][Cp] channels-last, +0 in the channel and frame padding"""
    B, n, H, T = xt.shape
    out = torch.zeros(B, H, Wp, Cp, dtype=torch.float32)
    out[:, :, :T, :n + 1] = torch.cat([xt, mix], 1).permute(0, 2, 3, 1)
    return out


# ================================================================================================ MX fp8
def mx_pack_ref(x, mut=None):
    """float32 [N][K] (row map and colscale already applied) -> (e4m3 bytes uint8 [N][K], E8M0 bytes uint8 [N][K/32])"""
    N, K = x.shape
    xb = x.float().reshape(-1, 32)
    k = mx_exponent(x)
    if mut == "e8m0_plus_1":
        k = (k + 1).clamp(max=126)
    y = (xb * torch.exp2(-k.float())[:, None]).clamp(-448.0, 448.0)
    if mut == "e4m3_truncated":
        a = y.abs().double()
        step = torch.exp2(torch.floor(torch.log2(a.clamp(min=2.0 ** -6))) - 3)
        y = (torch.sign(y).double() * torch.floor(a / step) * step).float()
    b = y.to(torch.float8_e4m3fn).view(torch.uint8)
    return b.reshape(N, K), (k + 127).to(torch.uint8).reshape(N, K // 32)


def mx_decode(b8, s8):
    """bytes [N][K], scale bytes [N][K/32] -> float64 [N][K]"""
    N, K = b8.shape
    sc = torch.exp2(s8.to(torch.int32).double() - 127).reshape(-1, 1)
    return (b8.contiguous().view(torch.float8_e4m3fn).double().reshape(-1, 32) * sc).reshape(N, K)


def e4m3_half_step(y):
    """half the e4m3 spacing at |y| <= 448 (subnormal spacing 2^-9 below 2^-6)"""
    a = y.abs().clamp(min=2.0 ** -6, max=448.0)
    return 0.5 * torch.exp2(torch.floor(torch.log2(a)) - 3)


def check_fp8_properties(x, b8, s8, what):
    """float64 properties of an MX packing of x [N][K] (the float32 values that were quantised), no element excused:
    2^k >= (amax / 448)(1 - 2^-22); 2^(k-1) < (amax / 448)(1 + 2^-22) unless k = -126; every dequantised value within
    half an e4m3 step of the exact value clamped to +-448.  -> worst rounding error over half a step"""
    xb = x.double().reshape(-1, 32)
    k = s8.reshape(-1).to(torch.int32).double() - 127
    amax = xb.abs().amax(1)
    sc = torch.exp2(k)
    small = sc < (amax / 448.0) * (1 - 2.0 ** -22)
    assert not small.any(), f"{what}: {int(small.sum())} block scales too small for their amax (values would clip)"
    big = (torch.exp2(k - 1) >= (amax / 448.0) * (1 + 2.0 ** -22)) & (k > -126)
    assert not big.any(), f"{what}: {int(big.sum())} block scales at least one exponent too large (a bit is lost)"
    y = (xb / sc[:, None]).clamp(-448.0, 448.0)
    got = b8.contiguous().view(torch.float8_e4m3fn).double().reshape(-1, 32)
    assert torch.isfinite(got).all(), f"{what}: non-finite e4m3 bytes"
    ratio = (got - y).abs() / e4m3_half_step(y)
    worst = float(ratio.max())
    print(f"{what}: worst e4m3 error / half a step {worst:.5f} ({xb.shape[0]} blocks)")
    assert worst <= 1.0, f"{what}: {int((ratio > 1).sum())} values beyond half an e4m3 step (worst {worst:.3f})"
    return worst


def fp8_edge_blocks():
    """the blocks of 32 every fp8 case plants (float32 [9][32]), in this order: all zeros; amax exactly 448 * 2^3; one
    float32 ulp above; one below; a negative maximum; one large value among values that land in e4m3's subnormals and
    on zero; round-to-even ties (1.0625 -> 1, 1.1875 -> 1.25, at block scale 2^0 and 2^-2); amax below 448 * 2^-126"""
    g = torch.Generator().manual_seed(77)
    small = lambda: (torch.rand(32, generator=g) * 2 - 1).float()
    top = torch.tensor(448.0 * 8, dtype=torch.float32)
    blocks = [torch.zeros(32)]
    for amax in (top, torch.nextafter(top, top * 2), torch.nextafter(top, top * 0)):
        b = small() * 100
        b[5] = amax
        blocks.append(b)
    b = small() * 10
    b[31] = -448.0 * 2.0 ** -5 * 1.3
    blocks.append(b)
    b = torch.zeros(32)                       # amax 1000 -> k = 2: y = x / 4
    b[0] = 1000.0
    b[1:9] = 4 * torch.tensor([2.0 ** -7, 3 * 2.0 ** -9, 2.0 ** -9, 2.0 ** -10, 0.6 * 2.0 ** -9, 2.0 ** -11, -2.0 ** -10,
                               -1.5 * 2.0 ** -9])
    blocks.append(b)
    b = torch.zeros(32)
    b[0] = 448.0
    b[1:5] = torch.tensor([1.0625, 1.1875, -1.0625, -1.1875])
    b[5:9] = torch.tensor([1.0625, 1.1875, -1.0625, -1.1875]) * 16
    blocks.append(b)
    b = torch.zeros(32)
    b[0] = 448.0 * 0.25
    b[1:5] = torch.tensor([1.0625, 1.1875, -1.0625, -1.1875]) * 0.25
    blocks.append(b)
    b = small() * 2.0 ** -121
    b[7] = 1.5 * 2.0 ** -120
    blocks.append(b)
    return torch.stack(blocks).float()


def fp8_source(N, K, seed):
    """float32 [N][K]: blocks of N(0, 1) times 2^e, e uniform in [-30, 30], the edge blocks planted first where there is room"""
    g = torch.Generator().manual_seed(seed)
    nb = N * K // 32
    x = torch.randn(nb, 32, generator=g) * torch.exp2(torch.randint(-30, 31, (nb, 1), generator=g).float())
    e = fp8_edge_blocks()
    if nb >= e.shape[0]:
        x[:e.shape[0]] = e
    return x.float().reshape(N, K)


# ================================================================================================ bounded formulas
def np64(t):
    return t.detach().cpu().double().numpy() if isinstance(t, torch.Tensor) else np.asarray(t, np.float64)


def wn_scale(v, g):
    """scale = g / sqrt(sum v^2) over a row of `inner` values.  A lane squares and adds ceil(inner / 64) values (one
    rounding per square, one per add but the first), the wave tree adds 6 times: ceil(inner / 64) + 6 roundings on a
    sum of non-negative terms, so the same relative error; the square root halves it (kept un-halved) and rounds once,
    the divide once: R = ceil(inner / 64) + 8, relative to the result."""
    v, g = np64(v), np64(g)
    want = g / np.sqrt((v * v).sum(1))
    return want, np.abs(want), -(-v.shape[1] // 64) + 8


def packed_row_sum(hi, lo):
    """hi, lo: float64 [N][K] decoded planes (lo None with one plane); the decoded values are exact in float32.  One
    plane: ceil(K / 64) additions per lane, the first onto an exact zero, and 6 of the wave tree: R = ceil(K / 64) + 5.
    Two planes add hi and lo separately, 2 ceil(K / 64) additions; the bound keeps the ceiling
    ceiling R + 1 = ceil(K / 64) + 8 there (a lo term is below 2^-8 of its hi, so the rounding of the sum it joins
    is the rounding its hi term already paid for, to first order)."""
    hi = np64(hi)
    m = -(-hi.shape[1] // 64)
    if lo is None:
        return hi.sum(1), np.abs(hi).sum(1), m + 5
    lo = np64(lo)
    return (hi + lo).sum(1), (np.abs(hi) + np.abs(lo)).sum(1), m + 7


def fp8_row_sum(deq):
    """deq: float64 [N][K] dequantised MX weight.  A lane takes ceil(K / 256) dwords; the four e4m3 values of a dword
    sum exactly in float32 (4 significant bits each, 20 bits apart at most) and the power-of-two scale is exact, so a
    lane rounds ceil(K / 256) - 1 times and the tree 6: R = ceil(K / 256) + 5."""
    deq = np64(deq)
    return deq.sum(1), np.abs(deq).sum(1), -(-deq.shape[1] // 256) + 5


def bias_plus_wbeta(W, beta, bias):
    """out = bias + sum_k W[n][k] beta[k]: a product (1), ceil(K / 64) - 1 lane additions, 6 of the tree, the bias:
    R = ceil(K / 64) + 7"""
    W, beta = np64(W), np64(beta)
    p = W * beta[None, :]
    b = 0.0 if bias is None else np64(bias)
    return p.sum(1) + b, np.abs(p).sum(1) + np.abs(b), -(-W.shape[1] // 64) + 7


SNAKE_EPS = f32(1e-9)


def snake_params(alpha, beta, exp_units=2):
    """a = expf(alpha): the function's error alone, R = exp_units.  ib = 1 / (expf(beta) + 1e-9f): expf, the sum and the
    divide, R = exp_units + 2; every term is positive, so both bounds are relative to the result."""
    alpha, beta = np64(alpha), np64(beta)
    a = np.exp(alpha)
    ib = 1.0 / (np.exp(beta) + SNAKE_EPS)
    return {"a": (a, a, exp_units), "ib": (ib, ib, exp_units + 2)}


def ncsn_output(pyr, t, w, bias, cin, n, T):
    """pyr [B][H][Wp][Cp], t [B], w [n][cin], bias [n] -> score [B T][n H]: acc = bias; acc += w (p (1 / t)) for cin
    channels.  1 / t, p times it, the product with w, then cin additions: R = cin + 3"""
    pyr, t, w, bias = np64(pyr), np64(t), np64(w), np64(bias)
    p = pyr[:, :, :T, :cin] / t[:, None, None, None]                          # [B][H][T][cin]
    want = np.einsum("bhtc,sc->btsh", p, w) + bias[None, None, :, None]
    A = np.einsum("bhtc,sc->btsh", np.abs(p), np.abs(w)) + np.abs(bias)[None, None, :, None]
    B = pyr.shape[0]
    return want.reshape(B * T, -1), A.reshape(B * T, -1), cin + 3


# ---- sinf / cosf / logf / powf: no accuracy table of the device's math library ships with the toolchain, so the function
# term is measured on the reference alone: the same float32 call in numpy against float64 at the float32 argument, in
# units of 2^-24 (absolute for sin / cos, whose values are at most 1; relative for log and pow), times 4, at least 2.
PI32 = f32(math.pi)


def function_units(fn32, fn64, arg32, relative):
    """4 x the worst error of the host's float32 `fn32` at the float32 arguments, in units of 2^-24, at least 2"""
    a = np.asarray(arg32, np.float32)
    got, want = fn32(a).astype(np.float64), fn64(a.astype(np.float64))
    err = np.abs(got - want)
    if relative:
        with np.errstate(divide="ignore", invalid="ignore"):
            err = np.where(want == 0, 0.0, err / np.abs(want))
    return max(2.0, 4.0 * float(err.max()) / U)


def sincos_units(phase32):
    return max(function_units(np.sin, np.sin, phase32, False), function_units(np.cos, np.cos, phase32, False))


def timestep_features(t, w):
    """[cos(f), sin(f)], f = (2 pi_f) t w: pi_f is pi rounded to float32 (half a unit, counted as one), two products:
    R_arg = 3 on |f|; plus the function term.  -> want [B][2 half], absolute bound [B][2 half], function units"""
    t, w = np64(t), np64(w)
    f = 2 * math.pi * t[:, None] * w[None, :]
    f32_ = (np.float32(2) * np.float32(PI32) * t.astype(np.float32)[:, None]) * w.astype(np.float32)[None, :]
    fu = sincos_units(f32_)
    bound = (3 + 1) * U * np.abs(f) + fu * U
    return np.concatenate([np.cos(f), np.sin(f)], 1), np.concatenate([bound, bound], 1), fu


def ncsn_fourier(t, w):
    """[sin(p), cos(p)], p = ((logf(t) w) 2) pi_f: logf (its function term, relative, rides on the phase), the product
    with w, the exact doubling, the product with pi_f and pi_f's own rounding: R_arg = log units + 3"""
    t, w = np64(t), np64(w)
    p = np.log(t)[:, None] * w[None, :] * 2 * math.pi
    t32 = t.astype(np.float32)
    lu = function_units(np.log, np.log, t32, True)
    p32 = np.log(t32)[:, None] * w.astype(np.float32)[None, :] * np.float32(2) * np.float32(PI32)
    fu = sincos_units(p32)
    bound = (lu + 3 + 1) * U * np.abs(p) + fu * U
    return np.concatenate([np.sin(p), np.cos(p)], 1), np.concatenate([bound, bound], 1), (lu, fu)


def rope_tables(S, rot):
    """cos / sin [S][rot] of f = p inv, inv = 1 / powf(10000, 2k / rot), k = d mod rot/2.  rot is a power of two, so the
    exponent is exact; powf (function term, relative), the reciprocal, the product with the exact position:
    R_arg = pow units + 2"""
    assert rot & (rot - 1) == 0, "the bound takes the exponent 2k / rot as exact"
    k = np.arange(rot) % (rot // 2)
    e = 2.0 * k / rot
    inv = 1.0 / np.power(10000.0, e)
    f = np.arange(S, dtype=np.float64)[:, None] * inv[None, :]
    e32 = e.astype(np.float32)
    pu = function_units(lambda a: np.power(np.float32(10000), a), lambda a: np.power(10000.0, a), e32, True)
    f32_ = np.arange(S, dtype=np.float32)[:, None] * (np.float32(1) / np.power(np.float32(10000), e32))[None, :]
    fu = sincos_units(f32_)
    bound = (pu + 2 + 1) * U * np.abs(f) + fu * U
    return np.cos(f), np.sin(f), bound, (pu, fu)


def check_abs(got, want, bound, what):
    """|got - want| <= bound per element (bound > 0); -> worst error over its bound"""
    got, want, bound = np64(got).reshape(-1), np64(want).reshape(-1), np64(bound).reshape(-1)
    assert got.shape == want.shape, f"{what}: {got.shape} values, {want.shape} expected"
    assert np.isfinite(got).all(), f"{what}: {int((~np.isfinite(got)).sum())} values are not finite (or were not written)"
    ratio = np.abs(got - want) / bound
    worst = float(ratio.max())
    print(f"{what}: worst error / bound {worst:.3f} ({got.size} values)")
    assert worst <= 1.0, f"{what}: {int((ratio > 1).sum())} of {got.size} values beyond the bound, worst {worst:.3g} x " \
                         f"at flat index {int(ratio.argmax())}"
    return worst


def check_planes_abs(raw, want, bound, prec, what):
    """raw int16 [P][n] planes of a float32 value within `bound` of want: the decoded planes lie within one unit of the
    operand format (fp16: of its subnormal spacing) plus the bound of emulate_split(float32(want)), as check_planes"""
    want = torch.from_numpy(np64(want).reshape(-1))
    ref = emulate_split(want.float(), prec)
    P, f16 = PLANES[prec], IS_F16[prec]
    unit = 2.0 ** -(MANT[f16] * P + (P - 1))
    tiny = 2.0 ** -14 if f16 else 2.0 ** -126
    full = unit * torch.maximum(ref.abs(), torch.full_like(ref, tiny)) + torch.from_numpy(np64(bound).reshape(-1))
    return check_abs(decode_bits(raw, prec), ref, full, what)
