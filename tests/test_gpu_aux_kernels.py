"""The hot-path kernels outside the implicit-GEMM family, one launch wrapper at a time, against float64 math of the same
operation: attention (attention.hip), fused to_qkv + rotary + attention (qkv_attn.hip), residual + LayerNorm and the
Oobleck edge convolutions (kernels.hip), GroupNorm statistics / apply and FIR resampling (ncsn_kernels.hip).

dsn_test_kernel passes the caller's arguments to the launch wrapper; which kernel runs is the wrapper's own dispatch,
and every case id names the branch its shape lands on (the `*_branch` functions restate the dispatch for the id only).
Every output buffer carries a sentinel -- NaN (fp32), 0x7fff (planes), 0xA5 (fp8 bytes and scale bytes) -- and every
case asserts that what the operation does not own is untouched.

Bounds.  unit = 2^-(MANT P + P - 1) is one unit of the operand format (tests/test_gpu_gemm_kernels.py::check_planes),
u = unit / 2 its unit roundoff.  A "floor" is the reference's own float32 error: the same formula evaluated in
float32 torch, its worst distance from float64 over the case, times 4 for accumulation order.
  attention   per (item, head) rel-L2 < TOL; per element |got - want| <= 4 u max|V| + floor (P rounded once, the
              output rounded once, the normaliser not rounded: 3 u max|V|)
  fused qkv   rel-L2 < TOL against float64 with q | k | v, P and the output rounded as the kernel rounds them
  LayerNorm, GroupNorm apply, conv-in1 planes    one unit + floor
  fp8 (MX)    every value within half an e4m3 step at the device's scale + floor; the scale byte equals
              tests/util.py::mx_exponent of the float64 values unless the block's amax lies within the floor of a step
              of the exponent (at most 1 % of the blocks, asserted on the reference alone)
  gn-stats    1e-5 (test_groupnorm_partials' bound)
  fir2d       (terms + 1) 2^-24 (sum |w| |x| + |add|): the weights and their products are exact binary fractions,
              so each of the <= 16 products and each of the sums rounds at most once
  conv-out1 / conv-in1 fp32                      floor

Figures of the reference alone (seed = the case's own, SEED0 + index; measured on the CPU):
  float32 floors (4 x worst |f32 - f64|): attention up to 5.5e-6, Gaussian and peaked alike (0 at S = 1, where the
    output is V itself); fused qkv out8 (its emulated roundings flip between float32 and float64) 2.3e-3 fp16, 1.2e-2 bf16;
    LayerNorm up to 5.1e-6, 1.5e-5 .. 9.5e-5 with the offset of 100; gn-apply 1e-6 .. 4.9e-5; conv-out1 up to 9.2e-6;
    conv-in1 3e-7 .. 4.5e-5
  peaked inputs: the reference weight of key S - 1 lies in [0.3, 0.7] for 100 % of the queries of every shape with
    S >= 2 (it is solved to 1/2 before the operands are rounded; S = 1 has one key, whose weight is 1)
  fp8 boundary blocks: 0 .. 0.05 % (attention), 0 .. 0.1 % (LayerNorm), 0.17 % / 0.51 % (fused qkv, fp16 / bf16)
"""
import math

import pytest
import torch
import torch.nn.functional as F

from tests.test_gpu_gemm_kernels import (BF16, DEV, FP16, FP16X3, IS_F16, MANT, PLANES, SENT16, TAIL, TOL, X3, act64, dev,
                                         emulate_split, nan_f32, nan_planes, randn)
from tests.util import make_engine, mx_exponent, rel_l2

pytestmark = pytest.mark.gpu

NAME = {BF16: "bf16", FP16: "fp16", X3: "bf16x3", FP16X3: "fp16x3"}
ALL = (BF16, FP16, X3, FP16X3)
SENT8 = 0xA5
SEED0 = 1234


@pytest.fixture(scope="module")
def eng():
    engs = {p: make_engine(precision=p) for p in ALL}
    yield engs
    for e in engs.values():
        e.close()


def unit_of(prec):
    P = PLANES[prec]
    return 2.0 ** -(MANT[IS_F16[prec]] * P + (P - 1))


def operands(v, prec):
    """float64 values -> (what the caller hands over in fp32, the float64 value the operand planes then hold)"""
    f = v.float()
    if PLANES[prec] == 1:
        f = emulate_split(f, prec).float()
    return f, emulate_split(f, prec)


def f32_floor(fn):
    """4 x the worst distance of the float32 evaluation of `fn(dtype)` from its float64 evaluation"""
    return 4.0 * float((fn(torch.float32).double() - fn(torch.float64)).abs().max())


def nan_bytes(n):
    return torch.full((n + TAIL,), SENT8, device=DEV, dtype=torch.uint8)


def read_planes(e, pl, n, what):
    """decoded float64 values of the first n elements; the tail of every plane must still hold the sentinel"""
    raw = pl.cpu()
    assert (raw[:, n:] == SENT16).all(), f"{what}: planes written past the output"
    got = e.decode_planes(pl).cpu()[:n]
    assert torch.isfinite(got).all(), f"{what}: non-finite (or unwritten) plane values"
    return got


def read_f32(buf, n, what):
    b = buf.cpu().double()
    assert torch.isnan(b[n:]).all(), f"{what}: fp32 output written past its end"
    assert torch.isfinite(b[:n]).all(), f"{what}: non-finite (or unwritten) fp32 output"
    return b[:n]


def check_unit(got, want, prec, floor, what):
    """decoded planes within one unit of the operand format (fp16: of its subnormal spacing) plus floor"""
    tiny = 2.0 ** -14 if IS_F16[prec] else 2.0 ** -126
    bound = unit_of(prec) * torch.maximum(want.abs(), torch.full_like(want, tiny)) + floor
    err = (got - want).abs()
    print(f"{what}: worst plane error {float(err.max()):.3e}, floor {floor:.3e}")
    assert not (err > bound).any(), f"{what}: {int((err > bound).sum())} plane values beyond one unit + floor " \
                                    f"(worst {float((err / bound).max()):.2f} x the bound)"


def e4m3_half_step(y):
    """half the e4m3 spacing at |y| (y already divided by the block scale)"""
    a = y.abs().clamp(min=2.0 ** -6, max=448.0)
    return 0.5 * torch.exp2(torch.floor(torch.log2(a)) - 3)


def mx_boundary(want, floor):
    """(exponent per block of the float64 values, blocks whose amax +- floor straddles a step of the exponent)"""
    w = want.reshape(-1, 32)
    amax = w.abs().amax(1, keepdim=True)
    one = torch.ones(1, 32, dtype=torch.float64)
    k = mx_exponent(w)
    lo, hi = mx_exponent((amax - floor).clamp(min=0) * one), mx_exponent((amax + floor) * one)
    return k, lo != hi


def check_fp8(b8, s8, want, floor, what):
    """b8 / s8: the device's e4m3 bytes and E8M0 scale bytes (with tails); want float64 [rows][D]"""
    n = want.numel()
    b8, s8 = b8.cpu(), s8.cpu()
    assert (b8[n:] == SENT8).all() and (s8[n // 32:] == SENT8).all(), f"{what}: fp8 output written past its end"
    k, edge = mx_boundary(want, floor)
    share = float(edge.double().mean())
    print(f"{what}: fp8 boundary blocks {100 * share:.2f} %, floor {floor:.3e}")
    assert share <= 0.01, f"{what}: {100 * share:.2f} % of the blocks lie on a scale boundary (reference alone)"
    kd = s8[:n // 32].to(torch.int32) - 127
    bad = (kd != k) & ~edge
    assert not bad.any(), f"{what}: {int(bad.sum())} scale bytes differ from mx_exponent"
    assert ((kd - k).abs() <= 1).all(), f"{what}: a boundary block's scale is more than one step off"
    sc = torch.exp2(kd.double())[:, None]
    got = b8[:n].view(torch.float8_e4m3fn).double().reshape(-1, 32) * sc
    w = want.reshape(-1, 32)
    bound = e4m3_half_step(w / sc) * sc + floor
    err = (got - w).abs()
    assert not (err > bound).any(), f"{what}: {int((err > bound).sum())} fp8 values beyond half a step + floor " \
                                    f"(worst {float((err / bound).max()):.2f} x the bound)"


# ================================================================================================ attention
def attention_branch(P, dh, S):
    """the branch of attention.hip::launch_t the shape lands on (for the case id)"""
    nkt = (S + 15) // 16
    if nkt > 16:
        return "long"
    if P * nkt * 16 * dh * 2 > 160 * 1024:
        return "long_lds"                      # whole-sequence V beyond the 160 KB of LDS
    if nkt <= 4:
        return "nkt4_prefetch" if dh == 64 else "nkt4"
    return "nkt16_W%d" % (8 if nkt >= 8 else 4) + ("_odd" if nkt % 2 else "")


S_ALL = [1, 15, 16, 17, 33, 49, 64, 65, 97, 113, 128, 161, 236, 241, 256, 257, 300, 384, 385]
ATT_CASES = [(p, 64, S) for p in ALL for S in S_ALL]
ATT_CASES += [(p, 128, S) for p in (FP16, X3) for S in (17, 64, 113, 161, 256, 257, 385)]
ATT_CASES += [(p, 256, S) for p in (BF16, FP16X3) for S in (17, 64, 113, 161, 256, 257, 385)]
ATT_CASES += [(X3, 256, S) for S in (161, 256)]


def att_id(c):
    p, dh, S = c
    return f"{NAME[p]}-dh{dh}-S{S}-{attention_branch(PLANES[p], dh, S)}"


def attention_inputs(prec, B, H, dh, S, peaked, seed):
    """q (pre-scaled by 1/sqrt(dh)), k, v [B, H, S, dh] float64 before rounding.  peaked: key S - 1 takes half of every
    query's mass and key 0 a quarter (features 0 / 1 carry the two peaks, the other keys are zero there), so key 0 of
    the next item -- what a kernel reads one row past the end -- weighs as much as a quarter of the whole row."""
    g = torch.Generator().manual_seed(seed)
    q = randn(g, B, H, S, dh) / math.sqrt(dh)
    k, v = randn(g, B, H, S, dh), randn(g, B, H, S, dh)
    if peaked:
        lam = 4.0
        q[..., :2] = 0
        k[..., :2] = 0
        mid = torch.exp(q @ k.transpose(-1, -2))[..., 1:S - 1].sum(-1).clamp(min=1.0) if S > 2 else torch.ones(B, H, S)
        k[:, :, S - 1, :] = 0
        k[:, :, S - 1, 0] = lam
        q[..., 0] = torch.log(2 * mid) / lam
        if S > 1:
            k[:, :, 0, :] = 0
            k[:, :, 0, 1] = lam
            q[..., 1] = torch.log(mid) / lam
    return q, k, v


def attention_ref(q, k, v, dt=torch.float64):
    w = torch.softmax(q.to(dt) @ k.to(dt).transpose(-1, -2), -1)
    return w @ v.to(dt), w


def pack_qkv(q, k, v):
    """[B, H, S, dh] x 3 -> token-major [B*S][3*H*dh], q | k | v sections, head-major inside a section"""
    B, H, S, dh = q.shape
    return torch.cat([t.permute(0, 2, 1, 3).reshape(B * S, H * dh) for t in (q, k, v)], 1).contiguous()


def attention_case(prec, dh, S, peaked, seed):
    """-> fp32 operand tensor, float64 reference [B*S][D], floor, max|V|"""
    B, H = (2, 2) if dh == 64 else (2, 1)
    q, k, v = attention_inputs(prec, B, H, dh, S, peaked, seed)
    (qf, q), (kf, k), (vf, v) = (operands(t, prec) for t in (q, k, v))
    ref, w = attention_ref(q, k, v)
    if peaked and S >= 2:
        ok = ((w[..., S - 1] >= 0.3) & (w[..., S - 1] <= 0.7)).double().mean()
        assert ok >= 0.9, f"peaked inputs: key S-1 holds [0.3, 0.7] of the mass for only {100 * float(ok):.0f} % of queries"
    floor = f32_floor(lambda dt: attention_ref(q, k, v, dt)[0])
    return pack_qkv(qf, kf, vf), ref, floor, float(v.abs().max()), (B, H)


@pytest.mark.parametrize("case", ATT_CASES, ids=att_id)
def test_attention(eng, case):
    prec, dh, S = case
    e = eng[prec]
    for peaked in (False, True):
        a, ref, floor, vmax, (B, H) = attention_case(prec, dh, S, peaked, SEED0 + S + dh)
        D = H * dh
        n = B * S * D
        pl = nan_planes(PLANES[prec], n)
        e.test_kernel("attention", a=dev(a), B=B, S=S, H=H, dh=dh, out_planes=pl)
        torch.cuda.synchronize()
        what = f"attention {att_id(case)} {'peaked' if peaked else 'gaussian'}"
        got = read_planes(e, pl, n, what).reshape(B, S, H, dh).permute(0, 2, 1, 3)
        err = (got - ref).abs()
        bound = 4 * (unit_of(prec) / 2) * vmax + floor
        worst_l2 = max(rel_l2(got[b, h], ref[b, h]) for b in range(B) for h in range(H))
        print(f"{what}: worst rel-L2 {worst_l2:.3e}, worst element {float(err.max()):.3e} (bound {bound:.3e}, "
              f"floor {floor:.3e})")
        assert worst_l2 < TOL[prec], f"{what}: rel-L2 {worst_l2:.3e} >= {TOL[prec]:.1e}"
        assert float(err.max()) <= bound, f"{what}: element error {float(err.max()):.3e} > {bound:.3e}"


@pytest.mark.parametrize("S", [33, 236, 300], ids=lambda S: f"fp16x3-dh64-S{S}-{attention_branch(2, 64, S)}-fp8")
def test_attention_fp8_output(eng, S):
    prec, dh = FP16X3, 64                    # split operands: the value that is quantised is exact to the floor
    a, ref, floor, _, (B, H) = attention_case(prec, dh, S, False, SEED0 + S)
    n = B * S * H * dh
    b8, s8 = nan_bytes(n), nan_bytes(n // 32)
    eng[prec].test_kernel("attention", a=dev(a), B=B, S=S, H=H, dh=dh, out_fp8=b8, out_fp8_scale=s8)
    torch.cuda.synchronize()
    check_fp8(b8, s8, ref.permute(0, 2, 1, 3).reshape(B * S, H * dh), floor, f"attention fp8 S {S}")


def test_attention_refusals(eng):
    a = dev(torch.zeros(2 * 16 * 3 * 96))
    with pytest.raises(RuntimeError, match="unsupported head width 96"):
        eng[FP16].test_kernel("attention", a=a, B=2, S=16, H=1, dh=96, out_planes=nan_planes(1, 2 * 16 * 96))
    with pytest.raises(RuntimeError, match="attention: a_numel"):
        eng[FP16].test_kernel("attention", a=a, B=2, S=17, H=1, dh=64, out_planes=nan_planes(1, 2 * 17 * 64))


# ================================================================================================ fused qkv + attention
def qkv_branch(S, ipp):
    nqt = (S + 15) // 16
    if ipp * S <= 144:
        return "QA(3,%d,144)" % (3 if nqt <= 3 else 5 if nqt <= 5 else 9)
    return "QA(2,%d,240)" % (9 if nqt <= 9 else 15)


# (S, ipp, H, items, bias, out8): items leave the last panel short where ipp > 1; panels x H is no multiple of 8
QKV_CASES = [(33, 4, 3, 6, True, False), (65, 2, 4, 5, False, False), (130, 1, 2, 3, True, False),
             (100, 2, 4, 5, True, False), (236, 1, 3, 3, False, False), (33, 4, 4, 9, True, True)]


QKV_OUT8_SEED = 2004


def qkv_id(c):
    S, ipp, H, B, bias, out8 = c
    return f"S{S}-ipp{ipp}-H{H}-{qkv_branch(S, ipp)}" + ("-bias" if bias else "") + ("-out8" if out8 else "")


def rope64(S):
    inv = 1.0 / (10000.0 ** (torch.arange(0, 32, 2, dtype=torch.float64) / 32))
    f = torch.outer(torch.arange(S, dtype=torch.float64), inv)
    f = torch.cat([f, f], -1)
    return f.cos(), f.sin()


def qkv_ref(a, w, bias, B, S, H, prec, dt=torch.float64, rounded=True):
    """float64 to_qkv GEMM + bias, rotary on the first 32 features of q and k (oracle/dit.py::apply_rope), q / 8,
    softmax, P V.  rounded: q | k | v, P (the normaliser sums the unrounded P) and the output are rounded to the operand
    format as the kernel rounds them."""
    D = H * 64
    rnd = (lambda t: emulate_split(t, prec).to(dt)) if rounded else (lambda t: t)
    # (products formed in float64 and rounded to dt: the float32 evaluation, whose roundings to the operand format
    # flip against float64, is then the same on every host whatever its BLAS sums first)
    mm = lambda x, z: (x.double() @ z.double()).to(dt)
    y = mm(a.to(dt).reshape(B, S, D), w.to(dt).t())
    if bias is not None:
        y = y + bias.to(dt)
    q, k, v = (t.reshape(B, S, H, 64).transpose(1, 2) for t in y.chunk(3, -1))
    cos, sin = (t.to(dt) for t in rope64(S))

    def rope(t):
        tr = t[..., :32]
        rot = torch.cat([-tr[..., 16:], tr[..., :16]], -1)
        return torch.cat([tr * cos + rot * sin, t[..., 32:]], -1)
    q, k, v = rnd(rope(q) * 0.125), rnd(rope(k)), rnd(v)
    s = mm(q, k.transpose(-1, -2))
    p = torch.exp(s - s.amax(-1, keepdim=True))
    o = mm(rnd(p), v) / p.sum(-1, keepdim=True)
    return o.transpose(1, 2).reshape(B * S, D).double()


@pytest.mark.parametrize("prec", [FP16, BF16], ids=lambda p: NAME[p])
@pytest.mark.parametrize("case", QKV_CASES, ids=qkv_id)
def test_qkv_attention(eng, case, prec):
    """One case per instantiation of qkv_attention_launch.  QA(2,9,240) needs 144 < ipp S <= 240 with S <= 144, that is
    several items in a tall panel: the engine only ever packs several items into the 144-row tile (ipp <= 144 / S), so
    it reaches this instantiation only under its DSN_QA_IPP override; the case stays."""
    S, ipp, H, B, with_bias, out8 = case
    e = eng[prec]
    D = H * 64
    # out8: the seed among 2000 .. 2023 whose reference has the largest float32 floor (flips of the emulated roundings
    # are rare events: most seeds see none in bf16) while at most 0.51 % of its blocks lie on a scale boundary
    g = torch.Generator().manual_seed(QKV_OUT8_SEED if out8 else SEED0 + S + H)
    af, a = operands(randn(g, B * S, D), prec)
    wf, w = operands(randn(g, 3 * D, D, scale=D ** -0.5), prec)
    bias = randn(g, 3 * D).float() if with_bias else None
    ref = qkv_ref(a, w, None if bias is None else bias.double(), B, S, H, prec)
    exact = qkv_ref(a, w, None if bias is None else bias.double(), B, S, H, prec, rounded=False)
    n = B * S * D
    rc, rs = nan_f32(S * 32), nan_f32(S * 32)
    kw = dict(a=dev(af), w=dev(wf), bias=None if bias is None else dev(bias), B=B, S=S, H=H, D=D, ipp=ipp, rope_cos=rc,
              rope_sin=rs)
    what = f"qkv_attention {qkv_id(case)} {NAME[prec]}"
    if out8:
        # the emulated roundings flip between float32 and float64: the floor is this reference's own error
        bf = None if bias is None else bias.double()
        floor = f32_floor(lambda dt: qkv_ref(a, w, bf, B, S, H, prec, dt))
        b8, s8 = nan_bytes(n), nan_bytes(n // 32)
        e.test_kernel("qkv_attention", out_fp8=b8, out_fp8_scale=s8, **kw)
        torch.cuda.synchronize()
        check_fp8(b8, s8, ref, floor, what)
    else:
        pl = nan_planes(1, n)
        e.test_kernel("qkv_attention", out_planes=pl, **kw)
        torch.cuda.synchronize()
        got = read_planes(e, pl, n, what).reshape(B * S, D)
        err, far = rel_l2(got, ref), rel_l2(got, exact)
        print(f"{what}: rel-L2 {err:.3e} (from the unrounded float64 result {far:.3e})")
        assert err < TOL[prec], f"{what}: rel-L2 {err:.3e} >= {TOL[prec]:.1e} (from the unrounded float64 result {far:.3e})"
    cos, sin = rope64(S)
    for buf, t in ((rc, cos), (rs, sin)):
        tab = read_f32(buf, S * 32, what + " rotary table").reshape(S, 32)
        assert float((tab - t).abs().max()) < 1e-6 * S + 1e-6, what + ": rotary table"   # fp32 angle: ulp(S) ~ 6e-8 S


def test_qkv_attention_refusals(eng):
    def call(prec, S=33, ipp=1, H=2, D=128, B=2):
        P = PLANES[prec]
        eng[prec].test_kernel("qkv_attention", a=dev(torch.zeros(B * S * D)), w=dev(torch.zeros(3 * D * D)), B=B, S=S,
                              H=H, D=D, ipp=ipp, rope_cos=nan_f32(S * 32), rope_sin=nan_f32(S * 32),
                              out_planes=nan_planes(P, B * S * D))
    for prec in (X3, FP16X3):                                        # two-plane modes
        with pytest.raises(RuntimeError, match="qkv_attention: refused"):
            call(prec)
    with pytest.raises(RuntimeError, match="qkv_attention: refused"):   # D != 64 H
        call(FP16, H=3, D=256)
    with pytest.raises(RuntimeError, match="qkv_attention: refused"):   # ipp S > 240
        call(FP16, S=61, ipp=4, B=4)
    call(FP16, S=60, ipp=4, B=4)                                     # (and 240 rows exactly are accepted)


# ================================================================================================ residual + LayerNorm
def ln_branch(rows, D, nslab):
    if D == 1024 and rows > 256 and nslab <= 4:
        return f"row_NS{nslab}"
    if D <= 1024 and rows <= 256:
        return f"batch_NS{min(nslab, 8)}"
    return (f"wave_NS{min(nslab, 8)}" if D <= 1024 else f"maxv16_NS{min(nslab, 8)}")


# (rows, D, nslab, bias, do_norm, beta, offset): bias present / null, do_norm 0 / 1 and beta null on every form
LN_CASES = [(1, 128, 0, False, 1, True, False), (5, 512, 1, True, 1, False, True), (256, 1024, 4, True, 0, False, False),
            (3, 128, 2, False, 1, True, True),
            (257, 512, 2, True, 1, False, True), (257, 1024, 5, False, 1, True, False), (300, 512, 1, True, 0, False, False),
            (257, 1024, 0, False, 1, True, True), (300, 1024, 3, True, 1, False, False), (257, 1024, 4, False, 0, False, True),
            (258, 1024, 1, True, 1, True, False),
            (3, 1536, 8, True, 1, True, False), (2, 4096, 1, False, 1, False, True), (2, 2048, 2, True, 0, False, False)]


def ln_id(c):
    rows, D, nslab, bias, do_norm, beta, offset = c
    return f"r{rows}-D{D}-{ln_branch(rows, D, nslab)}" + ("-bias" if bias else "") + ("-norm" if do_norm else "-copy") + \
           ("-beta" if beta else "") + ("-off100" if offset else "")


def ln_formula(x, gamma, beta, do_norm, dt):
    x = x.to(dt)
    if not do_norm:
        return x
    mean = x.mean(-1, keepdim=True)
    var = ((x - mean) ** 2).mean(-1, keepdim=True)
    y = (x - mean) * torch.rsqrt(var + 1e-5) * gamma.to(dt)
    return y + beta.to(dt) if beta is not None else y


def ln_run(e, prec, case, seed, fp8=False, bias_at_nslab0=False):
    rows, D, nslab, with_bias, do_norm, with_beta, offset = case
    g = torch.Generator().manual_seed(seed)
    f32 = lambda t: t.float().double()         # the device reads fp32 tensors: the reference sees the same values
    x0 = f32(randn(g, rows, D) + (100.0 if offset else 0.0))
    slabs = f32(randn(g, max(nslab, 1), rows * D + 8))
    bias = f32(randn(g, D)) if (with_bias or bias_at_nslab0) else None
    gamma = f32(1 + 0.3 * randn(g, D)) if do_norm else None
    beta = f32(randn(g, D)) if (do_norm and with_beta) else None
    terms = [x0] + ([bias.expand(rows, D)] if bias is not None and nslab else []) + \
            [slabs[z, :rows * D].reshape(rows, D) for z in range(nslab)]
    total = sum(terms)
    n = rows * D
    xb = nan_f32(n)
    xb[:n] = dev(x0).reshape(-1)
    kw = dict(x=xb, slabs=dev(slabs) if nslab else None, nslab=nslab, slab_stride=rows * D + 8,
              bias=None if bias is None else dev(bias), gamma=None if gamma is None else dev(gamma),
              beta=None if beta is None else dev(beta), rows=rows, D=D, eps=1e-5, do_norm=do_norm)
    what = f"residual_norm {ln_id(case)} {NAME[prec]}" + (" fp8" if fp8 else "")
    if fp8:
        b8, s8 = nan_bytes(n), nan_bytes(n // 32)
        e.test_kernel("residual_norm", out_fp8=b8, out_fp8_scale=s8, **kw)
    else:
        pl = nan_planes(PLANES[prec], n)
        e.test_kernel("residual_norm", out_planes=pl, **kw)
    torch.cuda.synchronize()
    xr = read_f32(xb, n, what + " x").reshape(rows, D)
    if nslab == 0:
        assert torch.equal(xr, x0), f"{what}: x changed although no slab was added"
    else:       # one fp32 rounding per addition, each of a partial sum no larger than the sum of the magnitudes
        bound = (len(terms) + 1) * 2.0 ** -24 * sum(t.abs() for t in terms)
        assert not ((xr - total).abs() > bound).any(), f"{what}: x is not the fp32 sum of x, bias and the slabs"
    # the LayerNorm of the device's own fp32 sum would hide a wrong sum: the reference normalises the float64 sum
    want = ln_formula(total, gamma, beta, do_norm, torch.float64)
    floor = f32_floor(lambda dt: ln_formula(total, gamma, beta, do_norm, dt))
    if fp8:
        check_fp8(b8, s8, want, floor, what)
    else:
        check_unit(read_planes(e, pl, n, what).reshape(rows, D), want, prec, floor, what)


@pytest.mark.parametrize("prec", ALL, ids=lambda p: NAME[p])
@pytest.mark.parametrize("case", LN_CASES, ids=ln_id)
def test_residual_norm(eng, case, prec):
    ln_run(eng[prec], prec, case, SEED0 + LN_CASES.index(case))


LN_FP8 = [(5, 128, 1, True, 1, True, False), (256, 1024, 2, False, 1, False, False), (257, 128, 1, True, 1, True, False),
          (257, 1024, 5, True, 1, False, False), (257, 1024, 0, False, 1, True, False), (300, 1024, 2, True, 0, False, False)]


@pytest.mark.parametrize("case", LN_FP8, ids=lambda c: ln_id(c) + "-fp8")
def test_residual_norm_fp8_output(eng, case):
    ln_run(eng[FP16], FP16, case, SEED0 + 50 + LN_FP8.index(case), fp8=True)


@pytest.mark.parametrize("case", [(5, 512, 0, False, 1, True, False), (257, 512, 0, False, 1, False, False),
                                  (257, 1024, 0, False, 1, True, False), (2, 2048, 0, False, 0, False, False)], ids=ln_id)
def test_residual_norm_ignores_bias_without_slabs(eng, case):
    """`bias` is the bias of the GEMM whose split-K slabs are pending: the engine's call sites pass it together with
    the slabs and null otherwise, and with nslab = 0 every form leaves x (bit-identical) and normalises x alone, a
    non-null bias included.  ln_run's reference adds the bias only when nslab > 0."""
    ln_run(eng[X3], X3, case, SEED0 + 77, bias_at_nslab0=True)


def test_residual_norm_refusals(eng):
    x = nan_f32(4 * 130)
    with pytest.raises(RuntimeError, match="residual_norm: needs x"):
        eng[FP16].test_kernel("residual_norm", x=x, rows=4, D=130, out_planes=nan_planes(1, 4 * 130))
    with pytest.raises(RuntimeError, match="residual_norm: nslab 9"):
        eng[FP16].test_kernel("residual_norm", x=x, rows=4, D=128, nslab=9, slabs=x, out_planes=nan_planes(1, 4 * 128))


# ================================================================================================ GroupNorm
def gn_geom(C):
    G = min(C // 4, 32)
    return G, C // G


def gn_stats64(x, HW, C):
    """float64 (mean, M2) per 64-row slice and channel quad of x [B, HW, C] -> [B, S, C/4, 2]"""
    B, S = x.shape[0], (HW + 63) // 64
    out = torch.zeros(B, S, C // 4, 2, dtype=torch.float64)
    for s in range(S):
        blk = x[:, 64 * s:min(64 * s + 64, HW)].reshape(B, -1, C // 4, 4).permute(0, 2, 1, 3).reshape(B, C // 4, -1)
        m = blk.mean(-1)
        out[:, s, :, 0] = m
        out[:, s, :, 1] = ((blk - m[..., None]) ** 2).sum(-1)
    return out


def gn_view(g, B, HW, C, offset, sliced):
    """-> (device buffer, view of it to pass as x, float64 values [B, HW, C], bstride, rstride)"""
    rs, coff = (C + 24, 8) if sliced else (C, 0)
    full = (randn(g, B, HW, rs) * 1.5 + (30.0 if offset else 0.0)).float()
    buf = dev(full.reshape(-1)).reshape(B, HW, rs)
    return buf, buf[:, :, coff:], full.double()[:, :, coff:coff + C], HW * rs, rs


def run_gn_stats(e, view, B, HW, C, bstride, rstride, what):
    S = (HW + 63) // 64
    n = B * S * (C // 4) * 2
    st = nan_f32(n)
    e.test_kernel("gn_stats", x=view, bstride=bstride, rstride=rstride, C=C, B=B, HW=HW, out_f32=st)
    torch.cuda.synchronize()
    return st, read_f32(st, n, what).reshape(B, S, C // 4, 2)


@pytest.mark.parametrize("C", [4, 60, 64, 68, 256], ids=lambda C: f"C{C}-nq{C // 4}")
def test_gn_stats(eng, C):
    """nq = 15 / 17: the last 16-quad wave of a slice is ragged by one quad either way; HW = 63 / 65 / 130: ragged slices"""
    e, B = eng[FP16], 2
    g = torch.Generator().manual_seed(SEED0 + C)
    for i, HW in enumerate([1, 63, 64, 65, 130]):
        for sliced in ((False, True) if HW in (65, 130) else (False,)):
            offset = (i + C // 4) % 2 == 1
            buf, view, x, bs, rs = gn_view(g, B, HW, C, offset, sliced)
            what = f"gn_stats C {C} HW {HW} {'slice of a wider buffer' if sliced else 'dense'} offset {offset}"
            _, got = run_gn_stats(e, view, B, HW, C, bs, rs, what)
            want = gn_stats64(x, HW, C)
            sd = 1.5
            dm = float((got[..., 0] - want[..., 0]).abs().max())
            assert dm <= 1e-5 * 4 * sd + 1e-5 * float(want[..., 0].abs().max()), f"{what}: mean off by {dm:.3e}"
            # (a slice of one row holds 4 values: M2 stays well away from zero, relative error is meaningful)
            r2 = float(((got[..., 1] - want[..., 1]).abs() / want[..., 1]).max())
            assert r2 <= 8e-5, f"{what}: M2 off by {r2:.3e} (relative)"


def gn_apply_formula(x, C, gamma, beta, silu, dt):
    B, HW, _ = x.shape
    G, cpg = gn_geom(C)
    v = x.to(dt).reshape(B, HW, G, cpg)
    mean = v.mean((1, 3), keepdim=True)
    var = ((v - mean) ** 2).mean((1, 3), keepdim=True)
    y = ((v - mean) * torch.rsqrt(var + 1e-6)).reshape(B, HW, C) * gamma.to(dt) + beta.to(dt)
    return y * torch.sigmoid(y) if silu else y


@pytest.mark.parametrize("prec", [FP16, X3], ids=lambda p: NAME[p])
@pytest.mark.parametrize("C", [64, 256], ids=lambda C: f"C{C}-qpg{gn_geom(C)[1] // 4}")
def test_gn_apply(eng, C, prec):
    e, B = eng[prec], 2
    g = torch.Generator().manual_seed(SEED0 + 3 * C)
    outs = [("f32",), ("planes",), ("f32", "planes")]
    for i, HW in enumerate([1, 63, 64, 65, 130]):
        for silu in (0, 1):
            which = outs[(i + silu) % 3]
            sliced = HW == 130 and silu == 1
            buf, view, x, bs, rs = gn_view(g, B, HW, C, offset=bool(i % 2), sliced=sliced)
            gamma, beta = (1 + 0.3 * randn(g, C)).float(), randn(g, C).float()
            what = f"gn_apply C {C} HW {HW} silu {silu} {'+'.join(which)} {NAME[prec]}"
            st, _ = run_gn_stats(e, view, B, HW, C, bs, rs, what + " stats")
            n = B * HW * C
            of = nan_f32(n) if "f32" in which else None
            pl = nan_planes(PLANES[prec], n) if "planes" in which else None
            e.test_kernel("gn_apply", x=view, bstride=bs, rstride=rs, C=C, B=B, HW=HW, stats=st, gamma=dev(gamma),
                          beta=dev(beta), eps=1e-6, silu=silu, out_f32=of, out_planes=pl)
            torch.cuda.synchronize()
            want = gn_apply_formula(x, C, gamma.double(), beta.double(), silu, torch.float64).reshape(-1)
            floor = f32_floor(lambda dt: gn_apply_formula(x, C, gamma.double(), beta.double(), silu, dt))
            if of is not None:
                got = read_f32(of, n, what)
                bound = 2.0 ** -23 * want.abs() + floor
                assert not ((got - want).abs() > bound).any(), \
                    f"{what}: fp32 output off by {float((got - want).abs().max()):.3e} (floor {floor:.3e})"
            if pl is not None:
                check_unit(read_planes(e, pl, n, what), want, prec, floor, what)


# ================================================================================================ FIR resampling
def fir64(x, up):
    """[B, H, W, C] float64: the separable [1, 3, 3, 1] 2x resampling as a plain convolution (zeros outside): up = zero
    insertion then taps / 4 per axis; down = taps / 8 per axis at stride 2"""
    B, H, W, C = x.shape
    t = x.permute(0, 3, 1, 2).reshape(B * C, 1, H, W)
    k1 = torch.tensor([1.0, 3.0, 3.0, 1.0], dtype=torch.float64)
    if up:
        k = torch.outer(k1, k1) / 16
        z = torch.zeros(B * C, 1, 2 * H, 2 * W, dtype=torch.float64)
        z[:, :, ::2, ::2] = t
        o = F.conv2d(F.pad(z, (2, 1, 2, 1)), k[None, None])
    else:
        k = torch.outer(k1, k1) / 64
        o = F.conv2d(F.pad(t, (1, 1, 1, 1)), k[None, None], stride=2)
    return o.reshape(B, C, o.shape[-2], o.shape[-1]).permute(0, 2, 3, 1).contiguous()


@pytest.mark.parametrize("prec", [FP16, X3], ids=lambda p: NAME[p])
@pytest.mark.parametrize("up", [1, 0], ids=["up", "down"])
def test_fir2d(eng, up, prec):
    e, B = eng[prec], 2
    g = torch.Generator().manual_seed(SEED0 + up)
    shapes = [(2, 2), (4, 6), (16, 8)] + ([(3, 5)] if up else [])
    k = 0
    for H, W in shapes:
        for C in (4, 36):
            for with_add in (False, True):
                k += 1
                sliced = k % 3 == 0
                rs, coff = (C + 12, 4) if sliced else (C, 0)
                full = randn(g, B, H * W, rs).float()
                buf = dev(full.reshape(-1)).reshape(B, H * W, rs)
                x = full.double()[:, :, coff:coff + C].reshape(B, H, W, C)
                want, mag = fir64(x, up), fir64(x.abs(), up)
                add = randn(g, *want.shape).float() if with_add else None
                if with_add:
                    want, mag = want + add.double(), mag + add.double().abs()
                n = want.numel()
                of, pl = nan_f32(n), nan_planes(PLANES[prec], n)
                what = f"fir2d {'up' if up else 'down'} {H}x{W} C {C} add {with_add} {'strided view' if sliced else 'dense'}"
                e.test_kernel("fir2d", x=buf[:, :, coff:], bstride=H * W * rs, rstride=rs, C=C, B=B, img_h=H, img_w=W,
                              up=up, add=None if add is None else dev(add), out_f32=of, out_planes=pl)
                torch.cuda.synchronize()
                got = read_f32(of, n, what)
                terms = 4 if up else 16
                bound = (terms + 1) * 2.0 ** -24 * mag.reshape(-1)
                err = (got - want.reshape(-1)).abs()
                assert not (err > bound).any(), f"{what}: fp32 output off by {float(err.max()):.3e}"
                check_unit(read_planes(e, pl, n, what), emulate_split(got, prec), prec, 0.0, what)


# ================================================================================================ edge convolutions
def conv_out1_branch(C, taps):
    return "rows7" if taps == 7 and C % 32 == 0 and C <= 1024 else "generic"


# generic kernel: 8-channel chunks, 4 channel quarters of whole float4s (C % 16 == 0), odd tap count, the tile in LDS
OUT1_CASES = [(32, 7), (128, 7), (48, 7), (32, 5)]


def conv_out1_formula(x, w, S, L, C, taps, tanh, dt):
    y = F.conv1d(x.to(dt).reshape(S, L, C).transpose(1, 2), w.to(dt).reshape(taps, C).t()[None], padding=taps // 2)
    y = y.reshape(S * L)
    return torch.tanh(y) if tanh else y


@pytest.mark.parametrize("prec", [FP16, X3], ids=lambda p: NAME[p])
@pytest.mark.parametrize("case", OUT1_CASES, ids=lambda c: f"C{c[0]}-k{c[1]}-{conv_out1_branch(*c)}")
def test_conv_out1(eng, case, prec):
    """S = 2 sequences back to back: a missing zero pad reads the neighbouring sequence's rows"""
    C, taps = case
    e, S = eng[prec], 2
    g = torch.Generator().manual_seed(SEED0 + C + taps)
    floors, done = [], []
    for i, L in enumerate([1, 6, 255, 256, 257, 300]):
        for tanh in (0, 1):
            xf, x = operands(randn(g, S * L, C), prec)             # exact in the operand format
            w = randn(g, taps, C, scale=(taps * C) ** -0.5 * (1.0 if tanh else 2.0)).float()
            out = nan_f32(S * L)
            what = f"conv_out1 {conv_out1_branch(C, taps)} C {C} taps {taps} L {L} tanh {tanh} {NAME[prec]}"
            e.test_kernel("conv_out1", a=dev(xf.reshape(-1)), w=dev(w), B=S, L=L, C=C, ktaps=taps, apply_tanh=tanh,
                          out_f32=out)
            torch.cuda.synchronize()
            want = conv_out1_formula(x, w.double(), S, L, C, taps, tanh, torch.float64)
            floors.append(f32_floor(lambda dt: conv_out1_formula(x, w.double(), S, L, C, taps, tanh, dt)))
            done.append((what, read_f32(out, S * L, what), want))
    floor = max(floors)                       # over the whole case: L = 1 alone has two outputs to measure it on
    for what, got, want in done:
        err = float((got - want).abs().max())
        print(f"{what}: worst error {err:.3e}, floor {floor:.3e}")
        assert err <= floor + 2.0 ** -23 * float(want.abs().max()), f"{what}: off by {err:.3e} (floor {floor:.3e})"


def conv_in1_branch(Cout, taps):
    return "vec" if Cout % 4 == 0 and 256 % (Cout // 4) == 0 and taps <= 8 else "scalar"


def conv_in1_formula(wav, w, bias, dt):
    return F.conv1d(wav.to(dt)[:, None, :], w.to(dt)[:, None, :], bias.to(dt), padding=w.shape[1] // 2).transpose(1, 2)


@pytest.mark.parametrize("prec", [FP16, X3], ids=lambda p: NAME[p])
@pytest.mark.parametrize("Cout", [32, 128, 12, 24], ids=lambda c: f"Cout{c}-{conv_in1_branch(c, 7)}")
def test_conv_in1(eng, Cout, prec):
    e, S, taps = eng[prec], 2, 7
    g = torch.Generator().manual_seed(SEED0 + Cout)
    floors, done = [], []
    for L in (1, 3, 7, 100):
        for act in (0, 1, 2):
            wav = randn(g, S, L).float()
            w, bias = randn(g, Cout, taps, scale=0.5).float(), randn(g, Cout).float()
            al = (torch.rand(Cout, generator=g, dtype=torch.float64) + 0.5).float()
            ib = (1 / (torch.rand(Cout, generator=g, dtype=torch.float64) + 0.5)).float()
            n = S * L * Cout
            of, pl = nan_f32(n), nan_planes(PLANES[prec], n)
            what = f"conv_in1 {conv_in1_branch(Cout, taps)} Cout {Cout} L {L} act {act} {NAME[prec]}"
            e.test_kernel("conv_in1", x=dev(wav), w=dev(w), bias=dev(bias), B=S, L=L, C=Cout, ktaps=taps, act=act,
                          act_a=dev(al) if act == 2 else None, act_b=dev(ib) if act == 2 else None, out_f32=of,
                          out_planes=pl)
            torch.cuda.synchronize()
            args = (wav.double(), w.double(), bias.double())
            want = conv_in1_formula(*args, torch.float64)
            floors.append(f32_floor(lambda dt: conv_in1_formula(*args, dt)))
            done.append((what, read_f32(of, n, what).reshape(S, L, Cout), read_planes(e, pl, n, what), want,
                         act64(want, act, al, ib, Cout), act))
    floor = max(floors)                       # over the whole case
    for what, got, planes, want, wa, act in done:
        err = float((got - want).abs().max())
        assert err <= floor + 2.0 ** -23 * float(want.abs().max()), f"{what}: fp32 off by {err:.3e} (floor {floor:.3e})"
        # planes: the activation of the float64 value, one unit; the activation's slope (<= 2 for Snake with
        # a / b <= 4, 1 for ELU) carries the floor, and the device's exp / sin are good to a few fp32 ulps (4e-6, as
        # tests/test_gpu_gemm_kernels.py allows)
        slack = (2 * floor + 4e-6 * (1 + float(wa.abs().max()))) if act else floor
        check_unit(planes, wa.reshape(-1), prec, slack, what)


def test_edge_conv_refusals(eng):
    with pytest.raises(RuntimeError, match="conv_out1: needs odd ktaps"):
        eng[FP16].test_kernel("conv_out1", a=dev(torch.zeros(2 * 8 * 20)), w=dev(torch.zeros(7 * 20)), B=2, L=8, C=20,
                              ktaps=7, out_f32=nan_f32(16))
    with pytest.raises(RuntimeError, match="conv_in1: unsupported activation 3"):
        eng[FP16].test_kernel("conv_in1", x=dev(torch.zeros(2 * 8)), w=dev(torch.zeros(12 * 7)), B=2, L=8, C=12, ktaps=7,
                              act=3, out_f32=nan_f32(2 * 8 * 12))
