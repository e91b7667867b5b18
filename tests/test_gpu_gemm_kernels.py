"""Every kernel of the implicit-GEMM family (ditsep_amd/csrc/igemm.hip) and every feature of its shared epilogue,
one at a time, against float64 math of the same operation (dsn_test_gemm: the kernel is named, never chosen for us).

Every output is pre-filled with a NaN sentinel (fp32) / 0x7fff (a NaN in both 16-bit formats), so that each case
also proves nothing was written outside the region the descriptor addresses.  The fp32 output is held to the
per-GEMM operand-rounding bound TOL (tests/test_gpu_kernels.py); operand-plane outputs to one unit of the operand
format against the kernel's own fp32 value, and GroupNorm partials to 1e-5 against float64 statistics of the
kernel's own fp32 output.
"""
import math
import os

import pytest
import torch
import torch.nn.functional as F

from tests.util import make_engine, rel_l2

pytestmark = pytest.mark.gpu

X3, BF16, FP16, FP16X3 = 2, 1, 3, 4
# per-GEMM relative-L2 bounds: operand rounding 2^-9 (bf16), 2^-12 (fp16), ~2^-17 / 2^-22 (split) -- as test_gpu_kernels
TOL = {X3: 2e-5, BF16: 1.5e-2, FP16: 1.5e-3, FP16X3: 2e-6}
PLANES = {X3: 2, BF16: 1, FP16: 1, FP16X3: 2}
IS_F16 = {X3: False, BF16: False, FP16: True, FP16X3: True}
# explicit mantissa bits of the operand format
MANT = {False: 7, True: 10}
SENT16 = 0x7FFF   # NaN as fp16 and as bf16
TAIL = 64         # sentinel elements past the end of every output buffer

HERE = os.path.dirname(os.path.abspath(__file__))
IGEMM_SRC = os.path.join(os.path.dirname(HERE), "ditsep_amd", "csrc", "igemm.hip")

# igemm2 instantiations, mirroring igemm2_launch_cfg: (planes, bm, bn, nst, bk).  LEAN = the CFGL lines (lean
# epilogue, accumulators seeded with bias + residual), FULL = the CFG lines, plus the 128 x 64 NCSN++ level-2 tile.
LEAN = [(1, 256, 256, 2, 64), (1, 256, 256, 3, 32), (2, 256, 256, 2, 32), (1, 256, 128, 3, 64),
        (1, 256, 128, 3, 32), (1, 256, 128, 2, 64), (1, 128, 128, 3, 32), (1, 128, 128, 2, 64)]
FULL = [(2, 128, 128, 2, 32), (2, 256, 128, 2, 32), (2, 128, 256, 2, 32), (2, 256, 256, 2, 32), (2, 256, 128, 3, 32),
        (1, 128, 128, 3, 32), (1, 256, 128, 3, 32), (1, 256, 256, 3, 32), (1, 128, 128, 2, 64), (1, 128, 128, 3, 64),
        (1, 256, 128, 2, 64), (1, 128, 256, 2, 64), (1, 256, 256, 2, 64), (1, 256, 128, 3, 64), (1, 128, 256, 3, 64)]
TILE_128x64 = (1, 128, 64, 3, 64)
SKINNY_MT = [3, 4, 5, 6, 7, 8]
PRECS = {1: (BF16, FP16), 2: (X3, FP16X3)}


@pytest.fixture(scope="module")
def eng():
    engs = {p: make_engine(precision=p) for p in (X3, BF16, FP16, FP16X3)}
    yield engs
    for e in engs.values():
        e.close()


DEV = torch.device("cuda", 0)


def dev(t):
    return t.to(device=DEV, dtype=torch.float32).contiguous()


def randn(g, *shape, scale=1.0):
    return torch.randn(shape, generator=g, dtype=torch.float64) * scale


# ------------------------------------------------------------------------------------------------ float64 reference
def conv_ref(a, w, *, B, Lin, Cin, N, taps, rows, in_stride=1, tap_dil=1, in_pad=0, row_elems=None, a_off=0,
             img=None):
    """out[b, j, n] = sum_{tap, ci} w[n][tap*Cin + ci] x[b][j*in_stride + tap*tap_dil - in_pad][ci], zero outside
    [0, Lin); x = channels a_off .. a_off + Cin of rows of row_elems.  img = (H, W): 3x3 conv, padding 1."""
    re_ = row_elems or Cin
    x = a.double().reshape(B, Lin, re_)[:, :, a_off:a_off + Cin]
    wk = w.double().reshape(N, taps, Cin)
    if img is not None:   # conv2d(padding=1) as im2col + one float64 GEMM on the device (the 256-row-tile cases are
        H, W = img        # ~10 GFLOP: too slow for a float64 CPU convolution)
        xi = x.reshape(B, H, W, Cin).permute(0, 3, 1, 2).to(DEV)
        cols = F.unfold(xi, 3, padding=1)                                   # [B, Cin*9, H*W], (ci, dy, dx) order
        wi = wk.reshape(N, 3, 3, Cin).permute(0, 3, 1, 2).reshape(N, Cin * 9).to(DEV)
        return torch.matmul(wi, cols).transpose(1, 2).cpu()
    if in_stride == 1 and rows == Lin + 2 * in_pad - tap_dil * (taps - 1):
        return F.conv1d(x.transpose(1, 2), wk.permute(0, 2, 1), dilation=tap_dil, padding=in_pad).transpose(1, 2)
    j = torch.arange(rows).view(rows, 1) * in_stride + torch.arange(taps).view(1, taps) * tap_dil - in_pad
    ok = (j >= 0) & (j < Lin)
    g = x[:, j.clamp(0, Lin - 1), :] * ok.view(1, rows, taps, 1)
    return torch.einsum("bjtc,ntc->bjn", g, wk)


def silu(v):
    return v / (1 + torch.exp(-v))


def act64(v, act, al=None, ib=None, mod=None):
    if act == 1:
        return torch.where(v > 0, v, torch.expm1(v))
    if act == 3:
        return silu(v)
    if act == 2:
        ch = torch.arange(v.shape[-1], device=v.device) % mod
        a, b = al.double()[ch], ib.double()[ch]
        return v + b * torch.sin(v * a) ** 2
    return v


def swiglu64(y):
    """packed [.., N] (groups of 32: 16 values, their 16 gates) -> [.., N/2]"""
    s = y.shape
    y = y.reshape(*s[:-1], s[-1] // 32, 2, 16)
    return (y[..., 0, :] * silu(y[..., 1, :])).reshape(*s[:-1], s[-1] // 2)


# ------------------------------------------------------------------------------------------------ checks
def scatter_positions(B, rows, n_out, bstride, row_elems, off, limit, M=None):
    """flat output offsets of the (b, j, n) the epilogue stores, and the (b, j, n) index triples"""
    b = torch.arange(B).view(B, 1, 1)
    j = torch.arange(rows).view(1, rows, 1)
    n = torch.arange(n_out).view(1, 1, n_out)
    rel = j * row_elems + off + n
    keep = ((rel >= 0) & (rel < limit)).expand(B, rows, n_out)
    if M is not None:
        keep = keep & (b * rows + j < M)
    flat = (b * bstride + rel).expand(B, rows, n_out)
    return flat[keep], keep


def check_f32(buf, ref, flat, keep, tol, what):
    buf = buf.cpu().double()
    got = buf[flat]
    want = ref.cpu()[keep]
    assert torch.isfinite(got).all(), f"{what}: non-finite in the written region"
    err = rel_l2(got, want)
    assert err < tol, f"{what}: rel-L2 {err:.3e} >= {tol:.1e}"
    untouched = torch.ones(buf.numel(), dtype=torch.bool)
    untouched[flat] = False
    assert torch.isnan(buf[untouched]).all(), f"{what}: {int((~torch.isnan(buf[untouched])).sum())} elements " \
                                              "written outside the output region"


def emulate_split(e, prec, planes=None):
    """dsn_split of float32(e): hi = fmt(sat(v)), lo = fmt(sat(v - hi)) (fp16 saturates at +-65504, bf16 does not)"""
    f16 = IS_F16[prec]
    dt = torch.float16 if f16 else torch.bfloat16
    sat = (lambda v: v.clamp(-65504.0, 65504.0)) if f16 else (lambda v: v)
    v = e.float()
    hi = sat(v).to(dt).float()
    out = hi.double()
    if (planes or PLANES[prec]) == 2:
        out = out + sat(v - hi).to(dt).double()
    return out


def check_planes(e, raw, flat, keep, expect, prec, what, slack=0.0):
    """raw int16 [P][ps] planes; expect = float64 value the planes encode (act of the kernel's own fp32 output)"""
    P, f16 = PLANES[prec], IS_F16[prec]
    raw = raw.cpu()
    for p in range(P):
        untouched = torch.ones(raw.shape[1], dtype=torch.bool)
        untouched[flat] = False
        assert (raw[p][untouched] == SENT16).all(), f"{what}: plane {p} written outside the output region"
    got = e.decode_planes(raw.to(DEV)).cpu()[flat]
    want = emulate_split(expect.cpu()[keep], prec)
    assert torch.isfinite(got).all(), f"{what}: non-finite plane values"
    # one unit of the format (P = 1), or of the lo plane (P = 2), at the value's magnitude; fp16 subnormals below 2^-14
    unit = 2.0 ** -(MANT[f16] * P + (P - 1))
    floor = 2.0 ** -14 if f16 else 2.0 ** -126
    bound = unit * torch.maximum(want.abs(), torch.full_like(want, floor)) + slack * (1 + want.abs())
    bad = (got - want).abs() > bound
    assert not bad.any(), f"{what}: {int(bad.sum())} plane values off by more than one unit " \
                          f"(worst {float((got - want).abs().max()):.3e})"
    return got


def gn64(v, B, rows, N):
    """float64 GroupNorm slice partials [B][rows/64][N/4][2] (mean, M2 of 64 rows x 4 channels) of v [B, rows, N]"""
    x = v.double().reshape(B, rows // 64, 64, N // 4, 4).permute(0, 1, 3, 2, 4).reshape(B, rows // 64, N // 4, 256)
    mean = x.mean(-1)
    return torch.stack([mean, ((x - mean.unsqueeze(-1)) ** 2).sum(-1)], -1)


def check_gn(got, want, what, rtol=1e-5):
    got = got.cpu().double()
    scale = want[..., 1].div(256).sqrt().mean().item()       # typical standard deviation of a slice
    dm = (got[..., 0] - want[..., 0]).abs().max().item()
    assert dm <= rtol * scale * 4 + rtol * want[..., 0].abs().max().item(), f"{what}: GroupNorm mean off by {dm:.3e}"
    r2 = ((got[..., 1] - want[..., 1]).abs() / want[..., 1]).max().item()
    assert r2 <= rtol * 8, f"{what}: GroupNorm M2 off by {r2:.3e} (relative)"


def nan_f32(n):
    return torch.full((n + TAIL,), float("nan"), device=DEV)


def nan_planes(P, n):
    return torch.full((P, n + TAIL), SENT16, device=DEV, dtype=torch.int16)


# ------------------------------------------------------------------------------------------------ one GEMM case
def run_case(e, prec, *, kernel, B, Lin, Cin, N, taps=1, rows=None, M=None, in_stride=1, tap_dil=1, in_pad=0,
             row_elems=None, a_off=0, img=None, bias=False, bias_mod=None, bbias=False, resid=None, out_scale=1.0,
             tanh=False, act=0, act_mod=None, swiglu=False, gn=False, gn2=None, f32=True, planes=True,
             out_geo=None, seed=0, tol=None, what="", **kern):
    """Build operands, run `kernel`, check every output; returns (float64 pre-activation v, fp32 output, gn)."""
    g = torch.Generator().manual_seed(seed)
    if img is not None:
        taps = 9
    rows = rows or (Lin if img is None else img[0] * img[1])
    Mv = M or B * rows
    re_ = row_elems or Cin
    a = randn(g, B * Lin * re_)
    w = randn(g, N, taps * Cin, scale=1 / math.sqrt(taps * Cin))
    y = conv_ref(a, w, B=B, Lin=Lin, Cin=Cin, N=N, taps=taps, rows=rows, in_stride=in_stride, tap_dil=tap_dil,
                 in_pad=in_pad, row_elems=re_, a_off=a_off, img=img)
    kw = dict(in_stride=in_stride, tap_dil=tap_dil, in_pad=in_pad, in_row_elems=row_elems or 0, a_off=a_off,
              M=M or 0, out_scale=out_scale)
    if img is not None:
        kw.update(img_h=img[0], img_w=img[1])
    n_out = N // 2 if swiglu else N
    bvec = bm_ = None
    if bias:
        bm_ = bias_mod or N
        bvec = randn(g, bm_)
        # (allocated N long: a kernel that indexed past bias_mod would read wrong values, not outside the tensor)
        kw.update(bias=dev(torch.cat([bvec, randn(g, max(N - bm_, 0))])), bias_mod=bm_)
        y = y + bvec[torch.arange(N) % bm_]
    if bbias:
        bb = randn(g, B, N + 12)
        kw.update(bbias=dev(bb), bbias_stride=N + 12)
        y = y + bb[:, None, :N]
    if swiglu:
        kw.update(swiglu=1)
        y = swiglu64(y)
    # output geometry
    og = dict(bstride=rows * n_out, row_elems=n_out, off=0, limit=rows * n_out)
    og.update(out_geo or {})
    if out_geo:
        kw.update(out_bstride=og["bstride"], out_row_elems=og["row_elems"], out_off=og["off"], out_limit=og["limit"])
    if resid is not None:   # (resid_row_elems, resid_off): a channel slice of a wider tensor
        rre, roff = resid
        rt = randn(g, B, rows, rre)
        kw.update(resid=dev(rt), resid_row_elems=rre, resid_off=roff, resid_bstride=rows * rre)
        y = y + rt[:, :, roff:roff + N]
    v = y * out_scale
    if tanh:
        kw.update(f32_op=1)
    al = ib = None
    if act:
        kw.update(act=act)
        if act == 2:
            am = act_mod or N
            al = torch.rand(am, generator=g, dtype=torch.float64) + 0.5
            ib = 1 / (torch.rand(am, generator=g, dtype=torch.float64) + 0.5)
            kw.update(act_a=dev(al), act_b=dev(ib), act_mod=am)
    span = B * og["bstride"]
    out = nan_f32(span) if f32 and not swiglu else None
    P = PLANES[prec]
    pl = nan_planes(P, span) if planes or swiglu else None
    gbuf = g2buf = None
    if gn:
        gbuf = nan_f32(B * (rows // 64) * (N // 4) * 2)
        kw.update(gn_stats=gbuf)
        if gn2:
            nq2, qoff2 = gn2
            g2buf = nan_f32(B * (rows // 64) * nq2 * 2)
            kw.update(gn_stats2=g2buf, gn_nq2=nq2, gn_qoff2=qoff2)
    kw.update(kern)
    if out is not None:
        kw["out_f32"] = out
    if pl is not None:
        kw["out_planes"] = pl
    e.test_gemm(dev(a), dev(w), kernel=kernel, B=B, Lin=Lin, Cin=Cin, N=N, taps=taps, rows_per_b=rows, **kw)
    torch.cuda.synchronize()
    flat, keep = scatter_positions(B, rows, n_out, og["bstride"], og["row_elems"], og["off"], og["limit"],
                                   M=Mv if M else None)
    tol = tol or TOL[prec]
    res = {"v": v, "flat": flat, "keep": keep}
    if out is not None:
        check_f32(out, torch.tanh(v) if tanh else v, flat, keep, tol, f"{what} fp32")
        res["out"] = out.cpu().double()
    if pl is not None:
        if out is not None and not tanh:
            # the planes encode act(the kernel's own fp32 value): one unit of the format (the fast exp / sin of the
            # activations differ from float64 by a few fp32 ulps: `slack`)
            own = torch.zeros(B, rows, n_out, dtype=torch.float64)
            own[keep] = res["out"][flat]
            check_planes(e, pl, flat, keep, act64(own, act, al, ib, act_mod or N), prec, f"{what} planes",
                         slack=4e-6 if act else 0.0)
        # and against float64 math, rounded (and fp16-saturated) as the planes are: the GEMM bound plus one rounding
        ref = emulate_split(v if swiglu else act64(v, act, al, ib, act_mod or N), prec)
        got = e.decode_planes(pl).cpu()
        untouched = torch.ones(span + TAIL, dtype=torch.bool)
        untouched[flat] = False
        assert (pl.cpu()[:, untouched] == SENT16).all(), f"{what}: planes written outside the output region"
        # one rounding of the last plane, relative to the whole value: half a unit for P = 1; for P = 2 half a unit
        # of the lo plane's share -- ~2^-12 of the value normally, but all of it beyond an fp16 hi that saturated
        rnd = 2.0 ** -(MANT[IS_F16[prec]] + 1)
        if P == 2:
            hi = emulate_split(ref, prec, planes=1)[keep]
            rnd *= float((ref[keep] - hi).norm() / ref[keep].norm())
        err = rel_l2(got[flat], ref[keep])
        assert err < tol + rnd, f"{what} planes vs float64: rel-L2 {err:.3e}"
        res["planes"] = got
    if gn:
        cnt = B * (rows // 64) * (N // 4) * 2
        gb = gbuf.cpu().double()
        assert torch.isnan(gb[cnt:]).all(), f"{what}: gn_stats written past its end"
        got = gb[:cnt].reshape(B, rows // 64, N // 4, 2)
        if out is not None and not tanh:
            check_gn(got, gn64(res["out"][flat].reshape(B, rows, N), B, rows, N), f"{what} gn_stats")
        else:    # fp32 output transformed: against the float64 values, to the GEMM bound
            want = gn64(v, B, rows, N)
            sd = want[..., 1].div(256).sqrt().mean().item()
            assert (got[..., 0] - want[..., 0]).abs().max() < 8 * tol * (sd + want[..., 0].abs().max()), what
            assert rel_l2(got[..., 1], want[..., 1]) < 8 * tol, f"{what} gn M2"
        res["gn"] = got
        if g2buf is not None:
            nq2, qoff2 = gn2
            g2 = g2buf.cpu().double()
            cnt2 = B * (rows // 64) * nq2 * 2
            assert torch.isnan(g2[cnt2:]).all(), f"{what}: gn_stats2 written past its end"
            g2 = g2[:cnt2].reshape(B, rows // 64, nq2, 2)
            assert torch.equal(g2[:, :, qoff2:qoff2 + N // 4], got), f"{what}: gn_stats2 differs from gn_stats"
            other = torch.ones(nq2, dtype=torch.bool)
            other[qoff2:qoff2 + N // 4] = False
            assert torch.isnan(g2[:, :, other]).all(), f"{what}: gn_stats2 quads outside [qoff2, qoff2 + N/4) written"
    return res


def prec_list(planes):
    return PRECS[planes]


# ------------------------------------------------------------------------------------------------ 1. igemm2 tiles
# (the check that LEAN / FULL / SKINNY_MT match igemm.hip runs without a GPU: tests/test_host_logic.py)
TILES = sorted(set(LEAN) | set(FULL) | {TILE_128x64})


@pytest.mark.parametrize("cfg", TILES, ids=lambda c: "P%d_%dx%d_s%d_k%d" % c)
def test_igemm2_tile_instantiation(eng, cfg):
    P_, bm, bn, nst, bk = cfg
    N = 2 * bn - 60                     # two column tiles, the last one ragged
    for prec in prec_list(P_):
        for kc, (taps, Cin, dil) in enumerate([(1, bk, 1), (1, 5 * bk, 1), (7, 2 * bk, 3)]):
            pad = 3 * dil if taps == 7 else 0
            # lean descriptor: bias + residual + Snake -> the LEAN_SEEDED kernel where a CFGL line exists; ragged M
            # with the last item short
            rows = bm + bm // 2 + 5
            run_case(eng[prec], prec, kernel="tile", bm=bm, bn=bn, nst=nst, bk=bk, B=3, Lin=rows, Cin=Cin, N=N,
                     taps=taps, tap_dil=dil, in_pad=pad, M=3 * rows - 37, bias=True, resid=(N, 0), act=2,
                     seed=kc, what=f"lean {cfg} prec {prec} K{kc}")
            # full descriptor: per-item bias + tanh + GroupNorm partials (whole 64-row items; M = 576 is ragged)
            rows = 192
            run_case(eng[prec], prec, kernel="tile", bm=bm, bn=bn, nst=nst, bk=bk, B=3, Lin=rows, Cin=Cin, N=N,
                     taps=taps, tap_dil=dil, in_pad=pad, bbias=True, tanh=True, gn=True, seed=10 + kc,
                     what=f"full {cfg} prec {prec} K{kc}")


# ------------------------------------------------------------------------------------------------ 2. epilogue features
@pytest.mark.parametrize("prec", [X3, FP16])
def test_epilogue_features_one_at_a_time(eng, prec):
    e = eng[prec]
    base = dict(kernel="tile", bm=128, bn=128, nst=PLANES[prec] == 2 and 2 or 3, bk=32, B=2, Lin=200, Cin=64, N=196)
    run_case(e, prec, bias=True, bias_mod=68, what="bias_mod < N", **base)
    run_case(e, prec, bbias=True, what="per-item bias", **base)
    run_case(e, prec, resid=(260, 36), what="residual channel slice", **base)
    run_case(e, prec, bias=True, resid=(196, 0), out_scale=0.7071067811865476, what="out_scale", **base)
    run_case(e, prec, bias=True, tanh=True, what="tanh", **base)
    for act in (1, 2, 3):
        run_case(e, prec, bias=True, act=act, act_mod=100 if act == 2 else None, what=f"act {act}", **base)
    # all at once
    run_case(e, prec, bias=True, bias_mod=68, bbias=True, resid=(260, 36), out_scale=0.5, act=2, act_mod=100,
             what="combined", **base)
    # the lean (seeded) kernel takes bias_mod / residual slices / Snake channels through seed_acc
    lean = dict(base, bm=256, bn=256 if PLANES[prec] == 2 else 128, N=452)
    run_case(e, prec, bias=True, bias_mod=68, resid=(520, 36), out_scale=0.5, act=2, act_mod=100,
             what="combined lean", **lean)


@pytest.mark.parametrize("prec", [FP16, FP16X3])
def test_fp16_plane_saturation(eng, prec):
    """fp16 plane outputs saturate at +-65504 instead of overflowing (emulate_split): values up to ~2e5 here"""
    r = run_case(eng[prec], prec, kernel="tile", bm=128, bn=128, nst=2 if PLANES[prec] == 2 else 3, bk=32, B=1,
                 Lin=256, Cin=64, N=128, out_scale=6e4, what="saturation")
    assert (r["planes"][r["flat"]].abs() >= 65504).any()


@pytest.mark.parametrize("prec", [BF16, FP16])
def test_swiglu_on_every_kernel(eng, prec):
    e = eng[prec]
    N = 320
    run_case(e, prec, kernel="v1", B=1, Lin=300, Cin=64, N=N, bias=True, swiglu=True, what="swiglu v1")
    run_case(e, prec, kernel="tile", bm=256, bn=128, nst=3, bk=64, B=1, Lin=300, Cin=128, N=N, bias=True,
             swiglu=True, what="swiglu tile")
    run_case(e, prec, kernel="panel", panel_rows=144, panel_bn=256, B=1, Lin=300, Cin=128, N=N + 192, bias=True,
             swiglu=True, what="swiglu panel")
    run_case(e, prec, kernel="skinny", B=1, Lin=37, Cin=128, N=N, bias=True, swiglu=True, what="swiglu skinny")


# ------------------------------------------------------------------------------------------------ 3. output clipping
@pytest.mark.parametrize("kernel", ["tile", "v1"])
def test_convtranspose_phase_clipping(eng, kernel):
    prec, N, rows, stride = FP16, 132, 150, 3
    kern = dict(bm=128, bn=128, nst=3, bk=32) if kernel == "tile" else {}
    for off in (-N, 0, N, 2 * N):
        limit = (rows - 1) * stride * N + off + N // 2 + 2   # cuts the last row inside a 64-column chunk
        run_case(eng[prec], prec, kernel=kernel, B=2, Lin=rows, Cin=64, N=N, bias=True, resid=(N, 0), act=1,
                 out_geo=dict(bstride=rows * stride * N, row_elems=stride * N, off=off, limit=limit),
                 what=f"phase clip off {off}", **kern)


# ------------------------------------------------------------------------------------------------ 4. split-K
@pytest.mark.parametrize("k", [2, 3, 8])
def test_split_k_slab_epilogue(eng, k):
    prec, B, rows, Cin, N = FP16, 2, 192, 320, 192      # 10 k-tiles of 32: 3 and 8 do not divide it
    e = eng[prec]
    tile = dict(bm=128, bn=128, nst=3, bk=32)
    for clip in (False, True):
        og = dict(bstride=rows * 2 * N, row_elems=2 * N, off=N if clip else 0,
                  limit=(rows - 1) * 2 * N + N + 100 if clip else rows * 2 * N)
        span = B * og["bstride"]
        slabs = nan_f32(k * span)
        feat = dict(bias=True, bbias=True, resid=(2 * N + 8, 4)) if not clip else dict(bias=True)
        r = run_case(e, prec, kernel="splitk", ksplit=k, slabs=slabs, slab_stride=span, B=B, Lin=rows, Cin=Cin,
                     N=N, gn=not clip, out_geo=og, seed=k, what=f"split-K {k} clip {clip}", **tile, **feat)
        s = slabs.cpu()
        assert torch.isnan(s[k * span:]).all(), "slab tail written"
        # the same GEMM unsplit, on the tile kernel
        u = run_case(e, prec, kernel="tile", B=B, Lin=rows, Cin=Cin, N=N, gn=not clip, out_geo=og, seed=k,
                     what="unsplit", **tile, **feat)
        assert rel_l2(r["out"][r["flat"]], u["out"][u["flat"]]) < TOL[prec]


@pytest.mark.parametrize("prec", [BF16, FP16])
def test_skinny_ksplit(eng, prec):
    g = torch.Generator().manual_seed(7)
    M, Cin, N = 40, 256, 196
    for ks in (2, 5, Cin // 32):
        a, w = randn(g, M * Cin), randn(g, N, Cin, scale=Cin ** -0.5)
        slabs = nan_f32(ks * M * N)
        eng[prec].test_gemm(dev(a), dev(w), kernel="skinny", B=1, Lin=M, Cin=Cin, N=N, ksplit=ks, out_f32=slabs,
                            slab_stride=M * N)
        s = slabs.cpu().double()
        assert torch.isnan(s[ks * M * N:]).all()
        tot = s[:ks * M * N].reshape(ks, M, N).sum(0)
        assert rel_l2(tot, a.reshape(M, Cin) @ w.t()) < TOL[prec]


# ------------------------------------------------------------------------------------------------ 5. GroupNorm partials
@pytest.mark.parametrize("prec", [BF16, FP16])
def test_groupnorm_partials(eng, prec):
    e = eng[prec]
    # tile kernel, own layout + concat layout (this tensor = quads 20.. of 80)
    run_case(e, prec, kernel="tile", bm=128, bn=128, nst=3, bk=64, B=2, Lin=256, Cin=128, N=192, bias=True,
             resid=(192, 0), out_scale=0.5, gn=True, gn2=(80, 20), what="gn tile")
    run_case(e, prec, kernel="tile", bm=128, bn=64, nst=3, bk=64, B=2, Lin=128, Cin=128, N=128, bias=True, gn=True,
             gn2=(64, 32), what="gn 128x64")
    # halo kernel
    run_case(e, prec, kernel="halo", B=2, Lin=256, Cin=64, N=196, img=(16, 16), bias=True, gn=True, gn2=(60, 7),
             what="gn halo")


# ------------------------------------------------------------------------------------------------ 6. halo 3x3 kernel
@pytest.mark.parametrize("prec", [BF16, FP16])
def test_halo3x3_kernel(eng, prec):
    e = eng[prec]
    for i, (H, W, Cin, N, B) in enumerate([(32, 8, 32, 132, 1), (16, 16, 96, 196, 2), (8, 32, 512, 132, 1),
                                           (16, 16, 64, 260, 3)]):
        run_case(e, prec, kernel="halo", B=B, Lin=H * W, Cin=Cin, N=N, img=(H, W), bias=True, resid=(N + 4, 4),
                 act=3, seed=i, what=f"halo {H}x{W} Cin {Cin} N {N}")
    # 256-row tiles: (M / 256) * cdiv(N, 128) >= 512
    run_case(e, prec, kernel="halo", B=64, Lin=256, Cin=32, N=964, img=(16, 16), bias=True, planes=False,
             what="halo 256-row tile")


@pytest.mark.parametrize("prec", [BF16, FP16])
def test_halo3x3_nin_shortcut(eng, prec):
    """out = (Conv_1(a) + b1 + Conv_2(x) + b2) / sqrt 2, Conv_2 a 1x1 conv over a channel prefix of x"""
    e = eng[prec]
    for i, (H, W, Cin, N, B, scin, sre, big) in enumerate([(16, 16, 64, 196, 2, 32, 48, False),
                                                          (32, 8, 128, 132, 1, 256, 260, False),
                                                          (8, 32, 32, 100, 2, 96, 96, False),
                                                          (16, 16, 32, 964, 64, 64, 72, True)]):
        g = torch.Generator().manual_seed(100 + i)
        rows = H * W
        xs = randn(g, B * rows * sre)
        ws = randn(g, N, scin, scale=scin ** -0.5)
        bs = randn(g, N)
        sc = torch.einsum("bjc,nc->bjn", xs.reshape(B, rows, sre)[:, :, :scin], ws) + bs
        r = run_case(e, prec, kernel="halo", B=B, Lin=rows, Cin=Cin, N=N, img=(H, W), bias=True,
                     out_scale=1 / math.sqrt(2), sc_a=dev(xs), sc_w=dev(ws), sc_bias=dev(bs), sc_Cin=scin,
                     sc_row_elems=sre, seed=i, f32=True, planes=not big, tol=1e30, what=f"halo shortcut {i}")
        v = r["v"] + sc / math.sqrt(2)
        err = rel_l2(r["out"][r["flat"]], v[r["keep"]])
        assert err < TOL[prec], f"halo shortcut {i}: rel-L2 {err:.3e}"


# ------------------------------------------------------------------------------------------------ 7. skinny kernel
@pytest.mark.parametrize("prec", [BF16, FP16])
def test_skinny_every_row_count(eng, prec):
    e = eng[prec]
    for M in list(range(1, 49)) + [49, 64, 65, 81, 97, 113, 128]:
        run_case(e, prec, kernel="skinny", B=1, Lin=M, Cin=96, N=132, bias=True, resid=(140, 8), act=3, seed=M,
                 what=f"skinny M {M}")


# ------------------------------------------------------------------------------------------------ 8. row panels
@pytest.mark.parametrize("prec", [X3, FP16])
def test_row_panel_instantiations(eng, prec):
    e = eng[prec]
    P_ = PLANES[prec]
    cases = [(72, 128), (112, 256), (144, 256), (144, 128), (208, 256), (208, 128), (272, 256), (272, 128)]
    if P_ == 2:   # split modes: the 9- and 17-sub-tile BK-32 rings only
        cases = [(144, 256), (144, 128), (272, 256), (272, 128)]
    for i, (rows, bn) in enumerate(cases):
        run_case(e, prec, kernel="panel", panel_rows=rows, panel_bn=bn, B=1, Lin=2 * rows + rows // 2 + 3, Cin=128,
                 N=2 * bn - 60, bias=True, resid=(2 * bn - 52, 8), act=2, seed=i, what=f"panel {rows} x {bn}")
        run_case(e, prec, kernel="panel", panel_rows=rows, panel_bn=bn, B=1, Lin=2 * rows + 7, Cin=128, N=2 * bn + 64,
                 bias=True, swiglu=True, seed=i, what=f"panel {rows} x {bn} swiglu")
    if P_ == 1:   # 8-wave panels (panel_wm = 2): every ring igemm_panel_launch accepts
        for rows, nst, bk in [(144, 3, 64), (272, 2, 64), (272, 4, 32)]:
            run_case(e, prec, kernel="panel", panel_rows=rows, panel_bn=256, panel_wm=2, nst=nst, bk=bk, B=1,
                     Lin=2 * rows + 11, Cin=128, N=452, bias=True, resid=(460, 4), act=1,
                     what=f"panel wm2 {rows} s{nst} k{bk}")


def test_refused_descriptor_fails_by_name(eng):
    """a launcher that refuses the descriptor is an error naming it -- no other kernel runs instead"""
    with pytest.raises(RuntimeError, match="igemm2 tile"):
        run_case(eng[FP16], FP16, kernel="tile", bm=192, bn=128, nst=3, bk=32, B=1, Lin=64, Cin=32, N=64)
    with pytest.raises(RuntimeError, match="halo"):
        run_case(eng[FP16], FP16, kernel="halo", B=1, Lin=100, Cin=32, N=64, img=(10, 10))
    # the split-K rule the ring launchers share: slices write raw partial sums, so no SwiGLU epilogue
    with pytest.raises(RuntimeError, match="igemm2 split-K tile refused or failed: invalid argument"):
        run_case(eng[FP16], FP16, kernel="splitk", ksplit=2, slabs=nan_f32(2 * 64 * 32), slab_stride=64 * 32, swiglu=True,
                 bm=128, bn=128, nst=3, bk=32, B=1, Lin=64, Cin=64, N=64)
