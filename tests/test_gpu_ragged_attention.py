"""The length-aware (VARLEN) instantiations of the three attention kernels alone, in the manner of
tests/test_gpu_aux_kernels.py (whose helpers and bounds these tests reuse): a batch of items padded to S tokens with
`lens[b]` valid ones each, against float64 attention of every item over its first lens[b] rows only.

What the padding holds is chosen so that a kernel which reads one key too many cannot pass; that is asserted on the
reference alone, before the device is touched:
  attention   valid rows carry q[..., 0] = 1 and k[..., 0] = 0; padded rows k[..., 0] = 8 and v = 100 (finite and exact
              in bf16 and fp16).  A padded key then weighs e^8 times an average valid one and pulls the output towards
              100: the float64 evaluation WITHOUT the mask differs from the masked one by rel-L2 > 10 for every
              (item, head) with lens[b] < S.  Smallest ratio over the five cases and four modes, measured on the CPU: 102.
  fused qkv   the `a` rows of padded tokens are scaled by PAD_GAIN = 4 (k and v of a padded token grow with it, and its
              scores spread fourfold, so the padded keys take the softmax over).  The unmasked float64 evaluation is
              then more than 10 x TOL[prec] away from the masked one for every item with lens[b] < S: smallest rel-L2
              over the plane cases 2.49 (fp16 and bf16 alike; the requirement is 0.015 and 0.15), over the fp8 case 1.6.
Bounds: those of test_attention and test_qkv_attention, taken over the valid rows.  Padded query rows are computed (over
the item's valid keys) and must be finite; their values are not compared.  The plane tails keep their sentinel.

Figures of the reference alone (measured on the CPU): float32 floors up to 4.2e-6 (attention), 2.4e-3 (fused qkv fp8
output, fp16); fp8 boundary blocks 0.00 % (attention S = 49), 0.00 % (fused qkv, fp16).
"""
import pytest
import torch

from tests.test_gpu_aux_kernels import (ALL, NAME, SEED0, SENT8, attention_branch, attention_inputs, attention_ref,
                                        check_fp8, f32_floor, nan_bytes, operands, pack_qkv, qkv_branch, qkv_ref,
                                        read_planes, unit_of)
from tests.test_gpu_gemm_kernels import BF16, DEV, FP16, FP16X3, PLANES, TOL, dev, nan_f32, nan_planes, randn
from tests.util import make_engine, rel_l2

pytestmark = pytest.mark.gpu

B_ATT, H_ATT, DH = 3, 2, 64
# (S, lens): the in-register kernel (S <= 256) and the long one; full length, a length on a 16-key tile edge, one key
# past a tile edge, a single key
ATT_CASES = [(17, (17, 16, 1)), (49, (49, 33, 2)), (161, (161, 145, 17)), (300, (300, 257, 40)), (385, (385, 384, 100))]
PAD_GAIN = 4.0
# (S, ipp, H, items, lens, bias): a short last panel with mixed lengths inside a panel; one item per panel in the
# 144-row and the 240-row tile
QKV_CASES = [(33, 4, 3, 6, (33, 17, 16, 2, 33, 9), True), (130, 1, 2, 3, (130, 113, 5), True),
             (236, 1, 3, 3, (236, 100, 17), False)]
QKV_OUT8_CASE = (33, 4, 4, 9, (33, 17, 16, 2, 33, 9, 1, 32, 20), True)
QKV_OUT8_SEED = 2004


@pytest.fixture(scope="module")
def eng():
    engs = {p: make_engine(precision=p) for p in ALL}
    yield engs
    for e in engs.values():
        e.close()


def lens_dev(lens):
    return torch.tensor(lens, dtype=torch.int32, device=DEV)


# ================================================================================================ attention
def ragged_attention_case(prec, S, lens, seed):
    """-> fp32 operand tensor [B*S][3 D], per-item float64 references [H, lens[b], dh], floor, max|V_valid|.  Asserts
    (reference alone) that the unmasked evaluation is far from the masked one."""
    B, H = B_ATT, H_ATT
    q, k, v = attention_inputs(prec, B, H, DH, S, False, seed)
    for b, L in enumerate(lens):
        q[b, :, :L, 0] = 1.0
        k[b, :, :L, 0] = 0.0
        k[b, :, L:, 0] = 8.0
        v[b, :, L:, :] = 100.0
    (qf, q), (kf, k), (vf, v) = (operands(t, prec) for t in (q, k, v))
    refs, floor, vmax, ratios = [], 0.0, 0.0, []
    for b, L in enumerate(lens):
        qb, kb, vb = q[b, :, :L], k[b, :, :L], v[b, :, :L]
        refs.append(attention_ref(qb, kb, vb)[0])
        floor = max(floor, f32_floor(lambda dt: attention_ref(qb, kb, vb, dt)[0]))
        vmax = max(vmax, float(vb.abs().max()))
        if L < S:
            full = attention_ref(q[b], k[b], v[b])[0][:, :L]
            ratios += [rel_l2(full[h], refs[b][h]) for h in range(H)]
    assert min(ratios) > 10, f"S {S}: the unmasked reference is only rel-L2 {min(ratios):.3g} from the masked one"
    return pack_qkv(qf, kf, vf), refs, floor, vmax, min(ratios)


def att_id(c):
    S, lens = c
    return f"S{S}-{attention_branch(1, DH, S)}-lens{'_'.join(map(str, lens))}"


@pytest.mark.parametrize("prec", ALL, ids=lambda p: NAME[p])
@pytest.mark.parametrize("case", ATT_CASES, ids=att_id)
def test_ragged_attention(eng, case, prec):
    S, lens = case
    e = eng[prec]
    B, H, D = B_ATT, H_ATT, H_ATT * DH
    a, refs, floor, vmax, ratio = ragged_attention_case(prec, S, lens, SEED0 + S)
    n = B * S * D
    pl = nan_planes(PLANES[prec], n)
    e.test_kernel("attention", a=dev(a), B=B, S=S, H=H, dh=DH, out_planes=pl, lens=lens_dev(lens))
    torch.cuda.synchronize()
    what = f"ragged attention {att_id(case)} {NAME[prec]}"
    got = read_planes(e, pl, n, what).reshape(B, S, H, DH).permute(0, 2, 1, 3)      # (finite on the padded rows too)
    bound = 4 * (unit_of(prec) / 2) * vmax + floor
    for b, L in enumerate(lens):
        err = (got[b, :, :L] - refs[b]).abs()
        worst_l2 = max(rel_l2(got[b, h, :L], refs[b][h]) for h in range(H))
        print(f"{what} item {b} (len {L}): worst rel-L2 {worst_l2:.3e}, worst element {float(err.max()):.3e} "
              f"(bound {bound:.3e}, floor {floor:.3e}; unmasked reference >= {ratio:.3g} away)")
        assert worst_l2 < TOL[prec], f"{what} item {b}: rel-L2 {worst_l2:.3e} >= {TOL[prec]:.1e}"
        assert float(err.max()) <= bound, f"{what} item {b}: element error {float(err.max()):.3e} > {bound:.3e}"


def check_fp8_valid_rows(b8, s8, refs, lens, S, D, floor, what):
    """check_fp8 over the valid rows of every item (refs: per item [lens[b]][D]); the tails of the whole buffers must
    hold the sentinel"""
    B = len(lens)
    n = B * S * D
    b8, s8 = b8.cpu(), s8.cpu()
    assert (b8[n:] == SENT8).all() and (s8[n // 32:] == SENT8).all(), f"{what}: fp8 output written past its end"
    rows = torch.cat([torch.arange(b * S, b * S + L) for b, L in enumerate(lens)])
    vb = torch.cat([b8[:n].reshape(B * S, D)[rows].reshape(-1), b8[n:]])
    vs = torch.cat([s8[:n // 32].reshape(B * S, D // 32)[rows].reshape(-1), s8[n // 32:]])
    check_fp8(vb, vs, torch.cat(refs), floor, what)


def test_ragged_attention_fp8_output(eng):
    prec, (S, lens) = FP16X3, ATT_CASES[1]
    B, H, D = B_ATT, H_ATT, H_ATT * DH
    a, refs, floor, _, _ = ragged_attention_case(prec, S, lens, SEED0 + S)
    n = B * S * D
    b8, s8 = nan_bytes(n), nan_bytes(n // 32)
    eng[prec].test_kernel("attention", a=dev(a), B=B, S=S, H=H, dh=DH, out_fp8=b8, out_fp8_scale=s8, lens=lens_dev(lens))
    torch.cuda.synchronize()
    refs = [r.permute(1, 0, 2).reshape(-1, D) for r in refs]
    check_fp8_valid_rows(b8, s8, refs, lens, S, D, floor, f"ragged attention fp8 S {S}")


def test_ragged_attention_refusals(eng):
    B, S, H = 3, 17, 2
    a = dev(torch.zeros(B * S * 3 * H * DH))
    for bad, msg in (((17, 0, 5), r"attention: lens\[1\] = 0 outside \[1, S = 17\]"),
                     ((17, 5, 18), r"attention: lens\[2\] = 18 outside \[1, S = 17\]")):
        with pytest.raises(RuntimeError, match=msg):
            eng[FP16].test_kernel("attention", a=a, B=B, S=S, H=H, dh=DH, out_planes=nan_planes(1, B * S * H * DH),
                                  lens=lens_dev(bad))
    with pytest.raises(RuntimeError, match="unsupported head width 128 with lens"):
        eng[FP16].test_kernel("attention", a=dev(torch.zeros(B * S * 3 * 128)), B=B, S=S, H=1, dh=128,
                              out_planes=nan_planes(1, B * S * 128), lens=lens_dev((17, 5, 1)))


# ================================================================================================ fused qkv + attention
def ragged_qkv_case(prec, case, seed, need_floor=False):
    """-> fp32 a, w, bias, per-item float64 references [lens[b]][D], floor (0 unless need_floor), smallest rel-L2 of the
    unmasked evaluation from the masked one.  Asserts the latter > 10 TOL[prec] on the reference alone."""
    S, ipp, H, B, lens, with_bias = case
    D = H * 64
    g = torch.Generator().manual_seed(seed)
    a = randn(g, B * S, D).reshape(B, S, D)
    for b, L in enumerate(lens):
        a[b, L:] *= PAD_GAIN
    af, a = operands(a.reshape(B * S, D), prec)
    wf, w = operands(randn(g, 3 * D, D, scale=D ** -0.5), prec)
    bias = randn(g, 3 * D).float() if with_bias else None
    bd = None if bias is None else bias.double()
    a = a.reshape(B, S, D)
    refs, floor, ratios = [], 0.0, []
    for b, L in enumerate(lens):
        ab = a[b, :L]
        refs.append(qkv_ref(ab, w, bd, 1, L, H, prec))
        if need_floor:
            floor = max(floor, f32_floor(lambda dt: qkv_ref(ab, w, bd, 1, L, H, prec, dt)))
        if L < S:
            ratios.append(rel_l2(qkv_ref(a[b], w, bd, 1, S, H, prec)[:L], refs[b]))
    assert min(ratios) > 10 * TOL[prec], (f"the unmasked reference is only rel-L2 {min(ratios):.3g} from the masked one "
                                          f"(needs > {10 * TOL[prec]:.3g})")
    return af, wf, bias, refs, floor, min(ratios)


def qkv_id(c):
    S, ipp, H, B, lens, bias = c
    return f"S{S}-ipp{ipp}-H{H}-{qkv_branch(S, ipp)}-lens{'_'.join(map(str, lens))}"


@pytest.mark.parametrize("prec", [FP16, BF16], ids=lambda p: NAME[p])
@pytest.mark.parametrize("case", QKV_CASES, ids=qkv_id)
def test_ragged_qkv_attention(eng, case, prec):
    S, ipp, H, B, lens, _ = case
    D = H * 64
    af, wf, bias, refs, _, ratio = ragged_qkv_case(prec, case, SEED0 + S + H)
    n = B * S * D
    e = eng[prec]
    pl = nan_planes(1, n)
    e.test_kernel("qkv_attention", a=dev(af), w=dev(wf), bias=None if bias is None else dev(bias), B=B, S=S, H=H, D=D,
                  ipp=ipp, rope_cos=nan_f32(S * 32), rope_sin=nan_f32(S * 32), out_planes=pl, lens=lens_dev(lens))
    torch.cuda.synchronize()
    what = f"ragged qkv_attention {qkv_id(case)} {NAME[prec]}"
    got = read_planes(e, pl, n, what).reshape(B, S, D)
    for b, L in enumerate(lens):
        err = rel_l2(got[b, :L], refs[b])
        print(f"{what} item {b} (len {L}): rel-L2 {err:.3e} (unmasked reference >= {ratio:.3g} away)")
        assert err < TOL[prec], f"{what} item {b}: rel-L2 {err:.3e} >= {TOL[prec]:.1e}"


def test_ragged_qkv_attention_fp8_output(eng):
    prec, case = FP16, QKV_OUT8_CASE
    S, ipp, H, B, lens, _ = case
    D = H * 64
    af, wf, bias, refs, floor, _ = ragged_qkv_case(prec, case, QKV_OUT8_SEED, need_floor=True)
    n = B * S * D
    b8, s8 = nan_bytes(n), nan_bytes(n // 32)
    eng[prec].test_kernel("qkv_attention", a=dev(af), w=dev(wf), bias=dev(bias), B=B, S=S, H=H, D=D, ipp=ipp,
                          rope_cos=nan_f32(S * 32), rope_sin=nan_f32(S * 32), out_fp8=b8, out_fp8_scale=s8,
                          lens=lens_dev(lens))
    torch.cuda.synchronize()
    check_fp8_valid_rows(b8, s8, refs, lens, S, D, floor, f"ragged qkv_attention {qkv_id(case)} fp8")


def test_ragged_qkv_attention_refusals(eng):
    B, S, H, D = 3, 33, 2, 128
    for bad, msg in (((33, 0, 5), r"qkv_attention: lens\[1\] = 0 outside \[1, S = 33\]"),
                     ((34, 5, 1), r"qkv_attention: lens\[0\] = 34 outside \[1, S = 33\]")):
        with pytest.raises(RuntimeError, match=msg):
            eng[FP16].test_kernel("qkv_attention", a=dev(torch.zeros(B * S * D)), w=dev(torch.zeros(3 * D * D)), B=B,
                                  S=S, H=H, D=D, ipp=1, rope_cos=nan_f32(S * 32), rope_sin=nan_f32(S * 32),
                                  out_planes=nan_planes(1, B * S * D), lens=lens_dev(bad))
