"""Sensitivity of the checks of tests/test_gpu_prep_kernels.py, without a GPU: each check function of
tests/prep_kernels_ref.py is fed the reference output with ONE mutation, as a device would return it, and must refuse it;
the unmutated reference must pass its own check.

A mutation that is the identity at a shape (a tap / channel swap with one tap or one channel) is asserted to be one.
"""
import numpy as np
import pytest
import torch

from tests import prep_kernels_ref as R
from tests.test_gpu_gemm_kernels import emulate_split

SEED0 = 9876


def gen(i=0):
    return torch.Generator().manual_seed(SEED0 + i)


def must_differ(got, want, what):
    with pytest.raises(AssertionError, match="differ in their bits"):
        R.check_bits(got, want, what)


@pytest.mark.parametrize("prec", R.ALL, ids=lambda p: R.NAME[p])
def test_plane_bits_is_emulate_split(prec):
    """the per-plane restatement decodes to emulate_split, edge values included, and +0 / -0 keep their sign bit"""
    v = R.weight(gen(), 40, 33)
    raw = R.plane_bits(v, prec)
    assert torch.equal(R.decode_bits(raw, prec), emulate_split(v.reshape(-1), prec))
    z = R.plane_bits(torch.tensor([0.0, -0.0]), prec)
    assert z[0].tolist() == [0, -32768] and (z.shape[0] == 1 or z[1].tolist() == [0, 0])
    if R.IS_F16[prec]:
        sat = R.decode_bits(R.plane_bits(torch.tensor([65520.0, -1e5]), prec), prec)
        assert sat.tolist() == ([65504.0, -65504.0] if R.PLANES[prec] == 1 else [65520.0, -1e5])


CONV_SHAPES = [(6, 5, 7), (16, 8, 1), (130, 12, 7)]
CONVT_SHAPES = [(8, 12, 2), (5, 3, 4), (16, 4, 8)]


@pytest.mark.parametrize("prec", R.ALL, ids=lambda p: R.NAME[p])
@pytest.mark.parametrize("shape", CONV_SHAPES, ids=str)
def test_conv_tap_channel_swap_is_caught(shape, prec):
    Cout, Cin, kw = shape
    v, s = R.weight(gen(1), Cout, Cin, kw), torch.rand(Cout, generator=gen(2)) + 0.5
    good = R.plane_bits(R.pack_weight_ref("conv", v, scale=s), prec)
    R.check_bits(good.clone(), good, "conv unmutated")
    bad = R.plane_bits(R.pack_weight_ref("conv", v, scale=s, mut="conv_tap_channel_swapped"), prec)
    if kw == 1 or Cin == 1:
        assert torch.equal(bad, good), "expected the identity at this shape"
    else:
        must_differ(bad, good, "conv tap / channel swapped")


@pytest.mark.parametrize("prec", R.ALL, ids=lambda p: R.NAME[p])
@pytest.mark.parametrize("mut", ["convt_phases_reversed", "convt_phase_major_taps"])
@pytest.mark.parametrize("shape", CONVT_SHAPES, ids=str)
def test_convt_mutations_are_caught(shape, mut, prec):
    Cin, Cout, s = shape
    v, sc = R.weight(gen(3), Cin, Cout, 2 * s), torch.rand(Cin, generator=gen(4)) + 0.5
    good = R.plane_bits(R.pack_weight_ref("convt", v, scale=sc), prec)
    R.check_bits(good.clone(), good, "convt unmutated")
    must_differ(R.plane_bits(R.pack_weight_ref("convt", v, scale=sc, mut=mut), prec), good, f"convt {mut}")


@pytest.mark.parametrize("prec", R.ALL, ids=lambda p: R.NAME[p])
def test_linear_mutations_are_caught(prec):
    N, K = 128, 40                      # (groups of 32 + 32 need N % 64 == 0)
    W, cs = R.weight(gen(5), N, K), torch.rand(K, generator=gen(6)) + 0.5
    good = R.plane_bits(R.pack_weight_ref("linear_swiglu", W, colscale=cs), prec)
    R.check_bits(good.clone(), good, "swiglu unmutated")
    for mut in ("swiglu_groups_of_32", "colscale_by_row"):
        must_differ(R.plane_bits(R.pack_weight_ref("linear_swiglu", W, colscale=cs, mut=mut), prec), good, mut)
    b = torch.arange(128.0)
    must_differ(R.f32_bits(R.swiglu_rows(b, 32)), R.f32_bits(R.swiglu_rows(b, 16)), "bias groups of 32")
    if R.PLANES[prec] == 2:
        lo_zero = good.clone()
        lo_zero[1] = 0
        assert torch.equal(lo_zero[0], good[0])
        must_differ(lo_zero, good, "hi plane right, lo plane zero")


@pytest.mark.parametrize("prec", R.ALL, ids=lambda p: R.NAME[p])
def test_negative_zero_padding_is_caught(prec):
    src = R.weight(gen(7), 10, 40, 9)
    good = R.plane_bits(R.pack_weight_ref("conv2d", src, N=12, cin_pad=64), prec)
    bad = R.plane_bits(R.pack_weight_ref("conv2d", src, N=12, cin_pad=64, mut="padding_negative_zero"), prec)
    assert torch.equal(R.decode_bits(bad, prec), R.decode_bits(good, prec))          # equal as numbers ...
    must_differ(bad, good, "conv2d padding -0")                                      # ... and still refused
    x = R.ncsn_pack_ref(torch.randn(2, 2, 4, 5, generator=gen(8)), torch.randn(2, 1, 4, 5, generator=gen(9)), 8, 32)
    neg = torch.where(x == 0, -torch.zeros_like(x), x)
    must_differ(R.f32_bits(neg), R.f32_bits(x), "ncsn_pack padding -0")


def test_zero_tail_off_by_one_is_caught():
    x = torch.randn(3, 2, 4, 9, generator=gen(10))
    lens = [1, 5, 10]
    good = R.zero_tail_ref(x, lens)
    assert (good[0] == 0).all() and (good[1, ..., :4] == x[1, ..., :4]).all() and (good[1, ..., 4:] == 0).all()
    assert torch.equal(good[2], x[2])                                 # lens = T + 1: nothing is cut
    R.check_f32_exact(good.clone(), good, "zero_tail unmutated")
    with pytest.raises(AssertionError, match="differ in their bits"):
        R.check_f32_exact(R.zero_tail_ref(x, lens, "cut_at_lens"), good, "zero_tail cut at lens")


@pytest.mark.parametrize("case", [(5, 160), (64, 128)], ids=str)
def test_fp8_mutations_are_caught(case):
    N, K = case
    x = R.fp8_source(N, K, SEED0)
    b8, s8 = R.mx_pack_ref(x)
    R.check_bits(b8.clone(), b8, "fp8 bytes unmutated")
    assert R.check_fp8_properties(x, b8, s8, "fp8 unmutated") <= 1.0
    bb, bs = R.mx_pack_ref(x, "e8m0_plus_1")
    must_differ(bs, s8, "E8M0 + 1")
    with pytest.raises(AssertionError, match="one exponent too large"):
        R.check_fp8_properties(x, bb, bs, "E8M0 + 1")
    tb, ts = R.mx_pack_ref(x, "e4m3_truncated")
    assert torch.equal(ts, s8)
    must_differ(tb, b8, "e4m3 truncated")
    with pytest.raises(AssertionError, match="beyond half an e4m3 step"):
        R.check_fp8_properties(x, tb, ts, "e4m3 truncated")
    ub, us = b8.clone(), (s8.to(torch.int32) - 1).clamp(min=1).to(torch.uint8)       # a scale one too small clips
    with pytest.raises(AssertionError, match="too small"):
        R.check_fp8_properties(x, ub, us, "E8M0 - 1")


def test_fp8_edge_blocks_are_what_they_claim():
    e = R.fp8_edge_blocks()
    b8, s8 = R.mx_pack_ref(e)
    k = s8.reshape(-1).to(torch.int32) - 127
    assert k.tolist() == [-126, 3, 4, 3, -5 + 1, 2, 0, -2, -126]
    q = b8.contiguous().view(torch.float8_e4m3fn).float()
    assert (q[0] == 0).all() and q[1, 5] == 448 and q[3, 5] == 448 and q[4, 31] < 0
    assert q[5, 1:9].tolist() == [2.0 ** -7, 3 * 2.0 ** -9, 2.0 ** -9, 0.0, 2.0 ** -9, 0.0, 0.0, -2.0 ** -8]  # ties to even
    assert q[6, 1:9].tolist() == [1.0, 1.25, -1.0, -1.25, 16.0, 20.0, -16.0, -20.0]
    assert q[7, 1:5].tolist() == [1.0, 1.25, -1.0, -1.25]
    assert float(e[8].abs().max()) < 448 * 2.0 ** -126 and (q[8] != 0).any()
    R.check_fp8_properties(e, b8, s8, "fp8 edge blocks")


def test_fp8_emulation_meets_its_properties_on_random_blocks():
    x = R.fp8_source(128, 1024, SEED0 + 1)                   # 4096 blocks over 2^+-30
    assert R.check_fp8_properties(x, *R.mx_pack_ref(x), "fp8 random blocks") <= 1.0


@pytest.mark.parametrize("prec", R.ALL, ids=lambda p: R.NAME[p])
def test_row_sum_over_unrounded_weights_is_caught(prec):
    """(one-plane formats: in the split formats the operand rounding, 2^-17 and 2^-23 of a weight, sums to less than
    the float32 summation bound itself, and the two sums cannot be told apart by any float32 result)"""
    N, K = 33, 200
    W = torch.randn(N, K, generator=gen(11))
    cs = torch.rand(K, generator=gen(12)) + 0.5
    raw = R.plane_bits(R.pack_weight_ref("linear", W, colscale=cs), prec).reshape(-1, N, K)
    dt = torch.float16 if R.IS_F16[prec] else torch.bfloat16
    hi = raw[0].contiguous().view(dt).double()
    lo = raw[1].contiguous().view(dt).double() if raw.shape[0] == 2 else None
    want, A, Rn = R.packed_row_sum(hi, lo)
    R.check(want.astype(np.float32), want, A, Rn, "packed_row_sum unmutated")
    unrounded = (W * cs[None, :]).double().sum(1).numpy().astype(np.float32)
    if R.PLANES[prec] == 2:
        return
    with pytest.raises(AssertionError, match="beyond"):
        R.check(unrounded, want, A, Rn, "row sum over the unrounded weights")


def test_fp8_row_sum_over_unrounded_weights_is_caught():
    x = torch.randn(5, 160, generator=gen(13))
    deq = R.mx_decode(*R.mx_pack_ref(x))
    want, A, Rn = R.fp8_row_sum(deq)
    R.check(want.astype(np.float32), want, A, Rn, "fp8_row_sum unmutated")
    with pytest.raises(AssertionError, match="beyond"):
        R.check(x.double().sum(1).numpy().astype(np.float32), want, A, Rn, "fp8 row sum over the unrounded weights")


def test_bounded_references_pass_their_own_checks():
    g = gen(14)
    v = torch.randn(5, 65, generator=g) * torch.exp2(torch.randint(-20, 21, (5, 1), generator=g).float())
    gg = torch.randn(5, generator=g)
    want, A, Rn = R.wn_scale(v, gg)
    R.check(want.astype(np.float32), want, A, Rn, "wn_scale")
    assert Rn + 1 <= -(-65 // 64) + 10
    W, beta, bias = torch.randn(5, 65, generator=g), torch.randn(65, generator=g), torch.randn(5, generator=g)
    want, A, Rn = R.bias_plus_wbeta(W, beta, bias)
    R.check(want.astype(np.float32), want, A, Rn, "bias_plus_wbeta")
    al = torch.cat([torch.rand(7, generator=g) * 8 - 4, torch.tensor([-30.0])])
    for name, (w, A, Rn) in R.snake_params(al, al).items():
        R.check(w.astype(np.float32), w, A, Rn, f"snake {name}")
    assert abs(R.snake_params(al, al)["ib"][0][-1] - 1e9) < 1e6               # the 1e-9 term dominates at beta = -30
    t = torch.rand(3, generator=g)
    want, bound, fu = R.timestep_features(t, torch.randn(128, generator=g))
    f32v = np.float32(2) * np.float32(R.PI32) * t.numpy()[:, None] * torch.randn(128, generator=gen(14)).numpy()[None, :]
    assert fu >= 2.0 and want.shape == bound.shape == (3, 256) and f32v.dtype == np.float32
    c, s, bound, (pu, fu) = R.rope_tables(385, 32)
    assert pu >= 2.0 and fu >= 2.0 and c.shape == bound.shape == (385, 32)
    R.check_abs(c.astype(np.float32), c, bound, "rope cos rounded to float32")
    for prec in R.ALL:
        R.check_planes_abs(R.plane_bits(torch.from_numpy(s).float(), prec), s, bound, prec, f"rope sin planes {R.NAME[prec]}")
        with pytest.raises(AssertionError, match="beyond the bound"):            # cos stored where sin belongs
            R.check_planes_abs(R.plane_bits(torch.from_numpy(c).float(), prec), s, bound, prec, "cos for sin")
