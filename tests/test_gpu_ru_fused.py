"""The fused 128-channel ResidualUnit (ditsep_amd/csrc/ru_fused.hip) alone, against float64 math of the same unit:
    x' = x + conv1x1(act_mid(conv_k7_dilated(a) + b7)) + b1,   planes(x') = act_out(x')
dsn_test_kernel's `ru_fused` kind calls ru_fused_launch once on caller-owned tensors; which kernel runs is the
launcher's own dispatch, and every case id starts with the variant = the kernel it lands on and the operand format:
    v2-bf16, v2-fp16        ru_fused2_kernel (256-row tiles), what the engine runs in the single-plane modes
    v1-bf16, v1-fp16        ru_fused_kernel<1> (128-row tiles), reached through DSN_RU_V1 as the full-size test does
    v1-bf16x3, v1-fp16x3    ru_fused_kernel<2>, the split modes

Reference (float64; the operands are exactly the values the operand planes hold): h = act_mid(conv1d(A, W7, dilation d,
padding 3 d) + b7), h rounded as dsn_split rounds it (the kernel keeps the intermediate in operand planes: one in the
single-plane modes, two in the split modes), want = X + h W1^T + b1, branch = want - X.

Checks.  Every output buffer ends in TAIL sentinels (NaN, 0x7fff) that must survive, and all before them is finite.
  per row   ||got - want|| over the 128 channels of each (sequence, position) <= 2 TOL ||branch row|| + sqrt(128) floor:
            TOL is the per-GEMM bound of tests/test_gpu_gemm_kernels.py and the unit chains two GEMMs; floor is
            f32_floor of the residual add alone.  A wrong halo row, tap or tile edge is O(1) in its own row and
            invisible in a whole-tensor norm.
  per case  rel-L2 of (got - want) against branch < TOL
  rounded   single-plane modes only: ||got - want|| < 1/2 ||want - want_unrounded||, want_unrounded the same formula
            with h left in float64.  The two references lie D = 2^-9 / sqrt(3) (bf16), 2^-12 / sqrt(3) (fp16) of the branch
            apart, which 2 TOL cannot tell from rounding; a kernel that rounds h lands on `want` to its accumulation
            error, one that does not lands D away.
  planes    act_out of the kernel's own fp32 output to one unit of the format (check_planes, slack 4e-6 with an
            activation); planes-only output bit-identical to the planes of the two-output run, in-place output
            (out_f32 == x) bit-identical to out-of-place in both outputs.

Figures.  Reference alone (CPU; S = 3, L = 600, dil 1 and 9, Snake / Snake): the same formula in float32 torch against
float64, worst row relative to its branch row.  Device (MI355X): the worst row over every case of this module, with
the case it fell on.  Both beside the 2 TOL bound:
                  float32 restatement   device                               2 TOL
    v2-bf16       1.1e-3                9.8e-4  (S2-L300-d6-elu-elu)         3e-2
    v1-bf16       1.1e-3                1.6e-3  (S3-L129-d9-elu-elu)         3e-2
    v2-fp16       2.0e-4                2.4e-4  (S3-L257-d1-elu-elu)         3e-3
    v1-fp16       2.0e-4                2.6e-4  (S3-L127-d9-elu-elu)         3e-3
    v1-bf16x3     5.5e-6                8.8e-6  (S3-L127-d9-elu-elu)         4e-5
    v1-fp16x3     1.2e-6                7.0e-7  (S2-L300-d3-snake-snake)     4e-6
  The single-plane figures are flips of the rounding of h between the evaluation at hand and float64 (one flip is one
  unit of the format in one of a row's 128 inputs).  The split modes drop the lo lo product of the operand planes;
  no variant comes near its bound.
  rounded: the float32 restatement lies 0.018 .. 0.026 D (bf16) / 0.073 .. 0.080 D (fp16) from `want`; the device at
  most 0.054 D (bf16) / 0.083 D (fp16).

Mutation check (CPU, mutated float64 formulas through check_rows / check_rounded of this module, S = 3, L = 600, dil 1
and 9, Snake / Snake): the previous sequence's tail in place of the leading zero padding (worst row 0.76 / 0.99 of its
branch row), the last tap lost on the last row of every tile (0.46 .. 0.49), the mid and out Snake vectors swapped
(0.50 .. 0.59) and, in the split modes, the hi lo cross terms dropped (5e-3 bf16x3, 6e-4 fp16x3) each fail the per-row
check in every variant.  The intermediate left unrounded does NOT fail the per-row check in the single-plane modes:
its worst row is 2.8e-3 (bf16) / 3.0e-4 (fp16) against bounds of 3e-2 / 3e-3, one rounding of h being ten times
smaller than what 2 TOL allows two GEMMs.  That is what the `rounded` check is for: there it is 1.0 D and fails.

The hook cannot express out_planes aliasing the input planes (the input planes are the engine's own workspace, made
from the caller's fp32 `a`); the launcher's refusal of it has no case here.
"""
import functools
import math
from types import SimpleNamespace

import pytest
import torch

from tests.test_gpu_aux_kernels import f32_floor, operands, read_f32, read_planes
from tests.test_gpu_gemm_kernels import (BF16, FP16, FP16X3, PLANES, SENT16, TOL, X3, act64, check_planes, conv_ref, dev,
                                         emulate_split, nan_f32, nan_planes, randn)
from tests.util import make_engine

pytestmark = pytest.mark.gpu

C = 128
SEED0 = 4321                                   # a case's seed is SEED0 + its index in CASES
NONE, ELU, SNAKE = 0, 1, 2
ACT = {NONE: "none", ELU: "elu", SNAKE: "snake"}
# (id, precision, DSN_RU_V1 set)
VARIANTS = [("v2-bf16", BF16, False), ("v2-fp16", FP16, False), ("v1-bf16", BF16, True), ("v1-fp16", FP16, True),
            ("v1-bf16x3", X3, False), ("v1-fp16x3", FP16X3, False)]

# (S, L, dil, act_mid, act_out).  L = 27 at dil 9 is exactly the halo, 127 .. 129 straddle the v1 tile, 255 .. 257 the
# v2 tile, 600 is several tiles with a ragged last one; S = 3 gives the middle sequence a neighbour on both sides
GEOMETRY = [(3, L, d, ELU, ELU) for L in (1, 27, 127, 128, 129, 255, 256, 257, 600) for d in (1, 9)]
DILATIONS = [(2, 300, d, ELU, ELU) for d in range(2, 9)]
ACTIVATIONS = [(2, 300, 3, am, ao) for am, ao in ((NONE, NONE), (ELU, SNAKE), (SNAKE, ELU), (SNAKE, SNAKE))]
CASES = GEOMETRY + DILATIONS + ACTIVATIONS
OUTPUTS_CASE = (2, 300, 3, SNAKE, SNAKE)
REPEAT_CASE = (3, 600, 9, ELU, ELU)


def case_id(c):
    S, L, d, am, ao = c
    return f"S{S}-L{L}-d{d}-{ACT[am]}-{ACT[ao]}"


@pytest.fixture(scope="module")
def eng():
    engs = {p: make_engine(precision=p) for p in (BF16, FP16, X3, FP16X3)}
    yield engs
    for e in engs.values():
        e.close()


@pytest.fixture
def variant(request, monkeypatch):
    name, prec, v1 = request.param
    if v1:
        monkeypatch.setenv("DSN_RU_V1", "1")
    else:
        monkeypatch.delenv("DSN_RU_V1", raising=False)
    return name, prec


def by_variant(fn):
    return pytest.mark.parametrize("variant", VARIANTS, indirect=True, ids=[v[0] for v in VARIANTS])(fn)


# ------------------------------------------------------------------------------------------------ float64 reference
def ru_formula(a, w7, w1, b7, b1, x, dil, act_mid, mid_a, mid_b, prec, round_h=True):
    """-> (x', branch) of a [S, L, 128] in float64; h rounded to the operand format as dsn_split rounds it"""
    S, L, _ = a.shape
    y = conv_ref(a, w7, B=S, Lin=L, Cin=C, N=C, taps=7, rows=L, tap_dil=dil, in_pad=3 * dil)
    h = act64(y + b7, act_mid, mid_a, mid_b, C)
    if round_h:
        h = emulate_split(h, prec)
    branch = h @ w1.t() + b1
    return x + branch, branch


@functools.lru_cache(maxsize=None)
def ru_case(c, prec):
    """operands and float64 reference of case c in the operand format of prec (shared by the variants and tests that use
    it; nothing in it is modified afterwards)"""
    S, L, dil, am, ao = c
    g = torch.Generator().manual_seed(SEED0 + CASES.index(c))
    af, a = operands(randn(g, S, L, C), prec)
    w7f, w7 = operands(randn(g, C, 7 * C, scale=1 / math.sqrt(7 * C)), prec)
    w1f, w1 = operands(randn(g, C, C, scale=1 / math.sqrt(C)), prec)
    f32 = lambda t: t.float().double()         # passed through in fp32: the reference sees the same values
    x, b7, b1 = f32(randn(g, S, L, C)), f32(randn(g, C, scale=0.1)), f32(randn(g, C, scale=0.1))
    # Snake parameters per channel, as run_case of test_gpu_gemm_kernels draws them; mid and out are different draws
    vec = lambda: (f32(torch.rand(C, generator=g, dtype=torch.float64) + 0.5),
                   f32(1 / (torch.rand(C, generator=g, dtype=torch.float64) + 0.5)))
    (mid_a, mid_b), (out_a, out_b) = vec(), vec()
    args = (a, w7, w1, b7, b1, x, dil, am, mid_a, mid_b, prec)
    want, branch = ru_formula(*args)
    unrounded = ru_formula(*args, round_h=False)[0]
    floor = f32_floor(lambda dt: x.to(dt) + branch.to(dt))
    return SimpleNamespace(S=S, L=L, dil=dil, am=am, ao=ao, n=S * L * C, af=af, w7f=w7f, w1f=w1f, a=a, w7=w7, w1=w1, x=x,
                           b7=b7, b1=b1, mid_a=mid_a, mid_b=mid_b, out_a=out_a, out_b=out_b, want=want, branch=branch,
                           unrounded=unrounded, floor=floor, args=args)


# ------------------------------------------------------------------------------------------------ checks (CPU only)
def check_rows(got, r, prec, what):
    """got float64 [S, L, 128]: the per-row and per-case fp32 bounds; returns the worst row relative to its branch row"""
    err = (got - r.want).norm(dim=-1)
    bnorm = r.branch.norm(dim=-1)
    bound = 2 * TOL[prec] * bnorm + math.sqrt(C) * r.floor
    worst = float((err / bnorm).max())
    rel = float((got - r.want).norm() / r.branch.norm())
    print(f"{what}: worst row {worst:.3e} of its branch row (2 TOL {2 * TOL[prec]:.1e}), whole case {rel:.3e}, "
          f"floor {r.floor:.3e}, branch rows {float(bnorm.min()):.1f} .. {float(bnorm.max()):.1f}")
    bad = err > bound
    assert not bad.any(), f"{what}: {int(bad.sum())} rows beyond 2 TOL x branch row + floor, first (sequence, position) " \
                          f"{tuple(int(i) for i in bad.nonzero()[0])}, worst {float((err / bound).max()):.1f} x the bound"
    assert rel < TOL[prec], f"{what}: rel-L2 against the branch {rel:.3e} >= {TOL[prec]:.1e}"
    return worst


def check_rounded(got, r, prec, what):
    """single-plane modes: the output sits on the reference with the rounded intermediate, not on the unrounded one"""
    if PLANES[prec] != 1:
        return
    d = float((r.want - r.unrounded).norm())
    e = float((got - r.want).norm())
    print(f"{what}: {e / d:.3f} of the distance between the rounded and unrounded references")
    assert e < 0.5 * d, f"{what}: the output is {e / d:.2f} D from the rounded-intermediate reference"


# ------------------------------------------------------------------------------------------------ one launch
def launch(e, prec, r, *, f32="new", planes=True, **over):
    """f32: "new" (own buffer), "inplace" (out_f32 == x) or None -> (fp32 output buffer or None, planes or None)"""
    xb = nan_f32(r.n)
    xb[:r.n] = dev(r.x.reshape(-1))
    of = {"new": nan_f32(r.n), "inplace": xb, None: None}[f32]
    pl = nan_planes(PLANES[prec], r.n) if planes else None
    snake = lambda kind, v: dev(v) if kind == SNAKE else None
    kw = dict(a=dev(r.af.reshape(-1)), w=dev(r.w7f), w2=dev(r.w1f), x=xb, bias=dev(r.b7), bias2=dev(r.b1), B=r.S, L=r.L,
              dil=r.dil, act=r.am, act_a=snake(r.am, r.mid_a), act_b=snake(r.am, r.mid_b), act_out=r.ao,
              out_act_a=snake(r.ao, r.out_a), out_act_b=snake(r.ao, r.out_b), out_f32=of, out_planes=pl)
    kw.update(over)
    e.test_kernel("ru_fused", **kw)
    torch.cuda.synchronize()
    if f32 != "inplace":
        assert torch.equal(read_f32(xb, r.n, "x").float(), r.x.reshape(-1).float()), "the residual stream x was modified"
    return of, pl


def check_case(e, prec, r, what):
    of, pl = launch(e, prec, r)
    got = read_f32(of, r.n, what).reshape(r.S, r.L, C)
    worst = check_rows(got, r, prec, what)
    check_rounded(got, r, prec, what)
    read_planes(e, pl, r.n, what)
    keep = torch.ones(r.S, r.L, C, dtype=torch.bool)
    check_planes(e, pl, torch.arange(r.n), keep, act64(got, r.ao, r.out_a, r.out_b, C), prec, what,
                 slack=4e-6 if r.ao else 0.0)
    return worst


# ------------------------------------------------------------------------------------------------ tests
@by_variant
@pytest.mark.parametrize("case", GEOMETRY, ids=case_id)
def test_ru_fused_geometry(eng, variant, case):
    name, prec = variant
    check_case(eng[prec], prec, ru_case(case, prec), f"ru_fused {name} {case_id(case)}")


@by_variant
@pytest.mark.parametrize("case", DILATIONS, ids=case_id)
def test_ru_fused_dilations(eng, variant, case):
    name, prec = variant
    check_case(eng[prec], prec, ru_case(case, prec), f"ru_fused {name} {case_id(case)}")


@by_variant
@pytest.mark.parametrize("case", ACTIVATIONS, ids=case_id)
def test_ru_fused_activations(eng, variant, case):
    name, prec = variant
    check_case(eng[prec], prec, ru_case(case, prec), f"ru_fused {name} {case_id(case)}")


@by_variant
def test_ru_fused_outputs(eng, variant):
    """planes only (what the engine asks of the last unit of every block), fp32 only and in place, against the
    two-output run: bit-identical wherever both write"""
    name, prec = variant
    e, r = eng[prec], ru_case(OUTPUTS_CASE, prec)
    what = f"ru_fused {name} {case_id(OUTPUTS_CASE)}"
    both_f, both_p = launch(e, prec, r)
    _, only_p = launch(e, prec, r, f32=None)
    only_f, _ = launch(e, prec, r, planes=False)
    in_f, in_p = launch(e, prec, r, f32="inplace")
    for buf, tag in ((only_f, "fp32 only"), (in_f, "in place")):
        got = read_f32(buf, r.n, f"{what} {tag}").reshape(r.S, r.L, C)
        check_rows(got, r, prec, f"{what} {tag}")
        assert torch.equal(buf[:r.n], both_f[:r.n]), f"{what}: {tag} fp32 output differs from the two-output run"
    for pl, tag in ((only_p, "planes only"), (in_p, "in place")):
        read_planes(e, pl, r.n, f"{what} {tag}")
        assert torch.equal(pl, both_p), f"{what}: {tag} planes differ from the two-output run"
    got = read_f32(both_f, r.n, what).reshape(r.S, r.L, C)
    check_planes(e, only_p, torch.arange(r.n), torch.ones(r.S, r.L, C, dtype=torch.bool),
                 act64(got, r.ao, r.out_a, r.out_b, C), prec, what + " planes only", slack=4e-6)


@by_variant
def test_ru_fused_repeatable(eng, variant):
    name, prec = variant
    e, r = eng[prec], ru_case(REPEAT_CASE, prec)
    runs = [launch(e, prec, r) for _ in range(3)]
    for of, pl in runs[1:]:
        assert torch.equal(of[:r.n], runs[0][0][:r.n]) and torch.equal(pl, runs[0][1]), \
            f"ru_fused {name} {case_id(REPEAT_CASE)}: two runs differ"


REFUSALS = [("dil0", dict(dil=0), "ru_fused: refused"), ("dil10", dict(dil=10), "ru_fused: refused"),
            ("S0", dict(B=0), "ru_fused: B and L must be positive"), ("L0", dict(L=0), "ru_fused: B and L must be positive"),
            ("act_mid3", dict(act=3), "ru_fused: refused"), ("act_out3", dict(act_out=3), "ru_fused: refused"),
            ("snake_mid_without_vectors", dict(act=SNAKE), "ru_fused: refused"),
            ("snake_out_without_one_vector", dict(act_out=SNAKE, out_act_a="mid_a"), "ru_fused: refused"),
            ("a_numel", dict(L=28), "ru_fused: a_numel"), ("w2_numel", dict(w2="short"), "ru_fused: a_numel"),
            ("no_bias2", dict(bias2=None), "ru_fused: x, bias or bias2 missing")]


@by_variant
@pytest.mark.parametrize("refusal", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_ru_fused_refusals(eng, variant, refusal):
    """each fails by name before any launch: every element of both outputs still holds its sentinel"""
    name, prec = variant
    _, over, msg = refusal
    e, r = eng[prec], ru_case((3, 27, 9, ELU, ELU), prec)
    over = {k: (dev(r.mid_a) if v == "mid_a" else dev(torch.zeros(C * C - 4)) if v == "short" else v)
            for k, v in over.items()}
    of, pl = nan_f32(r.n), nan_planes(PLANES[prec], r.n)
    with pytest.raises(RuntimeError, match=msg):
        launch(e, prec, r, out_f32=of, out_planes=pl, **over)
    torch.cuda.synchronize()
    assert torch.isnan(of).all() and (pl == SENT16).all(), f"ru_fused {name} {refusal[0]}: an output was written"


@by_variant
def test_ru_fused_refuses_no_output(eng, variant):
    name, prec = variant
    with pytest.raises(RuntimeError, match="ru_fused: refused"):
        launch(eng[prec], prec, ru_case((3, 27, 9, ELU, ELU), prec), f32=None, planes=False)
