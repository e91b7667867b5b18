"""The kernels that run between two score calls of every sampler, one launch wrapper at a time on caller-owned fp32
tensors (dsn_test_kernel), against float64 math of the same operation: the predictor and corrector updates, the prior
draws, the Langevin item norms, PriorMixSDE's running RMS, the Schroedinger-bridge step, the VAE latent sample and the
Philox generator (ditsep_amd/csrc/kernels.hip).

The formulas, their bounds and the check functions live in tests/sampler_kernels_ref.py (importable without a GPU:
tests/test_sampler_kernels_host.py feeds the same checks one mutated formula each), the generator's restatement in
tests/rng_restatement.py (pinned by tests/test_rng_host.py).

Bounds.  Update kernels: per element (R + 1) 2^-24 A, A the sum of the magnitudes of the formula's terms in float64 and
R the fp32 roundings on the longest path to the output, counted on the kernel's expression order with nothing contracted:
  pc_prior 2            pc_corrector xmean 2, x 3; Langevin form + 4 B + 9 (step and gain derived in fp32 from the norms)
  pc_predictor xmean 5, x 6 (both forms)               sb_update 3
  mix_prior n + 5       mix_corrector xmean n + 9, x n + 11       mix_predictor xmean n + 6, x n + 7
  sigma_mix avg_len + 3 (relative: every term is non-negative)
  vae_sample 7 (expf and log1pf at their documented 1 ulp = 2 units each, three more operations)
  pc_item_norms relative (ceil(per_item / 256) + 12) 2^-24        repeat_sources bit-exact
randn: |got - want| <= 24 2^-24 r against the restatement, r the radius of the value's pair (17 r derived in
sampler_kernels_ref.check_randn, the rest for a 2-ulp logf; float32 numpy reaches 7.3 r).  rand_uniform: one float32 ulp
of max(|lo|, |hi|), every value in [lo, hi].

Every output and in-place buffer carries a NaN tail that must survive, every input must come back bit-identical, and
each case prints its worst error over its bound.  Shapes: sampler_kernels_ref.SHAPES plus one case past the cap of
4096 blocks x 256 threads (1,048,576 work items), where the grid-stride loop runs: all of its elements are checked.

Figures of an MI355X, worst error over bound among all cases of a kernel (every case prints its own; the module prints
this table when its engine is closed): pc_prior 0.333, pc_corrector 0.462 (Langevin form 0.128), pc_item_norms 0.065,
pc_predictor 0.482, mix_prior 0.219, mix_corrector 0.164, mix_predictor 0.467, sb_update 0.616, sigma_mix 0.170,
vae_sample 0.244, rand_uniform 0.500 ulp.  randn: 0.302 of the bound, that is 7.25 r 2^-24 at worst (n = 2^23 across
the counter carry) -- what float32 numpy reaches on the same formula.
"""
import numpy as np
import pytest
import torch

from tests import rng_restatement as R
from tests import sampler_kernels_ref as K
from tests.test_gpu_gemm_kernels import DEV, FP16, TAIL, nan_f32
from tests.test_rng_host import LARGE, LARGE_ZERO_BLOCKS, UNIFORM_ONE
from tests.test_sampler_kernels_host import SIGMA_CASES, langevin_norms, sigma_inputs
from tests.util import make_engine

pytestmark = pytest.mark.gpu

SEED0 = 5150
S = K.SCAL

# worst error / bound per kernel over the cases that ran; printed when the module's engine is closed
DEVICE_FIGURES = {}


@pytest.fixture(scope="module")
def e():
    eng = make_engine(precision=FP16)
    yield eng
    eng.close()
    print("\nworst error / bound per kernel: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(DEVICE_FIGURES.items())))


def dv(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


def state(a):
    """an in-place buffer: the values followed by a NaN tail"""
    buf = nan_f32(a.size)
    buf[:a.size] = dv(a).reshape(-1)
    return buf


def read(buf, n, what):
    b = buf.cpu().numpy()
    assert np.isnan(b[n:]).all() and b.size == n + TAIL, f"{what}: written past its end"
    return b[:n].astype(np.float64)


class Inputs:
    """device copies of read-only inputs; same() asserts that the call left every one bit-identical"""

    def __init__(self, **arrs):
        self.host = {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in arrs.items() if v is not None}
        self.dev = {k: torch.from_numpy(v).to(DEV) for k, v in self.host.items()}

    def get(self, k):
        return self.dev.get(k)

    def same(self, what):
        for k, v in self.host.items():
            assert np.array_equal(self.dev[k].cpu().numpy().view(np.int32), v.view(np.int32)), f"{what}: input {k} changed"


def shape_id(s):
    return "x".join(map(str, s)) + ("-strides" if np.prod(s) > K.CAP else "")


ELEMENT_SHAPES = K.SHAPES + [K.STRIDE_ELEMENTS]
POSITION_SHAPES = K.SHAPES + [K.STRIDE_POSITIONS]
assert np.prod(K.STRIDE_ELEMENTS) > K.CAP and np.prod(K.STRIDE_POSITIONS) // K.STRIDE_POSITIONS[1] > K.CAP


def call(e, kind, i, outs, what, reads, *, xmean=None, out_only=False, **scal):
    """reads: which of y / score / z / smix the kernel is given.  xmean: True = pass a buffer, False = pass null and keep
    a sentinel buffer beside it, None = the kernel has no such argument."""
    B, n, D, T = i["x"].shape
    N = i["x"].size
    ro = Inputs(**{k: i["sc" if k == "score" else k] for k in reads})
    xb = nan_f32(N) if out_only else state(i["x"])
    xm = nan_f32(N) if xmean is not None else None
    kw = dict(x=xb, B=B, n=n, D=D, T=T, **{k: ro.get(k) for k in reads}, **scal)
    if xmean:
        kw["xmean"] = xm
    e.test_kernel(kind, **kw)
    torch.cuda.synchronize()
    got = {"x": read(xb, N, what + " x")}
    if xmean:
        got["xmean"] = read(xm, N, what + " xmean")
    elif xmean is False:
        assert torch.isnan(xm).all(), f"{what}: a buffer that was not passed was written"
        outs = {"x": outs["x"]}
    ro.same(what)
    if N > K.CAP:      # the grid-stride loop ran: what it wrote is finite (read) and right (below, every element)
        assert np.isfinite(got["x"][K.CAP:]).all() and got["x"][K.CAP:].size > 0
    return K.check_formula(got, outs, what)


def record(kernel, worst):
    DEVICE_FIGURES[kernel] = max(DEVICE_FIGURES.get(kernel, 0.0), worst)


# ================================================================================================ updates
@pytest.mark.parametrize("shape", ELEMENT_SHAPES, ids=shape_id)
def test_pc_prior(e, shape):
    for full in (0, 1):
        i = K.inputs(shape, SEED0 + full, full_mean=bool(full))
        w = call(e, "pc_prior", i, K.pc_prior(i, S), f"pc_prior {shape_id(shape)} mean_full {full}", ("y", "z"),
                 out_only=True, mean_full=full, stdT=S["stdT"])
        record("pc_prior", w)


@pytest.mark.parametrize("shape", ELEMENT_SHAPES, ids=shape_id)
def test_pc_corrector(e, shape):
    i = K.inputs(shape, SEED0 + 2)
    for xmean in (True, False):
        w = call(e, "pc_corrector", i, K.pc_corrector(i, S), f"pc_corrector {shape_id(shape)} xmean {xmean}",
                 ("score", "z"), xmean=xmean, step=S["step"], gain=S["gain"])
        record("pc_corrector", w)


@pytest.mark.parametrize("B", [1, 2, 5])
def test_pc_corrector_langevin(e, B):
    """step = 2 (snr mean|z| / mean|score|)^2 and gain = sqrt(2 step) from the norms on the device; the host scalars
    passed beside them are poison (NaN) that the Langevin form must not read"""
    i = K.inputs((B, 2, 32, 7), SEED0 + 10 + B)
    norms = langevin_norms(i)
    nd = Inputs(norms=norms)
    outs = K.pc_corrector(i, S, None, norms)
    w = call(e, "pc_corrector", i, outs, f"pc_corrector langevin B {B}", ("score", "z"), xmean=True,
             norms=nd.get("norms"), snr=S["snr"], step=float("nan"), gain=float("nan"))
    nd.same("langevin norms")
    record("pc_corrector langevin", w)


@pytest.mark.parametrize("shape", ELEMENT_SHAPES, ids=shape_id)
def test_pc_predictor(e, shape):
    i = K.inputs(shape, SEED0 + 3)
    for em in (0, 1):
        w = call(e, "pc_predictor", i, K.pc_predictor(i, S, em), f"pc_predictor {shape_id(shape)} em {em}",
                 ("y", "score", "z"), xmean=True, theta=S["theta"], dt=S["dt"], G=S["G"], g=S["g"], em=em)
        record("pc_predictor", w)


@pytest.mark.parametrize("shape", POSITION_SHAPES, ids=shape_id)
def test_mix_prior(e, shape):
    for smix in (False, True):
        i = K.inputs(shape, SEED0 + 4, smix=smix)
        w = call(e, "mix_prior", i, K.mix_prior(i, S), f"mix_prior {shape_id(shape)} smix {smix}",
                 ("y", "z") + (("smix",) if smix else ()), out_only=True, s1=S["s1"], s2=S["s2"])
        record("mix_prior", w)


@pytest.mark.parametrize("shape", POSITION_SHAPES, ids=shape_id)
def test_mix_corrector(e, shape):
    for smix in (False, True):
        i = K.inputs(shape, SEED0 + 5, smix=smix)
        w = call(e, "mix_corrector", i, K.mix_corrector(i, S), f"mix_corrector {shape_id(shape)} smix {smix}",
                 ("score", "z") + (("smix",) if smix else ()), xmean=not smix, s1=S["s1"], s2=S["s2"], snr=S["snr"])
        record("mix_corrector", w)


@pytest.mark.parametrize("shape", POSITION_SHAPES, ids=shape_id)
def test_mix_predictor(e, shape):
    for em in (0, 1):
        for smix in (False, True):
            if np.prod(shape) > K.CAP and smix != bool(em):
                continue                                   # the striding case: each em once, smix null and present
            i = K.inputs(shape, SEED0 + 6, smix=smix)
            w = call(e, "mix_predictor", i, K.mix_predictor(i, S, em), f"mix_predictor {shape_id(shape)} em {em} smix "
                     f"{smix}", ("score", "z") + (("smix",) if smix else ()), xmean=True, lam=S["lam"], dt=S["dt"],
                     g=S["g"], sqdt=S["sqdt"], em=em)
            record("mix_predictor", w)


@pytest.mark.parametrize("shape", ELEMENT_SHAPES, ids=shape_id)
def test_sb_update(e, shape):
    i = K.inputs(shape, SEED0 + 7)
    for third in (None, "y", "z"):
        reads = ("score",) + ((third,) if third else ())
        w = call(e, "sb_update", i, K.sb_update(i, S, third), f"sb_update {shape_id(shape)} third {third}", reads,
                 third_is_y=int(third == "y"), w_prev=S["w_prev"], w_est=S["w_est"], w3=S["w3"])
        record("sb_update", w)


@pytest.mark.parametrize("shape", ELEMENT_SHAPES, ids=shape_id)
def test_repeat_sources(e, shape):
    B, n, D, T = shape
    i = K.inputs(shape, SEED0 + 8)
    ro = Inputs(y=i["y"])
    xb = nan_f32(B * n * D * T)
    e.test_kernel("repeat_sources", x=xb, y=ro.get("y"), B=B, n=n, D=D, T=T)
    torch.cuda.synchronize()
    got = read(xb, B * n * D * T, "repeat_sources")
    ro.same("repeat_sources")
    assert np.array_equal(got.astype(np.float32).view(np.int32),
                          K.repeat_sources(i, n).astype(np.float32).reshape(-1).view(np.int32)), "repeat_sources: not y"


# ================================================================================================ norms, RMS, VAE sample
@pytest.mark.parametrize("per_item,offset", [(1, 0), (100, 0), (256, 0), (257, 0), (4099, 0), (1048583, 0), (4099, 100)],
                         ids=lambda v: str(v))
def test_pc_item_norms(e, per_item, offset):
    B = 3
    a = (np.random.default_rng(SEED0 + per_item).standard_normal((B, per_item)) + offset).astype(np.float32)
    ro = Inputs(a=a)
    out = nan_f32(B)
    e.test_kernel("pc_item_norms", x=ro.get("a"), count=per_item, B=B, out_f32=out)
    torch.cuda.synchronize()
    what = f"pc_item_norms per_item {per_item} offset {offset}"
    got = read(out, B, what)
    ro.same(what)
    record("pc_item_norms", K.check_norms(got, a.astype(np.float64), what))


@pytest.mark.parametrize("case", SIGMA_CASES, ids=lambda c: f"L{c[0]}-avg{c[1]}")
def test_sigma_mix(e, case):
    L, avg_len = case
    y = sigma_inputs(L, avg_len, SEED0 + L + avg_len)
    B = y.shape[0]
    ro = Inputs(y=y)
    out = nan_f32(B * L)
    e.test_kernel("sigma_mix", y=ro.get("y"), B=B, L=L, avg_len=avg_len, out_f32=out)
    torch.cuda.synchronize()
    what = f"sigma_mix L {L} avg_len {avg_len}"
    got = read(out, B * L, what)
    ro.same(what)
    want, A, Rn = K.sigma_mix(y, avg_len)
    assert (want[1] == 0.5 * 1e-2).all()                       # the clamp acts on the whole of item 1
    record("sigma_mix", K.check(got, want, A, Rn, what))


def test_vae_sample(e):
    Sq, D, T = 3, 32, 5
    enc, noise = K.vae_inputs(Sq, D, T, SEED0 + 9)
    assert {K.f32(v) for v in K.VAE_SCALES} <= set(enc[0, 0, D:].tolist())
    ro = Inputs(enc=enc, noise=noise)
    out = nan_f32(Sq * D * T)
    e.test_kernel("vae_sample", x=ro.get("enc"), z=ro.get("noise"), B=Sq, D=D, T=T, out_f32=out)
    torch.cuda.synchronize()
    got = read(out, Sq * D * T, "vae_sample")
    ro.same("vae_sample")
    want, A, Rn = K.vae_sample(enc, noise)
    record("vae_sample", K.check(got, want, A, Rn, "vae_sample"))


# ================================================================================================ generator
def draw(e, kind, n, seed, offset, **kw):
    out = nan_f32(n)
    e.test_kernel(kind, out_f32=out, count=n, seed=seed, offset=offset, **kw)
    torch.cuda.synchronize()
    return read(out, n, f"{kind} n {n} seed {seed:#x} offset {offset}")


@pytest.mark.parametrize("n", [1, 2, 3, 5, 1023, 4096])
def test_randn_small(e, n):
    """a seed with a non-zero high word; an odd tail (n % 4 != 0) leaves the NaN tail intact (draw -> read)"""
    seed = 0x1234567800000007
    got = draw(e, "randn", n, seed, 0)
    want, rad = R.randn(n, seed)
    record("randn", K.check_randn(got, want, rad, f"randn n {n}"))
    assert np.array_equal(got, draw(e, "randn", n, seed, 0)), "the same draw twice differs"


def test_randn_offset_is_the_tail_of_a_longer_draw(e):
    seed, k, n = 0xABCDEF0100000003, 37, 1001
    a = draw(e, "randn", n, seed, k)
    b = draw(e, "randn", 4 * k + n, seed, 0)
    assert np.array_equal(a.astype(np.float32).view(np.int32), b[4 * k:].astype(np.float32).view(np.int32))
    want, rad = R.randn(n, seed, k)
    record("randn", K.check_randn(a, want, rad, "randn offset 37"))


def test_randn_large_crosses_the_counter_carry(e):
    """seed 7, offset 2^32 - 1000, n = 2^23: the counter's low word wraps after block 999, the grid-stride loop runs
    (2^21 blocks of four values against 1,048,576 threads), and the pairs of the blocks LARGE_ZERO_BLOCKS have a radius
    uniform of exactly 1: the device must return +-0 there"""
    n = LARGE["n"]
    got = draw(e, "randn", n, LARGE["seed"], LARGE["offset"])
    want, rad = R.randn(n, LARGE["seed"], LARGE["offset"])
    for blk in LARGE_ZERO_BLOCKS:
        assert rad[4 * blk + 2] == 0 and got[4 * blk + 2] == 0 and got[4 * blk + 3] == 0
    assert n // 4 > K.CAP and np.isfinite(got[4 * K.CAP:]).all()
    record("randn", K.check_randn(got, want, rad, "randn 2^23 across the carry"))


def test_rand_uniform(e):
    for n, seed, offset, lo, hi in [(1, 5, 0, 0.03, 1.0), (4099, 0x9E3779B97F4A7C15 ^ 5, 0, 0.03, 1.0),
                                    (1000, 6, 2 ** 32 - 500, -2.0, 3.0)]:
        got = draw(e, "rand_uniform", n, seed, offset, lo=lo, hi=hi)
        want, _ = R.rand_uniform(n, seed, offset, lo, hi)
        record("rand_uniform", K.check_uniform(got, want, lo, hi, f"rand_uniform n {n} [{lo}, {hi}]"))
    seed, off = UNIFORM_ONE                      # word 0 of this block rounds to u = 1: exactly hi, not beyond
    for lo, hi in ((0.03, 1.0), (-2.0, 3.0), (0.1, 0.7)):
        got = draw(e, "rand_uniform", 3, seed, off - 1, lo=lo, hi=hi)
        assert got[1] == K.f32(hi) and got[0] < K.f32(hi) and got[2] < K.f32(hi)
        K.check_uniform(got, R.rand_uniform(3, seed, off - 1, lo, hi)[0], lo, hi, f"rand_uniform top draw [{lo}, {hi}]")


def test_rand_uniform_strides(e):
    n = K.CAP + 4099
    got = draw(e, "rand_uniform", n, 77, 0, lo=0.03, hi=1.0)
    want, _ = R.rand_uniform(n, 77, 0, 0.03, 1.0)
    record("rand_uniform", K.check_uniform(got, want, 0.03, 1.0, "rand_uniform past the cap"))


# ================================================================================================ refusals
def test_refusals_leave_every_buffer_alone(e):
    shape = (2, 2, 32, 7)
    B, n, D, T = shape
    i = K.inputs(shape, SEED0 + 20, smix=True)
    N = i["x"].size
    ro = Inputs(y=i["y"], score=i["sc"], z=i["z"], smix=i["smix"])
    x0 = i["x"].astype(np.float32)
    xb, xm, out = state(i["x"]), nan_f32(N), nan_f32(N)
    full = dict(x=xb, xmean=xm, y=ro.get("y"), score=ro.get("score"), z=ro.get("z"), B=B, n=n, D=D, T=T)

    def refused(kind, match, drop=(), **kw):
        args = {k: v for k, v in {**full, **kw}.items() if k not in drop}
        with pytest.raises(RuntimeError, match=match):
            e.test_kernel(kind, **args)

    needs = {"pc_prior": ("x", "y", "z"), "pc_corrector": ("x", "score", "z"), "pc_predictor": ("x", "xmean", "y", "score", "z"),
             "mix_prior": ("x", "y", "z"), "mix_corrector": ("x", "score", "z"), "mix_predictor": ("x", "xmean", "score", "z"),
             "sb_update": ("x", "score"), "repeat_sources": ("x", "y")}
    for kind, ptrs in needs.items():
        for p in ptrs:
            refused(kind, f"test_kernel {kind}: {p} missing", drop=(p,))
        for dim in ("B", "n", "D", "T"):
            for bad in (0, -1):
                refused(kind, f"test_kernel {kind}: B, n, D, T must be positive", **{dim: bad})
    # the mix_* kernels hold a position's sources in four-element arrays: n = 5 must never reach the device.  The
    # buffers are sized for n = 2, so a launch would also show in the sentinels.
    for kind in ("mix_prior", "mix_corrector", "mix_predictor"):
        refused(kind, f"test_kernel {kind}: n = 5 sources", n=5)
    e.test_kernel("pc_prior", **{**full, "n": 2, "stdT": 0.0, "x": out})       # (accepted; and n = 4 is, in the mix tests)
    refused("pc_item_norms", "pc_item_norms: B and count must be positive", drop=("xmean", "y", "score", "z", "n", "D", "T"),
            count=0, out_f32=out)
    refused("pc_item_norms", "pc_item_norms: B and count must be positive", drop=("xmean", "y", "score", "z", "n", "D", "T"),
            count=4, B=0, out_f32=out)
    refused("pc_item_norms", "pc_item_norms: x or out_f32 missing", drop=("xmean", "y", "score", "z", "n", "D", "T"), count=4)
    sig = dict(drop=("x", "xmean", "score", "z", "n", "D", "T"))
    refused("sigma_mix", "sigma_mix: avg_len 0 < 1", L=7, avg_len=0, out_f32=out, **sig)
    refused("sigma_mix", "sigma_mix: B and L must be positive", L=0, avg_len=3, out_f32=out, **sig)
    refused("sigma_mix", "sigma_mix: y or out_f32 missing", L=7, avg_len=3, **sig)
    vae = dict(drop=("xmean", "y", "score", "n"))
    refused("vae_sample", "vae_sample: B, D, T must be positive", D=0, out_f32=out, **vae)
    refused("vae_sample", "vae_sample: x \\(encoder output\\), z or out_f32 missing", **vae)
    rng = dict(drop=("x", "xmean", "y", "score", "z", "B", "n", "D", "T"))
    for kind in ("randn", "rand_uniform"):
        refused(kind, f"test_kernel {kind}: count 0 must be positive", count=0, out_f32=out, seed=1, **rng)
        refused(kind, f"test_kernel {kind}: count -3 must be positive", count=-3, out_f32=out, seed=1, **rng)
        refused(kind, f"test_kernel {kind}: out_f32 missing", count=5, seed=1, **rng)
    torch.cuda.synchronize()
    ro.same("refusals")
    assert torch.isnan(xm).all(), "a refused call wrote xmean"
    assert np.array_equal(read(xb, N, "refusals x").astype(np.float32).view(np.int32), x0.reshape(-1).view(np.int32)), \
        "a refused call wrote x"
    # `out` took the one accepted call (stdT = 0: the mean itself)
    assert np.array_equal(read(out, N, "accepted call"), K.pc_prior(i, dict(S, stdT=0.0))["x"][0].reshape(-1))
