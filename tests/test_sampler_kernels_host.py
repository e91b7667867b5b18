"""Sensitivity of the checks of tests/test_gpu_sampler_kernels.py, without a GPU: each check function is fed the float64
formula of tests/sampler_kernels_ref.py with ONE mutation, rounded to fp32 as a device would return it, and must refuse
it at every shape of the shape list; the unmutated formula, rounded the same way, must pass.

Three mutations are the identity at one shape each, which is asserted instead: the token-major and the channel-major
score index coincide when T = 1 ((b T + t) n D + s D + c = ((b n + s) D + c) T + t), there is no wrong item when B = 1,
and at L = 20 with avg_len = 50 every window of sigma_mix holds the whole item wherever it starts.
"""
import numpy as np
import pytest

from tests import rng_restatement as R
from tests import sampler_kernels_ref as K
from tests.test_rng_host import LARGE

SEED0 = 4321
SHAPE_IDS = ["x".join(map(str, s)) for s in K.SHAPES]


def device_like(outs):
    return {k: w.astype(np.float32).astype(np.float64) for k, (w, A, Rn) in outs.items()}


def must_fail(got, outs, what):
    with pytest.raises(AssertionError, match="beyond|not finite"):
        K.check_formula(got, outs, what)


# kernel -> (formula(i, mut), the mutations that apply to it)
def formulas(smix):
    s = K.SCAL
    return {
        "pc_prior": (lambda i, m: K.pc_prior(i, s, m), ["y_wrong_item"]),
        "pc_corrector": (lambda i, m: K.pc_corrector(i, s, m), ["score_channel_major", "gain_dropped"]),
        "pc_predictor_rd": (lambda i, m: K.pc_predictor(i, s, 0, m), ["score_channel_major", "y_wrong_item", "G_for_G2"]),
        "pc_predictor_em": (lambda i, m: K.pc_predictor(i, s, 1, m), ["score_channel_major", "y_wrong_item"]),
        "mix_prior": (lambda i, m: K.mix_prior(i, s, m), ["y_wrong_item", "mean_div_n_minus_1"]),
        "mix_corrector": (lambda i, m: K.mix_corrector(i, s, m),
                          ["score_channel_major", "mean_div_n_minus_1", "ald2_second_L_dropped"]),
        "mix_predictor_rd": (lambda i, m: K.mix_predictor(i, s, 0, m),
                             ["score_channel_major", "mean_div_n_minus_1", "G_for_G2"]),
        "mix_predictor_em": (lambda i, m: K.mix_predictor(i, s, 1, m), ["score_channel_major", "mean_div_n_minus_1"]),
        "sb_update_y": (lambda i, m: K.sb_update(i, s, "y", m),
                        ["score_channel_major", "y_wrong_item", "third_is_y_inverted"]),
        "sb_update_z": (lambda i, m: K.sb_update(i, s, "z", m), ["score_channel_major", "third_is_y_inverted"]),
    }


CASES = [(k, m) for k, (_, muts) in formulas(False).items() for m in muts]


@pytest.mark.parametrize("shape", K.SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("kernel,mut", CASES, ids=[f"{k}-{m}" for k, m in CASES])
def test_update_mutation_is_caught(kernel, mut, shape):
    B, n, D, T = shape
    for smix in ((False, True) if kernel.startswith("mix") else (False,)):
        i = K.inputs(shape, SEED0 + K.SHAPES.index(shape), smix=smix)
        fn = formulas(smix)[kernel][0]
        good = fn(i, None)
        K.check_formula(device_like(good), good, f"{kernel} unmutated")
        with np.errstate(invalid="ignore"):                   # (n - 1 = 0 sources: inf - inf)
            bad = device_like(fn(i, mut))
        if (mut == "score_channel_major" and T == 1) or (mut == "y_wrong_item" and B == 1):
            assert all(np.array_equal(bad[k], device_like(good)[k]) for k in bad), "expected the identity at this shape"
            continue
        with np.errstate(invalid="ignore"):
            must_fail(bad, good, f"{kernel} {mut}")


@pytest.mark.parametrize("shape", K.SHAPES, ids=SHAPE_IDS)
def test_repeat_sources_wrong_item(shape):
    B, n, D, T = shape
    i = K.inputs(shape, SEED0)
    good, bad = K.repeat_sources(i, n), K.repeat_sources(i, n, "y_wrong_item")
    assert np.array_equal(good, bad) == (B == 1)


@pytest.mark.parametrize("B", [1, 2, 5])
def test_langevin_form_mutations(B):
    shape = (B, 2, 32, 7)
    i = K.inputs(shape, SEED0 + B)
    norms = langevin_norms(i)
    good = K.pc_corrector(i, K.SCAL, None, norms)
    K.check_formula(device_like(good), good, "langevin unmutated")
    must_fail(device_like(K.pc_corrector(i, K.SCAL, "gain_dropped", norms)), good, "langevin gain dropped")
    swapped = np.concatenate([norms[B:], norms[:B]])      # the two halves of norms read the other way round
    if B > 1:                                             # (one item: |z| / |s| against |s| / |z|, off by some percent)
        must_fail(device_like(K.pc_corrector(i, K.SCAL, None, swapped)), good, "langevin norms swapped")


def langevin_norms(i):
    B = i["x"].shape[0]
    sn = np.sqrt((i["sc"].reshape(B, -1) ** 2).sum(1))
    zn = np.sqrt((i["z"].reshape(B, -1) ** 2).sum(1))
    return np.concatenate([sn, 1.3 * zn]).astype(np.float32).astype(np.float64)


SIGMA_CASES = [(37, 1), (37, 8), (37, 9), (20, 50), (448, 50)]


def sigma_inputs(L, avg_len, seed):
    """three items, the middle one at 1e-3 so that the 1e-4 clamp acts on it"""
    y = np.random.default_rng(seed).standard_normal((3, L))
    y[1] *= 1e-3
    return y.astype(np.float32).astype(np.float64)


@pytest.mark.parametrize("case", SIGMA_CASES, ids=lambda c: f"L{c[0]}-avg{c[1]}")
def test_sigma_mix_mutations(case):
    L, avg_len = case
    y = sigma_inputs(L, avg_len, SEED0 + L + avg_len)
    want, A, Rn = K.sigma_mix(y, avg_len)
    assert (want[1] == 0.5 * 1e-2).all() and (want[0] > 0.5 * 1e-2).any()          # the clamp acts on item 1 only
    K.check(want.astype(np.float32), want, A, Rn, "sigma_mix unmutated")
    for mut in ("window_shifted", "no_clamp"):
        bad = K.sigma_mix(y, avg_len, mut)[0].astype(np.float32)
        if mut == "window_shifted" and L <= avg_len // 2:       # every window holds the whole item, shifted or not
            assert np.array_equal(bad, want.astype(np.float32))
            continue
        with pytest.raises(AssertionError, match="beyond"):
            K.check(bad, want, A, Rn, f"sigma_mix {mut}")


def test_sigma_mix_window_restatement_agrees_with_avg_pool():
    """the cumulative-sum window that carries the shift mutation is avg_pool1d when it is not shifted"""
    y = sigma_inputs(37, 8, 5)
    B, L, k = 3, 37, 8
    sq = np.concatenate([np.zeros((B, k)), y * y, np.zeros((B, k))], 1)
    manual = np.stack([sq[:, l - k // 2 + k:l - k // 2 + 2 * k].sum(1) / k for l in range(L)], 1)
    want = 0.5 * np.sqrt(np.maximum(manual, 1e-4))
    assert np.abs(K.sigma_mix(y, k)[0] - want).max() <= 1e-15
    shifted = np.stack([sq[:, l - k // 2 + k + 1:l - k // 2 + 2 * k + 1].sum(1) / k for l in range(L)], 1)
    assert np.abs(K.sigma_mix(y, k, "window_shifted")[0] - 0.5 * np.sqrt(np.maximum(shifted, 1e-4))).max() <= 1e-15


def test_vae_sample_threshold_mutation():
    enc, noise = K.vae_inputs(3, 32, 5, SEED0)
    want, A, Rn = K.vae_sample(enc, noise)
    K.check(want.astype(np.float32), want, A, Rn, "vae_sample unmutated")
    with pytest.raises(AssertionError, match="beyond"):
        K.check(K.vae_sample(enc, noise, "softplus_threshold_0")[0].astype(np.float32), want, A, Rn, "vae_sample threshold 0")


@pytest.mark.parametrize("n", [1, 2, 3, 5, 1023, 4096])
@pytest.mark.parametrize("mut", ["sincos_swapped", "no_key_bump"])
def test_randn_mutations(mut, n):
    want, rad = R.randn(n, 0x1234567800000007)
    K.check_randn(want.astype(np.float32), want, rad, "randn unmutated")
    bad = R.randn(n, 0x1234567800000007, mutate=mut)[0].astype(np.float32)
    with pytest.raises(AssertionError, match="beyond"):
        K.check_randn(bad, want, rad, f"randn {mut}")


def test_randn_float32_evaluation_passes():
    """the kernel's formula evaluated in float32 numpy stays within the bound (7.3 r measured over three seeds at 2^23)"""
    n = 1 << 20
    want, rad = R.randn(n, 7)
    u = [R.to_uniform(w) for w in R.blocks(0, n // 4, 7, 0)]
    tw = np.float32(6.283185307179586)
    out = np.empty((n // 4, 4), np.float32)
    for p in (0, 1):
        r = np.sqrt(np.float32(-2) * np.log(u[2 * p]))
        out[:, 2 * p], out[:, 2 * p + 1] = r * np.cos(tw * u[2 * p + 1]), r * np.sin(tw * u[2 * p + 1])
    assert K.check_randn(out.reshape(-1), want, rad, "randn in float32 numpy") < 0.5


def test_randn_carry_mutation():
    """the counter's high word dropped shows only past the 32-bit carry: the large case's first 8192 values cross it"""
    n = 8192
    want, rad = R.randn(n, LARGE["seed"], LARGE["offset"])
    bad = R.randn(n, LARGE["seed"], LARGE["offset"], mutate="ctr_hi_dropped")[0]
    assert np.array_equal(bad[:4000], want[:4000])
    with pytest.raises(AssertionError, match="beyond"):
        K.check_randn(bad.astype(np.float32), want, rad, "randn counter high word dropped")
    # and a draw that stays below the carry cannot tell
    w2, r2 = R.randn(n, LARGE["seed"], 5)
    K.check_randn(R.randn(n, LARGE["seed"], 5, mutate="ctr_hi_dropped")[0].astype(np.float32), w2, r2, "below the carry")


def test_uniform_mutation():
    want, _ = R.rand_uniform(4096, 99, 3, 0.03, 1.0)
    K.check_uniform(want.astype(np.float32), want, 0.03, 1.0, "uniform unmutated")
    bad = R.rand_uniform(4096, 99, 3, 0.03, 1.0, mutate="no_key_bump")[0]
    with pytest.raises(AssertionError, match="off by"):
        K.check_uniform(bad.astype(np.float32), want, 0.03, 1.0, "uniform key bump omitted")


def test_item_norm_check_catches_a_dropped_tail():
    a = np.random.default_rng(3).standard_normal((2, 4099)).astype(np.float32).astype(np.float64)
    K.check_norms(np.sqrt((a * a).sum(1)).astype(np.float32), a, "norms")
    with pytest.raises(AssertionError, match="beyond"):
        K.check_norms(np.sqrt((a[:, :4096] ** 2).sum(1)).astype(np.float32), a, "norms without the last 3 values")
