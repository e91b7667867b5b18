"""float64 formulas, rounding counts and check functions for the sampler's kernels between two score calls
(ditsep_amd/csrc/kernels.hip), shared by tests/test_gpu_sampler_kernels.py (the device against them) and
tests/test_sampler_kernels_host.py (the checks against one mutation of a formula each).  No GPU is needed to import it.

Layouts: x, z, xmean [B,n,D,T]; y [B,D,T] (the reference's [B,1,D,T]); score token-major [B,T,n,D]; smix [B,D,T].
Every formula works on float64 copies of the fp32 inputs and of the fp32 scalars, and returns for each output
(want, A, R): the float64 value, the sum A of the absolute values of the formula's terms, and the number R of fp32
roundings on the longest path to that output when nothing is contracted to a fused multiply-add (contraction only
removes roundings).  The bound of an element is (R + 1) 2^-24 A: every intermediate is a partial sum of the terms, so
each rounding costs at most 2^-24 A, and the + 1 pays for the second-order terms.  R is derived in the docstring of each
formula from the kernel's own expression order, not from what a device returns.
"""
import math

import numpy as np

U = 2.0 ** -24
CAP = 4096 * 256                      # grid_for: 4096 blocks of 256 threads, beyond it the grid-stride loop runs

# (B, n, D, T): D != T, distinct sources, n = 1 .. 4, T = 1, odd and prime T
SHAPES = [(2, 2, 32, 7), (3, 1, 64, 1), (2, 3, 96, 13), (1, 4, 32, 9)]
STRIDE_ELEMENTS = (2, 3, 64, 2741)    # 1,052,544 elements
STRIDE_POSITIONS = (2, 2, 64, 8200)   # 1,049,600 positions of the per-position mix_* kernels


def f32(v):
    """the value a float scalar has once it is passed to the device"""
    return float(np.float32(v))


# every term of every formula within a factor of ten of the largest
SCAL = {k: f32(v) for k, v in dict(stdT=0.7, step=0.02, gain=0.2, snr=0.5, theta=1.5, dt=1 / 30, G=0.3, g=1.7, s1=0.8,
                                   s2=0.45, lam=2.0, sqdt=math.sqrt(1 / 30), w_prev=0.6, w_est=0.35, w3=0.25).items()}


def inputs(shape, seed, smix=False, full_mean=False):
    """unit-scale fp32 inputs (as float64 arrays holding fp32 values) of a case; the score at unit scale too"""
    B, n, D, T = shape
    g = np.random.default_rng(seed)
    r = lambda *s: g.standard_normal(s).astype(np.float32).astype(np.float64)
    i = dict(x=r(B, n, D, T), y=r(B, n, D, T) if full_mean else r(B, D, T), z=r(B, n, D, T), sc=r(B, T, n, D))
    i["smix"] = (0.5 + g.random((B, D, T))).astype(np.float32).astype(np.float64) if smix else None
    return i


def score_of(i, mut=None):
    """the score in the state's layout [B,n,D,T]"""
    B, T, n, D = i["sc"].shape
    if mut == "score_channel_major":
        return i["sc"].reshape(B, n, D, T)
    return i["sc"].transpose(0, 2, 3, 1)


def y_of(i, mut=None):
    y = i["y"]
    if mut == "y_wrong_item":
        y = np.roll(y, -1, axis=0)
    return y[:, None] if y.ndim == 3 else y


def src_mean(v, mut=None):
    """(mean over the sources, sum of its terms' magnitudes): n adds and one divide"""
    n = v.shape[1]
    d = (n - 1) if mut == "mean_div_n_minus_1" else n
    with np.errstate(divide="ignore", invalid="ignore"):
        return v.sum(1, keepdims=True) / d, np.abs(v).sum(1, keepdims=True) / n


def pc_prior(i, s, mut=None):
    """x = mean + z stdT: the product and the sum, R = 2"""
    y, t = y_of(i, mut), i["z"] * s["stdT"]
    return {"x": (y + t, np.abs(y) + np.abs(t), 2)}


def langevin_scalars(norms, snr):
    """float64 step and gain of the Langevin corrector from the per-item norms [2 B] (score, then noise)"""
    B = norms.size // 2
    q = snr * (norms[B:].sum() / B) / (norms[:B].sum() / B)
    step = 2 * q * q
    return step, math.sqrt(2 * step)


def pc_corrector(i, s, mut=None, norms=None):
    """xmean = x + step score (R = 2), x = xmean + z gain (R = 3).  With norms the device derives step and gain in fp32:
    each batch mean is B adds and a divide, q = snr mean / mean adds a product and a divide (2 B + 4 roundings),
    step = 2 q q doubles that and adds one (4 B + 9; the factor 2 is exact), gain = sqrt(2 step) halves it and adds one.
    The step's error rides on the score term: R = 4 B + 9 + 2 for xmean and 4 B + 9 + 3 for x."""
    step, gain, extra = s["step"], s["gain"], 0
    if norms is not None:
        step, gain = langevin_scalars(norms, s["snr"])
        extra = 4 * (norms.size // 2) + 9
    if mut == "gain_dropped":
        gain = 1.0
    a, b = step * score_of(i, mut), gain * i["z"]
    Am = np.abs(i["x"]) + np.abs(a)
    return {"xmean": (i["x"] + a, Am, 2 + extra), "x": (i["x"] + a + b, Am + np.abs(b), 3 + extra)}


def pc_predictor(i, s, em, mut=None):
    """em = 0: f = theta (y - x) dt (3 roundings), G2 = G G (1), rev = f - G2 score (4), xmean = x - rev (5),
    x = xmean + G z (6).  em = 1: g2 = g g, drift = theta (y - x) + (-g2 score) (3), drift (-dt) (4), xmean = x + . (5),
    x = xmean + G z (6).  R = 5 / 6 either way."""
    x, y, sc = i["x"], y_of(i, mut), score_of(i, mut)
    if em:
        g2 = s["g"] * s["g"]
        xm = x + (s["theta"] * (y - x) - g2 * sc) * (-s["dt"])
        Am = np.abs(x) + s["dt"] * (s["theta"] * (np.abs(y) + np.abs(x)) + g2 * np.abs(sc))
    else:
        G2 = s["G"] if mut == "G_for_G2" else s["G"] * s["G"]
        xm = x - (s["theta"] * (y - x) * s["dt"] - G2 * sc)
        Am = np.abs(x) + s["theta"] * s["dt"] * (np.abs(y) + np.abs(x)) + G2 * np.abs(sc)
    nz = s["G"] * i["z"]
    return {"xmean": (xm, Am, 5), "x": (xm + nz, Am + np.abs(nz), 6)}


def smix_of(i):
    return 1.0 if i["smix"] is None else i["smix"][:, None]


def mix_prior(i, s, mut=None):
    """x = 0.5 y + (s1 sm) mz + (s2 sm) (z - mz).  mz: n + 1 roundings; z - mz: n + 2; times (s2 sm), itself rounded
    beside it: n + 3; the two sums of the output: R = n + 5 (0.5 y is exact; the s1 path is one shorter)."""
    n = i["z"].shape[1]
    sm, y, z = smix_of(i), y_of(i, mut), i["z"]
    mz, Az = src_mean(z, mut)
    want = 0.5 * y + (s["s1"] * sm) * mz + (s["s2"] * sm) * (z - mz)
    A = 0.5 * np.abs(y) + np.abs(s["s1"] * sm) * Az + np.abs(s["s2"] * sm) * (np.abs(z) + Az)
    return {"x": (want, A, n + 5)}


def mix_corrector(i, s, mut=None):
    """a1 = sq1 sm, a2 = sq2 sm (1 each); ms, mz (n + 1).  u = a1 ms + a2 (s - ms): n + 4.  grad = a1 (a1 ms) +
    a2 (u - a1 ms): the difference n + 5, its product n + 6, the sum n + 7.  xmean = x + (2 snr snr) grad: n + 9.
    x = xmean + (2 snr a1) mz + (2 snr a2) (z - mz): two more sums, n + 11."""
    n = i["z"].shape[1]
    sm, x, z, sv = smix_of(i), i["x"], i["z"], score_of(i, mut)
    a1, a2, snr = s["s1"] * sm, s["s2"] * sm, s["snr"]
    ms, As = src_mean(sv, mut)
    mz, Az = src_mean(z, mut)
    u = a1 * ms + a2 * (sv - ms)
    Au = a1 * As + a2 * (np.abs(sv) + As)
    if mut == "ald2_second_L_dropped":
        grad, Ag = u, Au
    else:
        grad = a1 * (a1 * ms) + a2 * (u - a1 * ms)
        Ag = a1 * a1 * As + a2 * (Au + a1 * As)
    xm = x + 2 * snr * snr * grad
    Am = np.abs(x) + 2 * snr * snr * Ag
    xn = xm + (2 * snr * a1) * mz + (2 * snr * a2) * (z - mz)
    Ax = Am + 2 * snr * a1 * Az + 2 * snr * a2 * (np.abs(z) + Az)
    return {"xmean": (xm, Am, n + 9), "x": (xn, Ax, n + 11)}


def mix_predictor(i, s, em, mut=None):
    """mx: n + 1; x - mx: n + 2; times -lambda: n + 3.  em = 0: times dt (n + 4), rev = f - (G G) score (n + 5, G =
    (g sm) sqdt), xmean = x - rev (n + 6), x = xmean + G z (n + 7).  em = 1: drift = -lambda (x - mx) - (gs gs) score
    (n + 4), times -dt (n + 5), xmean (n + 6), x (n + 7)."""
    n = i["z"].shape[1]
    sm, x, z, sc = smix_of(i), i["x"], i["z"], score_of(i, mut)
    mx, Ax = src_mean(x, mut)
    gs = s["g"] * sm
    with np.errstate(invalid="ignore"):
        if em:
            xm = x + (-s["lam"] * (x - mx) - gs * gs * sc) * (-s["dt"])
            Am = np.abs(x) + s["dt"] * (s["lam"] * (np.abs(x) + Ax) + gs * gs * np.abs(sc))
        else:
            G = gs * s["sqdt"]
            G2 = G if mut == "G_for_G2" else G * G
            xm = x - (-s["lam"] * (x - mx) * s["dt"] - G2 * sc)
            Am = np.abs(x) + s["lam"] * s["dt"] * (np.abs(x) + Ax) + G2 * np.abs(sc)
    nz = gs * s["sqdt"] * z
    return {"xmean": (xm, Am, n + 6), "x": (xm + nz, Am + np.abs(nz), n + 7)}


def sb_update(i, s, third, mut=None):
    """x = w_prev x + w_est est + w3 third: three products beside each other and two sums, R = 3.  third: None, "y", "z" """
    if mut == "third_is_y_inverted" and third is not None:
        third = "z" if third == "y" else "y"
    a, b = s["w_prev"] * i["x"], s["w_est"] * score_of(i, mut)
    if third is None:
        c = 0.0
    elif third == "y":
        c = s["w3"] * y_of(i, mut)
    else:
        c = s["w3"] * i["z"]
    return {"x": (a + b + c, np.abs(a) + np.abs(b) + np.abs(c), 3)}


def repeat_sources(i, n, mut=None):
    y = y_of(i, mut)
    return np.broadcast_to(y, (y.shape[0], n) + y.shape[2:]).copy()


def sigma_mix(y, avg_len, mut=None):
    """y [B, L] -> 0.5 sqrt(clamp(avg_pool1d(y^2, avg_len, 1, avg_len // 2, count_include_pad=True)[..., :L], 1e-4)).
    Every term is non-negative: the squares (1 rounding), avg_len sums, the divide, the square root (which halves what
    came before) and nothing for the exact 0.5: relative, R = avg_len + 3."""
    import torch
    import torch.nn.functional as F

    B, L = y.shape
    if mut == "window_shifted":
        pad = avg_len // 2
        sq = np.concatenate([np.zeros((B, avg_len + 1)), y * y, np.zeros((B, avg_len + 1))], 1)
        cs = np.concatenate([np.zeros((B, 1)), np.cumsum(sq, 1)], 1)
        lo = np.arange(L) - pad + 1 + avg_len + 1
        pooled = (cs[:, lo + avg_len] - cs[:, lo]) / avg_len
    else:
        t = torch.from_numpy(y * y)[:, None]
        pooled = F.avg_pool1d(t, avg_len, 1, avg_len // 2, count_include_pad=True)[..., :L][:, 0].numpy()
    if mut != "no_clamp":
        pooled = np.maximum(pooled, 1e-4)
    want = 0.5 * np.sqrt(pooled)
    return want, want, avg_len + 3


def softplus64(s, threshold=20.0):
    with np.errstate(over="ignore"):
        return np.where(s > threshold, s, np.log1p(np.exp(np.minimum(s, 700.0))))


VAE_SCALES = (-100.0, -20.0, 0.0, 19.99, 20.0, 20.01, 60.0)


def vae_inputs(S, D, T, seed):
    """enc [S][T][2 D] (mean ++ scale), noise [S, D, T]; the listed scales planted in the first rows of item 0, the rest
    drawn from 3 N(0, 1) so that both sides of 0 and the whole softplus knee occur"""
    g = np.random.default_rng(seed)
    enc = g.standard_normal((S, T, 2 * D))
    enc[:, :, D:] *= 3.0
    enc[0, 0, D:D + len(VAE_SCALES)] = VAE_SCALES
    enc[S - 1, T - 1, 2 * D - len(VAE_SCALES):] = VAE_SCALES
    noise = g.standard_normal((S, D, T))
    return enc.astype(np.float32).astype(np.float64), noise.astype(np.float32).astype(np.float64)


def vae_sample(enc, noise, mut=None):
    """y = noise (softplus(scale) + 1e-4) + mean with softplus(s) = s beyond 20.  expf and log1pf are documented at one
    ulp, two units of 2^-24 each, and the softplus passes its argument's relative error on with a factor below one;
    then the sum with 1e-4, the product and the sum: R = 7.  A result of expf below the smallest normal float may be
    flushed to zero: 2^-126 |noise| on top."""
    S, T, D2 = enc.shape
    D = D2 // 2
    mean, scale = enc[:, :, :D].transpose(0, 2, 1), enc[:, :, D:].transpose(0, 2, 1)
    sp = softplus64(scale, 0.0 if mut == "softplus_threshold_0" else 20.0)
    want = noise * (sp + 1e-4) + mean
    A = np.abs(noise) * (sp + 1e-4) + np.abs(mean) + 2.0 ** -126 * np.abs(noise) / (8 * U)   # (8 = R + 1)
    return want, A, 7


# ------------------------------------------------------------------------------------------------ checks
def check(got, want, A, R, what):
    """every element finite and within (R + 1) 2^-24 A of the float64 formula; -> worst error over its bound"""
    want = np.asarray(want, np.float64)
    bound = (R + 1) * U * np.broadcast_to(np.asarray(A, np.float64), want.shape).reshape(-1)
    got, want = np.asarray(got, np.float64).reshape(-1), want.reshape(-1)
    assert got.shape == want.shape, f"{what}: {got.shape} values, {want.shape} expected"
    assert np.isfinite(got).all(), f"{what}: {int((~np.isfinite(got)).sum())} values are not finite (or were not written)"
    err = np.abs(got - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err == 0, 0.0, err / bound)
    worst = float(ratio.max())
    print(f"{what}: worst error / bound {worst:.3f} (R = {R}, {got.size} values)")
    assert worst <= 1.0, f"{what}: {int((ratio > 1).sum())} of {got.size} values beyond (R + 1) 2^-24 A, worst " \
                         f"{worst:.3g} x the bound at flat index {int(ratio.argmax())}"
    return worst


def check_formula(got, outs, what):
    """got: {name: values}; outs: what a formula above returned"""
    return max(check(got[k], w, A, R, f"{what} {k}") for k, (w, A, R) in outs.items())


def check_norms(got, a, what):
    """a [B, per_item] float64 of fp32 values.  The squares are non-negative, so the sum's relative error is at most the
    number of additions a term passes through: ceil(per_item / 256) in a thread's serial run, 6 shuffles, 4 waves, and
    the product: (ceil(per_item / 256) + 12) 2^-24 (the square root halves it; the bound is kept un-halved)."""
    per_item = a.shape[1]
    want = np.sqrt((a * a).sum(1))
    return check(got, want, want, -(-per_item // 256) + 11, what)


def check_randn(got, want, rad, what):
    """|got - want| <= 24 2^-24 r, r the radius sqrt(-2 ln u) of the value's pair: the angle 2 pi u carries at most 9.4
    units of 2^-24 (the rounded 2 pi and the product's rounding at up to 2 pi), sin / cos up to 4, r 2, the final product
    1: 17 r; the margin to 24 covers a 2-ulp device logf.  A pair of radius 0 must be exactly +-0."""
    return check(got, want, rad, 23, what)


def ulp32(v):
    return 2.0 ** (math.floor(math.log2(abs(v))) - 23)


def check_uniform(got, want, lo, hi, what):
    """within one float32 ulp of max(|lo|, |hi|) of the restatement (the multiply-add may or may not be fused), and
    inside [lo, hi]"""
    got = np.asarray(got, np.float64)
    assert np.isfinite(got).all(), f"{what}: values not finite (or not written)"
    assert (got >= f32(lo)).all() and (got <= f32(hi)).all(), f"{what}: values outside [lo, hi]"
    err = float(np.abs(got - want).max()) / ulp32(max(abs(lo), abs(hi)))
    print(f"{what}: worst error {err:.3f} ulp of max(|lo|, |hi|)")
    assert err <= 1.0, f"{what}: off by {err:.3g} ulp of max(|lo|, |hi|)"
    return err
