"""The numpy restatement of the device generator (tests/rng_restatement.py), pinned on the CPU: the published
Philox4x32-10 vectors, and the properties that a bit-level comparison of the device against the restatement
(tests/test_gpu_sampler_kernels.py) cannot give -- the distribution of the normals, the independence of the four outputs
of a block, of neighbouring values and of the streams the engine derives from one seed.

Every statistic is held to five standard errors of its own sampling distribution under the hypothesis (independent
standard normals), n = 2^22:
  mean                       1 / sqrt(n)
  variance                   sqrt(2 / n)
  fourth moment              sqrt((E z^8 - 9) / n) = sqrt(96 / n)
  ECDF at q                  sqrt(Phi(q) (1 - Phi(q)) / n)
  a correlation of m pairs   1 / sqrt(m)
Figures of the restatement, seed 123: mean -4.0e-4, variance 1.00019, fourth moment 3.0000, sqrt(n) |ECDF - Phi| at most
0.91 over q = -3 .. 3 in steps of 0.25 (0.44 at the integers), correlations (values and squares) inside a block at most 2.2e-3 (m = 2^20), lag 1 -7.9e-4.
"""
import math

import numpy as np
import pytest

from tests import rng_restatement as R

N = 1 << 22
SEED = 123
# found by scanning word 0 of the blocks of seed 11 on the CPU: (word >> 8) == 2^24 - 1, the uniform rounds to 1
UNIFORM_ONE = (11, 858091)
# the large device case (seed 7, offset 2^32 - 1000, n = 2^23): blocks whose word 2 gives a radius uniform of exactly 1
LARGE = dict(seed=7, offset=2 ** 32 - 1000, n=1 << 23)
LARGE_ZERO_BLOCKS = (36425, 1095650)


@pytest.fixture(scope="module")
def z():
    return R.randn(N, SEED)[0]


def corr(a, b):
    a, b = a - a.mean(), b - b.mean()
    return float((a * b).mean() / math.sqrt((a * a).mean() * (b * b).mean()))


def test_philox_known_answers():
    """Random123's kat_vectors for philox4x32 with 10 rounds"""
    hx = lambda w: " ".join("%08x" % int(x[0]) for x in w)
    assert hx(R.philox4x32_10((0, 0, 0, 0), (0, 0))) == "6627e8d5 e169c58d bc57ac4c 9b00dbd8"
    assert hx(R.philox4x32_10((0xFFFFFFFF,) * 4, (0xFFFFFFFF, 0xFFFFFFFF))) == "408f276d 41c83b0e a20bc7c6 6d5451fd"
    assert hx(R.philox4x32_10((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0))) == \
        "d16cfe09 94fdcceb 5001e420 24126ea1"


def test_counter_and_key_layout():
    """block i of (seed, offset) is Philox of counter {lo, hi of i + offset, 0, 0} under key {lo, hi of seed}"""
    seed, offset = 0x0123456789ABCDEF, (1 << 32) - 2
    w = R.blocks(0, 4, seed, offset)
    for i in range(4):
        c = i + offset
        one = R.philox4x32_10((c & 0xFFFFFFFF, c >> 32, 0, 0), (seed & 0xFFFFFFFF, seed >> 32))
        assert [int(x[i]) for x in w] == [int(x[0]) for x in one]
    # offset k: the same blocks as the tail of a draw from offset 0
    a, _ = R.randn(40, seed, offset=5)
    b, _ = R.randn(60, seed, offset=0)
    assert np.array_equal(a, b[20:])


def test_uniform_mapping():
    w = np.array([0, 255, 256, 0xFFFFFEFF, 0xFFFFFF00, 0xFFFFFFFF], np.uint32)
    u = R.to_uniform(w)
    assert u.dtype == np.float32
    assert float(u[0]) == 2.0 ** -25 and float(u[1]) == 2.0 ** -25 and float(u[2]) == 1.5 * 2.0 ** -24
    assert float(u[3]) == 1.0 - 2.0 ** -23            # 2^24 - 1.5 rounds to even: 2^24 - 2
    assert float(u[4]) == 1.0 and float(u[5]) == 1.0  # 2^24 - 0.5 rounds to 2^24
    assert (u > 0).all() and (u <= 1).all()


def test_moments(z):
    n = z.size
    mean, var, m4 = float(z.mean()), float(z.var()), float((z ** 4).mean())
    print(f"mean {mean:.2e} variance {var:.5f} fourth moment {m4:.4f}")
    assert abs(mean) <= 5 / math.sqrt(n)
    assert abs(var - 1) <= 5 * math.sqrt(2 / n)
    assert abs(m4 - 3) <= 5 * math.sqrt(96 / n)


def test_distribution_function(z):
    n = z.size
    zs = np.sort(z)
    worst = 0.0
    for q in np.arange(-3.0, 3.01, 0.25):
        phi = 0.5 * math.erfc(-q / math.sqrt(2))
        d = abs(np.searchsorted(zs, q) / n - phi)
        worst = max(worst, math.sqrt(n) * d)
        assert d <= 5 * math.sqrt(phi * (1 - phi) / n), f"ECDF at {q}: off by {d:.2e}"
    print(f"sqrt(n) |ECDF - Phi| at most {worst:.2f}")


def test_outputs_of_a_block_are_uncorrelated(z):
    b = z.reshape(-1, 4)
    m = b.shape[0]
    worst = 0.0
    for i in range(4):
        for j in range(i + 1, 4):
            for f in (lambda v: v, np.square):         # the pair (r cos, r sin) shares its radius: squares too
                c = corr(f(b[:, i]), f(b[:, j]))
                worst = max(worst, abs(c))
                assert abs(c) <= 5 / math.sqrt(m), f"outputs {i}, {j}: correlation {c:.2e}"
    print(f"worst correlation inside a block {worst:.2e}")


def test_neighbours_are_uncorrelated(z):
    for lag in (1, 4, 1024):
        c = corr(z[:-lag], z[lag:])
        assert abs(c) <= 5 / math.sqrt(z.size - lag), f"lag {lag}: correlation {c:.2e}"


def test_streams_of_one_seed_are_independent(z):
    """seed and seed + 1, and the three streams engine.hip derives from one seed (sampler, encoder noise, loss times)"""
    for other in (SEED + 1, SEED ^ R.SEED_ENCODER, SEED ^ R.SEED_LOSS_T):
        o = R.randn(N, other)[0]
        c = corr(z, o)
        assert abs(c) <= 5 / math.sqrt(N), f"seed {SEED} against {other:#x}: correlation {c:.2e}"
        assert not np.array_equal(z[:64], o[:64])
    enc, tl = R.randn(N, SEED ^ R.SEED_ENCODER)[0], R.randn(N, SEED ^ R.SEED_LOSS_T)[0]
    assert abs(corr(enc, tl)) <= 5 / math.sqrt(N)
    # the loss times are uniforms of word 0: against the normals of the sampler's stream built from the same blocks
    u = R.rand_uniform(N // 4, SEED ^ R.SEED_LOSS_T, 0, 0.03, 1.0)[0]
    assert abs(corr(u, z[::4])) <= 5 / math.sqrt(N // 4)


def test_uniform_range_and_top_draw():
    v, u = R.rand_uniform(1 << 20, SEED, 0, 0.03, 1.0)
    assert (v >= 0.03).all() and (v <= 1.0).all()
    m = float(u.astype(np.float64).mean())
    assert abs(m - 0.5) <= 5 * math.sqrt(1 / 12 / u.size)
    seed, off = UNIFORM_ONE
    v, u = R.rand_uniform(3, seed, off - 1, -2.0, 3.0)
    assert float(u[1]) == 1.0 and float(v[1]) == 3.0 and float(u[0]) < 1.0 and float(u[2]) < 1.0


def test_large_case_crosses_the_carry_and_holds_exact_zeros():
    """what the device's large case relies on: the counter's low word wraps inside the draw, dropping the high word
    changes the values from there on, and two pairs have a radius of exactly 0"""
    nb = LARGE["n"] // 4
    w = R.blocks(0, nb, LARGE["seed"], LARGE["offset"])
    assert LARGE["offset"] + nb > 2 ** 32 > LARGE["offset"]
    u2 = R.to_uniform(w[2])
    assert tuple(np.nonzero(u2 == 1.0)[0]) == LARGE_ZERO_BLOCKS
    assert not any((R.to_uniform(x) == 1.0).any() for x in (w[0], w[1], w[3]))
    for blk in LARGE_ZERO_BLOCKS:
        zz, rr = R.randn(4, LARGE["seed"], LARGE["offset"] + blk)
        assert rr[2] == 0.0 and zz[2] == 0.0 and zz[3] == 0.0 and rr[0] > 0
    d = R.blocks(990, 20, LARGE["seed"], LARGE["offset"], mutate="ctr_hi_dropped")
    same = np.array([all(int(a[990 + i]) == int(b[i]) for a, b in zip(w, d)) for i in range(20)])
    assert same[:10].all() and not same[10:].any()
