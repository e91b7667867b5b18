"""numpy restatement of the device generator (ditsep_amd/csrc/kernels.hip: randn_kernel, rand_uniform_kernel).

Philox4x32-10 (Salmon et al., SC'11).  Block i of a stream has the counter {lo32(i + offset), hi32(i + offset), 0, 0} and
the key {lo32(seed), hi32(seed)}; the key is bumped by 0x9E3779B9 / 0xBB67AE85 after every round.  Each 32-bit word w
becomes the uniform u = (float32(w >> 8) + 0.5f) * 2^-24, evaluated in float32 as the kernel does: the sum rounds to even
at 24 bits, so u lies in (0, 1] and the top word pattern (w >> 8 == 2^24 - 1) gives u = 1 exactly.
  randn         words 0, 1 -> z0 = r cos(2 pi u1), z1 = r sin(2 pi u1) with r = sqrt(-2 ln u0); words 2, 3 -> z2, z3 alike.
                Box-Muller is evaluated here in float64 on the float32 uniforms.  Value j of a draw is output j % 4 of
                block j / 4 + offset.
  rand_uniform  word 0 of block i + offset only: min(lo + (hi - lo) u, hi)

The `mutate` argument of the functions below restates one defect each, for tests/test_sampler_kernels_host.py.
"""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK32 = np.uint64(0xFFFFFFFF)
SEED_ENCODER = 0x5851F42D4C957F2D      # engine.hip: encoder noise of a seed
SEED_LOSS_T = 0x9E3779B97F4A7C15       # engine.hip: loss times of a seed


def philox4x32_10(ctr, key, bump=True):
    """ctr: four uint32 arrays (or scalars), key: two Python ints -> four uint32 arrays"""
    c = [np.atleast_1d(np.asarray(x)).astype(np.uint64) for x in ctr]
    n = max(x.size for x in c)
    c = [np.broadcast_to(x, (n,)).copy() for x in c]
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0 = np.uint64(M0) * c[0]
        p1 = np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & MASK32,
             (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & MASK32]
        if bump:
            k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return [x.astype(np.uint32) for x in c]


def blocks(first, count, seed, offset, mutate=None):
    """words of the blocks first .. first + count - 1 of the stream (seed, offset): four uint32 arrays"""
    seed, offset = int(seed) & (2 ** 64 - 1), int(offset) & (2 ** 64 - 1)
    ctr = (np.arange(first, first + count, dtype=np.uint64) + np.uint64(offset))      # wraps mod 2^64 as the kernel's
    hi = (ctr >> np.uint64(32)).astype(np.uint32)
    if mutate == "ctr_hi_dropped":
        hi = np.zeros_like(hi)
    zero = np.zeros(1, np.uint32)
    return philox4x32_10(((ctr & MASK32).astype(np.uint32), hi, zero, zero), (seed & 0xFFFFFFFF, seed >> 32),
                         bump=mutate != "no_key_bump")


def to_uniform(w):
    """float32 uniforms in (0, 1] of uint32 words, the kernel's own float32 expression"""
    return (((w >> np.uint32(8)).astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -24)).astype(np.float32)


def randn(n, seed, offset=0, mutate=None):
    """the first n values of the normal stream (seed, offset) -> (float64 values, float64 radius of each value's pair)"""
    nb = (n + 3) // 4
    w = blocks(0, nb, seed, offset, mutate)
    u = [to_uniform(x).astype(np.float64) for x in w]
    out = np.empty((nb, 4), np.float64)
    rad = np.empty((nb, 4), np.float64)
    tw = 2.0 * np.pi
    for p in (0, 1):
        r = np.sqrt(-2.0 * np.log(u[2 * p]))
        c, s = np.cos(tw * u[2 * p + 1]), np.sin(tw * u[2 * p + 1])
        if mutate == "sincos_swapped":
            c, s = s, c
        out[:, 2 * p], out[:, 2 * p + 1] = r * c, r * s
        rad[:, 2 * p] = rad[:, 2 * p + 1] = r
    return out.reshape(-1)[:n], rad.reshape(-1)[:n]


def rand_uniform(n, seed, offset, lo, hi, mutate=None):
    """-> (float64 value of min(lo + (hi - lo) u, hi) on the float32 lo, hi, u; the float32 uniforms)"""
    u = to_uniform(blocks(0, n, seed, offset, mutate)[0])
    lo64, hi64 = float(np.float32(lo)), float(np.float32(hi))
    d = float(np.float32(np.float32(hi) - np.float32(lo)))
    return np.minimum(lo64 + d * u.astype(np.float64), hi64), u
