"""dsn_window_stitch (ditsep_amd/csrc/stitch.hip) through Engine.window_stitch on an engine with no score network and
no codec, against the float64 restatement (tests/stitch_restatement.py).

Bounds.
* perms: exact.  On the decisive inputs (built as in tests/test_stitch_host.py) against the restatement's own table;
  on arbitrary inputs against what the restatement's rule gives from the device's OWN gram, which holds whatever the
  margins are.
* gram: 2^-50 sum_k |a_k b_k| per entry: float32 x float32 products are exact in float64, so only the order of the
  float64 additions differs from math.fsum.
* out: bit for bit where a sample is copied.  Inside an overlap the device forms fl(fl(f a) + fl(r b)) in float32
  (u = 2^-24): |fl(f a) - f a| <= u |f a|, the same for r b, and the sum adds u |fl(f a) + fl(r b)| <=
  u (1 + u)(|f a| + |r b|): together below 2 u (1 + u)(|f a| + |r b|) < 2^-22 (|f a| + |r b|).  A fused
  multiply-add rounds once less and lies inside the same bound.  f, r are the float32 tables both sides share."""
import math

import numpy as np
import pytest
import torch

from ditsep_amd import native
from tests import stitch_restatement as sr
from tests.util import make_engine

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    e = make_engine()
    assert e.cfg.score_kind == native.SCORE_NONE
    yield e
    e.close()


def run(eng, chunks, L, O, kind="hann", align=True):
    out, perms, gram = eng.window_stitch(torch.from_numpy(np.ascontiguousarray(chunks)), L, O, fade=kind, align=align)
    torch.cuda.synchronize()
    W, n, _ = chunks.shape
    assert tuple(out.shape) == (n, L) and out.dtype == torch.float32 and out.is_cuda
    assert tuple(perms.shape) == (W, n) and perms.dtype == torch.long
    assert tuple(gram.shape) == (W - 1, n, n) and gram.dtype == torch.float64
    return out.cpu().numpy(), perms.numpy(), gram.numpy()


def check_out(out, chunks, P, L, O, kind, what):
    f, r, _ = sr.fade(O, kind)
    want, bound, copied = sr.crossfade(chunks, P, L, O, f, r)
    assert np.array_equal(out[:, copied], want[:, copied].astype(np.float32)), f"{what}: a copied sample differs"
    err = np.abs(out.astype(np.float64) - want)
    worst = float((err / np.maximum(bound, 1e-300))[:, ~copied].max()) if (~copied).any() else 0.0
    print(f"{what}: cross-fade error / bound, worst {worst:.3f}")
    assert np.all(err[:, ~copied] <= bound[:, ~copied]), f"{what}: {worst:.3f} x the bound"


def check_gram(gram, G, A, what):
    err = np.abs(gram - G)
    worst = float((err / np.maximum(2.0 ** -50 * A, 1e-300)).max()) if G.size else 0.0
    print(f"{what}: gram error / bound, worst {worst:.3f}")
    assert np.all(err <= 2.0 ** -50 * A), f"{what}: {worst:.3f} x the bound"


# (Lw, O, W, n, L): odd sizes (no alignment, ragged tile tails, the last window mostly padding); 2 O = Lw, aligned;
# a long chain of 24-candidate decisions; a single window; more than one Gram tile on the vector and the scalar path
DECISIVE = [(1537, 517, 4, 1, 3910), (1537, 517, 4, 2, 3910), (1537, 517, 4, 3, 3910), (1537, 517, 4, 4, 3910),
            (2048, 1024, 2, 2, 3000), (64, 16, 300, 4, 14400), (1537, 517, 1, 2, 1000),
            (10240, 5000, 2, 2, 15000), (10241, 4999, 2, 2, 15001)]


@pytest.mark.parametrize("Lw,O,W,n,L", DECISIVE, ids=lambda v: str(v))
def test_stitch_decisive(eng, Lw, O, W, n, L):
    chunks, _, _, _ = sr.decisive_case(100 + n + W, n, L, Lw, O)
    assert chunks.shape == (W, n, Lw) and native.window_plan(L, Lw, O) == (W, Lw - O)
    _, _, _, P, G, A = sr.stitch(chunks, L, O)
    # the inputs decide: a table entry moves by at most 2^-50 A, a score by n times that, so two candidates whose
    # scores differ by more than 2 n 2^-50 max A compare alike on the device and in the restatement
    for w, (best, second) in enumerate(sr.margins(G)):
        if second is not None:
            assert best - second > 2 * n * 2.0 ** -50 * A[w].max() * 1e6, (w, best, second)
    what = f"decisive Lw {Lw} O {O} W {W} n {n}"
    out, perms, gram = run(eng, chunks, L, O)
    assert np.array_equal(perms, P), what
    check_gram(gram, G, A, what)
    check_out(out, chunks, P, L, O, "hann", what)


ARBITRARY = [(1537, 517, 4, 3, 3910, "hann"), (64, 16, 300, 4, 14400, "linear"), (2048, 1024, 2, 2, 3000, "hann"),
             (2048, 1024, 2, 2, 2999, "linear"), (2048, 512, 3, 4, 5001, "hann")]


@pytest.mark.parametrize("Lw,O,W,n,L,kind", ARBITRARY, ids=lambda v: str(v))
def test_stitch_arbitrary(eng, Lw, O, W, n, L, kind):
    """Gaussian chunks with no structure: small margins.  The device's decisions follow from its own gram by the rule,
    and its output is the cross-fade under its own table."""
    chunks = np.random.default_rng(Lw + W).standard_normal((W, n, Lw)).astype(np.float32)
    what = f"arbitrary Lw {Lw} O {O} W {W} n {n}"
    out, perms, gram = run(eng, chunks, L, O, kind)
    G, A = sr.gram(chunks, O)
    check_gram(gram, G, A, what)
    assert np.array_equal(perms, sr.perms_from_gram(gram, W, n)), what
    check_out(out, chunks, perms, L, O, kind, what)


def test_stitch_tie_rule(eng):
    ident = lambda W, n: np.tile(np.arange(n), (W, 1))
    rng = np.random.default_rng(7)
    Lw, O, hop = 64, 16, 48
    chunks = rng.standard_normal((3, 3, Lw)).astype(np.float32)
    zero = chunks.copy()
    zero[1:, :, :O] = 0
    out, perms, gram = run(eng, zero, 150, O)
    assert np.array_equal(perms, ident(3, 3)) and not gram.any()
    check_out(out, zero, perms, 150, O, "hann", "zero overlap")
    zero = chunks.copy()
    zero[:-1, :, hop:] = 0
    assert np.array_equal(run(eng, zero, 150, O)[1], ident(3, 3))
    same = chunks.copy()
    same[1:, 1] = same[1:, 0]
    same[1:, 2] = same[1:, 0]
    assert np.array_equal(run(eng, same, 150, O)[1], ident(3, 3))
    two = rng.standard_normal((2, 2, Lw)).astype(np.float32)
    two[1, 1] = two[1, 0]
    assert np.array_equal(run(eng, two, 100, O)[1], ident(2, 2))
    out, perms, gram = run(eng, chunks, 3 * Lw - 7, 0)               # overlap = 0: a concatenation
    assert np.array_equal(perms, ident(3, 3)) and not gram.any()
    assert np.array_equal(out, np.concatenate(list(chunks), axis=1)[:, :3 * Lw - 7])


def test_stitch_align_off(eng):
    """align=False: every P_w is the identity; the Gram stage is skipped and gram comes back as zeros"""
    Lw, O, L, n = 1537, 517, 3910, 3
    chunks, _, _, P = sr.decisive_case(3, n, L, Lw, O)
    assert not np.array_equal(P, np.tile(np.arange(n), (4, 1)))
    out, perms, gram = run(eng, chunks, L, O, align=False)
    assert np.array_equal(perms, np.tile(np.arange(n), (4, 1))) and gram.shape == (3, n, n) and not gram.any()
    check_out(out, chunks, perms, L, O, "hann", "align off")


def test_stitch_single_window(eng):
    chunks = np.random.default_rng(9).standard_normal((1, 2, 1537)).astype(np.float32)
    for L in (1, 1000, 1537):
        out, perms, gram = run(eng, chunks, L, 517)
        assert np.array_equal(out, chunks[0][:, :L]) and perms.tolist() == [[0, 1]] and gram.shape == (0, 2, 2)


def test_stitch_reruns_are_bit_identical(eng):
    chunks = np.random.default_rng(21).standard_normal((5, 4, 10240)).astype(np.float32)
    L = 4 * 5240 + 9000
    a, b = run(eng, chunks, L, 5000), run(eng, chunks, L, 5000)
    for x, y in zip(a, b):
        assert np.array_equal(x.view(np.uint8).reshape(-1), y.view(np.uint8).reshape(-1))


def test_stitch_past_2_31_elements(eng):
    """chunks and out of more than 2^31 elements: 64-bit index arithmetic.  Checked on the device, slice by slice."""
    W, n, Lw, O = 3, 2, 1 << 29, 4104
    hop = Lw - O
    L = 2 * hop + Lw - 5
    g = torch.Generator(device="cuda").manual_seed(5)
    chunks = torch.empty((W, n, Lw), device="cuda", dtype=torch.float32)
    assert chunks.numel() > 2 ** 31 and n * L > 2 ** 31
    for w in range(W):
        chunks[w].normal_(generator=g)
    out, perms, gram = eng.window_stitch(chunks, L, O)
    torch.cuda.synchronize()
    tails = chunks[:-1, :, hop:].cpu().numpy()
    heads = chunks[1:, :, :O].cpu().numpy()
    G = np.zeros((W - 1, n, n))
    A = np.zeros_like(G)
    for w in range(W - 1):
        for i in range(n):
            for j in range(n):
                p = tails[w, i].astype(np.float64) * heads[w, j].astype(np.float64)
                G[w, i, j], A[w, i, j] = math.fsum(p.tolist()), math.fsum(np.abs(p).tolist())
    check_gram(gram.numpy(), G, A, "past 2^31")
    P = sr.perms_from_gram(gram.numpy(), W, n)
    assert np.array_equal(perms.numpy(), P)
    f, r, _ = sr.fade(O)
    for i in range(n):
        for w in range(W):
            lo, hi = w * hop + (O if w else 0), min((w + 1) * hop if w < W - 1 else L, L)
            assert torch.equal(out[i, lo:hi], chunks[w, P[w, i], lo - w * hop:hi - w * hop]), (i, w)
            if w:
                a, b = tails[w - 1, P[w - 1, i]].astype(np.float64), heads[w - 1, P[w, i]].astype(np.float64)
                fa, rb = f.astype(np.float64) * a, r.astype(np.float64) * b
                got = out[i, w * hop:w * hop + O].cpu().numpy().astype(np.float64)
                assert np.all(np.abs(got - (fa + rb)) <= 2.0 ** -22 * (np.abs(fa) + np.abs(rb))), (i, w)


def test_stitch_refusals_launch_nothing(eng):
    """every DSN_EINVAL by message, straight at the library, with the workspace unchanged across the refused call"""
    W, n, Lw, O = 3, 2, 64, 16
    L = 2 * 48 + 40
    chunks = torch.zeros((W, n, Lw), device="cuda")
    out = torch.empty((n, 4 * Lw), device="cuda")
    eng.window_stitch(chunks, L, O)                                  # (a valid call first: the refusals follow one)

    def refused(reason, W=W, n=n, Lw=Lw, O=O, L=L, fade=0, chunks_p=native._ptr(chunks), out_p=native._ptr(out)):
        before = eng.workspace_bytes()
        rc = eng.lib.dsn_window_stitch(eng.ctx, chunks_p, W, n, Lw, O, L, fade, 1, out_p, None, None, eng._stream())
        msg = eng.lib.dsn_last_error(eng.ctx).decode()
        assert rc == -1 and "dsn_window_stitch" in msg and reason in msg, (rc, msg)
        assert eng.workspace_bytes() == before, "a refused call grew the workspace"

    refused("chunks or out is null", chunks_p=None)
    refused("chunks or out is null", out_p=None)
    refused("n = 0 outside [1, 4]", n=0)
    refused("n = 5 outside [1, 4]", n=5)
    refused("W = 0 < 1", W=0)
    refused("Lw = 0 < 1", Lw=0, O=0)
    refused("overlap = -1 < 0", O=-1)
    refused("2 * overlap = 66 > Lw = 64", O=33)
    refused("fade = 2 is neither 0 (hann) nor 1 (linear)", fade=2)
    refused("L = 112 outside (112, 160] for W = 3", L=2 * 48 + 16)   # the last overlap would hold padding
    refused("L = 161 outside (112, 160] for W = 3", L=161)
    refused("L = 0 outside [1, Lw = 64] for W = 1", W=1, L=0)
    refused("L = 65 outside [1, Lw = 64] for W = 1", W=1, L=65)
    with pytest.raises(ValueError, match="fade must be one of"):
        eng.window_stitch(chunks, L, O, fade="triangle")
    with pytest.raises(ValueError, match=r"chunks must be \[W, n, Lw\]"):
        eng.window_stitch(chunks[0], L, O)
    with pytest.raises(RuntimeError, match="L = 161 outside"):
        eng.window_stitch(chunks, 161, O)
