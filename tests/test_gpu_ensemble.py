"""dsn_ensemble_combine (ditsep_amd/csrc/ensemble.hip) through Engine.ensemble_combine on an engine with no score
network and no codec, and the `samples` / `combine` keywords of LatentDiffSep against the same steps done by hand.

Three kinds of checks.
  constructed truth   candidates built from known sources under known permutations, independent noise 10 dB below
                      the sources: `perm` recovers the permutations relative to the anchor's.  No restatement involved.
  the restatement     tests/ensemble_restatement.py forms the Gram exactly rounded.  A device entry is a float64 sum of
                      L exact products in some fixed order, so it is within L 2^-53 sum_t |x_p[t]| |x_q[t]| of it (the
                      bound the header states); resid_db and agree_db must lie in the intervals the restatement gets at
                      the ends of G +- bound (plus 1e-12 relative for log10's own rounding).  perm, anchor and best are
                      equal: every case first asserts, on the restatement's side, that each discrete choice beats its
                      runner-up by more than twice what the bound allows the compared values.  Given equal perm the
                      combine is float32 arithmetic in a stated order: bit for bit in all four modes.
  identities          K = 1, permuted copies, the least noisy candidate, an exact sum, ragged items against the items
                      alone, permuted batches, reruns, the vector against the scalar load path: bit for bit.
With n > L the sources cannot be linearly independent and no permutation can be recovered: the constructed-truth
cases at L = 1 and L = 3 take n <= L, the comparison with the restatement (any data) covers n > L."""
import math

import numpy as np
import pytest
import torch

from ditsep_amd import files, native, wavio
from tests import ensemble_restatement as er
from tests import pcm_restatement as pr
from tests.util import make_engine, rel_l2

pytestmark = pytest.mark.gpu

TILE = 2048                                  # ENS_TILE of csrc/kernels.h
MODES = er.MODES


@pytest.fixture(scope="module")
def eng():
    e = make_engine()
    assert e.cfg.score_kind == native.SCORE_NONE
    yield e
    e.close()


def bits(x):
    x = np.atleast_1d(x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x))
    return x.view(np.int64 if x.dtype == np.float64 else np.int32)


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def offset_by_one_float(t, device):
    """the same values on the device, the base pointer 4 bytes past a 16-byte boundary"""
    flat = torch.empty(t.numel() + 1, device=device, dtype=torch.float32)
    v = flat[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


def run(eng, cands, mix=None, lens=None, mode="mean", offset=False):
    """numpy [B, K, n, L] (+ [B, L]) -> (out numpy [B, n, L], info)"""
    c = torch.from_numpy(np.ascontiguousarray(cands)).to(eng.device)
    m = None if mix is None else torch.from_numpy(np.ascontiguousarray(mix)).to(eng.device)
    if offset:
        c, m = offset_by_one_float(c, eng.device), (None if m is None else offset_by_one_float(m, eng.device))
    out, info = eng.ensemble_combine(c, m, lens=lens, mode=mode, return_info=True)
    assert out.is_cuda and out.dtype == torch.float32 and tuple(out.shape) == (cands.shape[0],) + cands.shape[2:]
    return out.cpu().numpy(), info


def info_same(a, b, item=None, alone=0):
    for k in ("perm", "anchor", "best", "resid_db", "agree_db", "gram"):
        x, y = (a[k], b[k]) if item is None else (a[k][item], b[k][alone])
        if not same(x, y):
            return False
    return True


# ------------------------------------------------------------------ constructed truth
@pytest.mark.parametrize("L", [1, 3, 257, 4099, 2 * TILE + 5])
@pytest.mark.parametrize("K", [1, 2, 3, 8, 16])
def test_constructed_truth(eng, K, L):
    for n in (1, 2, 3, 4):
        if n > L:
            continue
        cands, mix, perms, _ = er.make_case(7000 * K + 13 * n + L, K, n, L)
        out, info = run(eng, cands[None], mix[None])
        a = int(info["anchor"][0])
        perm = info["perm"][0].numpy()
        assert 0 <= a < K and 0 <= int(info["best"][0]) < K
        for k in range(K):
            assert sorted(perm[k]) == list(range(n)), (K, n, L, k, perm[k])
            assert all(perms[k][perm[k][i]] == perms[a][i] for i in range(n)), (K, n, L, k, perm[k], perms[k], perms[a])
        assert np.array_equal(perm[a], np.arange(n)) and bool(torch.isposinf(info["agree_db"][0, a]).all())
        assert np.all(np.isfinite(out))
        # the scalar path from a base pointer that is 4 bytes off: the same bits
        out1, info1 = run(eng, cands[None], mix[None], offset=True)
        assert same(out, out1) and info_same(info, info1), (K, n, L)


@pytest.mark.parametrize("L", [260, 2 * TILE + 4])
def test_vector_and_scalar_paths_give_the_same_bits(eng, L):
    """L a multiple of 4 and aligned bases take 16-byte loads and stores; one float off, scalar ones"""
    for K, n in ((3, 2), (16, 4), (1, 1), (8, 3)):
        cands, mix, _, _ = er.make_case(K + n + L, K, n, L)
        cb, mb = np.stack([cands, cands[::-1]]), np.stack([mix, mix])
        for mode in MODES:
            out, info = run(eng, cb, mb, mode=mode)
            out1, info1 = run(eng, cb, mb, mode=mode, offset=True)
            assert same(out, out1) and info_same(info, info1), (K, n, L, mode)
            lens = [L - 3, L - 5]
            out, info = run(eng, cb, mb, lens=lens, mode=mode)
            out1, info1 = run(eng, cb, mb, lens=lens, mode=mode, offset=True)
            assert same(out, out1) and info_same(info, info1), (K, n, L, mode, "ragged")


def test_ragged_items_nan_padding_permuted_batches_reruns(eng):
    K, n = 3, 2
    lens = [2 * TILE + 5, 257, TILE + 2]
    for Lmax in (max(lens) + 3, max(lens) + 1):          # a multiple of 4 (vector loads up to each ragged end), and not
        cands = np.full((3, K, n, Lmax), np.nan, dtype=np.float32)
        mix = np.full((3, Lmax), np.nan, dtype=np.float32)
        for b, v in enumerate(lens):
            cands[b, ..., :v], mix[b, :v], _, _ = er.make_case(50 + b, K, n, v)
        for mode in MODES:
            out, info = run(eng, cands, mix, lens=lens, mode=mode)
            assert not np.isnan(out).any() and not bool(torch.isnan(info["gram"]).any())
            assert not bool(torch.isnan(info["resid_db"]).any()) and not bool(torch.isnan(info["agree_db"]).any())
            for b, v in enumerate(lens):
                alone, ia = run(eng, cands[b:b + 1, ..., :v], mix[b:b + 1, :v], mode=mode)
                assert same(out[b, :, :v], alone[0]), f"item {b} differs from the item alone ({mode})"
                assert info_same(info, ia, b), f"item {b}: info differs from the item alone ({mode})"
                assert np.all(out[b, :, v:] == 0), f"item {b}: not zero past its end"
                assert float(np.abs(alone).max()) > 0
            order = [2, 0, 1]
            again, i2 = run(eng, cands[order], mix[order], lens=[lens[p] for p in order], mode=mode)
            assert same(again, out[order])
            assert all(info_same(i2, info, j, p) for j, p in enumerate(order))
            twice, i3 = run(eng, cands, mix, lens=lens, mode=mode)
            assert same(twice, out) and info_same(i3, info)


# ------------------------------------------------------------------ against the restatement
def random_case(seed, K, n, L):
    """a common random part and an independent one per candidate, any n and L"""
    g = np.random.default_rng(seed)
    base = g.standard_normal((n, L))
    cands = np.stack([base[g.permutation(n)] + 0.4 * g.standard_normal((n, L)) for _ in range(K)])
    return (0.3 * cands).astype(np.float32), (0.3 * (base.sum(axis=0) + 0.1 * g.standard_normal(L))).astype(np.float32)


RESTATED = [(1, 1, 1, True), (3, 4, 1, True), (2, 3, 3, True), (16, 4, 3, True), (3, 2, 257, True), (8, 3, 257, False),
            (2, 1, 4099, True), (8, 2, 4099, True), (16, 4, 2 * TILE + 5, True), (16, 2, 2 * TILE + 4, True),
            (3, 4, 2 * TILE + 8, False), (4, 2, 260, True)]


@pytest.mark.parametrize("K,n,L,with_mix", RESTATED)
def test_against_the_restatement(eng, K, n, L, with_mix):
    cands, mix = random_case(100 * K + 10 * n + L, K, n, L)
    mix = mix if with_mix else None
    res = er.restate_item(cands, mix)
    m = res["margins"]
    # the discrete choices are out of rounding's reach -- asserted for every case, none is left out
    assert er.margins_clear(res, 2.0), m
    assert np.array_equal(res["perm"], res["perm_lsa"]) and res["anchor"] == res["anchor_lsa"]
    outs = {}
    for mode in MODES:
        if mode == "best" and mix is None:
            continue
        out, info = run(eng, cands[None], None if mix is None else mix[None], mode=mode)
        outs[mode] = out[0]
    G = info["gram"][0].numpy()
    err = np.abs(G - res["gram"])
    print(f"K {K} n {n} L {L}: worst Gram error / bound {float((err / np.maximum(res['bound'], 1e-300)).max()):.3f}; "
          f"margins over their allowance: perm {min(d / max(e, 1e-300) for d, e in zip(m['perm'], m['perm_err'])):.3g} "
          f"anchor {m['anchor'] / max(m['anchor_err'], 1e-300):.3g} best {m['best'] / max(m['best_err'], 1e-300):.3g}")
    assert np.all(err <= res["bound"]), float((err / np.maximum(res["bound"], 1e-300)).max())
    assert np.array_equal(G, G.T)
    assert np.array_equal(info["perm"][0].numpy(), res["perm"])
    assert int(info["anchor"][0]) == res["anchor"] and int(info["best"][0]) == res["best"]
    for key in ("resid_db", "agree_db"):
        got, lo, hi = info[key][0].numpy(), res[key + "_lo"], res[key + "_hi"]
        assert np.array_equal(np.isnan(got), np.isnan(res[key])), key
        ok = ~np.isnan(got)
        slack = 1e-12 * np.maximum(1.0, np.abs(np.where(np.isfinite(got), got, 0.0)))
        assert np.all((got >= lo - slack)[ok]) and np.all((got <= hi + slack)[ok]), (key, got, lo, hi)
    for mode, out in outs.items():
        assert same(out, res["out"][mode]), f"{mode}: not the float32 restatement's bits"


# ------------------------------------------------------------------ identities
def test_one_candidate_is_returned_as_it_is(eng):
    for n, L in ((1, 1), (2, 259), (4, TILE + 8), (3, 2 * TILE + 1)):
        cands, mix, _, _ = er.make_case(n + L, 1, n, max(L, n))
        for mode in MODES:
            out, info = run(eng, cands[None], mix[None], mode=mode)
            assert same(out[0], cands[0]), (n, L, mode)
            assert int(info["anchor"][0]) == 0 and int(info["best"][0]) == 0
        for mode in ("mean", "median", "medoid"):
            out, info = run(eng, cands[None], None, mode=mode)
            assert same(out[0], cands[0]) and int(info["best"][0]) == -1
            assert bool(torch.isnan(info["resid_db"]).all())


def copies_case(K, n, L):
    g = np.random.default_rng(K * n + L)
    one = (0.3 * g.standard_normal((n, L))).astype(np.float32)
    return np.stack([one[g.permutation(n)] for _ in range(K)]), one.sum(axis=0, dtype=np.float32)


@pytest.mark.parametrize("K", [2, 3, 4, 8, 16])
def test_permuted_copies_of_one_candidate(eng, K):
    """median, best and medoid hand the candidate back (in the anchor's source order)"""
    for n, L in ((2, 257), (4, TILE + 4), (3, 1001)):
        cands, mix = copies_case(K, n, L)
        for mode in ("median", "best", "medoid"):
            out, info = run(eng, cands[None], mix[None], mode=mode)
            assert same(out[0], cands[int(info["anchor"][0])]), (K, n, L, mode)


@pytest.mark.parametrize("K", [2, 4, 8, 16])
def test_mean_of_permuted_copies(eng, K):
    """The mean of K = 2, 4, 8, 16 copies is the copy bit for bit.  The bare sequential float32 sum gives that at K = 2
    and 4 only (from 5x on the partial sums round and the errors do not cancel: 43-44 % of the samples off by up to 2
    units in the last place at K = 8, 69-72 % by up to 4 at K = 16, on the device and in numpy alike); the device and
    the restatement collect every addition's rounding error with a two-sum and give it back, and K x is then exact."""
    for n, L in ((2, 257), (4, TILE + 4), (3, 1001)):
        cands, mix = copies_case(K, n, L)
        out, info = run(eng, cands[None], mix[None], mode="mean")
        want = cands[int(info["anchor"][0])]
        ulps = np.abs(bits(out[0]).astype(np.int64) - bits(want).astype(np.int64))
        print(f"mean of {K} copies, n {n} L {L}: {float((ulps > 0).mean()):.3f} of the samples differ, by at most "
              f"{int(ulps.max())} units in the last place")
        assert same(out[0], want), (K, n, L)


def test_best_is_the_least_noisy_candidate(eng):
    for K, n, L, levels in ((4, 2, 4099, (-10, -14, -25, -12)), (8, 3, 600, (-10, -8, -12, -9, -11, -30, -7, -13)),
                            (2, 1, 257, (-20, -10))):
        cands, mix, _, _ = er.make_case(K + L, K, n, L, levels)
        want = int(np.argmin(levels))
        out, info = run(eng, cands[None], mix[None], mode="best")
        assert int(info["best"][0]) == want
        r = info["resid_db"][0].numpy()
        assert np.all(np.abs(r - np.array(levels, dtype=np.float64)) < 2.0), (r, levels)
        perm = info["perm"][0].numpy()
        assert same(out[0], cands[want][perm[want]])


def test_a_candidate_that_sums_exactly_to_the_mixture(eng):
    L = 2 * TILE + 5
    g = np.random.default_rng(9)
    src = (g.integers(-512, 512, (2, L)) / 1024.0).astype(np.float32)        # sums and products are exact
    off = src + (g.integers(-8, 8, (2, L)) / 1024.0).astype(np.float32)
    mix = src[0] + src[1]
    _, info = run(eng, np.stack([off, src[::-1]])[None], mix[None], mode="best")
    r = info["resid_db"][0].numpy()
    floor = 10.0 * math.log10(L * 2.0 ** -53)
    assert int(info["best"][0]) == 1 and (r[1] == -math.inf or r[1] < floor) and r[0] > -60.0, r


def test_refusals_launch_nothing(eng):
    B, K, n, L = 2, 3, 2, 300
    cands = torch.zeros((B, K, n, L), device=eng.device)
    mix = torch.zeros((B, L), device=eng.device)
    out = torch.full((B, n, L), 7.0, device=eng.device)
    good = dict(cands=cands, mix=mix, B=B, K=K, n=n, Lmax=L, lens=None, mode=0, out=out)

    def call(**kw):
        a = dict(good, **kw)
        lens = None if a["lens"] is None else (native.C.c_int32 * len(a["lens"]))(*a["lens"])
        return eng.lib.dsn_ensemble_combine(eng.ctx, native._ptr(a["cands"]), native._ptr(a["mix"]), a["B"], a["K"],
                                            a["n"], a["Lmax"], lens, a["mode"], native._ptr(a["out"]), None, None, None,
                                            None, None, None, eng._stream())

    for kw, msg in ((dict(cands=None), "cands or out is null"), (dict(out=None), "cands or out is null"),
                    (dict(B=0), "B = 0 outside [1, 65535]"), (dict(K=0), "K = 0 outside [1, 16]"),
                    (dict(K=17), "K = 17 outside [1, 16]"), (dict(n=0), "n = 0 outside [1, 4]"),
                    (dict(n=5), "n = 5 outside [1, 4]"), (dict(Lmax=0), "Lmax = 0 outside [1, 2^30]"),
                    (dict(mode=4), "mode = 4 is not one of"), (dict(mode=-1), "mode = -1 is not one of"),
                    (dict(mode=2, mix=None), "mode best ranks the candidates by their residual against the mixture"),
                    (dict(lens=[300, 0]), "lens[1] = 0 outside [1, Lmax = 300]"),
                    (dict(lens=[301, 300]), "lens[0] = 301 outside [1, Lmax = 300]"),
                    (dict(out=cands[0, 1]), "out overlaps cands")):
        assert call(**kw) != 0, kw
        assert msg in eng.lib.dsn_last_error(eng.ctx).decode(), (kw, eng.lib.dsn_last_error(eng.ctx).decode())
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((cands == 0.0).all())
    assert call() == 0
    torch.cuda.synchronize()
    assert bool((out == 0.0).all())
    with pytest.raises(ValueError, match="mode 'best' ranks the candidates"):
        eng.ensemble_combine(cands, None, mode="best")
    # flattened latents without a mixture; out alone without the info
    lat = torch.randn((1, 4, 2, 64 * 5), generator=torch.Generator().manual_seed(1))
    got = eng.ensemble_combine(lat, mode="medoid")
    _, info = eng.ensemble_combine(lat, mode="medoid", return_info=True)
    assert torch.is_tensor(got) and same(got[0], lat[0, int(info["anchor"][0])])


# ------------------------------------------------------------------ the samples keyword of LatentDiffSep
FS = 16000
N_STEPS = 4


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    """the tiny DiT and the two-block Oobleck with hop 8 of tests/test_gpu_mask_refine.py behind LatentDiffSep"""
    import json

    from ditsep_amd import LatentDiffSep
    from oracle import dit as odit
    from oracle import oobleck as ovae
    from oracle.make_golden import tiny_vae_weights

    vcfg = ovae.OobleckConfig(channels=128, c_mults=(1, 2), strides=(2, 4))
    dcfg = odit.DiTConfig(n_src=2, embed_dim=128, depth=2, num_heads=2)
    blk = {"channels": 128, "c_mults": [1, 2], "strides": [2, 4]}
    vae_json = {"model_type": "autoencoder", "sample_rate": FS,
                "model": {"encoder": {"type": "oobleck", "config": {"in_channels": 1, "latent_dim": 128, **blk}},
                          "decoder": {"type": "oobleck", "config": {"out_channels": 1, "latent_dim": 64, **blk}},
                          "bottleneck": {"type": "vae"}, "latent_dim": 64, "downsampling_ratio": vcfg.hop,
                          "io_channels": 1}}
    p = tmp_path_factory.mktemp("ensemble") / "vae.json"
    p.write_text(json.dumps(vae_json))
    cfg = {"model": {"n_speakers": 2, "t_eps": 0.03, "fs": FS,
                     "score_model": {"_target_": "ditsep_amd.score_models.DiTScoreModel", "embed_dim": 128, "depth": 2,
                                     "num_heads": 2},
                     "vae": {"config_path": str(p), "ckpt_path": None, "trainable_vae": False},
                     "sde": {"_target_": "sdes.sdes.OUVESDE", "theta": 1.5, "sigma_min": 0.96, "sigma_max": 10.0,
                             "N": N_STEPS},
                     "sampler": {"N": N_STEPS, "snr": 0.5, "corrector_steps": 1}}}
    m = LatentDiffSep(cfg, precision="bf16x3")
    sd = {"score_model." + k: v for k, v in odit.random_dit_weights(dcfg, 32, out_gain=0.005).items()}
    sd.update({"vae." + k: v for k, v in tiny_vae_weights(vcfg, 23).items()})
    m.load_state_dict(sd)
    assert m.fs == FS and m.hop_length == 8
    yield m
    m.close()


def test_separate_with_samples(model):
    eng = model.engine
    g = torch.Generator().manual_seed(51)
    mix = 0.3 * torch.randn((2, 1, 600), generator=g)
    plain, nfe = model.separate(mix, seed=3)
    assert same(model.separate(mix, seed=3, samples=None)[0], plain)
    one, nfe1 = model.separate(mix, seed=3, samples=1)
    assert same(one, plain) and nfe1 == nfe
    cands, _ = model.separate(mix.repeat_interleave(4, 0), seed=3)
    assert tuple(cands.shape) == (8, 2, 608)
    padded = torch.nn.functional.pad(mix, (0, 8))
    outs = {}
    for mode in MODES:
        got, nfe4 = model.separate(mix, seed=3, samples=4, combine=mode)
        want, info = eng.ensemble_combine(cands.reshape(2, 4, 2, 608), padded, mode=mode, return_info=True)
        assert nfe4 == nfe and tuple(got.shape) == (2, 2, 608) and same(got, want), mode
        got2, _, info2 = model.separate(mix, seed=3, samples=4, combine=mode, return_info=True)
        assert same(got2, want) and info_same(info, info2)
        outs[mode] = got
    assert not same(outs["mean"], outs["median"]) and not same(outs["mean"], plain)
    # with target_dim the mixture is as long as the estimates; at another rate the combine runs at the model's rate
    cut, _ = model.separate(mix.repeat_interleave(4, 0), target_dim=600, seed=3)
    assert same(model.separate(mix, target_dim=600, seed=3, samples=4, combine="best")[0],
                eng.ensemble_combine(cut.reshape(2, 4, 2, 600), mix, mode="best"))
    x = 0.3 * torch.randn((1, 2, 1300), generator=g)
    at_fs = eng.resample(x, 32000, FS, downmix=True)
    sep = model.separate(at_fs.repeat_interleave(2, 0), seed=5)[0]
    m = torch.nn.functional.pad(at_fs, (0, sep.shape[-1] - at_fs.shape[-1]))
    hand = eng.resample(eng.ensemble_combine(sep[None], m, mode="median"), FS, 32000)[..., :1300]
    assert same(model.separate(x, seed=5, sample_rate=32000, samples=2, combine="median")[0], hand)
    # refined after the combine: the outputs sum to the mixture (the bound of tests/test_gpu_mask_refine.py)
    ref, _ = model.separate(mix, seed=3, samples=4, refine=True)
    assert same(ref, eng.mask_refine(padded, outs["mean"]))
    peak = float(mix.abs().max())
    assert float((ref.sum(dim=1).cpu() - padded[:, 0]).abs().max()) < 1e-5 * peak
    with pytest.raises(ValueError, match="samples= combines waveforms: with latent=True"):
        model.separate(torch.zeros(1, 64, 75), latent=True, samples=2)
    with pytest.raises(ValueError, match="samples= does not go with intermediate"):
        model.separate(mix, samples=2, intermediate=True)
    with pytest.raises(ValueError, match="samples = 17 is not an int in"):
        model.separate(mix, samples=17)
    with pytest.raises(ValueError, match="combine must be one of"):
        model.separate(mix, samples=2, combine="vote")
    with pytest.raises(ValueError, match="return_info=True hands back the info of the combine"):
        model.separate(mix, return_info=True)


def test_separate_batch_with_samples(model):
    """two lengths, two draws each, the draws given: every item gets what separate(samples=2) gives it alone, under the
    ragged tests' tolerance (rel-L2 1e-3, tests/test_gpu_ragged_paths.py)"""
    eng = model.engine
    g = torch.Generator().manual_seed(53)
    K, lens = 2, (300, 611)
    mixes = [0.3 * torch.randn((1, L), generator=g) for L in lens]
    frames = [eng.latent_frames(L) for L in lens]
    vae_noise = [torch.randn((64, frames[b]), generator=g) for b in range(2) for _ in range(K)]
    noise = torch.randn((1 + 2 * N_STEPS, 2 * K, 2, 64, max(frames)), generator=g)
    est, nfe, info = model.separate_batch(mixes, vae_noise=vae_noise, noise=noise, samples=K, return_info=True)
    assert nfe == 2 * N_STEPS and len(est) == 2 and tuple(info["perm"].shape) == (2, K, 2)
    for b, L in enumerate(lens):
        alone, _, ia = model.separate(mixes[b][None], target_dim=L, samples=K, return_info=True,
                                      vae_noise=torch.stack(vae_noise[b * K:(b + 1) * K]),
                                      noise=noise[:, b * K:(b + 1) * K, ..., :frames[b]].contiguous())
        assert tuple(est[b].shape) == (2, L)
        err = rel_l2(est[b], alone[0])
        print(f"separate_batch(samples={K}) item {b} (L {L}): rel-L2 {err:.3e} against separate(samples={K}) alone")
        assert torch.equal(info["perm"][b], ia["perm"][0]) and err < 1e-3, (b, err)
    # by hand: the repeated list, then one combine call with the items' lengths
    rep, _ = model.separate_batch([m for m in mixes for _ in range(K)], vae_noise=vae_noise, noise=noise)
    c = torch.zeros((2, K, 2, max(lens)), device=eng.device)
    mp = torch.zeros((2, max(lens)), device=eng.device)
    for b, L in enumerate(lens):
        mp[b, :L] = mixes[b][0]
        for k in range(K):
            c[b, k, :, :L] = rep[b * K + k]
    for mode in MODES:
        got, _ = model.separate_batch(mixes, vae_noise=vae_noise, noise=noise, samples=K, combine=mode)
        want = eng.ensemble_combine(c, mp, lens=list(lens), mode=mode)
        assert all(same(got[b], want[b, :, :L]) for b, L in enumerate(lens)), mode
    plain, _ = model.separate_batch(mixes, seed=7)
    assert all(same(a, b) for a, b in zip(model.separate_batch(mixes, seed=7, samples=None)[0], plain))
    assert all(same(a, b) for a, b in zip(model.separate_batch(mixes, seed=7, samples=1)[0], plain))
    ref, _ = model.separate_batch(mixes, seed=7, samples=K, refine=True)
    assert all(same(a, b) for a, b in zip(ref, eng.mask_refine(mixes, model.separate_batch(mixes, seed=7, samples=K)[0])))


def test_separate_files_with_samples(model, tmp_path):
    eng = model.engine
    g = np.random.default_rng(57)
    src = tmp_path / "in"
    src.mkdir()
    wavio.write_wav(src / "a.wav", (0.3 * g.standard_normal(300) * 2 ** 15).astype("<i2").tobytes(), FS, 1, "s16")
    wavio.write_wav(src / "b.wav", (0.3 * g.standard_normal(2 * 900)).astype("<f4").tobytes(), 32000, 2, "f32")
    wavio.write_wav(src / "c.wav", (0.3 * g.standard_normal(260) * 2 ** 15).astype("<i2").tobytes(), 8000, 1, "s16")
    paths = sorted(src.glob("*.wav"))
    hs = [wavio.read_header(p) for p in paths]
    out = tmp_path / "out"
    recs = model.separate_files(paths, out, batch=4, seed=5, samples=2, combine="best")
    plan = files.plan_files(hs, FS, 8, batch=2)
    assert [r["batch"] for r in recs] == [next(k for k, b in enumerate(plan["batches"]) if i in b) for i in range(3)]
    assert len(plan["batches"]) == 2
    for k, idx in enumerate(plan["batches"]):
        clips = [torch.from_numpy(pr.decode(wavio.read_payload(paths[i], hs[i]), hs[i].frames, hs[i].channels,
                                            hs[i].encoding)) for i in idx]
        at_fs = eng.to_model_rate(clips, [hs[i].rate for i in idx], FS)
        est, _ = model.separate_batch(at_fs, codec="padded", seed=5 + k, samples=2, combine="best")
        back = eng.from_model_rate(est, [hs[i].rate for i in idx], FS, [hs[i].frames for i in idx])
        for j, i in enumerate(idx):
            for s in range(2):
                p = out / f"s{s}" / paths[i].name
                ho = wavio.read_header(p)
                assert ho[:4] == (hs[i].rate, 1, hs[i].frames, "s16")
                want, clipped = pr.quantise(back[j][s].cpu().numpy(), "s16")
                assert wavio.read_payload(p, ho) == want, f"{p} is not the quantised combined estimate"
                assert recs[i]["clipped"][s] == clipped
    with pytest.raises(ValueError, match=r"b\.wav is longer than long_after = 0.02 s .* samples= has no separate_long form"):
        model.separate_files(paths, tmp_path / "never", samples=2, long_after=0.02)
    assert not (tmp_path / "never").exists()
