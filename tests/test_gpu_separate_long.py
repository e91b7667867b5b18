"""Engine.separate_long / LatentDiffSep.separate_long: long recordings cut into overlapping windows, separated as one
pooled batch and stitched on the device (dsn_window_stitch), against the CPU oracle run on every window ALONE
(pipeline.separate, used as it is) and stitched by the float64 restatement (tests/stitch_restatement.py).  The tiny DiT
and Oobleck of tests/test_gpu_ragged_paths.py; explicit VAE and sampler noise, so both sides consume the same draws.

The rel-L2 bound, 1e-3 per recording, is the one test_separate_ragged_vs_oracle holds the same networks to per item:
outside the overlaps the stitched recording is a copy of the windows, inside it is a convex combination of two of
them, which cannot enlarge an absolute error."""
import numpy as np
import pytest
import torch

from oracle import dit as odit
from oracle import oobleck as ovae
from oracle import pipeline, sampler
from oracle.make_golden import tiny_vae_weights
from tests import stitch_restatement as sr
from tests.test_gpu_gemm_kernels import FP16, X3
from tests.util import make_engine, rel_l2

pytestmark = pytest.mark.gpu

DCFG = odit.DiTConfig(n_src=2, embed_dim=128, depth=2, num_heads=2)
N_STEPS = 4
WINDOW, OVERLAP = 4096, 2048
LENGTHS = (9000, 5000)          # 4 + 2 windows; with batch = 3 the second minibatch straddles the two recordings
SHORT = 3000                    # not longer than one window
KW = dict(N=N_STEPS, corrector_steps=1, snr=0.5, t_eps=0.03)


@pytest.fixture(scope="module")
def nets():
    vcfg = ovae.OobleckConfig(channels=32)
    return odit.random_dit_weights(DCFG, 32, out_gain=0.005), vcfg, tiny_vae_weights(vcfg, 31)


def oracle_windows(nets, mixes, seed0):
    """every window of every recording through the oracle alone -> (vae_noise [Wtot,D,Tw], noise [draws,Wtot,n,D,Tw],
    per recording the separated windows [W,n,window] as numpy)"""
    dsd, vcfg, vsd = nets
    refs, counts = [], []
    for m in mixes:
        win = sr.cut(m.numpy(), WINDOW, OVERLAP)[:, 0]                       # [W, window]
        counts.append(win.shape[0])
        for x in win:
            refs.append(pipeline.separate(odit.DiTScore(dsd, DCFG), vsd, vcfg, torch.from_numpy(x.copy())[None, None],
                                          sampler.OUVE(N=N_STEPS), seed0 + len(refs), n_spkrs=2, eps=0.03, snr=0.5,
                                          corrector_steps=1, target_dim=WINDOW))
    vae_noise = torch.cat([r["vae_noise"] for r in refs], dim=0)
    noise = torch.cat([r["noise"] for r in refs], dim=1)
    wavs = np.stack([r["wav"][0].numpy() for r in refs])
    return vae_noise, noise, [wavs[sum(counts[:r]):sum(counts[:r + 1])] for r in range(len(mixes))]


def stitched(chunks, L, P=None):
    W, n, _ = chunks.shape
    f, r, _ = sr.fade(OVERLAP)
    P = np.tile(np.arange(n), (W, 1)) if P is None else P
    return torch.from_numpy(sr.crossfade(chunks, P, L, OVERLAP, f, r)[0])


@pytest.fixture(scope="module")
def case(nets):
    g = torch.Generator().manual_seed(33)
    mixes = [0.3 * torch.randn((1, L), generator=g) for L in LENGTHS]
    vae_noise, noise, wins = oracle_windows(nets, mixes, 50)
    assert [w.shape[0] for w in wins] == [4, 2] and noise.shape[:3] == (1 + 2 * N_STEPS, 6, 2)
    return mixes, vae_noise, noise, wins, [stitched(w, L) for w, L in zip(wins, LENGTHS)]


@pytest.fixture(scope="module")
def short_case(nets):
    g = torch.Generator().manual_seed(35)
    mix = 0.3 * torch.randn((1, SHORT), generator=g)
    vae_noise, noise, wins = oracle_windows(nets, [mix], 70)
    assert wins[0].shape[0] == 1
    return mix, vae_noise, noise, torch.from_numpy(wins[0][0][:, :SHORT])


@pytest.mark.parametrize("prec", [X3, FP16], ids=["bf16x3", "fp16"])
def test_separate_long_vs_oracle(nets, case, short_case, prec):
    dsd, vcfg, vsd = nets
    mixes, vae_noise, noise, _, refs = case
    eng = make_engine(DCFG, dsd, vcfg, vsd, precision=prec)
    est, nfe = eng.separate_long(mixes, window=WINDOW, overlap=OVERLAP, align=False, batch=3, vae_noise=vae_noise,
                                 noise=noise, **KW)
    assert isinstance(est, list) and len(est) == 2 and nfe == 2 * 2 * N_STEPS        # two minibatches
    for r, L in enumerate(LENGTHS):
        assert tuple(est[r].shape) == (2, L) and est[r].is_cuda
        err = rel_l2(est[r], refs[r])
        print(f"separate_long prec {prec} recording {r} (L {L}): rel-L2 {err:.3e}")
        assert err < 1e-3, f"recording {r}: rel-L2 {err:.3e} >= 1e-3"
    # one recording as a tensor, not longer than one window: the oracle's separation of its zero-extended window, cut
    # to the recording
    mix, vn, nz, ref = short_case
    one, nfe = eng.separate_long(mix, window=WINDOW, overlap=OVERLAP, vae_noise=vn, noise=nz, **KW)
    assert torch.is_tensor(one) and tuple(one.shape) == (2, SHORT) and nfe == 2 * N_STEPS
    err = rel_l2(one, ref)
    print(f"separate_long prec {prec} single window: rel-L2 {err:.3e}")
    assert err < 1e-3
    eng.close()


def test_separate_long_aligned_info(nets, case):
    """align=True: the result is the stitch of the returned windows, and the decisions follow from the returned
    tables.  (No comparison of the permutations with the oracle: with random weights the two estimated sources of a
    window are nearly alike and the decision has no margin; tests/test_gpu_stitch.py covers the decisive case.)"""
    dsd, vcfg, vsd = nets
    mixes, vae_noise, noise, wins, _ = case
    eng = make_engine(DCFG, dsd, vcfg, vsd, precision=X3)
    est, nfe, info = eng.separate_long(mixes, window=WINDOW, overlap=OVERLAP, batch=3, vae_noise=vae_noise, noise=noise,
                                       return_info=True, **KW)
    assert info["W"] == [4, 2] and info["hop"] == [2048, 2048] and tuple(info["chunks"].shape) == (6, 2, WINDOW)
    assert rel_l2(info["chunks"], torch.from_numpy(np.concatenate(wins))) < 1e-3
    o = 0
    for r, L in enumerate(LENGTHS):
        W = info["W"][r]
        out, perms, gram = eng.window_stitch(info["chunks"][o:o + W], L, OVERLAP)
        assert torch.equal(out, est[r]) and torch.equal(perms, info["perms"][r]) and torch.equal(gram, info["gram"][r])
        assert np.array_equal(perms.numpy(), sr.perms_from_gram(gram.numpy(), W, 2))
        assert tuple(gram.shape) == (W - 1, 2, 2) and bool((gram != 0).all())
        o += W
    with pytest.raises(ValueError, match="batch = 0 < 1"):
        eng.separate_long(mixes, window=WINDOW, batch=0, **KW)
    with pytest.raises(ValueError, match="2 \\* overlap = 4098 > window = 4096"):
        eng.separate_long(mixes, window=WINDOW, overlap=2049, **KW)
    # default overlap: window // 4
    est4, _, info4 = eng.separate_long(mixes[1], window=WINDOW, return_info=True, seed=3, **KW)
    assert info4["hop"] == [WINDOW - WINDOW // 4] and info4["W"] == [2] and tuple(est4.shape) == (2, LENGTHS[1])
    # a single window: the chunk's first L samples, bit for bit
    chunk = info["chunks"][:1]
    out, perms, gram = eng.window_stitch(chunk, SHORT, OVERLAP)
    assert torch.equal(out, chunk[0, :, :SHORT]) and perms.tolist() == [[0, 1]] and tuple(gram.shape) == (0, 2, 2)
    eng.close()


def test_latentdiffsep_separate_long(nets, case, short_case, tmp_path):
    from ditsep_amd import LatentDiffSep
    from tests.test_gpu_kernels import _tiny_config

    dsd, vcfg, vsd = nets
    mixes, vae_noise, noise, _, refs = case
    model = LatentDiffSep(_tiny_config(tmp_path), precision="bf16x3")
    sd = {"score_model." + k: v for k, v in dsd.items()}
    sd.update({"vae." + k: v for k, v in vsd.items()})
    model.load_state_dict(sd)
    est, nfe = model.separate_long(mixes, WINDOW, overlap=OVERLAP, align=False, batch=3, vae_noise=vae_noise,
                                   noise=noise)
    assert isinstance(est, list) and nfe == 2 * 2 * N_STEPS
    for r in range(2):
        err = rel_l2(est[r], refs[r])
        print(f"LatentDiffSep.separate_long recording {r}: rel-L2 {err:.3e}")
        assert tuple(est[r].shape) == (2, LENGTHS[r]) and err < 1e-3
    mix, vn, nz, ref = short_case
    one, nfe, info = model.separate_long(mix, WINDOW, overlap=OVERLAP, vae_noise=vn, noise=nz, return_info=True)
    assert torch.is_tensor(one) and nfe == 2 * N_STEPS and info["W"] == [1] and rel_l2(one, ref) < 1e-3
    model.close()
