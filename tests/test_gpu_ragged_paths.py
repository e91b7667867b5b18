"""Mixtures of different lengths in one batch through the public interface, against the CPU oracle run on every item
ALONE (odit.DiTScore, sampler.pc_sample, pipeline.separate, used as they are): the tiny DiT of the other GPU tests
(embed_dim 128, depth 2, 2 heads, out_gain 0.005) and OobleckConfig(channels=32).  The bounds are those of the dense
tests of the same path: test_dit_tiny_vs_golden / test_dit_long_sequences (score), test_pc_sampler_tiny_dit_vs_oracle
(sampler), test_separate_tiny_vs_oracle (end to end).  The padded region of every input holds Gaussian values (larger
than the valid ones for the score inputs), never zeros: what an item gets must not depend on it."""
import ctypes as C

import pytest
import torch

from ditsep_amd import native
from oracle import dit as odit
from oracle import ncsnpp as oncs
from oracle import oobleck as ovae
from oracle import pipeline, sampler
from oracle.make_golden import tiny_vae_weights
from tests.test_gpu_gemm_kernels import FP16, X3
from tests.util import make_engine, rel_l2

pytestmark = pytest.mark.gpu

DCFG = odit.DiTConfig(n_src=2, embed_dim=128, depth=2, num_heads=2)
FRAMES_A, FRAMES_B, T = (20, 15, 3), (7, 20, 12), 20
N_STEPS = 4


@pytest.fixture(scope="module")
def dsd():
    return odit.random_dit_weights(DCFG, 32, out_gain=0.005)


@pytest.fixture(scope="module")
def vae():
    vcfg = ovae.OobleckConfig(channels=32)
    return vcfg, tiny_vae_weights(vcfg, 31)


# ------------------------------------------------------------------ score
def score_case(dsd, T_, frames, seed):
    """-> xt, t, mix (padded; the padding holds 10 x Gaussian values) and the oracle's score of every item alone"""
    g = torch.Generator().manual_seed(seed)
    B = len(frames)
    xt = 2.0 * torch.randn((B, 2, 64, T_), generator=g)
    mix = torch.randn((B, 1, 64, T_), generator=g)
    for b, f in enumerate(frames):
        xt[b, ..., f:] *= 10.0
        mix[b, ..., f:] *= 10.0
    t = torch.tensor([0.7, 0.2, 0.03])[:B]
    score = odit.DiTScore(dsd, DCFG)
    refs = [score(xt[b:b + 1, ..., :f], t[b:b + 1], mix[b:b + 1, ..., :f]) for b, f in enumerate(frames)]
    return xt, t, mix, refs


@pytest.fixture(scope="module")
def score_short(dsd):
    return score_case(dsd, T, FRAMES_A, 41)


def check_score(eng, case, frames, tol, what, site="dit.attention"):
    """`site`: the attention call site the score call must go through (dsn_profile_rows) -- the separate attention
    launch, or the fused to_qkv + attention one"""
    xt, t, mix, refs = case
    eng.profile_begin()
    eng.score(xt, t, mix, frames=frames)
    sites = {r["site"] for r in eng.profile_end()["rows"]}
    other = ({"dit.attention", "dit.qkv_attention"} - {site}).pop()
    assert site in sites and other not in sites, f"{what}: expected the {site} launch, profiled {sorted(sites)}"
    out = eng.score(xt, t, mix, frames=frames)
    assert torch.isfinite(out).all(), f"{what}: non-finite score (padded rows must stay finite)"
    for b, f in enumerate(frames):
        err = rel_l2(out[b:b + 1, ..., :f], refs[b])
        print(f"{what} item {b} ({f} frames): rel-L2 {err:.3e} (bound {tol:.0e})")
        assert err < tol, f"{what} item {b}: rel-L2 {err:.3e} >= {tol:.0e}"


@pytest.mark.parametrize("prec,tol", [(X3, 1e-4), (FP16, 4e-3)], ids=["bf16x3", "fp16"])
def test_score_ragged(dsd, score_short, prec, tol):
    """token counts 21, 16 and 4: the separate attention launch, its in-register kernel"""
    eng = make_engine(DCFG, dsd, precision=prec)
    check_score(eng, score_short, FRAMES_A, tol, f"score ragged prec {prec}")
    eng.close()


def test_score_ragged_fused_qkv(dsd, score_short, monkeypatch):
    """fp16 with the skinny window closed and one item per panel forced: the fused to_qkv + attention variant runs"""
    monkeypatch.setenv("DSN_SKINNY_MAX", "0")
    monkeypatch.setenv("DSN_QA_IPP", "1")
    eng = make_engine(DCFG, dsd, precision=FP16)
    check_score(eng, score_short, FRAMES_A, 4e-3, "score ragged fp16 fused qkv", site="dit.qkv_attention")
    eng.close()


def test_score_ragged_long_kernel(dsd):
    """301 and 259 tokens: the blocked-key online-softmax kernel, the second item ending 3 keys into its last block"""
    frames = (300, 258)
    eng = make_engine(DCFG, dsd, precision=X3)
    check_score(eng, score_case(dsd, 300, frames, 42), frames, 1e-4, "score ragged T 300")
    eng.close()


# ------------------------------------------------------------------ sampler
def sampler_case(dsd, frames, seed):
    """-> y, noise (padded with Gaussian values) and sampler.pc_sample of every item alone on its slices"""
    g = torch.Generator().manual_seed(seed)
    B = len(frames)
    y = torch.randn((B, 1, 64, T), generator=g)
    noise = sampler.draw_noise(seed + 1, 1 + N_STEPS * 2, (B, 2, 64, T))
    score = odit.DiTScore(dsd, DCFG)
    refs = []
    for b, f in enumerate(frames):
        x, nfe = sampler.pc_sample(score, y[b:b + 1, ..., :f].contiguous(), noise[:, b:b + 1, ..., :f].contiguous(),
                                   sampler.OUVE(N=N_STEPS), eps=0.03, snr=0.5, corrector_steps=1, denoise=True, n_spkrs=2)
        assert nfe == N_STEPS * 2
        refs.append(x)
    return y, noise, refs


@pytest.fixture(scope="module")
def sampler_a(dsd):
    return sampler_case(dsd, FRAMES_A, 51)


@pytest.fixture(scope="module")
def sampler_b(dsd):
    return sampler_case(dsd, FRAMES_B, 61)


def check_sample(eng, case, frames, what):
    y, noise, refs = case
    out, nfe = eng.pc_sample(y, noise, N=N_STEPS, corrector_steps=1, snr=0.5, t_eps=0.03, frames=frames)
    assert nfe == N_STEPS * 2
    for b, f in enumerate(frames):
        err = rel_l2(out[b:b + 1, ..., :f], refs[b])
        print(f"{what} item {b} ({f} frames): rel-L2 {err:.3e}")
        assert err < 1e-4, f"{what} item {b}: rel-L2 {err:.3e} >= 1e-4"
        assert (out[b, ..., f:] == 0).all(), f"{what} item {b}: x_out past its length is not zero"
    return out


def test_pc_sample_ragged(dsd, sampler_a):
    eng = make_engine(DCFG, dsd, precision=X3)
    check_sample(eng, sampler_a, FRAMES_A, "pc_sample ragged")
    # full lengths: the length-aware kernels on a dense batch agree with the dense call
    y, noise, _ = sampler_a
    dense, _ = eng.pc_sample(y, noise, N=N_STEPS, corrector_steps=1, snr=0.5, t_eps=0.03)
    full, _ = eng.pc_sample(y, noise, N=N_STEPS, corrector_steps=1, snr=0.5, t_eps=0.03, frames=(T, T, T))
    err = rel_l2(full, dense)
    print(f"pc_sample frames = (T, T, T) vs dense: rel-L2 {err:.3e}, identical bits: {torch.equal(full, dense)}")
    assert err < 1e-6
    eng.close()


def test_pc_sample_ragged_graphs(dsd, sampler_a, sampler_b):
    """the lengths are data of the captured graph: eager warm-up, capture and replay with one set of lengths, then
    three replays with another at the same (B, T)"""
    eng = make_engine(DCFG, dsd, precision=X3)
    eng.enable_graphs(True)
    for k in range(3):
        check_sample(eng, sampler_a, FRAMES_A, f"graphs call {k} lens A")
    for k in range(3):
        check_sample(eng, sampler_b, FRAMES_B, f"graphs call {k} lens B")
    eng.close()


# ------------------------------------------------------------------ end to end
LENGTHS = (4000, 6143, 9000)            # T = 2, 3, 5: every item its own codec group, 6143 on the pad-rule edge


@pytest.fixture(scope="module")
def e2e(dsd, vae):
    """three mixtures, pipeline.separate of each alone -> mixes, vae noise list, padded sampler noise, reference wavs"""
    vcfg, vsd = vae
    g = torch.Generator().manual_seed(33)
    mixes = [0.3 * torch.randn((1, L), generator=g) for L in LENGTHS]
    refs = [pipeline.separate(odit.DiTScore(dsd, DCFG), vsd, vcfg, m[None], sampler.OUVE(N=N_STEPS), 34 + b, n_spkrs=2,
                              eps=0.03, snr=0.5, corrector_steps=1, target_dim=m.shape[-1])
            for b, m in enumerate(mixes)]
    frames = [r["y"].shape[-1] for r in refs]
    assert frames == [2, 3, 5]
    noise = torch.randn((1 + N_STEPS * 2, len(mixes), 2, 64, max(frames)), generator=g)
    for b, r in enumerate(refs):
        noise[:, b, ..., :frames[b]] = r["noise"][:, 0]
    return mixes, [r["vae_noise"][0] for r in refs], noise, [r["wav"][0] for r in refs]


@pytest.mark.parametrize("prec", [X3, FP16], ids=["bf16x3", "fp16"])
def test_separate_ragged_vs_oracle(dsd, vae, e2e, prec):
    vcfg, vsd = vae
    mixes, vae_noise, noise, wavs = e2e
    eng = make_engine(DCFG, dsd, vcfg, vsd, precision=prec)
    est, nfe = eng.separate_ragged(mixes, vae_noise=vae_noise, noise=noise, N=N_STEPS, corrector_steps=1, snr=0.5,
                                   t_eps=0.03)
    assert nfe == N_STEPS * 2 and len(est) == len(mixes)
    for b, L in enumerate(LENGTHS):
        assert tuple(est[b].shape) == (2, L)
        err = rel_l2(est[b], wavs[b])
        print(f"separate_ragged prec {prec} item {b} (L {L}): rel-L2 {err:.3e}")
        assert err < 1e-3, f"item {b}: rel-L2 {err:.3e} >= 1e-3"
    eng.close()


def test_evaluate_batches_ragged(dsd, vae, e2e, tmp_path):
    from ditsep_amd import LatentDiffSep
    from ditsep_amd.evaluate import evaluate_batches, length_batches
    from tests.test_gpu_kernels import _tiny_config

    vcfg, vsd = vae
    mixes, vae_noise, noise, wavs = e2e
    model = LatentDiffSep(_tiny_config(tmp_path), precision="bf16x3")
    sd = {"score_model." + k: v for k, v in dsd.items()}
    sd.update({"vae." + k: v for k, v in vsd.items()})
    model.load_state_dict(sd)
    # the facade's batch entry point meets the same oracle
    est, nfe = model.separate_batch(mixes, vae_noise=vae_noise, noise=noise)
    assert nfe == N_STEPS * 2
    for b in range(len(mixes)):
        assert rel_l2(est[b], wavs[b]) < 1e-3
    # one ragged batch (the order length_batches gives) -> one record per item with its own length
    order = length_batches([m.shape[-1] for m in mixes], 8)
    assert order == [[0, 1, 2]]
    batch = ([mixes[i] for i in order[0]], [wavs[i] for i in order[0]])
    res = evaluate_batches(model, [batch], 16000, N=N_STEPS, seed=3, start_idx=10)
    assert sorted(res) == [10, 11, 12]
    for j, i in enumerate(order[0]):
        rec = res[10 + j]
        assert rec["len_s"] == LENGTHS[i] / 16000 and rec["nfe"] == N_STEPS * 2
        assert len(rec["si_sdr"]) == 2 and all(v == v for v in rec["si_sdr"]) and rec["runtime"] > 0
    assert len({rec["runtime"] for rec in res.values()}) == 1          # the batch time divided by B
    model.close()


# ------------------------------------------------------------------ refusals
def test_ragged_refusals_launch_nothing(dsd):
    """the C entry points refuse by name before anything is allocated or launched (the Python layer refuses the same
    cases earlier, tests/test_ragged_host.py: these calls go to the library directly)"""
    B = 3
    y = torch.zeros((B, 1, 64, T), device="cuda")
    xt = torch.zeros((B, 2, 64, T), device="cuda")
    t = torch.ones(B, device="cuda")
    out = torch.empty_like(xt)
    opts = native.DsnSamplerOpts(0, 0, 1, 0.5, 0.03, 1, None, None, None)
    nfe = C.c_int()

    def refused(eng, frames, corrector, reason):
        fr = (C.c_int32 * B)(*frames)
        opts.corrector = corrector
        before = eng.workspace_bytes()
        rc = eng.lib.dsn_pc_sample_ragged(eng.ctx, native._ptr(y), fr, None, 0, native._ptr(out), B, T, N_STEPS,
                                          C.byref(opts), C.byref(nfe), eng._stream())
        msg = eng.lib.dsn_last_error(eng.ctx).decode()
        assert rc != 0 and reason in msg, (rc, msg)
        if corrector == 0:
            rc = eng.lib.dsn_score_ragged(eng.ctx, native._ptr(xt), native._ptr(t), native._ptr(y), fr, native._ptr(out),
                                          B, T, eng._stream())
            msg = eng.lib.dsn_last_error(eng.ctx).decode()
            assert rc != 0 and reason in msg, (rc, msg)
        assert eng.workspace_bytes() == before, "a refused call grew the workspace"

    eng = make_engine(DCFG, dsd, precision=X3)
    refused(eng, (20, 0, 3), 0, "frames[1] = 0 outside [1, T = 20]")
    refused(eng, (20, 15, 21), 0, "frames[2] = 21 outside [1, T = 20]")
    refused(eng, (20, 15, 3), 1, "langevin corrector")
    with pytest.raises(ValueError, match="langevin corrector has no ragged form"):
        eng.pc_sample(y, None, N=N_STEPS, corrector="langevin", frames=(20, 15, 3))
    with pytest.raises(ValueError, match=r"frames\[2\] = 21 outside"):
        eng.score(xt, t, y, frames=(20, 15, 21))
    eng.close()
    ncfg = oncs.NCSNppConfig(n_src=2, nf=32)
    neng = make_engine(ncfg=ncfg, nsd=oncs.random_ncsnpp_weights(ncfg, 41), precision=X3)
    refused(neng, (20, 15, 3), 0, "need the DiT score network")
    with pytest.raises(ValueError, match="need the DiT score network"):
        neng.pc_sample(y, None, N=N_STEPS, frames=(20, 15, 3))
    neng.close()
