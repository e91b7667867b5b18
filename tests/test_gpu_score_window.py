"""Long recordings sampled as ONE latent each with a window-blended DiT score (dsn_score_windowed, dsn_pc_sample_windowed,
dsn_separate_windowed; Engine.score / pc_sample (window=), Engine.separate_long(mode="score")), against
tests/score_window_restatement.py: the plan restated from the seams outwards, a float64 blend, and `windowed`, which
wraps the CPU oracle's DiTScore into the long-latent score so that oracle.sampler.pc_sample and oracle.pipeline.separate
run it unchanged -- on every recording ALONE and at its full length.  The tiny DiT (embed 128, depth 2, 2 heads) and
Oobleck (channels 32) of tests/test_gpu_separate_long.py; explicit VAE and sampler noise.

Windows of Tw = 8 latent frames sharing To = 2 or 4.  Shapes: T = Tw + 1 (two windows, the second shifted back by
Tw - 1), T = 2 Tw - To (exact tiling), T = 3 Tw - 2 To + 1, and a ragged trio with one T < Tw (a short window: the
length-aware attention runs).  End to end the hop length is 2048 samples, so the 9000- and 5000-sample recordings of
the existing long-recording test have 5 and 3 frames: they run with ITS window, 4096 samples sharing 2048 (Tw = 2,
To = 1: 4 + 2 windows), and a second pair (20000 and 17000 samples, 10 and 9 frames) runs with Tw = 8, To = 2.

Bounds.  The blend is fmaf(rise, b, fall a) in fp32: one rounding of the product, one of the fused sum, so
|device - float64| <= 2 * 2^-24 (|a| + |b|) and the tests hold it to 4 * 2^-24 (|a| + |b|); outside seams and past a
recording's end it is a copy / zero, bit for bit.  Against the oracle: the score to the bounds
tests/test_gpu_ragged_paths.py holds this network to (rel-L2 1e-4 in bf16x3, 4e-3 in fp16; a convex combination of two
window scores cannot enlarge an absolute error, and the test first checks on the CPU that the blended score is not small
against the window scores it is made of), sampler and separation to 1e-3 per recording, the bound of
tests/test_gpu_separate_long.py.

Measured on an MI355X: blend error at most 0.37 of its bound; score rel-L2 7.5e-6 (bf16x3) and 4.7e-4 (fp16); sampler
2.6e-6 and 1.8e-4; separation 1.4e-5 and, in fp16, 8.7e-4 .. 9.6e-4 -- close to the 1e-3 bound, with the sampler's
latent at 1.8e-4: most of it is added after the sampler.  The module runs in about 3 s.

Graphs: nothing in the library tells a replay from a capture, so the test shows what a replay must get right -- after
the graph was captured with one set of lengths, calls with other lengths at the same (R, Tmax, Wtot) give their eager
bits (the tables are data of the graph, not constants of it)."""
import ctypes as C

import numpy as np
import pytest
import torch

from ditsep_amd import native
from oracle import dit as odit
from oracle import ncsnpp as oncs
from oracle import oobleck as ovae
from oracle import pipeline, sampler
from oracle.make_golden import tiny_vae_weights
from tests import score_window_restatement as swr
from tests.test_gpu_gemm_kernels import FP16, X3
from tests.util import make_engine, rel_l2

pytestmark = pytest.mark.gpu

DCFG = odit.DiTConfig(n_src=2, embed_dim=128, depth=2, num_heads=2)
TW = 8
N_STEPS = 4
KW = dict(N=N_STEPS, corrector_steps=1, snr=0.5, t_eps=0.03)
U = 2.0 ** -24


def shapes(To):
    long3 = 3 * TW - 2 * To + 1
    return [[TW + 1], [2 * TW - To], [long3], [long3, 5, TW + 1]]


@pytest.fixture(scope="module")
def nets():
    vcfg = ovae.OobleckConfig(channels=32)
    return odit.random_dit_weights(DCFG, 32, out_gain=0.005), vcfg, tiny_vae_weights(vcfg, 31)


@pytest.fixture(scope="module")
def engines(nets):
    eng = {p: make_engine(DCFG, nets[0], precision=p) for p in (X3, FP16)}
    yield eng
    for e in eng.values():
        e.close()


def dev(a, dtype=None):
    return torch.as_tensor(a, dtype=dtype).cuda().contiguous()


def blend_terms(ws, plan):
    """ws [Wtot, Twin, C] float64 numpy -> (a, b, want) [R T, C]: the two window rows of every frame (b = 0 outside
    seams, both 0 past the end) and the float64 blend with the plan's float32 weights"""
    tab, wts = plan["table"], plan["weights"].astype(np.float64)
    flat = ws.reshape(-1, ws.shape[-1])
    i0 = np.where(tab[:, 0] >= 0, tab[:, 0] * plan["Twin"] + tab[:, 1], 0)
    i1 = np.where(tab[:, 2] >= 0, tab[:, 2] * plan["Twin"] + tab[:, 3], 0)
    a = np.where((tab[:, 0] >= 0)[:, None], flat[i0], 0.0)
    b = np.where((tab[:, 2] >= 0)[:, None], flat[i1], 0.0)
    want = np.where((tab[:, 2] >= 0)[:, None], wts[:, :1] * a + wts[:, 1:] * b, a)
    return a, b, want


def check_blend(got, ws, plan, what):
    """got [R T, C] float32 (device result, on the host) against the float64 blend of ws"""
    a, b, want = blend_terms(ws, plan)
    seam = plan["table"][:, 2] >= 0
    d = np.abs(got.astype(np.float64) - want)
    bound = 4 * U * (np.abs(a) + np.abs(b))
    worst = float((d[seam] / np.maximum(bound[seam], 1e-300)).max()) if seam.any() else 0.0
    print(f"{what}: worst blend error / bound {worst:.3f} over {int(seam.sum())} seam frames")
    assert (d[seam] <= bound[seam]).all(), f"{what}: a seam element misses 4 * 2^-24 (|a| + |b|) ({worst:.3f} of it)"
    assert np.array_equal(got[~seam].view(np.int32), want[~seam].astype(np.float32).view(np.int32)), \
        f"{what}: a frame outside the seams is not a bit-exact copy (or not zero past the end)"


# ------------------------------------------------------------------ the kernels alone
@pytest.mark.parametrize("To", [2, 4])
@pytest.mark.parametrize("prec", [X3, FP16], ids=["bf16x3", "fp16"])
def test_win_pack_tokens(engines, prec, To):
    """equals, bit for bit (fp32 and every operand plane), the dense pack of the same windows cut on the host"""
    eng, P = engines[prec], 2 if prec == X3 else 1
    g = torch.Generator().manual_seed(7 + To)
    for frames in shapes(To):
        plan = native.score_window_plan(frames, TW, To)
        R, T, W, Twin = len(frames), plan["T"], plan["Wtot"], plan["Twin"]
        xt, mix = torch.randn((R, 128, T), generator=g), torch.randn((R, 64, T), generator=g)
        for r, F in enumerate(frames):                      # past a recording's end: never read
            xt[r, :, F:] = float("nan")
            mix[r, :, F:] = float("nan")
        windows = [tuple(w) for w in plan["windows"].tolist()]
        n = W * Twin * 192
        out = {}
        for kind in ("win", "dense"):
            of = torch.full((n,), float("nan"), device="cuda")
            pl = torch.full((P, n), 0x7FC1, dtype=torch.int16, device="cuda")
            if kind == "win":
                eng.test_kernel("win_pack_tokens", x=dev(xt), y=dev(mix), wtab=dev(plan["windows"]), B=W, T=Twin, C0=128,
                                C1=64, R=R, Tsrc=T, out_f32=of, out_planes=pl)
            else:
                eng.test_kernel("pack_tokens", x=dev(swr.cut(xt, windows, Twin)), y=dev(swr.cut(mix, windows, Twin)), B=W,
                                T=Twin, C0=128, C1=64, out_f32=of, out_planes=pl)
            torch.cuda.synchronize()
            out[kind] = (of.cpu(), pl.cpu())
        assert torch.isfinite(out["win"][0]).all(), f"frames {frames}: a window read past its recording's end"
        assert torch.equal(out["win"][0].view(torch.int32), out["dense"][0].view(torch.int32)), f"frames {frames} fp32"
        assert torch.equal(out["win"][1], out["dense"][1]), f"frames {frames} planes"


@pytest.mark.parametrize("To", [2, 4])
def test_win_blend_tokens(engines, To):
    eng = engines[X3]
    g = torch.Generator().manual_seed(17 + To)
    for frames in shapes(To):
        plan = native.score_window_plan(frames, TW, To)
        R, T, W, Twin = len(frames), plan["T"], plan["Wtot"], plan["Twin"]
        ws = torch.randn((W, Twin, 128), generator=g)
        for w, (_, _, l) in enumerate(plan["windows"].tolist()):       # a short window's padding: never read
            ws[w, l:] = float("nan")
        out = torch.full((R * T, 128), float("nan"), device="cuda")
        eng.test_kernel("win_blend_tokens", x=dev(ws), ftab=dev(plan["table"]), fw=dev(plan["weights"]), B=W, T=Twin,
                        C=128, rows=R * T, out_f32=out)
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        assert np.isfinite(got).all(), f"frames {frames}: the blend read a short window's padding"
        check_blend(got, np.nan_to_num(ws.double().numpy()), plan, f"win_blend_tokens To {To} frames {frames}")
        for r, F in enumerate(frames):
            assert (got.reshape(R, T, 128)[r, F:] == 0).all(), f"frames {frames}: recording {r} not zero past its end"
    with pytest.raises(RuntimeError, match="names window 9 offset 0 outside B = 2"):
        bad = plan["table"].copy()
        bad[0, 0] = 9
        eng.test_kernel("win_blend_tokens", x=dev(ws), ftab=dev(bad), fw=dev(plan["weights"]), B=2, T=Twin, C=128,
                        rows=R * T, out_f32=out)


# ------------------------------------------------------------------ score: gather, DiT and blend chained
def score_inputs(frames, seed):
    g = torch.Generator().manual_seed(seed)
    R, T = len(frames), max(frames)
    xt = 2.0 * torch.randn((R, 2, 64, T), generator=g)
    mix = torch.randn((R, 1, 64, T), generator=g)
    for r, F in enumerate(frames):                          # the padding holds 10 x Gaussian values, never zeros
        xt[r, ..., F:] *= 10.0
        mix[r, ..., F:] *= 10.0
    return xt, torch.tensor([0.7, 0.2, 0.03])[:R], mix


@pytest.fixture(scope="module")
def score_cases(nets):
    """per To: the ragged trio's inputs and the oracle's windowed score, checked not to be small against the window
    scores it blends (else a relative bound would say nothing there)"""
    out = {}
    for To in (2, 4):
        frames = shapes(To)[-1]
        xt, t, mix = score_inputs(frames, 40 + To)
        fn = swr.windowed(odit.DiTScore(nets[0], DCFG), TW, To, frames)
        ref = fn(xt, t, mix)
        parts = swr.window_scores(odit.DiTScore(nets[0], DCFG), xt, t, mix, fn.windows)
        for r, F in enumerate(frames):
            mine = [p for p, w in zip(parts, fn.windows) if w[0] == r]
            rms_w = float(torch.cat([p.reshape(-1) for p in mine]).double().pow(2).mean().sqrt())
            rms_b = float(ref[r, ..., :F].double().pow(2).mean().sqrt())
            assert rms_b > 0.5 * rms_w, f"To {To} recording {r}: blended rms {rms_b:.3e} vs window rms {rms_w:.3e}"
            assert (ref[r, ..., F:] == 0).all()
        out[To] = (frames, xt, t, mix, ref)
    return out


@pytest.mark.parametrize("To", [2, 4])
@pytest.mark.parametrize("prec,tol", [(X3, 1e-4), (FP16, 4e-3)], ids=["bf16x3", "fp16"])
def test_score_windowed(engines, score_cases, prec, tol, To):
    eng = engines[prec]
    frames, xt, t, mix, ref = score_cases[To]
    plan = native.score_window_plan(frames, TW, To)
    R, T, Twin = len(frames), plan["T"], plan["Twin"]
    got = eng.score(xt, t, mix, frames=frames, window=(TW, To))
    # the same windows cut on the host, one batch of the same (Wtot, Twin): the same dit_plan, so the same window scores
    windows = [tuple(w) for w in plan["windows"].tolist()]
    tw = torch.stack([t[w[0]] for w in windows])
    assert plan["short"]
    ws = eng.score(swr.cut(xt, windows, Twin), tw, swr.cut(mix, windows, Twin), frames=[w[2] for w in windows])
    ws = torch.nan_to_num(ws.cpu().reshape(len(windows), 128, Twin).permute(0, 2, 1)).double().numpy()
    for w, (_, _, l) in enumerate(windows):
        ws[w, l:] = 0.0                                                             # (unspecified rows: never read)
    check_blend(got.cpu().reshape(R, 128, T).permute(0, 2, 1).reshape(R * T, 128).contiguous().numpy(), ws, plan,
                f"score windowed prec {prec} To {To}")
    for r, F in enumerate(frames):
        err = rel_l2(got[r, ..., :F], ref[r, ..., :F])
        print(f"score windowed prec {prec} To {To} recording {r} ({F} frames): rel-L2 {err:.3e} (bound {tol:.0e})")
        assert err < tol, f"recording {r}: rel-L2 {err:.3e} >= {tol:.0e}"
        assert (got[r, ..., F:] == 0).all()
    # batch smaller than Wtot: consecutive slices, a seam's two windows in different slices -> the same bits
    assert plan["Wtot"] == 7
    for batch in (4, 1):
        assert torch.equal(eng.score(xt, t, mix, frames=frames, window=(TW, To), batch=batch), got), f"batch {batch}"


@pytest.mark.parametrize("prec", [X3, FP16], ids=["bf16x3", "fp16"])
def test_score_windowed_single_window_is_the_plain_call(engines, prec):
    """no recording longer than a window: the windowed call is the plain call, bit for bit"""
    eng = engines[prec]
    xt, t, mix = score_inputs([6, 6], 48)
    assert torch.equal(eng.score(xt, t, mix, frames=[6, 6], window=(TW, 2)), eng.score(xt, t, mix))
    xt, t, mix = score_inputs([TW, TW, TW], 49)
    assert torch.equal(eng.score(xt, t, mix, frames=[TW] * 3, window=(TW, 4)), eng.score(xt, t, mix))


# ------------------------------------------------------------------ sampler
def sampler_case(nets, frames, To, seed, predictor="reverse_diffusion", corrector="ald", together=False):
    """-> y, noise (padded with Gaussian values) and the oracle's sampler with the windowed score on every recording
    alone at its full length (together: the whole batch in one call -- the langevin corrector's norms are batch means)"""
    g = torch.Generator().manual_seed(seed)
    R, T = len(frames), max(frames)
    y = torch.randn((R, 1, 64, T), generator=g)
    draws = sampler.noise_draws(N_STEPS, 1, predictor)
    noise = sampler.draw_noise(seed + 1, draws, (R, 2, 64, T))
    score = odit.DiTScore(nets[0], DCFG)
    kw = dict(eps=0.03, snr=0.5, corrector_steps=1, denoise=True, n_spkrs=2, predictor=predictor, corrector=corrector)
    if together:
        assert len(set(frames)) == 1
        x, nfe = sampler.pc_sample(swr.windowed(score, TW, To, frames), y, noise, sampler.OUVE(N=N_STEPS), **kw)
        assert nfe == N_STEPS * 2
        return y, noise, list(x[:, None])
    refs = []
    for r, F in enumerate(frames):
        x, nfe = sampler.pc_sample(swr.windowed(score, TW, To, [F]), y[r:r + 1, ..., :F].contiguous(),
                                   noise[:, r:r + 1, ..., :F].contiguous(), sampler.OUVE(N=N_STEPS), **kw)
        assert nfe == N_STEPS * 2
        refs.append(x)
    return y, noise, refs


def check_sample(eng, case, frames, To, what, **kw):
    y, noise, refs = case
    out, nfe = eng.pc_sample(y, noise, frames=frames, window=(TW, To), **KW, **kw)
    assert nfe == N_STEPS * 2                                # summed once: the whole pool shares every evaluation
    for r, F in enumerate(frames):
        err = rel_l2(out[r:r + 1, ..., :F], refs[r])
        print(f"{what} recording {r} ({F} frames): rel-L2 {err:.3e}")
        assert err < 1e-3, f"{what} recording {r}: rel-L2 {err:.3e} >= 1e-3"
        assert (out[r, ..., F:] == 0).all(), f"{what} recording {r}: x_out past its length is not zero"
    return out


@pytest.fixture(scope="module")
def sampler_cases(nets):
    return {To: sampler_case(nets, shapes(To)[-1], To, 50 + To) for To in (2, 4)}


@pytest.mark.parametrize("To", [2, 4])
@pytest.mark.parametrize("prec", [X3, FP16], ids=["bf16x3", "fp16"])
def test_pc_sample_windowed(engines, sampler_cases, prec, To):
    frames = shapes(To)[-1]
    out = check_sample(engines[prec], sampler_cases[To], frames, To, f"pc_sample windowed prec {prec} To {To}")
    y, noise, _ = sampler_cases[To]
    sliced, _ = engines[prec].pc_sample(y, noise, frames=frames, window=(TW, To), batch=4, **KW)
    assert torch.equal(sliced, out), "batch = 4 < Wtot = 7 changes the sampler's bits"


@pytest.mark.parametrize("predictor", ["euler_maruyama", "none"])
def test_pc_sample_windowed_predictors(engines, nets, predictor):
    frames = [2 * TW - 2, 5]
    case = sampler_case(nets, frames, 2, 60, predictor=predictor)
    check_sample(engines[X3], case, frames, 2, f"pc_sample windowed {predictor}", predictor=predictor)


def test_pc_sample_windowed_langevin_equal_lengths(engines, nets):
    frames = [TW + 1, TW + 1]
    case = sampler_case(nets, frames, 2, 62, corrector="langevin", together=True)
    check_sample(engines[X3], case, frames, 2, "pc_sample windowed langevin", corrector="langevin")


def test_pc_sample_windowed_graphs(engines, nets):
    """(R, Tmax, Wtot) = (3, 21, 9) with two different sets of lengths: eager, then graphs -- warm-up, capture and
    replay with the first set, then the second set at the same key"""
    eng = engines[X3]
    sets = ([21, 9, 15], [20, 10, 21])
    assert [native.score_window_plan(f, TW, 2, T=21)["Wtot"] for f in sets] == [9, 9]
    g = torch.Generator().manual_seed(71)
    y = torch.randn((3, 1, 64, 21), generator=g)
    noise = torch.randn((1 + 2 * N_STEPS, 3, 2, 64, 21), generator=g)
    eager = [eng.pc_sample(y, noise, frames=f, window=(TW, 2), **KW)[0] for f in sets]
    assert not torch.equal(eager[0], eager[1])
    eng.enable_graphs(True)
    try:
        for k in range(3):
            assert torch.equal(eng.pc_sample(y, noise, frames=sets[0], window=(TW, 2), **KW)[0], eager[0]), f"call {k}"
        for k in range(2):
            assert torch.equal(eng.pc_sample(y, noise, frames=sets[1], window=(TW, 2), **KW)[0], eager[1]), \
                f"lengths B call {k}: the tables are constants of the captured graph"
        assert torch.equal(eng.pc_sample(y, noise, frames=sets[0], window=(TW, 2), **KW)[0], eager[0])
    finally:
        eng.enable_graphs(False)


# ------------------------------------------------------------------ end to end
def e2e_case(nets, lengths, window, overlap, seed):
    """pipeline.separate with the windowed DiTScore on every recording alone, at full length -> mixes, vae noise
    list, padded sampler noise, reference wavs"""
    dsd, vcfg, vsd = nets
    Tw, To = window // vcfg.hop, overlap // vcfg.hop
    g = torch.Generator().manual_seed(seed)
    mixes = [0.3 * torch.randn((1, L), generator=g) for L in lengths]
    frames = [native.latent_frames_of(L, vcfg.hop) for L in lengths]
    refs = [pipeline.separate(swr.windowed(odit.DiTScore(dsd, DCFG), Tw, To, [frames[r]]), vsd, vcfg, m[None],
                              sampler.OUVE(N=N_STEPS), seed + 1 + r, n_spkrs=2, eps=0.03, snr=0.5, corrector_steps=1,
                              target_dim=m.shape[-1]) for r, m in enumerate(mixes)]
    assert [r["y"].shape[-1] for r in refs] == frames and all(r["nfe"] == 2 * N_STEPS for r in refs)
    noise = torch.randn((1 + N_STEPS * 2, len(mixes), 2, 64, max(frames)), generator=g)
    for r, ref in enumerate(refs):
        noise[:, r, ..., :frames[r]] = ref["noise"][:, 0]
    return mixes, [r["vae_noise"][0] for r in refs], noise, [r["wav"][0] for r in refs], frames


E2E = {"w4096": ((9000, 5000), 4096, 2048, [4, 2]),          # the existing long-recording test's recordings and window
       "w16384": ((20000, 17000), 16384, 4096, [2, 2]),      # Tw = 8, To = 2: 10 and 9 frames
       "single": ((3000,), 4096, 2048, [1])}                 # not longer than a window


@pytest.fixture(scope="module")
def e2e(nets):
    return {k: e2e_case(nets, L, w, o, 80 + i) for i, (k, (L, w, o, _)) in enumerate(E2E.items())}


@pytest.mark.parametrize("name", list(E2E))
@pytest.mark.parametrize("prec", [X3, FP16], ids=["bf16x3", "fp16"])
def test_separate_long_score_vs_oracle(nets, e2e, prec, name):
    dsd, vcfg, vsd = nets
    lengths, window, overlap, W = E2E[name]
    mixes, vae_noise, noise, wavs, frames = e2e[name]
    eng = make_engine(DCFG, dsd, vcfg, vsd, precision=prec)
    arg = mixes[0] if name == "single" else mixes
    est, nfe, info = eng.separate_long(arg, window=window, overlap=overlap, mode="score", batch=3, vae_noise=vae_noise,
                                       noise=noise, return_info=True, **KW)
    assert nfe == 2 * N_STEPS and info["W"] == W and info["frames"] == frames and "perms" not in info
    assert info["windows"].shape == (sum(W), 3)
    est = [est] if name == "single" else est
    assert torch.is_tensor(est[0]) and len(est) == len(lengths)
    for r, L in enumerate(lengths):
        assert tuple(est[r].shape) == (2, L) and est[r].is_cuda
        err = rel_l2(est[r], wavs[r])
        print(f"separate_long mode=score {name} prec {prec} recording {r} (L {L}): rel-L2 {err:.3e}")
        assert err < 1e-3, f"recording {r}: rel-L2 {err:.3e} >= 1e-3"
    eng.close()


def test_latentdiffsep_separate_long_score(nets, e2e, tmp_path):
    from ditsep_amd import LatentDiffSep
    from tests.test_gpu_kernels import _tiny_config

    dsd, vcfg, vsd = nets
    mixes, vae_noise, noise, wavs, _ = e2e["w4096"]
    model = LatentDiffSep(_tiny_config(tmp_path), precision="bf16x3")
    sd = {"score_model." + k: v for k, v in dsd.items()}
    sd.update({"vae." + k: v for k, v in vsd.items()})
    model.load_state_dict(sd)
    # (the configured sampler keywords: N = 4, snr 0.5, one corrector step; t_eps 0.03 -- the values of KW)
    est, nfe = model.separate_long(mixes, 4096, overlap=2048, mode="score", vae_noise=vae_noise, noise=noise)
    ref, nfe2 = model.engine.separate_long(mixes, window=4096, overlap=2048, mode="score", vae_noise=vae_noise,
                                           noise=noise, **KW)
    assert nfe == nfe2 == 2 * N_STEPS
    for r in range(2):
        assert torch.equal(est[r], ref[r]), f"recording {r}: the facade and the engine call disagree"
        assert rel_l2(est[r], wavs[r]) < 1e-3
    with pytest.raises(NotImplementedError, match="unsupported sampler keywords: \\['schedule'\\]"):
        model.separate_long(mixes, 4096, overlap=2048, mode="score", schedule="log")
    model.close()


# ------------------------------------------------------------------ refusals
def test_windowed_refusals_launch_nothing(nets):
    """the C entry points refuse by name before anything is allocated or launched; the Python layer refuses the same
    cases (and a window that is no multiple of the hop) before the library is touched"""
    dsd, vcfg, vsd = nets
    R, T = 2, 20
    y = torch.zeros((R, 1, 64, T), device="cuda")
    xt = torch.zeros((R, 2, 64, T), device="cuda")
    t = torch.ones(R, device="cuda")
    out = torch.empty_like(xt)
    opts = native.DsnSamplerOpts(0, 0, 1, 0.5, 0.03, 1, None, None, None)
    nfe = C.c_int()

    def refused(eng, frames, Tw, To, corrector, reason, score=True):
        fr = (C.c_int32 * R)(*frames)
        opts.corrector = corrector
        before = eng.workspace_bytes()
        rc = eng.lib.dsn_pc_sample_windowed(eng.ctx, native._ptr(y), fr, None, 0, native._ptr(out), R, T, N_STEPS, Tw, To,
                                            0, 0, C.byref(opts), C.byref(nfe), eng._stream())
        msg = eng.lib.dsn_last_error(eng.ctx).decode()
        assert rc != 0 and reason in msg, (rc, msg)
        if score:
            rc = eng.lib.dsn_score_windowed(eng.ctx, native._ptr(xt), native._ptr(t), native._ptr(y), fr,
                                            native._ptr(out), R, T, Tw, To, 0, 0, eng._stream())
            msg = eng.lib.dsn_last_error(eng.ctx).decode()
            assert rc != 0 and reason in msg, (rc, msg)
        assert eng.workspace_bytes() == before, "a refused call grew the workspace"

    eng = make_engine(DCFG, dsd, vcfg, vsd, precision=X3)
    refused(eng, (20, 15), 8, 5, 0, "2 * overlap = 10 > window = 8")
    refused(eng, (20, 21), 8, 2, 0, "frames[1] = 21 outside [1, T = 20]")
    refused(eng, (20, 15), 8, 2, 1, "langevin corrector", score=False)
    with pytest.raises(ValueError, match="2 \\* overlap = 10 > window = 8"):
        eng.score(xt, t, y, frames=(20, 15), window=(8, 5))
    with pytest.raises(ValueError, match="langevin corrector has no form for recordings of different lengths"):
        eng.pc_sample(y, None, N=N_STEPS, corrector="langevin", frames=(20, 15), window=(8, 2))
    mix = torch.zeros((1, 9000))
    before = eng.workspace_bytes()
    with pytest.raises(ValueError, match="window = 4000 and overlap = 2048 must be multiples of the hop length 2048"):
        eng.separate_long(mix, window=4000, overlap=2048, mode="score", **KW)
    with pytest.raises(ValueError, match="2 \\* overlap = 4 > window = 2"):
        eng.separate_long(mix, window=4096, overlap=4096, mode="score", **KW)
    with pytest.raises(ValueError, match="mode must be one of"):
        eng.separate_long(mix, window=4096, mode="latent", **KW)
    assert eng.workspace_bytes() == before
    eng.close()
    ncfg = oncs.NCSNppConfig(n_src=2, nf=32)
    neng = make_engine(ncfg=ncfg, nsd=oncs.random_ncsnpp_weights(ncfg, 41), precision=X3)
    refused(neng, (20, 15), 8, 2, 0, "need the DiT score network")
    with pytest.raises(ValueError, match="need the DiT score network"):
        neng.pc_sample(y, None, N=N_STEPS, frames=(20, 15), window=(8, 2))
    with pytest.raises(ValueError, match="need the DiT score network"):
        neng.score(xt, t, y, frames=(20, 15), window=(8, 2))
    neng.close()
