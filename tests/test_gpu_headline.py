"""GPU parity of the kernels the headline number actually times.

bench.py's workload is BASELINE config C2 at its own batch: 64 mixtures, T = 32 -> M = 64 * 33 = 2112 token rows.
Batch decides the code path (csrc/engine.hip::dit_forward: M <= 80 rows -> weight-streaming skinny GEMMs, else
row panels whose sub-tile count follows M; NCSN++: halo 3x3 tiles of 256 rows need >= 512 workgroups, single
mixtures reduce split-K slabs in igemm_slab_epilogue_kernel), so the B = 2 chains of test_gpu_configs.py run
other instantiations than the bench.  Every test here runs the benchmarked batch through the C-ABI and compares
with the fp32 CPU oracle on identical inputs:

  * one score call over the whole batch (every panel, incl. the masked last sub-tile, is checked);
  * N = 30 chains at B = 64 in which a few items (first / middle / last panel) carry the oracle's latents and
    injected noise -- mixtures are independent, so those items must meet the north-star bound
    (waveform rel-L2 < 1e-3, |SI-SDR delta| < 0.05 dB) whatever the other 61 items hold;
  * batch invariance: items of the B = 64 result against the same items run as B = 2 (skinny kernels).

Reference path: src/diffsep_latent.py:471-487 (separate), src/models/diffsep/score_models.py:173-186.
"""

import pytest
import torch

from oracle import dit as odit
from oracle import metrics
from oracle import ncsnpp as oncs
from oracle import oobleck as ovae
from oracle import sampler
from tests.util import make_engine, rel_l2

pytestmark = pytest.mark.gpu

X3, BF16, FP16, FP16X3, FP8 = 2, 1, 3, 4, 5
REL_L2_TOL, SI_SDR_TOL_DB = 1e-3, 0.05       # BASELINE.json north_star
SCORE_CALL_TOL = 3e-3                        # one fp16 score call of a random-weight net (not contractive)
B64, T32, L = 64, 32, 64000
PICK = (0, 31, 63)                           # first, middle and last row panel of the batch


def _log(msg):
    print(msg)


@pytest.fixture(scope="module")
def dit_models():
    from ditsep_amd import synthetic
    torch.set_num_threads(16)
    dcfg = synthetic.DiTConfig()
    vcfg = synthetic.OobleckConfig()
    dsd = synthetic.random_dit_weights(dcfg, 1, out_gain=0.002, skip_gain=0.02)
    vsd = synthetic.vae_weights(vcfg, 2, dec_in_gain=0.08)
    return dcfg, vcfg, dsd, vsd


@pytest.fixture(scope="module")
def ncsn_models():
    from ditsep_amd import synthetic
    torch.set_num_threads(16)
    ncfg = synthetic.NCSNppConfig()
    vcfg = synthetic.OobleckConfig()
    nsd = synthetic.random_ncsnpp_weights(ncfg, 1, out_gain=0.01)
    vsd = synthetic.vae_weights(vcfg, 2, dec_in_gain=0.08)
    return ncfg, vcfg, nsd, vsd


def _score_inputs(B, T, seed):
    g = torch.Generator().manual_seed(seed)
    xt = 3.0 * torch.randn((B, 2, 64, T), generator=g)
    mix = torch.randn((B, 1, 64, T), generator=g)
    t = torch.linspace(0.97, 0.03, B) if B > 1 else torch.tensor([0.6])
    return xt, t, mix


def _chain_with_oracle_items(eng, score, vsd, vcfg, y_full, src, pick, N, seed, tag, sdr_vs="sources"):
    """Run the N-step PC chain + decode natively on the whole batch (graphs on: eager, capture, replay) with the
    oracle's latents / noise planted in items `pick`; compare those items with the CPU oracle.

    sdr_vs: what the SI-SDR pair is measured against.  "sources": the synthetic sources (DiT: its linear skip path
    makes the sampler contract towards the mixture latent like a trained OU score, so the estimates correlate with the
    sources).  "operating-point": the random-init NCSN++ has no such path -- its estimates are uncorrelated with the
    sources (SI-SDR around -55 dB), where a dB delta measures the projection of a 1e-3 waveform error on a 1e-3
    correlation, not separation quality -- so the criterion is evaluated where a working separator operates: targets =
    oracle waveform + seeded noise 10 dB below it (SI-SDR of the reference ~ +10 dB); the raw figure against the
    sources is logged."""
    B, _, D, T = y_full.shape
    y_sel = y_full[list(pick)].cpu()
    draws = sampler.noise_draws(N, 1)
    noise_sel = sampler.draw_noise(seed, draws, (len(pick), 2, D, T))
    with torch.no_grad():
        x_ref, nfe_ref = sampler.pc_sample(score, y_sel, noise_sel, sampler.OUVE(N=N), eps=0.03, snr=0.5,
                                           corrector_steps=1, denoise=True, n_spkrs=2)
        wav_ref = ovae.decode_sources(vsd, vcfg, x_ref, L, "decoder.")
    noise = torch.randn((draws, B, 2, D, T), generator=torch.Generator().manual_seed(seed + 1))
    noise[:, list(pick)] = noise_sel
    noise = noise.to(eng.device)
    eng.enable_graphs(True)
    for rep in range(3):
        x, nfe = eng.pc_sample(y_full, noise, N=N, corrector_steps=1, snr=0.5, t_eps=0.03)
        wav = eng.decode(x, L)
        assert nfe == nfe_ref == 2 * N
        e_x, e_w = rel_l2(x[list(pick)], x_ref), rel_l2(wav[list(pick)], wav_ref)
        _log(f"{tag} rep {rep}: B={B} N={N} items {pick}: latent rel-L2 {e_x:.3e}, waveform rel-L2 {e_w:.3e}")
        assert e_x < REL_L2_TOL and e_w < REL_L2_TOL, (tag, rep, e_x, e_w)
    for j, b in enumerate(pick):               # per item as well: one bad panel must not hide in the average
        e = rel_l2(wav[b], wav_ref[j])
        assert e < REL_L2_TOL, (tag, b, e)
    tgt = src[list(pick)]
    s_gpu, p_gpu = metrics.si_sdr_pit(tgt, wav[list(pick)].cpu())
    s_ref, p_ref = metrics.si_sdr_pit(tgt, wav_ref)
    d = float((s_gpu - s_ref).abs().max())
    _log(f"{tag}: vs the synthetic sources: reference SI-SDR {float(s_ref.mean()):.1f} dB, |SI-SDR delta| {d:.4f} dB")
    if sdr_vs == "operating-point":
        g = torch.Generator().manual_seed(seed + 2)
        rms = wav_ref.pow(2).mean(-1, keepdim=True).sqrt()
        tgt = wav_ref + 10 ** (-10 / 20) * rms * torch.randn(wav_ref.shape, generator=g)
        s_gpu, p_gpu = metrics.si_sdr_pit(tgt, wav[list(pick)].cpu())
        s_ref, p_ref = metrics.si_sdr_pit(tgt, wav_ref)
        d = float((s_gpu - s_ref).abs().max())
        _log(f"{tag}: at a working separator's operating point: reference SI-SDR {float(s_ref.mean()):.1f} dB, "
             f"|SI-SDR delta| {d:.4f} dB")
    assert torch.equal(p_gpu, p_ref) and d < SI_SDR_TOL_DB, d
    return x, wav


# ------------------------------------------------------------------ DiT, the north-star score network
def test_dit_c2_batch64_score_call_vs_oracle(dit_models):
    """One dsn_score call at the benchmarked shape (fp16, B = 64, T = 32, M = 2112): the balanced row-panel kernels
    -- FF-in on 264-row panels with the masked 17th sub-tile and the folded LayerNorm, QKV + RoPE, split-K FF-out,
    to_out as the residual-stream producer with row statistics -- against oracle.dit.DiTScore over ALL 64 items,
    plus batch invariance against the skinny kernels (the same items as B = 2)."""
    dcfg, vcfg, dsd, vsd = dit_models
    xt, t, mix = _score_inputs(B64, T32, 70)
    with torch.no_grad():
        ref = odit.DiTScore(dsd, dcfg)(xt, t, mix)
    eng = make_engine(dcfg, dsd, precision=FP16)
    out = eng.score(xt, t, mix)
    assert torch.isfinite(out).all()
    e = rel_l2(out, ref)
    worst = max(rel_l2(out[b], ref[b]) for b in range(B64))
    _log(f"dit score call fp16 B=64: rel-L2 {e:.3e}, worst item {worst:.3e}")
    assert e < SCORE_CALL_TOL and worst < 2 * SCORE_CALL_TOL, (e, worst)
    assert torch.equal(eng.score(xt, t, mix), out)            # bit-reproducible
    for lo in (0, 30, 62):                                     # same items through the M = 66 skinny path
        small = eng.score(xt[lo:lo + 2], t[lo:lo + 2], mix[lo:lo + 2])
        d = rel_l2(out[lo:lo + 2], small)
        assert d < SCORE_CALL_TOL, (lo, d)
        assert rel_l2(small, ref[lo:lo + 2]) < SCORE_CALL_TOL
    eng.close()


def test_dit_c4_three_speakers_batch64_score_call_vs_oracle():
    """BASELINE config 4's score network (3 sources: io 192 + 64 concat channels) at the benchmark batch: one score
    call over 64 mixtures on the panel / fused-attention kernels against the CPU oracle (the N = 30 three-speaker
    chain with PIT runs at B = 2 in test_gpu_configs.py)."""
    from ditsep_amd import synthetic
    torch.set_num_threads(16)
    dcfg = synthetic.DiTConfig(n_src=3)
    dsd = synthetic.random_dit_weights(dcfg, 5, out_gain=0.002, skip_gain=0.02)
    g = torch.Generator().manual_seed(75)
    xt = 3.0 * torch.randn((B64, 3, 64, T32), generator=g)
    mix = torch.randn((B64, 1, 64, T32), generator=g)
    t = torch.linspace(0.97, 0.03, B64)
    with torch.no_grad():
        ref = odit.DiTScore(dsd, dcfg)(xt, t, mix)
    eng = make_engine(dcfg, dsd, precision=FP16)
    out = eng.score(xt, t, mix)
    e = rel_l2(out, ref)
    worst = max(rel_l2(out[b], ref[b]) for b in range(B64))
    _log(f"dit (3 speakers) score call fp16 B=64: rel-L2 {e:.3e}, worst item {worst:.3e}")
    assert e < SCORE_CALL_TOL and worst < 2 * SCORE_CALL_TOL, (e, worst)
    assert torch.equal(eng.score(xt, t, mix), out)
    eng.close()


@pytest.mark.parametrize("B,T,ipp,prec,tol", [(5, 8, 4, FP16, 4e-3), (7, 8, 16, FP16, 4e-3), (3, 40, 2, BF16, 3e-2),
                                               (2, 100, 1, FP16, 4e-3), (9, 31, 4, FP16, 4e-3), (1, 143, 1, FP16, 4e-3),
                                               (2, 235, 1, FP16, 4e-3), (3, 144, 1, BF16, 3e-2), (1, 239, 1, FP16, 4e-3)])
def test_fused_qkv_attention_odd_shapes_vs_oracle(B, T, ipp, prec, tol, monkeypatch):
    """qkv_attn.hip (to_qkv GEMM + rotary + attention in one launch) away from the benchmark shape, forced through
    DSN_QA_IPP on a 2-head DiT (generic head mapping, K = 128 = two k-tiles): a last panel with fewer items, panels of
    16 items of 9 tokens, 2 / 1 items of 41 / 101 / 144 tokens (3, 7 and 9 key tiles), bf16 operands, and the tall
    240-row tile (2-stage ring) at 236 (BASELINE config 5), 145 and 240 tokens; one score call
    against the CPU oracle at the tolerance of the unfused tiny-DiT tests, bit-reproducible."""
    monkeypatch.setenv("DSN_QA_IPP", str(ipp))
    dcfg = odit.DiTConfig(n_src=2, embed_dim=128, depth=2, num_heads=2)
    dsd = odit.random_dit_weights(dcfg, 32, out_gain=0.005)
    xt, t, mix = _score_inputs(B, T, 300 + B * T)
    with torch.no_grad():
        ref = odit.DiTScore(dsd, dcfg)(xt, t, mix)
    eng = make_engine(dcfg, dsd, precision=prec)
    out = eng.score(xt, t, mix)
    assert torch.isfinite(out).all()
    assert rel_l2(out, ref) < tol, rel_l2(out, ref)
    assert torch.equal(eng.score(xt, t, mix), out)
    eng.close()


def test_dit_c2_batch64_chain_n30_vs_oracle(dit_models):
    """BASELINE C2 at its own batch: 64 mixtures, N = 30 + 1 corrector (60 score calls on the M = 2112 panel
    kernels, hipGraph replay) + decode of 128 sequences; items 0 / 31 / 63 against the CPU oracle under the
    north-star bound."""
    from ditsep_amd import synthetic
    dcfg, vcfg, dsd, vsd = dit_models
    src = synthetic.synthetic_sources(B64, 2, L, 16000, seed=1234)
    eng = make_engine(dcfg, dsd, vcfg, vsd, precision=FP16)
    y = eng.encode(src.sum(1, keepdim=True), seed=7)
    assert y.shape[-1] == T32
    _chain_with_oracle_items(eng, odit.DiTScore(dsd, dcfg), vsd, vcfg, y, src, PICK, 30, 170, "dit-c2-b64")
    eng.close()


def test_dit_c5_fp8_long_form_chain_parity_figure(dit_models):
    """BASELINE config 5 in its named precision: 30 s mixture (T = 235, 236 tokens), fp8 (MX e4m3) DiT GEMMs,
    hipGraph-captured sampler loop (N = 3), against the fp32 oracle.  fp8 is a reported-only mode (3 mantissa
    bits cannot meet 1e-3): the tolerance is loose (5e-2 on the latent / waveform) and the figure is logged so
    config 5 has a parity number; the fp16 run of the same inputs must meet the 1e-3 bound."""
    from ditsep_amd import synthetic
    dcfg, vcfg, dsd, vsd = dit_models
    L5, N = 480000, 3
    src = synthetic.synthetic_sources(1, 2, L5, 16000, seed=99)
    e16 = make_engine(dcfg, dsd, vcfg, vsd, precision=FP16)
    y = e16.encode(src.sum(1, keepdim=True), seed=5)
    assert y.shape[-1] == 235
    noise = sampler.draw_noise(94, sampler.noise_draws(N, 1), (1, 2, 64, 235))
    with torch.no_grad():
        x_ref, _ = sampler.pc_sample(odit.DiTScore(dsd, dcfg), y.cpu(), noise, sampler.OUVE(N=N), eps=0.03, snr=0.5,
                                     corrector_steps=1, denoise=True, n_spkrs=2)
        wav_ref = ovae.decode_sources(vsd, vcfg, x_ref, L5, "decoder.")
    x16, _ = e16.pc_sample(y, noise, N=N, corrector_steps=1, snr=0.5, t_eps=0.03)
    assert rel_l2(x16, x_ref) < REL_L2_TOL
    e16.close()
    e8 = make_engine(dcfg, dsd, vcfg, vsd, precision=FP8)
    e8.enable_graphs(True)
    for rep in range(3):                                       # eager, capture, replay
        x8, nfe = e8.pc_sample(y, noise, N=N, corrector_steps=1, snr=0.5, t_eps=0.03)
        assert nfe == 6 and torch.isfinite(x8).all()
        ex = rel_l2(x8, x_ref)
        assert ex < 5e-2, (rep, ex)
    wav8 = e8.decode(x8, L5)
    ew = rel_l2(wav8, wav_ref)
    s8, p8 = metrics.si_sdr_pit(src, wav8.cpu())
    sr, pr = metrics.si_sdr_pit(src, wav_ref)
    _log(f"C5 fp8 (T=235, N={N}, graphs): latent rel-L2 {ex:.3e}, waveform rel-L2 {ew:.3e}, "
         f"|SI-SDR delta| {float((s8 - sr).abs().max()):.4f} dB (reported-only mode)")
    assert ew < 5e-2
    e8.close()


# ------------------------------------------------------------------ NCSN++, the score network the reference wires in
@pytest.mark.parametrize("B", [64, 1, 5])
def test_ncsnpp_full_size_fp16_score_call_vs_oracle(ncsn_models, B):
    """nf = 128 NCSN++ in the headline fp16 mode.  B = 64: igemm_halo3x3_kernel<1,256,4> at level 0 (>= 512
    workgroups), <1,128,1> at level 1, GroupNorm partials from the GEMM epilogues; B = 1: split-K +
    igemm_slab_epilogue_kernel; B = 5: a batch between the two regimes."""
    ncfg, vcfg, nsd, vsd = ncsn_models
    xt, t, mix = _score_inputs(B, T32, 80 + B)
    with torch.no_grad():
        ref = oncs.NCSNppScore(nsd, ncfg)(xt, t, mix)
    eng = make_engine(ncfg=ncfg, nsd=nsd, precision=FP16)
    out = eng.score(xt, t, mix)
    assert torch.isfinite(out).all()
    e = rel_l2(out, ref)
    worst = max(rel_l2(out[b], ref[b]) for b in range(B))
    _log(f"ncsnpp score call fp16 B={B}: rel-L2 {e:.3e}, worst item {worst:.3e}")
    assert e < SCORE_CALL_TOL and worst < 2 * SCORE_CALL_TOL, (e, worst)
    assert torch.equal(eng.score(xt, t, mix), out)
    eng.close()


def test_ncsnpp_groupnorm_epilogue_partials_describe_their_tensor(ncsn_models):
    """The GroupNorm (mean, M2) slice partials a conv GEMM's epilogue writes (igemm.hip::epilogue_gen, here the halo
    3x3 kernel on conv_in at the C2 batch) against the same statistics recomputed in fp64 from the tensor the launch
    stored.  Round 3 found the one-pass "shifted sums" form of these partials wrong in ~0.4 % of the (slice, quad)
    entries of one fixed accumulator position at B = 64 -- run-to-run different, invisible at B <= 16 -- while the
    tensor itself was right; the accumulation was rewritten (Chan's running update) and this test pins it."""
    ncfg, vcfg, nsd, vsd = ncsn_models
    B, T, nf, H0 = B64, T32, ncfg.nf, ncfg.image_size
    xt, t, mix = _score_inputs(B, T, 81)
    eng = make_engine(ncfg=ncfg, nsd=nsd, precision=FP16)
    for rep in range(2):
        eng.score(xt, t, mix)
        # conv_in's output = channels [nf, 2 nf) of the last up-path concat buffer; its partials = statistics slot 0
        out = eng.debug_read("ncs_cb8_f", (B * H0 * T * 2 * nf,)).view(B, H0 * T, 2 * nf)[:, :, nf:].double()
        S, Q = H0 * T // 64, nf // 4
        st = eng.debug_read("ncs_stats", (B * S * Q * 2,)).view(B, S, Q, 2).double()
        x = out.reshape(B, S, 64, Q, 4)
        mean = x.mean(dim=(2, 4))
        m2 = ((x - mean[:, :, None, :, None]) ** 2).sum(dim=(2, 4))
        bad = ((st[..., 0] - mean).abs() > 1e-5 + 1e-4 * mean.abs()) | ((st[..., 1] - m2).abs() > 1e-4 * m2)
        assert int(bad.sum()) == 0, (rep, int(bad.sum()), bad.nonzero()[:8].tolist())
    eng.close()


@pytest.mark.parametrize("B", [64, 8])
def test_ncsnpp_producer_finished_groupnorm_is_bit_identical(ncsn_models, B, monkeypatch):
    """GroupNorm_1 of a ResnetBlockBigGANpp finished by the conv that feeds it (igemm_halo3x3_kernel, GemmDesc::gnf_out:
    slice partials handed over between the row-tile workgroups of an image inside the launch, silu(GroupNorm(h)) written
    from the accumulators, no fp32 h, no gn_apply launch) against the separate statistics + apply pass
    (DSN_NO_GN_FIN=1): same combine order, same expression -> the same bits, launch after launch."""
    ncfg, vcfg, nsd, vsd = ncsn_models
    xt, t, mix = _score_inputs(B, T32, 91 + B)
    outs = []
    for off in (False, True):
        if off:
            monkeypatch.setenv("DSN_NO_GN_FIN", "1")
        eng = make_engine(ncfg=ncfg, nsd=nsd, precision=FP16)
        o = eng.score(xt, t, mix)
        assert torch.isfinite(o).all()
        for _ in range(3):
            assert torch.equal(eng.score(xt, t, mix), o)
        outs.append(o.clone())
        eng.close()
    assert torch.equal(outs[0], outs[1]), float((outs[0] - outs[1]).abs().max())


def test_ncsnpp_c2_batch64_chain_n30_vs_oracle(ncsn_models):
    """The reference's literal drop-in (LatentScoreModelNCSNpp) at the C2 batch: N = 30 chain + decode at B = 64,
    fp16, graphs on; items 0 / 31 / 63 against the CPU oracle under the north-star bound."""
    from ditsep_amd import synthetic
    ncfg, vcfg, nsd, vsd = ncsn_models
    src = synthetic.synthetic_sources(B64, 2, L, 16000, seed=1234)
    eng = make_engine(vcfg=vcfg, vsd=vsd, precision=FP16, ncfg=ncfg, nsd=nsd)
    y = eng.encode(src.sum(1, keepdim=True), seed=7)
    _chain_with_oracle_items(eng, oncs.NCSNppScore(nsd, ncfg), vsd, vcfg, y, src, PICK, 30, 180, "ncsnpp-c2-b64",
                             sdr_vs="operating-point")
    eng.close()


def test_ncsnpp_c2_batch2_chain_n30_vs_oracle(ncsn_models):
    """The same chain at B = 2 (the small-batch tile choices) and at B = 1 (split-K + slab epilogue)."""
    from ditsep_amd import synthetic
    ncfg, vcfg, nsd, vsd = ncsn_models
    src = synthetic.synthetic_sources(2, 2, L, 16000, seed=4321)
    eng = make_engine(vcfg=vcfg, vsd=vsd, precision=FP16, ncfg=ncfg, nsd=nsd)
    y = eng.encode(src.sum(1, keepdim=True), seed=9)
    _chain_with_oracle_items(eng, oncs.NCSNppScore(nsd, ncfg), vsd, vcfg, y, src, (0, 1), 30, 190, "ncsnpp-c2-b2",
                             sdr_vs="operating-point")
    _chain_with_oracle_items(eng, oncs.NCSNppScore(nsd, ncfg), vsd, vcfg, y[:1], src[:1], (0,), 30, 191, "ncsnpp-c2-b1",
                             sdr_vs="operating-point")
    eng.close()
