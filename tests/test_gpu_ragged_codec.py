"""The codec on a ragged batch as ONE padded pass (dsn_decode_ragged / dsn_encode_ragged / dsn_separate_ragged): the
tail-zero kernel alone, the padded pass against the grouped one (one codec call per group of equal frame count, which
is what every item gets alone) on one engine, the padded route against the CPU oracle run on every item alone, graph
replay with the lengths as data, the refusals, and the dense decode's launch sequence.

Bounds: padded against grouped is the same network on the same operand planes -- rounding of the operands does not
differ, only the summation order where a layer's split-K factor depends on the batch's row count (pick_ksplit) -- so
the bounds are those of tests/test_gpu_ragged_paths.py for the same precisions, 1e-4 (bf16x3) and 4e-3 (fp16) rel-L2
per item over its valid samples; against the oracle the end-to-end bound of test_separate_ragged_vs_oracle, 1e-3."""
import ctypes as C

import pytest
import torch

from ditsep_amd import native
from oracle import oobleck as ovae
from oracle.make_golden import tiny_vae_weights
from tests.test_gpu_gemm_kernels import FP16, X3
from tests.test_gpu_ragged_paths import DCFG, LENGTHS, N_STEPS, dsd, e2e, vae  # noqa: F401  (fixtures)
from tests.util import make_engine, rel_l2

pytestmark = pytest.mark.gpu

N_SRC = 2
FRAMES, T = [1, 5, 2, 5, 3], 5      # 1 frame: shorter than the dilation-9 reach; two items at T: a group of two
SITE = "vae.ragged_tail_zero"


# ------------------------------------------------------------------ the kernel alone
@pytest.mark.parametrize("prec", [X3, FP16], ids=["bf16x3", "fp16"])
@pytest.mark.parametrize("Cn", [8, 128])
def test_tail_zero_kernel(prec, Cn):
    """S = 4 items of L = 24 rows, rep = 2, mul = 4, frames = [1, 6]: items 0, 1 keep 4 rows, items 2, 3 all 24"""
    eng = make_engine(precision=prec)
    S, L, rep, mul = 4, 24, 2, 4
    P = eng._PLANES[prec][0]
    dev = eng.device
    frames = torch.tensor([1, 6], dtype=torch.int32, device=dev)
    n = S * L * Cn
    planes0 = (torch.arange(P * n, device=dev) % 30000 + 1).to(torch.int16).reshape(P, n)
    xf0 = (torch.arange(n, device=dev, dtype=torch.float32) + 1.0).reshape(S, L, Cn)
    of0 = -xf0 - 0.5
    valid = native.codec_valid_rows([1, 6], rep, mul, S)
    assert valid == [4, 4, 24, 24]

    def run(with_planes=True, with_x=True, with_out=True):
        pl, xf, of = planes0.clone(), xf0.clone(), of0.clone()
        eng.test_kernel("codec_tail_zero", B=S, L=L, C=Cn, rep=rep, mul=mul, lens=frames,
                        out_planes=pl if with_planes else None, x=xf if with_x else None,
                        out_f32=of if with_out else None)
        torch.cuda.synchronize()
        return pl, xf, of

    def check(pl, xf, of, with_planes=True, with_x=True, with_out=True):
        for got, ref, used in ((xf, xf0, with_x), (of, of0, with_out)):
            if not used:
                assert torch.equal(got, ref), "a null destination's buffer was written"
                continue
            for s, v in enumerate(valid):
                assert torch.equal(got[s, :v], ref[s, :v]), f"item {s}: valid rows changed"
                assert (got[s, v:] == 0).all(), f"item {s}: tail rows not zero"
        plv, plr = pl.reshape(P, S, L, Cn), planes0.reshape(P, S, L, Cn)
        if not with_planes:
            assert torch.equal(pl, planes0)
            return
        for p in range(P):
            for s, v in enumerate(valid):
                assert torch.equal(plv[p, s, :v], plr[p, s, :v]), f"plane {p} item {s}: valid rows changed"
                assert (plv[p, s, v:] == 0).all(), f"plane {p} item {s}: tail rows not zero"

    check(*run())
    for off in ("with_planes", "with_x", "with_out"):                   # each destination null once
        kw = {off: False}
        check(*run(**kw), **kw)
    # refused by name: a channel count that is no multiple of 8, rows past L
    with pytest.raises(RuntimeError, match="multiple of 8"):
        eng.test_kernel("codec_tail_zero", B=S, L=L, C=12, rep=rep, mul=mul, lens=frames, x=xf0.clone())
    with pytest.raises(RuntimeError, match=r"outside \[0, L = 24\]"):
        eng.test_kernel("codec_tail_zero", B=S, L=L, C=Cn, rep=rep, mul=5, lens=frames, x=xf0.clone())
    eng.close()


# ------------------------------------------------------------------ padded against grouped on one engine
def vae_case(kind, act):
    """'tiny': the 32-channel fixture configuration (2-GEMM ResidualUnits but for its one 128-channel block); 'fused':
    128-channel blocks only, where ru_fusable holds and the fused ResidualUnit kernel runs"""
    snake = act == "snake"
    if kind == "tiny":
        cfg = ovae.OobleckConfig(channels=32, use_snake=snake)
        return cfg, tiny_vae_weights(cfg, 21)
    cfg = ovae.OobleckConfig(channels=128, c_mults=(1, 2), strides=(2, 4), use_snake=snake)
    return cfg, tiny_vae_weights(cfg, 23)


def sites_of(eng, fn):
    eng.profile_begin()
    fn()
    return {r["site"]: r for r in eng.profile_end()["rows"]}


def units_ok(kind, rows):
    """the ResidualUnit call sites of a profiled ragged pass: 'tiny' runs the 2-GEMM path (all its blocks but the
    128-channel one), 'fused' nothing but the fused kernel"""
    if kind == "tiny":
        assert "vae.residual_unit_2gemm" in rows, sorted(rows)
    else:
        assert "vae.residual_unit_fused" in rows and "vae.residual_unit_2gemm" not in rows, sorted(rows)


@pytest.mark.parametrize("prec,tol", [(X3, 1e-4), (FP16, 4e-3)], ids=["bf16x3", "fp16"])
@pytest.mark.parametrize("act", ["elu", "snake"])
@pytest.mark.parametrize("kind", ["tiny", "fused"])
def test_padded_vs_grouped(kind, act, prec, tol):
    cfg, sd = vae_case(kind, act)
    eng = make_engine(vcfg=cfg, vsd=sd, precision=prec, n_src=N_SRC)
    hop, B, nb = cfg.hop, len(FRAMES), len(cfg.strides)
    assert eng.hop_length == hop
    g = torch.Generator().manual_seed(71)
    # ---- decode: finite garbage in the padded region of est
    est = torch.randn((B, N_SRC, cfg.latent_dim, T), generator=g)
    for b, f in enumerate(FRAMES):
        est[b, ..., f:] = 10.0 * est[b, ..., f:] + 3.0
    full = [hop * T] * B
    grouped = eng.decode_ragged(est, FRAMES, [f * hop for f in FRAMES])
    padded = eng.decode_ragged(est, FRAMES, full, codec="padded")
    for b, f in enumerate(FRAMES):
        err = rel_l2(padded[b][:, :f * hop], grouped[b])
        print(f"decode {kind} {act} prec {prec} item {b} ({f} frames): rel-L2 {err:.3e} (bound {tol:.0e})")
        assert err < tol, f"decode item {b}: rel-L2 {err:.3e} >= {tol:.0e}"
        assert (padded[b][:, f * hop:] == 0).all(), f"decode item {b}: wav past its end is not zero"
    rows = sites_of(eng, lambda: eng.decode_ragged(est, FRAMES, full, codec="padded"))
    # one tail launch after the latent pack, conv_in, every transposed conv, every ResidualUnit and conv_out
    assert SITE in rows and rows[SITE]["launches"] == 2 + 4 * nb + 1 and rows[SITE]["bytes"] > 0, rows.get(SITE)
    units_ok(kind, rows)
    # ---- encode
    lens = [f * hop - 1 - b % 3 for b, f in enumerate(FRAMES)]         # (hop is 8 in the fused configuration)
    assert [eng.latent_frames(L) for L in lens] == FRAMES
    mixes = [0.3 * torch.randn((1, L), generator=g) for L in lens]
    vn = [torch.randn((cfg.latent_dim, f), generator=g) for f in FRAMES]
    yg, fg = eng.encode_ragged(mixes, vn)
    yp, fp = eng.encode_ragged(mixes, vn, codec="padded")
    assert fg == fp == FRAMES and yg.shape == yp.shape == (B, 1, cfg.latent_dim, T)
    for b, f in enumerate(FRAMES):
        err = rel_l2(yp[b, ..., :f], yg[b, ..., :f])
        print(f"encode {kind} {act} prec {prec} item {b} ({f} frames): rel-L2 {err:.3e} (bound {tol:.0e})")
        assert err < tol, f"encode item {b}: rel-L2 {err:.3e} >= {tol:.0e}"
        assert (yp[b, ..., f:] == 0).all(), f"encode item {b}: latent past its end is not zero"
    rows = sites_of(eng, lambda: eng.encode_ragged(mixes, vn, codec="padded"))
    # conv_in1, every ResidualUnit, every strided conv, conv_out
    assert SITE in rows and rows[SITE]["launches"] == 1 + 4 * nb + 1, rows.get(SITE)
    units_ok(kind, rows)
    eng.close()


# ------------------------------------------------------------------ padded route against the oracle
@pytest.mark.parametrize("prec", [X3, FP16], ids=["bf16x3", "fp16"])
def test_separate_ragged_padded_vs_oracle(dsd, vae, e2e, prec):
    """the fixture of test_separate_ragged_vs_oracle: three mixtures, pipeline.separate of each alone"""
    vcfg, vsd = vae
    mixes, vae_noise, noise, wavs = e2e
    eng = make_engine(DCFG, dsd, vcfg, vsd, precision=prec)
    est, nfe = eng.separate_ragged(mixes, vae_noise=vae_noise, noise=noise, N=N_STEPS, corrector_steps=1, snr=0.5,
                                   t_eps=0.03, codec="padded")
    assert nfe == N_STEPS * 2 and len(est) == len(mixes)
    for b, L in enumerate(LENGTHS):
        assert tuple(est[b].shape) == (2, L)
        err = rel_l2(est[b], wavs[b])
        print(f"separate_ragged padded prec {prec} item {b} (L {L}): rel-L2 {err:.3e}")
        assert err < 1e-3, f"item {b}: rel-L2 {err:.3e} >= 1e-3"
    eng.close()


def test_facade_and_evaluation_pass_codec_through(dsd, vae, e2e, tmp_path):
    """LatentDiffSep.separate_batch and evaluate_batches with codec="padded": the same oracle, and tail launches in
    the evaluation route's decode"""
    from ditsep_amd import LatentDiffSep
    from ditsep_amd.evaluate import evaluate_batches
    from tests.test_gpu_kernels import _tiny_config

    vcfg, vsd = vae
    mixes, vae_noise, noise, wavs = e2e
    model = LatentDiffSep(_tiny_config(tmp_path), precision="bf16x3")
    sd = {"score_model." + k: v for k, v in dsd.items()}
    sd.update({"vae." + k: v for k, v in vsd.items()})
    model.load_state_dict(sd)
    est, nfe = model.separate_batch(mixes, vae_noise=vae_noise, noise=noise, codec="padded")
    assert nfe == N_STEPS * 2
    for b in range(len(mixes)):
        err = rel_l2(est[b], wavs[b])
        print(f"separate_batch padded item {b}: rel-L2 {err:.3e}")
        assert tuple(est[b].shape) == (2, LENGTHS[b]) and err < 1e-3
    with pytest.raises(ValueError, match="codec must be one of"):
        model.separate_batch(mixes, codec="fused")
    res = evaluate_batches(model, [(list(mixes), list(wavs))], 16000, N=N_STEPS, seed=3, codec="padded")
    assert sorted(res) == [0, 1, 2]
    for b, rec in res.items():
        assert rec["len_s"] == LENGTHS[b] / 16000 and rec["nfe"] == N_STEPS * 2
        assert len(rec["si_sdr"]) == 2 and all(v == v for v in rec["si_sdr"])
    model.close()


# ------------------------------------------------------------------ graphs
def test_decode_ragged_graphs():
    """the lengths are data of the captured graph: eager warm-up, capture and replay with one set of lengths, then
    replays with another at the same (B, T); each equals the ungraphed result bit for bit"""
    cfg, sd = vae_case("tiny", "elu")
    eng = make_engine(vcfg=cfg, vsd=sd, precision=X3, n_src=N_SRC)
    g = torch.Generator().manual_seed(72)
    est = torch.randn((len(FRAMES), N_SRC, cfg.latent_dim, T), generator=g)
    full = [cfg.hop * T] * len(FRAMES)
    sets = (FRAMES, [5, 2, 4, 1, 1])
    eager = [torch.stack(eng.decode_ragged(est, fr, full, codec="padded")).clone() for fr in sets]
    assert not torch.equal(eager[0], eager[1])
    before = None
    eng.enable_graphs(True)
    for k, (fr, ref) in enumerate(((sets[0], eager[0]),) * 3 + ((sets[1], eager[1]),) * 2 + ((sets[0], eager[0]),)):
        out = torch.stack(eng.decode_ragged(est, fr, full, codec="padded"))
        assert torch.equal(out, ref), f"graphs call {k} (frames {fr}): differs from the ungraphed result"
        if k == 2:
            before = eng.workspace_bytes()
    assert eng.workspace_bytes() == before, "another set of lengths grew the workspace (a new graph key?)"
    eng.close()


# ------------------------------------------------------------------ refusals
def test_codec_ragged_refusals_launch_nothing():
    cfg, sd = vae_case("tiny", "elu")
    B, hop = 3, cfg.hop
    est = torch.zeros((B, N_SRC, cfg.latent_dim, T), device="cuda")
    wav = torch.zeros((B, N_SRC, hop * T), device="cuda")
    mix = torch.zeros((B, 1, hop * T), device="cuda")
    y = torch.zeros((B, 1, cfg.latent_dim, T), device="cuda")

    def refused(eng, frames, reason, decode=True, encode=True):
        fr = (C.c_int32 * B)(*frames)
        before = eng.workspace_bytes()
        calls = []
        if decode:
            calls.append(lambda: eng.lib.dsn_decode_ragged(eng.ctx, native._ptr(est), fr, native._ptr(wav), B, T,
                                                           eng._stream()))
        if encode:
            calls.append(lambda: eng.lib.dsn_encode_ragged(eng.ctx, native._ptr(mix), fr, None, 0, native._ptr(y), B, T,
                                                           eng._stream()))
        for call in calls:
            rc = call()
            msg = eng.lib.dsn_last_error(eng.ctx).decode()
            assert rc != 0 and reason in msg, (rc, msg)
        assert eng.workspace_bytes() == before, "a refused call grew the workspace"

    eng = make_engine(vcfg=cfg, vsd=sd, precision=X3, n_src=N_SRC)          # no score network: the codec needs none
    refused(eng, (5, 0, 3), "frames[1] = 0 outside [1, T = 5]")
    refused(eng, (5, 2, 6), "frames[2] = 6 outside [1, T = 5]")
    with pytest.raises(ValueError, match=r"frames\[2\] = 6 outside"):
        eng.decode_ragged(est, (5, 2, 6), [hop * T] * B, codec="padded")
    # dsn_separate_ragged is the sampler's route: DiT only
    opts = native.DsnSamplerOpts(0, 0, 1, 0.5, 0.03, 1, None, None, None)
    nfe = C.c_int()
    before = eng.workspace_bytes()
    rc = eng.lib.dsn_separate_ragged(eng.ctx, native._ptr(mix), (C.c_int32 * B)(5, 2, 3), None, None, 0, native._ptr(wav),
                                     B, T, N_STEPS, C.byref(opts), C.byref(nfe), eng._stream())
    assert rc != 0 and "need the DiT score network" in eng.lib.dsn_last_error(eng.ctx).decode()
    assert eng.workspace_bytes() == before
    eng.close()
    enc_only = make_engine(vcfg=cfg, vsd={k: v for k, v in sd.items() if k.startswith("encoder.")}, precision=X3,
                           n_src=N_SRC)
    refused(enc_only, (5, 2, 3), "decoder not configured", encode=False)
    enc_only.close()
    dec_only = make_engine(vcfg=cfg, vsd={k: v for k, v in sd.items() if k.startswith("decoder.")}, precision=X3,
                           n_src=N_SRC)
    refused(dec_only, (5, 2, 3), "encoder not configured", decode=False)
    dec_only.close()


# ------------------------------------------------------------------ the dense path
def test_dense_decode_has_no_tail_launch():
    cfg, sd = vae_case("tiny", "elu")
    eng = make_engine(vcfg=cfg, vsd=sd, precision=X3, n_src=N_SRC)
    g = torch.Generator().manual_seed(73)
    est = torch.randn((2, N_SRC, cfg.latent_dim, 3), generator=g)
    mix = 0.3 * torch.randn((2, 1, 4000), generator=g)
    dense = sites_of(eng, lambda: eng.decode(est))
    assert dense and SITE not in dense, sorted(dense)
    assert SITE not in sites_of(eng, lambda: eng.encode(mix, seed=1))
    assert SITE not in sites_of(eng, lambda: eng.decode_ragged(est, [3, 3], [6000, 6000]))
    padded = sites_of(eng, lambda: eng.decode_ragged(est, [3, 2], [6000, 4000], codec="padded"))
    assert set(padded) == set(dense) | {SITE}, (sorted(padded), sorted(dense))
    eng.close()
