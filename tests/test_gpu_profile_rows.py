"""The per-call-site profile table (profile_begin / profile_end: `rows`, the implicit-GEMM family totals and the
HBM-bound totals) that bench.py prints, pinned from first principles: which call sites record, how many launches each,
and their algorithmic flops and bytes, all computed here from the model configuration and csrc/engine.hip's shape
rules -- not from a recorded run.  Flops and bytes are sums of products of small integers in double precision, so they
are compared exactly.  A profiled call must also return what the same call returns without profiling, bit for bit.

Small VAE: channels 64 with c_mults (1, 2, 4) gives both coders 128-channel blocks (the fused ResidualUnit kernel) and
64-channel blocks (the two-GEMM ResidualUnit).  Tiny DiT: embed_dim 256 = 4 heads x 64, depth 2, single-plane fp16.
"""
import pytest
import torch

from ditsep_amd import synthetic
from tests.util import make_engine

pytestmark = pytest.mark.gpu

FP16 = 3
P = 1                      # operand planes of the single-plane modes
S, T = 2, 16               # VAE: sequences and latent frames
VCFG = synthetic.OobleckConfig(channels=64, c_mults=(1, 2, 4), strides=(2, 2, 2))
DCFG = synthetic.DiTConfig(n_src=2, embed_dim=256, depth=2, num_heads=4)
QA_MAX_ROWS = 240          # tallest panel of the fused to_qkv + attention kernel (qkv_attn.hip)


def cdiv(a, b):
    return -(-a // b)


def gemm_flops(M, N, taps, Cin):
    return 2.0 * M * N * taps * Cin


class Expect(dict):
    """site -> [launches, flops, bytes]"""

    def add(self, site, launches=1, flops=0.0, nbytes=0.0):
        row = self.setdefault(site, [0, 0.0, 0.0])
        row[0] += launches
        row[1] += flops
        row[2] += nbytes


def add_res_units(exp, ch, rows):
    """The three ResidualUnits of a block on `rows` = S * L positions of `ch` channels (engine.hip: res_unit, run_ru)."""
    for j in range(3):
        if ch == 128:      # fused: k7 + k1 = 8 taps of 128 x 128; planes in, fp32 in, fp32 out (kept for units 0, 1), planes out
            exp.add("vae.residual_unit_fused", 1, 2.0 * rows * 128 * 128 * 8,
                    rows * 128.0 * (2.0 * P + 4.0 + (4.0 if j < 2 else 0.0) + 2.0 * P))
        else:
            exp.add("vae.residual_unit_2gemm", 2, gemm_flops(rows, ch, 7, ch) + gemm_flops(rows, ch, 1, ch))


def decoder_expect(cfg, S, T):
    m, ch, exp = cfg.mults, cfg.channels, Expect()
    exp.add("vae.dec_conv_in", 1, gemm_flops(S * T, m[-1] * ch, 7, cfg.latent_dim))
    L = T
    for i in range(len(m) - 1, 0, -1):
        cin, cout, st = m[i] * ch, m[i - 1] * ch, cfg.strides[i - 1]
        exp.add("vae.dec_convT", 1, gemm_flops(S * (L + 1), st * cout, 2, cin))   # 2-tap phase GEMM over L + 1 rows
        L *= st
        add_res_units(exp, cout, S * L)
    exp.add("vae.dec_conv_out", 1, 0.0, S * L * (m[0] * ch * 2.0 * P + 4.0))
    return exp


def encoder_expect(cfg, S, L):
    m, ch, exp = cfg.mults, cfg.channels, Expect()
    for i in range(len(m) - 1):
        cin, cout, st = m[i] * ch, m[i + 1] * ch, cfg.strides[i]
        add_res_units(exp, cin, S * L)
        L //= st
        exp.add("vae.enc_strided_conv", 1, gemm_flops(S * L, cout, 2 * st, cin))
    exp.add("vae.enc_conv_out", 1, gemm_flops(S * L, cfg.enc_latent_dim, 3, m[-1] * ch))
    return exp


NOT_GEMM = {"vae.dec_conv_out", "dit.residual_norm", "dit.attention"}      # records outside the implicit-GEMM family


def check_table(prof, exp, with_bytes):
    rows = {r["site"]: r for r in prof["rows"]}
    assert len(rows) == len(prof["rows"]) and set(rows) == set(exp)
    for site, (launches, flops, nbytes) in exp.items():
        r = rows[site]
        assert r["launches"] == launches, (site, r)
        assert r["flops"] == flops, (site, r, flops)
        if with_bytes:
            assert r["bytes"] == nbytes, (site, r, nbytes)
    assert prof["gemm_launches"] == sum(v[0] for k, v in exp.items() if k not in NOT_GEMM)
    assert prof["gemm_flops"] == sum(v[1] for v in exp.values())
    fused = exp.get("vae.residual_unit_fused", [0, 0.0, 0.0])
    assert prof["hbm_launches"] == fused[0] and prof["hbm_bytes"] == fused[2]


@pytest.fixture(scope="module")
def vae_engine():
    eng = make_engine(vcfg=VCFG, vsd=synthetic.vae_weights(VCFG, 7), precision=FP16, n_src=S)
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def dit_engine():
    eng = make_engine(DCFG, synthetic.random_dit_weights(DCFG, 8, out_gain=0.01), precision=FP16)
    yield eng
    eng.close()


def profiled(eng, call):
    plain = call()
    eng.profile_begin()
    out = call()
    prof = eng.profile_end()
    assert torch.equal(out, plain)
    return prof


def test_decode_profile_rows(vae_engine):
    exp = decoder_expect(VCFG, S, T)
    nb = len(VCFG.c_mults)
    # both ResidualUnit kinds, and the launch counts of the issue spelled out
    assert exp["vae.dec_convT"][0] == nb and exp["vae.dec_conv_in"][0] == exp["vae.dec_conv_out"][0] == 1
    assert exp["vae.residual_unit_fused"][0] == 3 and exp["vae.residual_unit_2gemm"][0] == 2 * 3 * (nb - 1)
    est = torch.randn((1, S, VCFG.latent_dim, T), generator=torch.Generator().manual_seed(1))
    check_table(profiled(vae_engine, lambda: vae_engine.decode(est)), exp, with_bytes=True)


def test_encode_profile_rows(vae_engine):
    L = VCFG.hop * T - 1                                        # padded to T frames
    assert vae_engine.latent_frames(L) == T
    exp = encoder_expect(VCFG, S, VCFG.hop * T)
    nb = len(VCFG.c_mults)
    assert exp["vae.enc_strided_conv"][0] == nb and exp["vae.enc_conv_out"][0] == 1
    assert exp["vae.residual_unit_fused"][0] == 3 and exp["vae.residual_unit_2gemm"][0] == 2 * 3 * (nb - 1)
    g = torch.Generator().manual_seed(2)
    wav = 0.3 * torch.randn((S, 1, L), generator=g)
    noise = torch.randn((S, VCFG.latent_dim, T), generator=g)
    check_table(profiled(vae_engine, lambda: vae_engine.encode(wav, noise)), exp, with_bytes=True)


def dit_expect(cfg, B, T, qa_force):
    """dit_forward's shape rules in the single-plane fp16 mode (skinny window, folded ff_norm, fused to_qkv + attention)
    and the records they lead to."""
    D, H, depth = cfg.embed_dim, cfg.num_heads, cfg.depth
    Sq, Mt = T + 1, B * T
    M = B * Sq
    skinny = M <= 80 and D % 256 == 0
    fold = False
    if D % 64 == 0 and not skinny:                              # panels of at most 80 rows that fill whole rounds
        fold = any(cdiv(M, 256 * rounds // cdiv(D, 128)) <= 80 for rounds in range(1, 5))
    qa_ipp = 0
    if not skinny and D == H * 64 and Sq <= QA_MAX_ROWS:
        ipp = min(B, max(1, 144 // Sq))
        while ipp > 1 and cdiv(B, ipp) * H < 256:
            ipp -= 1
        if cdiv(B, ipp) * H >= 128:
            qa_ipp = ipp
        if qa_force and qa_force * Sq <= QA_MAX_ROWS:
            qa_ipp = qa_force
    exp = Expect()
    exp.add("dit.project_in", 1, gemm_flops(Mt, D, 1, cfg.dim_in))
    exp.add("dit.time_embed", 2, gemm_flops(B, D, 1, 256) + gemm_flops(B, D, 1, D))
    exp.add("dit.residual_norm", (depth if fold else 2 * depth) + 1)
    if qa_ipp:
        exp.add("dit.qkv_attention", depth, depth * (gemm_flops(M, 3 * D, 1, D) + 4.0 * B * H * Sq * Sq * 64))
    else:
        exp.add("dit.qkv", depth, depth * gemm_flops(M, 3 * D, 1, D))
        exp.add("dit.attention", depth)
    exp.add("dit.attn_out", depth, depth * gemm_flops(M, D, 1, D))
    exp.add("dit.ff_in", depth, depth * gemm_flops(M, 8 * D, 1, D))
    exp.add("dit.ff_out", depth, depth * gemm_flops(M, D, 1, 4 * D))
    exp.add("dit.project_out", 1, gemm_flops(Mt, cfg.io_channels, 1, D))
    return exp, skinny, fold, qa_ipp


@pytest.mark.parametrize("B,T,qa_force,family", [(1, 16, 0, "skinny"), (4, 31, 0, "panel"), (4, 31, 2, "panel+fused")])
def test_score_profile_rows(dit_engine, B, T, qa_force, family, monkeypatch):
    for name in ("DSN_SKINNY_MAX", "DSN_QA_IPP"):
        monkeypatch.delenv(name, raising=False)
    if qa_force:       # the rule wants half a round of workgroups (panels x heads >= 128) before it fuses: not at this size
        monkeypatch.setenv("DSN_QA_IPP", str(qa_force))
    exp, skinny, fold, qa_ipp = dit_expect(DCFG, B, T, qa_force)
    assert (skinny, fold, bool(qa_ipp)) == {"skinny": (True, False, False), "panel": (False, True, False),
                                            "panel+fused": (False, True, True)}[family]
    g = torch.Generator().manual_seed(10 * B + T)
    xt = torch.randn((B, DCFG.n_src, DCFG.latent_dim, T), generator=g)
    mix = torch.randn((B, 1, DCFG.latent_dim, T), generator=g)
    t = torch.linspace(0.9, 0.2, B)
    check_table(profiled(dit_engine, lambda: dit_engine.score(xt, t, mix)), exp, with_bytes=False)
