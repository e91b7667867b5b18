"""Shared helpers for the GPU parity tests: build a native Engine from the
oracle's seeded weights (reference key names)."""
import torch

from oracle import dit as odit
from oracle import oobleck as ovae
from oracle.make_golden import tiny_vae_weights


def rel_l2(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm())


def mx_exponent(x: torch.Tensor) -> torch.Tensor:
    """E8M0 exponent k of each block of 32 along the last dim: 2^k >= amax/448, k from the float exponent exactly as
    csrc/common.h::dsn_mx_exp (int32, one per block, flattened)"""
    amax = x.float().reshape(-1, 32).abs().amax(dim=1)
    scaled = (amax * torch.tensor(1.0 / 448.0, dtype=torch.float32)).float()
    bits = scaled.view(torch.int32)
    k = ((bits >> 23) & 0xff) - 127 + ((bits & 0x7fffff) != 0).to(torch.int32)
    return k.clamp(-126, 126)


def mx_quant(x: torch.Tensor) -> torch.Tensor:
    """CPU emulation of the device's fp8 operand format: blocks of 32 along the last dim, E8M0 scale 2^k with
    2^k >= amax/448 (mx_exponent), e4m3 round-to-nearest."""
    shp = x.shape
    xb = x.float().reshape(-1, 32)
    k = mx_exponent(x).float()
    q = (xb * torch.exp2(-k)[:, None]).clamp(-448, 448).to(torch.float8_e4m3fn).float() * torch.exp2(k)[:, None]
    return q.reshape(shp)


def make_engine(dcfg=None, dsd=None, vcfg=None, vsd=None, precision=2, ncfg=None, nsd=None, **kw):
    from ditsep_amd import native

    args = dict(precision=precision, score_kind=native.SCORE_NONE, vae_has_encoder=False, vae_has_decoder=False)
    if dcfg is not None:
        args.update(score_kind=native.SCORE_DIT, n_src=dcfg.n_src, latent_dim=dcfg.latent_dim,
                    dit_embed_dim=dcfg.embed_dim, dit_depth=dcfg.depth, dit_heads=dcfg.num_heads)
    if ncfg is not None:
        args.update(score_kind=native.SCORE_NCSNPP, n_src=ncfg.n_src, latent_dim=ncfg.image_size,
                    ncsn_nf=ncfg.nf, ncsn_ch_mult=ncfg.ch_mult, ncsn_num_res_blocks=ncfg.num_res_blocks,
                    ncsn_attn_resolution=ncfg.attn_resolutions[0], ncsn_image_size=ncfg.image_size,
                    ncsn_max_latent_length=ncfg.max_latent_length)
    if vcfg is not None:
        args.update(vae_channels=vcfg.channels, vae_c_mults=vcfg.c_mults, vae_strides=vcfg.strides,
                    vae_enc_latent_dim=vcfg.enc_latent_dim, vae_use_snake=vcfg.use_snake,
                    vae_final_tanh=vcfg.final_tanh, latent_dim=vcfg.latent_dim,
                    vae_has_encoder=any(k.startswith("encoder.") for k in vsd),
                    vae_has_decoder=any(k.startswith("decoder.") for k in vsd))
    args.update(kw)
    eng = native.Engine(**args)
    if dsd is not None:
        eng.load_state_dict(dsd, prefix="score_model.")
    if nsd is not None:
        eng.load_state_dict(nsd, prefix="score_model.")
    if vsd is not None:
        eng.load_state_dict(vsd, prefix="vae.")
    eng.finalize()
    return eng
