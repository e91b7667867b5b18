"""ctypes binding of libditsep_hip.so (C-ABI: include/ditsep_hip.h).

The HIP library is the product; this module only marshals torch device tensors
(raw pointers + the current HIP stream) across the C boundary.  There is no
fallback: if the library is missing or a call fails, a RuntimeError is raised.
"""
from __future__ import annotations

import ctypes as C
import math
import os
import warnings
from typing import Mapping, Optional

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("DSN_LIB", os.path.join(_HERE, "libditsep_hip.so"))

PREC_BF16 = 1
PREC_BF16X3 = 2
PREC_FP16 = 3
PREC_FP16X3 = 4
PREC_FP8 = 5
SCORE_NONE, SCORE_DIT, SCORE_NCSNPP = 0, 1, 2
MAX_VAE_BLOCKS = 8

EXPORTS = [
    "dsn_create", "dsn_destroy", "dsn_last_error", "dsn_load_tensor", "dsn_finalize_weights", "dsn_finalize_weights_ex",
    "dsn_score", "dsn_score_ragged", "dsn_pc_sample_ragged", "dsn_decode_ragged", "dsn_encode_ragged",
    "dsn_separate_ragged", "dsn_ouve_schedule", "dsn_pc_sample", "dsn_pc_sample_sched", "dsn_pc_sample_ex", "dsn_pc_sample_mix", "dsn_sb_sample", "dsn_decode",
    "dsn_encode", "dsn_decode_chunked", "dsn_encode_chunked",
    "dsn_latent_frames", "dsn_hop_length", "dsn_separate", "dsn_enable_graphs",
    "dsn_workspace_bytes", "dsn_profile_begin", "dsn_profile_end", "dsn_profile_hbm", "dsn_profile_rows",
    "dsn_test_gemm", "dsn_test_kernel", "dsn_dit_plan", "dsn_bench_igemm", "dsn_debug_read", "dsn_si_sdr_pit", "dsn_si_bss_eval",
    "dsn_stoi", "dsn_ode_sample", "dsn_score_loss", "dsn_composite", "dsn_mrstft_loss",
    "dsn_si_bss_eval_ragged", "dsn_stoi_ragged", "dsn_composite_ragged", "dsn_window_stitch",
    "dsn_score_window_plan", "dsn_score_windowed", "dsn_pc_sample_windowed", "dsn_separate_windowed",
    "dsn_resample_plan", "dsn_resample_length", "dsn_resample",
    "dsn_pcm_decode", "dsn_pcm_encode", "dsn_scale_output",
    "dsn_bss_eval", "dsn_bss_eval_plan",
    "dsn_mask_refine",
    "dsn_ensemble_combine",
    "dsn_stems", "dsn_pcm_encode_frames",
    "dsn_beamform", "dsn_beamform_spatial", "dsn_beamform_track", "dsn_dereverb",
    "dsn_beamform_design", "dsn_beamform_spatial_design", "dsn_beamform_track_design", "dsn_beamform_solve",
    "dsn_score_loss_ragged", "dsn_mrstft_loss_ragged",
    "dsn_kweight_coeffs", "dsn_loudness", "dsn_apply_gain",
    "dsn_limiter_curve", "dsn_apply_curve",
    "dsn_activity", "dsn_activity_gate",
]


PREDICTORS = {"reverse_diffusion": 0, "euler_maruyama": 1, "none": 2}
CORRECTORS = {"ald": 0, "langevin": 1}


class DsnSamplerOpts(C.Structure):
    _fields_ = [
        ("predictor", C.c_int), ("corrector", C.c_int), ("corrector_steps", C.c_int),
        ("snr", C.c_float), ("t_eps", C.c_float), ("denoise", C.c_int),
        ("timesteps", C.POINTER(C.c_float)), ("prior_mean", C.c_void_p), ("intermediates", C.c_void_p),
    ]


class DsnMixOpts(C.Structure):
    _fields_ = [
        ("prior_mix", C.c_int), ("d_lambda", C.c_float), ("sigma_min", C.c_float), ("sigma_max", C.c_float),
        ("avg_len", C.c_int), ("predictor", C.c_int), ("corrector", C.c_int), ("corrector_steps", C.c_int),
        ("snr", C.c_float), ("t_eps", C.c_float), ("denoise", C.c_int),
    ]


class DsnOdeOpts(C.Structure):
    _fields_ = [
        ("method", C.c_int), ("rtol", C.c_double), ("atol", C.c_double), ("t_eps", C.c_double), ("denoise", C.c_int),
        ("N", C.c_int), ("first_step", C.c_double), ("max_step", C.c_double), ("max_attempts", C.c_int),
    ]


class DsnOdeStats(C.Structure):
    _fields_ = [
        ("nfev", C.c_int), ("n_accepted", C.c_int), ("n_rejected", C.c_int), ("t_final", C.c_double),
        ("status", C.c_int),
    ]


class DsnLossOpts(C.Structure):
    _fields_ = [("mode", C.c_int), ("reduction", C.c_int), ("t_eps", C.c_float)]


class DsnCompositeOut(C.Structure):
    _fields_ = [(k, C.POINTER(C.c_float)) for k in ("llr", "wss", "segsnr", "snr", "csig", "cbak", "covl")] + [
        ("frames", C.POINTER(C.c_int))]


class DsnBssEvalOpts(C.Structure):
    _fields_ = [("filter_length", C.c_int), ("perm_by", C.c_int), ("clamp_db", C.c_double), ("load_diag", C.c_double),
                ("sir_sar", C.c_int), ("workspace_budget", C.c_int64)]


class DsnBssEvalOut(C.Structure):
    _fields_ = [(k, C.POINTER(C.c_double)) for k in ("sdr", "sir", "sar", "sdr_pairs", "sir_pairs")] + [
        ("perm_out", C.POINTER(C.c_int)), ("status", C.POINTER(C.c_int))]


class DsnMrstftConfig(C.Structure):
    _fields_ = [("n_res", C.c_int), ("fft", C.POINTER(C.c_int)), ("hop", C.POINTER(C.c_int)),
                ("win", C.POINTER(C.c_int)), ("w_sc", C.c_float), ("w_log_mag", C.c_float), ("w_lin_mag", C.c_float),
                ("taps", C.POINTER(C.c_float)), ("n_taps", C.c_int)]


class DsnMrstftOut(C.Structure):
    _fields_ = [(k, C.POINTER(C.c_double)) for k in ("sc", "log_mag", "lin_mag", "l1", "l2")]


MRSTFT_FFT_SIZES = (2048, 1024, 512, 256, 128, 64, 32)
MRSTFT_HOP_SIZES = (512, 256, 128, 64, 32, 16, 8)
LOSS_MODES = {"dsm": 0, "init_pit": 1}
LOSS_REDUCTIONS = {"none": 0, "mean": 1}
ODE_METHODS = {"RK45": 0, "RK23": 1}
ODE_STATUS = {-1: "running", 0: "finished", 1: "step size too small", 2: "max_attempts reached"}
MIX_CORRECTORS = {"ald2": 0, "none": 1}
SB_TYPES = {"sde": 0, "ode": 1}


class DsnConfig(C.Structure):
    _fields_ = [
        ("device", C.c_int32), ("precision", C.c_int32), ("n_src", C.c_int32), ("latent_dim", C.c_int32),
        ("score_kind", C.c_int32), ("dit_embed_dim", C.c_int32), ("dit_depth", C.c_int32),
        ("dit_heads", C.c_int32),
        ("ncsn_nf", C.c_int32), ("ncsn_n_levels", C.c_int32), ("ncsn_ch_mult", C.c_int32 * 4),
        ("ncsn_num_res_blocks", C.c_int32), ("ncsn_attn_resolution", C.c_int32), ("ncsn_image_size", C.c_int32),
        ("ncsn_max_latent_length", C.c_int32),
        ("vae_channels", C.c_int32), ("vae_n_blocks", C.c_int32),
        ("vae_c_mults", C.c_int32 * MAX_VAE_BLOCKS), ("vae_strides", C.c_int32 * MAX_VAE_BLOCKS),
        ("vae_enc_latent_dim", C.c_int32), ("vae_use_snake", C.c_int32), ("vae_final_tanh", C.c_int32),
        ("vae_has_encoder", C.c_int32), ("vae_has_decoder", C.c_int32),
        ("sde_theta", C.c_float), ("sde_sigma_min", C.c_float), ("sde_sigma_max", C.c_float),
    ]


class DsnDitPlan(C.Structure):
    """dsn_dit_plan (include/ditsep_hip.h): what one DiT score call would run; needs no GPU"""
    _fields_ = [(k, C.c_int) for k in (
        "M", "S", "skinny", "fold_rows", "qa_ipp", "qkv_rows", "attn_out_ksplit", "attn_out_rows", "ff_in_rows",
        "ff_out_ksplit", "ff_out_rows", "project_out_rows")]


# dsn_test_gemm (include/ditsep_hip.h): which kernel of the implicit-GEMM family runs the descriptor
TEST_GEMM_KERNELS = {"auto": 0, "tile": 1, "v1": 2, "panel": 3, "skinny": 4, "halo": 5, "splitk": 6}
ACT_NONE, ACT_ELU, ACT_SNAKE, ACT_SILU = 0, 1, 2, 3
F32_NONE, F32_TANH = 0, 1


class DsnTestGemm(C.Structure):
    _fields_ = [
        ("kernel", C.c_int), ("bm", C.c_int), ("bn", C.c_int), ("nst", C.c_int), ("bk", C.c_int),
        ("panel_rows", C.c_int), ("panel_bn", C.c_int), ("panel_wm", C.c_int), ("ksplit", C.c_int),
        ("B", C.c_int), ("Lin", C.c_int), ("Cin", C.c_int), ("N", C.c_int), ("taps", C.c_int), ("in_stride", C.c_int),
        ("tap_dil", C.c_int), ("in_pad", C.c_int), ("rows_per_b", C.c_int), ("M", C.c_int),
        ("in_row_elems", C.c_int), ("a_off", C.c_int), ("in_bstride", C.c_int64),
        ("img_h", C.c_int), ("img_w", C.c_int), ("out_bstride", C.c_int64),
        ("out_row_elems", C.c_int), ("out_off", C.c_int), ("out_limit", C.c_int64),
        ("a", C.c_void_p), ("a_numel", C.c_int64), ("w", C.c_void_p),
        ("bias", C.c_void_p), ("bias_mod", C.c_int), ("bbias", C.c_void_p), ("bbias_stride", C.c_int),
        ("resid", C.c_void_p), ("resid_bstride", C.c_int64), ("resid_row_elems", C.c_int), ("resid_off", C.c_int),
        ("out_scale", C.c_float), ("f32_op", C.c_int), ("act", C.c_int), ("act_a", C.c_void_p), ("act_b", C.c_void_p),
        ("act_mod", C.c_int), ("swiglu", C.c_int), ("gn_stats", C.c_void_p), ("gn_stats2", C.c_void_p),
        ("gn_nq2", C.c_int), ("gn_qoff2", C.c_int),
        ("sc_a", C.c_void_p), ("sc_a_numel", C.c_int64), ("sc_w", C.c_void_p), ("sc_bias", C.c_void_p),
        ("sc_Cin", C.c_int), ("sc_row_elems", C.c_int),
        ("out_f32", C.c_void_p), ("out_planes", C.c_void_p), ("out_ps", C.c_int64),
        ("slabs", C.c_void_p), ("slab_stride", C.c_int64),
    ]


# dsn_test_kernel (include/ditsep_hip.h): which launch wrapper of the non-GEMM kernels runs
TEST_KERNEL_KINDS = {"attention": 1, "qkv_attention": 2, "residual_norm": 3, "gn_stats": 4, "gn_apply": 5, "fir2d": 6,
                     "conv_out1": 7, "conv_in1": 8, "ru_fused": 9,
                     "pc_prior": 10, "pc_corrector": 11, "pc_item_norms": 12, "pc_predictor": 13, "sigma_mix": 14,
                     "mix_prior": 15, "mix_corrector": 16, "mix_predictor": 17, "sb_update": 18, "repeat_sources": 19,
                     "vae_sample": 20, "randn": 21, "rand_uniform": 22, "codec_tail_zero": 23,
                     "wn_scale": 24, "pack_weight": 25, "pack_bias_swiglu": 26, "pack_weight_fp8": 27,
                     "packed_row_sum": 28, "fp8_row_sum": 29, "bias_plus_wbeta": 30, "snake_params": 31,
                     "pack_tokens": 32, "unpack_tokens": 33, "copy_rows": 34, "to_planes": 35, "zero_tail": 36,
                     "vae_sample_ragged": 37, "timestep_features": 38, "rope_tables": 39, "ncsn_pack": 40,
                     "ncsn_fourier": 41, "ncsn_output": 42, "win_pack_tokens": 43, "win_blend_tokens": 44}
# `mode` of the pack_weight kind (DSN_PACK_*); pack_weight_fp8 takes the first two
PACK_MODES = {"linear": 0, "linear_swiglu": 1, "conv": 2, "convt": 3, "conv2d": 4, "nin": 5}


class DsnTestKernel(C.Structure):
    _fields_ = [
        ("kind", C.c_int), ("B", C.c_int), ("S", C.c_int), ("H", C.c_int), ("dh", C.c_int), ("D", C.c_int),
        ("ipp", C.c_int), ("rows", C.c_int), ("nslab", C.c_int), ("do_norm", C.c_int), ("eps", C.c_float),
        ("slab_stride", C.c_int64),
        ("C", C.c_int), ("HW", C.c_int), ("rstride", C.c_int), ("img_h", C.c_int), ("img_w", C.c_int), ("up", C.c_int),
        ("silu", C.c_int), ("bstride", C.c_int64),
        ("L", C.c_int), ("ktaps", C.c_int), ("apply_tanh", C.c_int), ("act", C.c_int),
        ("dil", C.c_int), ("act_out", C.c_int),
        ("a", C.c_void_p), ("a_numel", C.c_int64), ("w", C.c_void_p), ("w_numel", C.c_int64), ("w2", C.c_void_p),
        ("w2_numel", C.c_int64), ("x", C.c_void_p),
        ("slabs", C.c_void_p), ("bias", C.c_void_p), ("bias2", C.c_void_p), ("gamma", C.c_void_p), ("beta", C.c_void_p),
        ("stats", C.c_void_p), ("add", C.c_void_p), ("act_a", C.c_void_p), ("act_b", C.c_void_p),
        ("out_act_a", C.c_void_p), ("out_act_b", C.c_void_p), ("rope_cos", C.c_void_p), ("rope_sin", C.c_void_p),
        ("out_f32", C.c_void_p), ("out_planes", C.c_void_p), ("out_ps", C.c_int64), ("out_fp8", C.c_void_p),
        ("out_fp8_scale", C.c_void_p),
        # the sampler's kernels (fp32 only)
        ("n", C.c_int), ("T", C.c_int), ("avg_len", C.c_int), ("em", C.c_int), ("mean_full", C.c_int),
        ("third_is_y", C.c_int),
        ("stdT", C.c_float), ("step", C.c_float), ("gain", C.c_float), ("snr", C.c_float), ("theta", C.c_float),
        ("dt", C.c_float), ("G", C.c_float), ("g", C.c_float), ("s1", C.c_float), ("s2", C.c_float), ("lam", C.c_float),
        ("sqdt", C.c_float), ("w_prev", C.c_float), ("w_est", C.c_float), ("w3", C.c_float), ("lo", C.c_float),
        ("hi", C.c_float),
        ("seed", C.c_uint64), ("offset", C.c_uint64), ("count", C.c_int64),
        ("y", C.c_void_p), ("score", C.c_void_p), ("z", C.c_void_p), ("smix", C.c_void_p), ("norms", C.c_void_p),
        ("xmean", C.c_void_p),
        ("lens", C.c_void_p),
        ("rep", C.c_int), ("mul", C.c_int),
        # weight preparation, movers and feature kernels
        ("mode", C.c_int), ("N", C.c_int), ("K", C.c_int), ("Cin", C.c_int), ("Cout", C.c_int), ("kw", C.c_int),
        ("stride", C.c_int),
        ("scale", C.c_void_p), ("colscale", C.c_void_p), ("in_planes", C.c_void_p), ("in_ps", C.c_int64),
        ("in_fp8", C.c_void_p), ("in_fp8_scale", C.c_void_p),
        ("C0", C.c_int), ("C1", C.c_int), ("dst_stride", C.c_int64),
        ("Wp", C.c_int), ("Cp", C.c_int), ("cin", C.c_int), ("half", C.c_int),
        ("out2_f32", C.c_void_p),
        ("wtab", C.c_void_p), ("ftab", C.c_void_p), ("fw", C.c_void_p), ("Tsrc", C.c_int), ("R", C.c_int),
    ]


def latent_frames_of(L: int, hop: int) -> int:
    """Latent frames of an L-sample mixture under the reference's pad rule (utils.pad / dsn_latent_frames): pad to the
    next multiple of hop, a full extra hop when L % hop == 0."""
    return int(L) // int(hop) + 1


def ragged_extended_length(L: int, hop: int) -> int:
    """Samples an item of a ragged batch is zero-extended to before its group is encoded: latent_frames_of(L) * hop - 1,
    the longest length with the same frame count.  dsn_encode's own pad rule then adds the one remaining zero, so the
    encoder sees exactly the padded signal it sees for the item alone (L <= T hop - 1 always holds)."""
    return latent_frames_of(L, hop) * int(hop) - 1


def frame_groups(frames) -> dict:
    """{frame count: [item indices]} in order of first appearance: the codec runs once per group (its convolutions see
    zero padding at an item's end when it runs alone, non-zero activations in a padded batch)."""
    groups: dict = {}
    for i, f in enumerate(frames):
        groups.setdefault(int(f), []).append(i)
    return groups


CODEC_MODES = ("grouped", "padded")


def check_codec_mode(codec: str) -> str:
    """codec= of the ragged entry points: "grouped" (one codec call per group of equal frame count) or "padded" (one
    pass over the padded batch, dsn_decode_ragged / dsn_encode_ragged)."""
    if codec not in CODEC_MODES:
        raise ValueError(f"codec must be one of {CODEC_MODES} (got {codec!r})")
    return codec


def codec_level_rows(strides, side: str) -> list:
    """Rows per latent frame (`mul` of the tail launch) of every level of a ragged codec pass, in launch order.
    "decoder": the latent (1), then the output of each up-sampling block, the product of the strides so far in the
    decoder's order (the reversed `strides`); the last entry is the hop length, the waveform.  "encoder": the waveform
    level (hop), then the output of each down-sampling block, hop divided by the product so far; the last entry is 1."""
    st = [int(v) for v in strides]
    if side == "decoder":
        out = [1]
        for v in reversed(st):
            out.append(out[-1] * v)
        return out
    if side != "encoder":
        raise ValueError(f"side must be 'decoder' or 'encoder' (got {side!r})")
    out = [math.prod(st)]
    for v in st:
        out.append(out[-1] // v)
    return out


def codec_valid_rows(frames, rep: int, mul: int, S: int) -> list:
    """Valid rows of each of the S codec items at a level: frames[s // rep] * mul (rep = n_src in the decoder, whose
    S = B * n_src items share their mixture's length; 1 in the encoder)."""
    if rep < 1 or mul < 1 or S != len(frames) * rep:
        raise ValueError(f"S = {S} items need S / rep = {S / max(rep, 1):g} frame counts with rep, mul >= 1 "
                         f"(got {len(frames)} counts, rep = {rep}, mul = {mul})")
    return [int(frames[s // rep]) * mul for s in range(S)]


def check_ragged(score_kind: int, frames, B: int, T: int, corrector: str = "ald", need_dit: bool = True) -> list:
    """The refusals of the ragged entry points (include/ditsep_hip.h), raised by name before the library is touched:
    a score network other than the DiT (need_dit: the score call and the samplers, not the codec), a frame count
    outside [1, T] (or not one per item), the langevin corrector.  Returns the frame counts as a list of ints."""
    if need_dit and score_kind != SCORE_DIT:
        raise ValueError("ragged batches need the DiT score network: NCSN++ convolves across time, so padding would "
                         "change an item's result")
    fr = [int(f) for f in frames]
    if len(fr) != B:
        raise ValueError(f"frames must hold one frame count per item (B = {B}), got {len(fr)}")
    for b, f in enumerate(fr):
        if f < 1 or f > T:
            raise ValueError(f"frame count frames[{b}] = {f} outside [1, T = {T}]")
    if corrector == "langevin":
        raise ValueError("the langevin corrector has no ragged form: its per-item norms would run over the padding")
    return fr


def composite_min_samples(fs: int) -> Optional[int]:
    """Samples one frame plus one hop of the composite measures takes at `fs` (window 30 ms, hop a quarter of it), or
    None for a signal rate the library has no kernel for (it refuses that rate itself)."""
    return {8000: 300, 16000: 600}.get(int(fs))


def check_lens(lens, B: int, Lmax: int, min_len: Optional[int] = None, what: str = "") -> list:
    """The refusals of the ragged metric calls (include/ditsep_hip.h), raised by name before the library is touched:
    not one sample count per item, a count outside [1, Lmax], and with min_len (the composite measures) an item shorter
    than one frame plus one hop.  Returns the counts as a list of ints."""
    ln = [int(v) for v in lens]
    if len(ln) != B:
        raise ValueError(f"lens must hold one sample count per item (B = {B}), got {len(ln)}")
    for b, v in enumerate(ln):
        if v < 1 or v > Lmax:
            raise ValueError(f"sample count lens[{b}] = {v} outside [1, Lmax = {Lmax}]")
    if min_len is not None:
        for b, v in enumerate(ln):
            if v < min_len:
                raise ValueError(f"item {b} (lens[{b}] = {v}) is shorter than one frame "
                                 f"({min_len} samples needed{what})")
    return ln


BSS_MAX_SRC, BSS_MAX_TAPS, BSS_TILE, BSS_DEFAULT_BUDGET = 4, 512, 4096, 512 << 20
BSS_PERM_BY = {"sdr": 0, "sir": 1}


def bss_eval_plan(B: int, n: int, L: int, F: int = 512, budget: int = 0) -> dict:
    """What Engine.bss_eval does with a [B, n, L] batch and F filter taps under a workspace budget in bytes (0: 512 MiB),
    restated from dsn_bss_eval_plan: "tiles" time tiles of 4096 samples for the longest item, "M" = n F unknowns,
    "items_per_chunk", "per_item_bytes" -- the float64 tile partials [2 n^2 + n][tiles][F], lag tables [2 n^2 + n][F]
    and systems (one of M and n - 1 of F unknowns: a packed lower triangle plus n right-hand sides) of one item -- and "workspace_bytes" of one chunk.  ValueError
    where the library returns DSN_EINVAL."""
    B, n, L, F, budget = int(B), int(n), int(L), int(F), int(budget)
    if B < 1 or L < 1:
        raise ValueError(f"bss_eval: B = {B}, L = {L} (both at least 1)")
    if n < 1 or n > BSS_MAX_SRC:
        raise ValueError(f"bss_eval: n = {n} outside [1, {BSS_MAX_SRC}]")
    if F < 1 or F > BSS_MAX_TAPS:
        raise ValueError(f"bss_eval: filter_length = {F} outside [1, {BSS_MAX_TAPS}]")
    if budget < 0:
        raise ValueError(f"bss_eval: workspace_budget = {budget} < 0")
    tiles, M, jobs = (L + BSS_TILE - 1) // BSS_TILE, n * F, 2 * n * n + n
    per_item = 8 * (jobs * tiles * F + jobs * F + M * (M + 1) // 2 + n * M + (n - 1) * (F * (F + 1) // 2 + n * F))
    fit = (budget or BSS_DEFAULT_BUDGET) // per_item
    if fit < 1:
        raise ValueError(f"bss_eval: workspace_budget = {budget} bytes is smaller than one item ({per_item} bytes at "
                         f"n = {n}, L = {L}, filter_length = {F})")
    ipc = min(fit, B, 65535)
    return {"tiles": tiles, "M": M, "items_per_chunk": ipc, "per_item_bytes": per_item,
            "workspace_bytes": per_item * ipc}


def check_bss_eval(shape, est_shape, *, filter_length=512, perm_by="sir", load_diag=0.0, perm=None, lens=None,
                   workspace_budget=0) -> tuple:
    """The refusals of dsn_bss_eval (include/ditsep_hip.h), raised by name before the library is touched.  Returns
    (plan, perm_by code, lens as a list or None, perm as a flat list or None)."""
    if len(shape) != 3 or tuple(est_shape) != tuple(shape):
        raise ValueError(f"ref and est must both be [B,n,L] (got {tuple(shape)} and {tuple(est_shape)})")
    B, n, L = (int(v) for v in shape)
    if perm_by not in BSS_PERM_BY:
        raise ValueError(f"bss_eval: perm_by = {perm_by!r} (one of {sorted(BSS_PERM_BY)})")
    if not float(load_diag) >= 0.0:
        raise ValueError(f"bss_eval: load_diag = {load_diag} < 0")
    plan = bss_eval_plan(B, n, L, filter_length, workspace_budget)
    if lens is not None:
        lens = check_lens(lens, B, L)
    if perm is not None:
        perm = torch.as_tensor(perm, dtype=torch.int32).reshape(-1).tolist()
        if len(perm) != B * n:
            raise ValueError(f"perm must hold B*n = {B * n} entries (got {len(perm)})")
        for k, v in enumerate(perm):
            if v < 0 or v >= n:
                raise ValueError(f"bss_eval: perm[{k}] = {v} outside [0, {n})")
    return plan, BSS_PERM_BY[perm_by], lens, perm


FADES = {"hann": 0, "linear": 1}


def window_plan(L: int, window: int, overlap: int):
    """(W, hop) of cutting an L-sample recording into windows of `window` samples that share `overlap` samples with
    their neighbour: hop = window - overlap, window w covers [w hop, w hop + window), W = 1 for L <= window, else
    1 + ceil((L - window) / hop); the last window is zero-extended past L.  With this W the last window starts inside
    the recording and its overlap with the one before holds real samples only ((W-1) hop + overlap < L).  Refused by
    name: window < 1, overlap < 0, L < 1, and 2 overlap > window -- a sample may lie in at most two windows
    (dsn_window_stitch's cross-fade is a gather)."""
    L, window, overlap = int(L), int(window), int(overlap)
    if window < 1:
        raise ValueError(f"window = {window} < 1")
    if overlap < 0:
        raise ValueError(f"overlap = {overlap} < 0")
    if L < 1:
        raise ValueError(f"L = {L} < 1")
    if 2 * overlap > window:
        raise ValueError(f"2 * overlap = {2 * overlap} > window = {window}: a sample may lie in at most two windows")
    hop = window - overlap
    return (1 if L <= window else 1 + -((window - L) // hop)), hop


def fade_table(overlap: int, fade: str = "hann"):
    """(fall32, rise32), float32 numpy arrays [overlap]: the cross-fade weights of dsn_window_stitch over the overlap
    position k.  rise[k] = sin^2(pi (k + 1/2) / (2 overlap)) ("hann") or (k + 1/2) / overlap ("linear"),
    fall[k] = 1 - rise[k]; both in float64 (the C library's sin), rounded once to float32 -- the library builds the same
    tables, so a restatement that uses these differs from the device by the cross-fade's own rounding only."""
    rise = fade_rise64(overlap, fade)
    return (1.0 - rise).astype("float32"), rise.astype("float32")


def fade_rise64(overlap: int, fade: str = "hann"):
    """The rising weight of fade_table before it is rounded: float64 numpy array [overlap]."""
    import numpy as np

    if fade not in FADES:
        raise ValueError(f"fade must be one of {sorted(FADES)} (got {fade!r})")
    O = int(overlap)
    if O < 0:
        raise ValueError(f"overlap = {O} < 0")
    if fade == "linear":
        return np.asarray([(k + 0.5) / float(O) for k in range(O)], dtype=np.float64)
    sn = [math.sin(math.pi * (k + 0.5) / (2.0 * float(O))) for k in range(O)]
    return np.asarray([s * s for s in sn], dtype=np.float64)


def score_window_plan(frames, Tw: int, To: int, fade: str = "hann", T: Optional[int] = None) -> dict:
    """The plan of a window-blended score call (dsn_score_windowed; mirrored by csrc/score_window.h): `frames` holds one
    latent frame count per recording, `Tw` is the window and `To` the overlap in frames, `T` (default max(frames)) the
    padded length of the tensors.  A recording of F <= Tw frames is one window [0, F).  Otherwise hop = Tw - To and
    W = 1 + ceil((F - Tw) / hop) (window_plan's W) full windows, window w starting at min(w hop, F - Tw): the last one is
    shifted back into the recording, not zero-extended.  Seam j is the To frames [(j+1) hop, (j+1) hop + To), the last
    To frames of window j; left of it a frame takes window j, right of it window j+1, inside it
    fall[k] s_j + rise[k] s_{j+1} with fade_table(To, fade).  -> dict of
      "W"       windows per recording;  "Wtot" their sum;  "Twin" the DiT call's length: Tw, or max(frames) when no
                recording is longer than a window;  "T";  "short": some window is shorter than Twin
      "windows" int32 [Wtot, 3] = (recording, start, length), the windows of all recordings in order
      "table"   int32 [R T, 4] = (window0, offset0, window1, offset1): window1 = -1 outside seams, window0 = -1 past the
                recording's end (the score there is written as zero)
      "weights" float32 [R T, 2] = (fall, rise); (1, 0) outside seams
    Refused in window_plan's words: Tw < 1, To < 0, 2 To > Tw, a frame count outside [1, T]."""
    import numpy as np

    fr = [int(f) for f in frames]
    Tw, To = int(Tw), int(To)
    T = max(fr) if T is None else int(T)
    for r, F in enumerate(fr):
        if F < 1 or F > T:
            raise ValueError(f"frame count frames[{r}] = {F} outside [1, T = {T}]")
        window_plan(F, Tw, To)                                             # (the refusals, by name)
    fall, rise = fade_table(To, fade)
    hop, R = Tw - To, len(fr)
    windows, counts = [], []
    table = np.zeros((R * T, 4), dtype=np.int32)
    table[:, 0] = table[:, 2] = -1
    weights = np.zeros((R * T, 2), dtype=np.float32)
    weights[:, 0] = 1.0
    for r, F in enumerate(fr):
        base = len(windows)
        W = window_plan(F, Tw, To)[0]
        start = [0] if W == 1 else [min(w * hop, F - Tw) for w in range(W)]
        windows += [(r, s, min(F, Tw)) for s in start]
        counts.append(W)
        for f in range(F):
            w = 0 if W == 1 else min(f // hop, W - 1)
            k = f - w * hop
            if w >= 1 and k < To:
                table[r * T + f] = (base + w - 1, f - start[w - 1], base + w, f - start[w])
                weights[r * T + f] = (fall[k], rise[k])
            else:
                table[r * T + f, :2] = (base + w, f - start[w])
    windows = np.asarray(windows, dtype=np.int32).reshape(-1, 3)
    Twin = int(windows[:, 2].max())
    return {"W": counts, "Wtot": len(windows), "Twin": Twin, "T": T, "short": bool((windows[:, 2] != Twin).any()),
            "windows": windows, "table": table, "weights": weights}


def check_windowed(score_kind: int, frames, R: int, T: int, window, corrector: str = "ald") -> tuple:
    """The refusals of the window-blended entry points, raised by name before the library is touched: a score network
    other than the DiT, score_window_plan's, and the langevin corrector when the lengths differ.  -> (frames, Tw, To)"""
    if score_kind != SCORE_DIT:
        raise ValueError("window-blended scores need the DiT score network: its windows are batch items of the trained "
                         "length")
    if frames is None:
        raise ValueError("window= needs frames=, one latent frame count per recording")
    fr = [int(f) for f in frames]
    if len(fr) != R:
        raise ValueError(f"frames must hold one frame count per recording (R = {R}), got {len(fr)}")
    Tw, To = (int(v) for v in window)
    for r, F in enumerate(fr):
        if F < 1 or F > T:
            raise ValueError(f"frame count frames[{r}] = {F} outside [1, T = {T}]")
        window_plan(F, Tw, To)
    if corrector == "langevin" and len(set(fr)) > 1:
        raise ValueError("the langevin corrector has no form for recordings of different lengths: its per-item norms "
                         "would run over the padding")
    return fr, Tw, To


LONG_MODES = ("stitch", "score")


def cut_windows(mixes, window: int, overlap, device):
    """list of [1, L_r] recordings -> (pool [Wtot, 1, window] on `device`, plans [(W_r, hop, L_r)], overlap): every
    recording zero-extended to its plan's (W_r - 1) hop + window samples and unfolded into its W_r windows, the
    windows of all recordings in order.  overlap None: window // 4."""
    window = int(window)
    overlap = window // 4 if overlap is None else int(overlap)
    rows, plans = [], []
    for r, m in enumerate(mixes):
        if m.dim() != 2 or m.shape[0] != 1:
            raise ValueError(f"recording {r} must be [1, L] (got {tuple(m.shape)})")
        L = int(m.shape[-1])
        W, hop = window_plan(L, window, overlap)
        x = _dev32(m, device).reshape(-1)
        x = torch.nn.functional.pad(x, (0, (W - 1) * hop + window - L))
        rows.append(x.unfold(0, window, hop))
        plans.append((W, hop, L))
    return torch.cat(rows, dim=0).unsqueeze(1).contiguous(), plans, overlap


def check_rates(fs_in, fs_out) -> tuple:
    """The sample rates of a resampling call as ints; refused by name: a rate that is not a positive integer."""
    for name, fs in (("fs_in", fs_in), ("fs_out", fs_out)):
        if int(fs) != fs or int(fs) < 1:
            raise ValueError(f"sample rates must be positive integers ({name} = {fs!r})")
    return int(fs_in), int(fs_out)


def resample_length(fs_in: int, fs_out: int, L: int) -> int:
    """Samples an L-sample row has after resampling (dsn_resample_length): ceil(new L / orig) with
    orig = fs_in / gcd, new = fs_out / gcd, in integer arithmetic."""
    fs_in, fs_out = check_rates(fs_in, fs_out)
    if int(L) < 0:
        raise ValueError(f"L = {L} < 0")
    return int(load_library().dsn_resample_length(fs_in, fs_out, int(L)))


def resample_plan(fs_in: int, fs_out: int) -> dict:
    """The plan of a resampling call (dsn_resample_plan, csrc/resample_plan.h; needs no GPU): the default filter of
    torchaudio.transforms.Resample(fs_in, fs_out) -- sinc_interp_hann, lowpass_filter_width 6, rolloff 0.99 -- as a
    polyphase table cut down to the taps that are not exactly 0.0 in float32.  -> dict of
      "orig", "new"  the rates over their gcd;  "width" = ceil(6 orig / (0.99 min(orig, new)));  "K" = 2 width + orig, the
                     taps per phase of the dense table
      "support"      S: the longest run, over the phases, from the first to the last non-zero tap
      "k0"           int32 [new]: the first non-zero tap of each phase
      "taps"         float32 [new, S]: taps[p, j] = h[p, k0[p] + j], zero-filled on the right
    out[m new + p] = sum_j taps[p, j] x[m orig + k0[p] + j - width] with x read as zero outside its samples."""
    import numpy as np

    fs_in, fs_out = check_rates(fs_in, fs_out)
    lib = load_library()
    o, n, w, S = C.c_int(), C.c_int(), C.c_int(), C.c_int()
    rc = lib.dsn_resample_plan(fs_in, fs_out, C.byref(o), C.byref(n), C.byref(w), C.byref(S), None, None)
    if rc != 0:
        raise ValueError(f"dsn_resample_plan({fs_in}, {fs_out}) refused ({rc})")
    k0 = np.zeros(n.value, dtype=np.int32)
    taps = np.zeros((n.value, S.value), dtype=np.float32)
    lib.dsn_resample_plan(fs_in, fs_out, None, None, None, None, k0.ctypes.data_as(C.POINTER(C.c_int32)),
                          taps.ctypes.data_as(C.POINTER(C.c_float)))
    return {"orig": o.value, "new": n.value, "width": w.value, "K": 2 * w.value + o.value, "support": S.value,
            "k0": k0, "taps": taps}


def check_resample(fs_in, fs_out, shape, lens=None) -> tuple:
    """The refusals of Engine.resample (dsn_resample's), raised by name before the library is touched: a non-positive
    rate; x that is not [L], [C, L] or [B, C, L]; C < 1 or L < 1; lens that is not one count in [1, L] per item.
    -> (fs_in, fs_out, (B, C, L), lens as a list or None)"""
    fs_in, fs_out = check_rates(fs_in, fs_out)
    if len(shape) not in (1, 2, 3):
        raise ValueError(f"x must be [L], [C, L] or [B, C, L] (got {tuple(shape)})")
    B, Cn, L = (1,) * (3 - len(shape)) + tuple(int(v) for v in shape)
    if B < 1 or Cn < 1:
        raise ValueError(f"x must hold at least one item and one channel (got {tuple(shape)}: C = {Cn} < 1 or B = {B} < 1)")
    if L < 1:
        raise ValueError(f"x must hold at least one sample (L = {L} < 1)")
    return fs_in, fs_out, (B, Cn, L), (None if lens is None else check_lens(lens, B, L))


MASK_REFINE_DEFAULTS = dict(n_fft=512, hop=128, power=2, eps=1e-10)
MASK_REFINE_MAX_SRC = 4


def _options(who, value, defaults, forms, shorthand, validate=None) -> Optional[dict]:
    """A keyword of the separation entry points (`who`) as its Engine method's keywords: None -> None; a value
    `shorthand` maps to a dict of replacements, or a dict of `defaults`' keys -> the defaults with those replaced (and
    `validate`d); anything else is refused by name, `forms` naming what is accepted besides a dict."""
    if value is None:
        return None
    short = shorthand(value)
    if short is not None:
        return dict(defaults, **short)
    if isinstance(value, Mapping):
        extra = sorted(set(value) - set(defaults))
        if extra:
            raise ValueError(f"{who}: unknown keys {extra} (a dict of {sorted(defaults)})")
        opts = dict(defaults, **value)
        if validate is not None:
            validate(opts)
        return opts
    raise ValueError(f"{who} must be {forms} or a dict of {sorted(defaults)} (got {value!r})")


def refine_options(refine) -> Optional[dict]:
    """The `refine` keyword of the separation entry points as Engine.mask_refine's keywords: None (off, the default)
    -> None; True or "mask" -> MASK_REFINE_DEFAULTS; a dict of n_fft / hop / power / eps -> the defaults with those
    replaced.  Anything else, False included, is refused by name."""
    return _options("refine", refine, MASK_REFINE_DEFAULTS, "None, True, 'mask'",
                    lambda v: {} if v is True or v == "mask" else None)


def _check_stft(who, B, n, n_fft, hop, power, eps) -> tuple:
    """B, n and the STFT parameters as dsn_mask_refine takes them -> (n_fft, hop, power, eps)"""
    if B < 1:
        raise ValueError(f"{who}: B = {B} < 1")
    if n < 1 or n > MASK_REFINE_MAX_SRC:
        raise ValueError(f"{who}: n = {n} outside [1, {MASK_REFINE_MAX_SRC}]")
    if int(n_fft) != n_fft or int(n_fft) < 64 or int(n_fft) > 2048 or int(n_fft) & (int(n_fft) - 1):
        raise ValueError(f"{who}: n_fft = {n_fft!r} is not a power of two in [64, 2048]")
    n_fft = int(n_fft)
    if int(hop) != hop or int(hop) < 1 or n_fft % int(hop) or n_fft // int(hop) not in (2, 4, 8):
        raise ValueError(f"{who}: n_fft / hop = {n_fft} / {hop!r} is not one of 2, 4, 8")
    if power not in (1, 2):
        raise ValueError(f"{who}: power = {power!r} is not 1 or 2")
    eps = float(eps)
    if not math.isfinite(eps) or not eps > 0.0:
        raise ValueError(f"{who}: eps = {eps} is not a finite positive number")
    return n_fft, int(hop), int(power), eps


def _check_item_lens(who, lens, B, L, n_fft) -> Optional[list]:
    """One sample count per item, each long enough for one reflection -> lens as a list or None"""
    need = n_fft // 2 + 1
    ln = [L] if lens is None else [int(v) for v in lens]
    if lens is not None and len(ln) != B:
        raise ValueError(f"lens must hold one sample count per item (B = {B}), got {len(ln)}")
    for b, v in enumerate(ln):
        if v < need or v > L:
            raise ValueError(f"{who}: item {b} has {v} samples, outside [n_fft / 2 + 1 = {need}, L = {L}] "
                             f"({need} samples needed: one reflection must reach the item)")
    return None if lens is None else ln


def _check_reg(who, reg) -> float:
    reg = float(reg)
    if not math.isfinite(reg) or reg < 0.0:
        raise ValueError(f"{who}: reg = {reg} is not a finite number >= 0")
    return reg


def _check_channels(who, channels, B, Cn) -> Optional[list]:
    """One channel count in [1, C] per item -> channels as a list or None"""
    if channels is None:
        return None
    ch = [int(v) for v in channels]
    if len(ch) != B:
        raise ValueError(f"{who}: channels must hold one channel count per item (B = {B}), got {len(ch)}")
    for b, v in enumerate(ch):
        if v < 1 or v > Cn:
            raise ValueError(f"{who}: item {b} has channels = {v}, outside [1, C = {Cn}]")
    return ch


def _check_budget(who, workspace_budget, default, per_item, at) -> int:
    """A workspace budget in bytes (0: `default`) that holds at least one item of `per_item` bytes -> the budget"""
    budget = int(workspace_budget)
    if budget < 0:
        raise ValueError(f"{who}: workspace_budget = {budget} < 0")
    if (budget or default) < per_item:
        raise ValueError(f"{who}: workspace_budget = {budget} bytes is smaller than one item ({per_item} bytes at "
                         f"{at})")
    return budget


def check_mask_refine(mix_shape, est_shape, lens=None, n_fft=512, hop=128, power=2, eps=1e-10) -> tuple:
    """The refusals of dsn_mask_refine (include/ditsep_hip.h), raised by name before the library is touched: mix that
    is not [B, L] or [B, 1, L] and est that is not [B, n, L] of the same B and L; n outside [1, 4]; n_fft not a power
    of two in [64, 2048]; n_fft / hop not in {2, 4, 8}; power not 1 or 2; eps not finite or <= 0; an item shorter than
    n_fft / 2 + 1 samples (one reflection must reach it) or lens[b] > L.
    -> ((B, n, L), lens as a list or None, n_fft, hop, power, eps)"""
    mix_shape, est_shape = tuple(int(v) for v in mix_shape), tuple(int(v) for v in est_shape)
    if len(mix_shape) == 3 and mix_shape[1] == 1:
        mix_shape = (mix_shape[0], mix_shape[2])
    if len(mix_shape) != 2 or len(est_shape) != 3 or (est_shape[0], est_shape[2]) != mix_shape:
        raise ValueError(f"mask_refine: mix must be [B, L] or [B, 1, L] and est [B, n, L] of the same B and L (got "
                         f"{mix_shape} and {est_shape})")
    B, n, L = est_shape
    n_fft, hop, power, eps = _check_stft("mask_refine", B, n, n_fft, hop, power, eps)
    return (B, n, L), _check_item_lens("mask_refine", lens, B, L, n_fft), n_fft, hop, power, eps


STEMS_MODES = {"mask": 0, "wiener": 1}                                              # DSN_STEMS_*
STEMS_MAX_CHANNELS = {"mask": 8, "wiener": 2}
STEMS_DEFAULTS = dict(mode="wiener", n_fft=512, hop=128, power=2, eps=1e-10, reg=1e-3)


def _check_stems_mode(mode) -> None:
    if mode not in STEMS_MODES:
        raise ValueError(f"stems: mode must be one of {sorted(STEMS_MODES)} (got {mode!r})")


def stems_options(stems) -> Optional[dict]:
    """The `stems` keyword of the separation entry points as Engine.stems' keywords: None (off, the default) -> None;
    "mask" or "wiener" -> STEMS_DEFAULTS with that mode; a dict of mode / n_fft / hop / power / eps / reg -> the
    defaults with those replaced.  Anything else, an unknown key or mode included, is refused by name."""
    return _options("stems", stems, STEMS_DEFAULTS, "None, 'mask', 'wiener'",
                    lambda v: {"mode": v} if isinstance(v, str) and v in STEMS_MODES else None,
                    lambda opts: _check_stems_mode(opts["mode"]))


def _check_mix_est(who, mix_shape, est_shape) -> tuple:
    """mix [B, C, L] and est [B, n, L] of the same B and L -> (B, C, n, L)"""
    mix_shape, est_shape = tuple(int(v) for v in mix_shape), tuple(int(v) for v in est_shape)
    if len(mix_shape) != 3 or len(est_shape) != 3 or (est_shape[0], est_shape[2]) != (mix_shape[0], mix_shape[2]):
        raise ValueError(f"{who}: mix must be [B, C, L] and est [B, n, L] of the same B and L (got {mix_shape} and "
                         f"{est_shape})")
    return mix_shape[0], mix_shape[1], est_shape[1], mix_shape[2]


def check_stems(mix_shape, est_shape, lens=None, channels=None, mode="wiener", n_fft=512, hop=128, power=2, eps=1e-10,
                reg=1e-3) -> tuple:
    """The refusals of dsn_stems (include/ditsep_hip.h), raised by name before the library is touched: an unknown
    mode; mix that is not [B, C, L] and est that is not [B, n, L] of the same B and L; C outside [1, 8] (mask) or
    [1, 2] (wiener); what check_mask_refine refuses (n, n_fft, hop, power, eps, an item too short for one reflection);
    reg not finite or < 0; not one channel count per item, or one outside [1, C].
    -> ((B, C, n, L), lens or None, channels or None, the DSN_STEMS_* mode, n_fft, hop, power, eps, reg)"""
    _check_stems_mode(mode)
    B, Cn, n, L = _check_mix_est("stems", mix_shape, est_shape)
    if Cn < 1 or Cn > STEMS_MAX_CHANNELS[mode]:
        raise ValueError(f"stems: C = {Cn} outside [1, {STEMS_MAX_CHANNELS[mode]}] for mode {mode!r}"
                         + (" (the Wiener filter solves 1 x 1 and 2 x 2 systems)" if mode == "wiener" else ""))
    n_fft, hop, power, eps = _check_stft("stems", B, n, n_fft, hop, power, eps)
    ln = _check_item_lens("stems", lens, B, L, n_fft)
    reg = _check_reg("stems", reg)
    ch = _check_channels("stems", channels, B, Cn)
    return (B, Cn, n, L), ln, ch, STEMS_MODES[mode], n_fft, hop, power, eps, reg


BEAMFORM_POSTFILTERS = {None: 0, "none": 0, "mask": 1}                               # DSN_BEAMFORM_POST_*
BEAMFORM_MAX_CHANNELS, BEAMFORM_MAX_OWNERS, BEAMFORM_DEFAULT_BUDGET = 8, 16, 512 << 20
# n_fft, hop, power, eps and reg are STEMS_DEFAULTS' values: they are not tuned for beamforming.
BEAMFORM_DEFAULTS = dict(ref=0, n_fft=STEMS_DEFAULTS["n_fft"], hop=STEMS_DEFAULTS["hop"], power=STEMS_DEFAULTS["power"],
                         eps=STEMS_DEFAULTS["eps"], reg=STEMS_DEFAULTS["reg"], postfilter=None)


def _check_postfilter(postfilter) -> None:
    if postfilter not in BEAMFORM_POSTFILTERS:
        raise ValueError(f"beamform: postfilter must be None, 'none' or 'mask' (got {postfilter!r})")


def _beamform_shorthand(v) -> Optional[dict]:
    if v is True:
        return {}
    if isinstance(v, int) and not isinstance(v, bool):
        if v < 0:
            raise ValueError(f"beamform: the reference channel {v} is negative")
        return {"ref": int(v)}
    return None


def beamform_options(beamform) -> Optional[dict]:
    """The `beamform` keyword of the separation entry points as Engine.beamform's keywords: None (off, the default)
    -> None; True -> BEAMFORM_DEFAULTS; an int -> the defaults with that reference channel; a dict of ref / n_fft /
    hop / power / eps / reg / postfilter -> the defaults with those replaced.  Anything else, False and an unknown key
    or post-filter included, is refused by name."""
    return _options("beamform", beamform, BEAMFORM_DEFAULTS, "None, True, a reference channel", _beamform_shorthand,
                    lambda opts: _check_postfilter(opts["postfilter"]))


def beamform_item_bytes(n_fft: int, hop: int, L: int, Cn: int, n: int) -> int:
    """The workspace one item of a [B, C, L] batch needs in dsn_beamform: the float64 partials of its owners and their
    sum, (owners + 1) n C (C + 1) (n_fft / 2 + 1) doubles, owners = min(16, spans of L)."""
    F, base = 1 + (L + hop - 1) // hop, (4096 if n_fft >= 2048 else 2048) // hop
    owners = min(BEAMFORM_MAX_OWNERS, (F + base - 1) // base)
    return 8 * (owners + 1) * n * Cn * (Cn + 1) * (n_fft // 2 + 1)


def _check_ref(who, ref, ch, Cn) -> int:
    """A reference channel every item has (ch: the items' channel counts, or None: Cn each) -> ref as an int"""
    if isinstance(ref, bool) or int(ref) != ref:
        raise ValueError(f"{who}: ref = {ref!r} is not a channel index")
    ref = int(ref)
    for b, v in enumerate(ch if ch is not None else [Cn]):
        if ref < 0 or ref >= v:
            raise ValueError(f"{who}: ref = {ref} outside [0, {v}): item {b} has {v} channels")
    return ref


def check_beamform(mix_shape, est_shape, lens=None, channels=None, ref=0, n_fft=512, hop=128, power=2, eps=1e-10,
                   reg=1e-3, postfilter=None, workspace_budget=0) -> tuple:
    """The refusals of dsn_beamform (include/ditsep_hip.h), raised by name before the library is touched: mix that is
    not [B, C, L] and est that is not [B, n, L] of the same B and L; C outside [1, 8]; what check_mask_refine refuses
    (n, n_fft, hop, power, eps, an item too short for one reflection); reg not finite or < 0; an unknown post-filter;
    not one channel count per item, or one outside [1, C]; ref outside [0, channels[b]) for any item; a negative
    workspace budget or one smaller than one item.
    -> ((B, C, n, L), lens or None, channels or None, ref, n_fft, hop, power, eps, reg, the DSN_BEAMFORM_POST_* code,
    workspace_budget)"""
    _check_postfilter(postfilter)
    B, Cn, n, L = _check_mix_est("beamform", mix_shape, est_shape)
    if Cn < 1 or Cn > BEAMFORM_MAX_CHANNELS:
        raise ValueError(f"beamform: C = {Cn} outside [1, {BEAMFORM_MAX_CHANNELS}]")
    n_fft, hop, power, eps = _check_stft("beamform", B, n, n_fft, hop, power, eps)
    ln = _check_item_lens("beamform", lens, B, L, n_fft)
    reg = _check_reg("beamform", reg)
    ch = _check_channels("beamform", channels, B, Cn)
    ref = _check_ref("beamform", ref, ch, Cn)
    budget = _check_budget("beamform", workspace_budget, BEAMFORM_DEFAULT_BUDGET,
                           beamform_item_bytes(n_fft, hop, L, Cn, n),
                           f"C = {Cn}, n = {n}, n_fft = {n_fft}, hop = {hop}, L = {L}")
    return (B, Cn, n, L), ln, ch, ref, n_fft, hop, power, eps, reg, BEAMFORM_POSTFILTERS[postfilter], budget


SPATIAL_MAX_ITERATIONS, SPATIAL_MAX_NOISE, SPATIAL_DEFAULT_BUDGET = 16, 0.9, 512 << 20
# one pass, a tenth of the prior mass for the noise class and a tenth spread over the sources; reg and eps load the
# classes' covariances.  These are not tuned.
SPATIAL_DEFAULTS = dict(iterations=1, noise=0.1, floor=0.1, reg=1e-3, eps=1e-10)


def spatial_options(spatial) -> Optional[dict]:
    """The `spatial` keyword of the separation entry points as the mask-refinement keywords of Engine.beamform_spatial
    (reg and eps are its mask_reg and mask_eps): None (off, the default) -> None; True -> SPATIAL_DEFAULTS; a dict of
    iterations / noise / floor / reg / eps -> the defaults with those replaced.  Anything else, False and an unknown key
    included, is refused by name."""
    return _options("spatial", spatial, SPATIAL_DEFAULTS, "None, True", lambda v: {} if v is True else None)


def spatial_beamform_keywords(beam: dict, spatial: Optional[dict]) -> dict:
    """The keywords of the beamforming step of the separation entry points: `beam` (beamform_options) for
    Engine.beamform, or, with `spatial` (spatial_options), those of Engine.beamform_spatial.  spatial= without
    beamform= and spatial= with the mask post-filter are refused by name."""
    if spatial is None:
        return dict(beam)
    if beam is None:
        raise ValueError("spatial= refines the masks of the beamformer: it needs beamform=")
    if BEAMFORM_POSTFILTERS[beam["postfilter"]]:
        raise ValueError("spatial= does not go with postfilter='mask': the post-filter would apply the estimates' masks, "
                         "not the refined ones (there is no gamma post-filter)")
    kw = {k: v for k, v in beam.items() if k != "postfilter"}
    return dict(kw, iterations=spatial["iterations"], noise=spatial["noise"], floor=spatial["floor"],
                mask_reg=spatial["reg"], mask_eps=spatial["eps"])


def spatial_item_bytes(n_fft: int, hop: int, L: int, Cn: int, n: int) -> int:
    """The workspace one item of a [B, C, L] batch needs in dsn_beamform_spatial: per bin the statistics of n + 1
    classes (C (C + 1) doubles each), the spectra (C x Fs complex floats), the masks (n x Fs floats) and a flag, Fs =
    1 + ceil(L / hop) frames.  The one formula: the C side computes the same number."""
    bins, Fs = n_fft // 2 + 1, 1 + (L + hop - 1) // hop
    return bins * (8 * (n + 1) * Cn * (Cn + 1) + Fs * (8 * Cn + 4 * n) + 4)


def check_spatial(mix_shape, est_shape, lens=None, channels=None, ref=0, n_fft=512, hop=128, power=2, eps=1e-10,
                  reg=1e-3, iterations=1, noise=0.1, floor=0.1, mask_reg=1e-3, mask_eps=1e-10,
                  workspace_budget=0) -> tuple:
    """The refusals of dsn_beamform_spatial (include/ditsep_hip.h), raised by name before the library is touched: what
    check_beamform refuses (there is no post-filter); iterations outside [0, 16]; noise outside [0, 0.9]; floor outside
    [0, 1]; mask_reg not finite or < 0; mask_eps not finite or <= 0; a workspace budget smaller than one item.
    -> ((B, C, n, L), lens or None, channels or None, ref, n_fft, hop, power, eps, reg, iterations, noise, floor,
    mask_reg, mask_eps, workspace_budget)"""
    who = "beamform_spatial"
    B, Cn, n, L = _check_mix_est(who, mix_shape, est_shape)
    if Cn < 1 or Cn > BEAMFORM_MAX_CHANNELS:
        raise ValueError(f"{who}: C = {Cn} outside [1, {BEAMFORM_MAX_CHANNELS}]")
    n_fft, hop, power, eps = _check_stft(who, B, n, n_fft, hop, power, eps)
    ln = _check_item_lens(who, lens, B, L, n_fft)
    reg = _check_reg(who, reg)
    ch = _check_channels(who, channels, B, Cn)
    ref = _check_ref(who, ref, ch, Cn)
    if isinstance(iterations, bool) or int(iterations) != iterations or not 0 <= int(iterations) <= SPATIAL_MAX_ITERATIONS:
        raise ValueError(f"{who}: iterations = {iterations!r} outside [0, {SPATIAL_MAX_ITERATIONS}]")
    noise, floor = float(noise), float(floor)
    if not 0.0 <= noise <= SPATIAL_MAX_NOISE:
        raise ValueError(f"{who}: noise = {noise} outside [0, {SPATIAL_MAX_NOISE}]")
    if not 0.0 <= floor <= 1.0:
        raise ValueError(f"{who}: floor = {floor} outside [0, 1]")
    mask_reg, mask_eps = float(mask_reg), float(mask_eps)
    if not math.isfinite(mask_reg) or mask_reg < 0.0:
        raise ValueError(f"{who}: mask_reg = {mask_reg} is not a finite number >= 0")
    if not math.isfinite(mask_eps) or not mask_eps > 0.0:
        raise ValueError(f"{who}: mask_eps = {mask_eps} is not a finite positive number")
    budget = _check_budget(who, workspace_budget, SPATIAL_DEFAULT_BUDGET, spatial_item_bytes(n_fft, hop, L, Cn, n),
                           f"C = {Cn}, n = {n}, n_fft = {n_fft}, hop = {hop}, L = {L}")
    return ((B, Cn, n, L), ln, ch, ref, n_fft, hop, power, eps, reg, int(iterations), noise, floor, mask_reg, mask_eps,
            budget)


TRACK_MIN_BLOCK, TRACK_MAX_BLOCK, TRACK_MAX_CONTEXT, TRACK_MAX_BLOCKS, TRACK_DEFAULT_BUDGET = 4, 1 << 20, 64, 4096, 512 << 20
# blocks of 0.8 s (100 frames at 16 kHz and hop 128) with one block of context each side, interpolated.  These are not
# tuned.
TRACK_DEFAULTS = dict(block=0.8, context=1, interpolate=True)


def _track_shorthand(v) -> Optional[dict]:
    if v is True:
        return {}
    if isinstance(v, (int, float)) and not isinstance(v, bool):
        return {"block": float(v)}
    return None


def _check_track_options(opts) -> None:
    block, context, interp = opts["block"], opts["context"], opts["interpolate"]
    if isinstance(block, bool) or not isinstance(block, (int, float)) or not math.isfinite(block) or not block > 0:
        raise ValueError(f"track: block = {block!r} is not a positive number of seconds")
    if isinstance(context, bool) or not isinstance(context, int) or not 0 <= context <= TRACK_MAX_CONTEXT:
        raise ValueError(f"track: context = {context!r} outside [0, {TRACK_MAX_CONTEXT}]")
    if not isinstance(interp, bool):
        raise ValueError(f"track: interpolate = {interp!r} is not True or False")


def track_options(track) -> Optional[dict]:
    """The `track` keyword of the separation entry points: None (off, the default) -> None; True -> TRACK_DEFAULTS; a
    number -> the defaults with that block length in seconds; a dict of block / context / interpolate -> the defaults
    with those replaced.  Anything else, False, an unknown key, a block that is not a positive number, a context
    outside [0, 64] and an interpolate that is not a bool included, is refused by name."""
    return _options("track", track, TRACK_DEFAULTS, "None, True, a block length in seconds", _track_shorthand,
                    _check_track_options)


def track_block_frames(block: float, fs: int, hop: int) -> int:
    """A block of `block` seconds in frames of `hop` samples at `fs`: max(4, block fs / hop rounded to nearest, halves
    up)"""
    return max(TRACK_MIN_BLOCK, int(math.floor(float(block) * int(fs) / int(hop) + 0.5)))


def track_beamform_keywords(beam: Optional[dict], track: Optional[dict], fs: Optional[int], spatial=None) -> dict:
    """The keywords of Engine.beamform_track for the beamforming step of the separation entry points: `beam`
    (beamform_options) and `track` (track_options) at the model's rate fs (None: only the refusals are made).  track=
    without beamform= and track= together with spatial= are refused by name."""
    if beam is None:
        raise ValueError("track= adapts the weights of the beamformer block by block: it needs beamform=")
    if spatial is not None:
        raise ValueError("track= does not go with spatial=: the cACGMM sums its statistics inside its solve workgroup, "
                         "and cutting those per block is a separate piece of work (not implemented)")
    frames = None if fs is None else track_block_frames(track["block"], fs, beam["hop"])
    return dict(beam, block_frames=frames, context=track["context"], interpolate=track["interpolate"])


def track_item_bytes(n_fft: int, hop: int, L: int, Cn: int, n: int, block_frames: int) -> int:
    """The workspace one item of a [B, C, L] batch needs in dsn_beamform_track: per block (Kmax = ceil(F / block_frames),
    F = 1 + ceil(L / hop)) the float64 partials and their context sums (n C (C + 1) bins doubles each), the weights
    (n bins C complex doubles) and one int32.  The one formula: the C side computes the same number."""
    F = 1 + (L + hop - 1) // hop
    kmax = (F + block_frames - 1) // block_frames
    return kmax * (8 * n * (n_fft // 2 + 1) * (2 * Cn * (Cn + 1) + 2 * Cn) + 4)


def track_plan(F: int, block_frames: int, interpolate=True) -> tuple:
    """Frame t = 0 .. F - 1 of an item of F frames -> (k0 [F] int64, alpha [F] float64) on the host: the frame is
    filtered with w^(k0) + alpha (w^(k0+1) - w^(k0)).  The integer arithmetic of the kernel (include/ditsep_hip.h):
    centre to centre between neighbouring blocks, the first and the last half block hold, alpha in [0, 1)."""
    F, Tb = int(F), int(block_frames)
    K = (F + Tb - 1) // Tb
    t = torch.arange(F, dtype=torch.int64)
    zero = torch.zeros(F, dtype=torch.float64)
    if not interpolate:
        return t // Tb, zero
    num = 2 * t + 1 - Tb
    k0 = torch.where(num <= 0, 0, num // (2 * Tb))
    alpha = torch.where(num <= 0, zero, (num % (2 * Tb)).to(torch.float64) / float(2 * Tb))
    last = k0 >= K - 1
    return torch.where(last, K - 1, k0), torch.where(last, zero, alpha)


def check_track(mix_shape, est_shape, lens=None, channels=None, ref=0, n_fft=512, hop=128, power=2, eps=1e-10,
                reg=1e-3, postfilter=None, block_frames=100, context=1, interpolate=True, workspace_budget=0) -> tuple:
    """The refusals of dsn_beamform_track (include/ditsep_hip.h), raised by name before the library is touched: what
    check_beamform refuses; block_frames outside [4, 2^20]; context outside [0, 64]; interpolate not a bool (or 0 / 1);
    more than 4096 blocks; a workspace budget smaller than one item.
    -> ((B, C, n, L), lens or None, channels or None, ref, n_fft, hop, power, eps, reg, the DSN_BEAMFORM_POST_* code,
    block_frames, context, interpolate as 0 / 1, the blocks Kmax, workspace_budget)"""
    who = "beamform_track"
    _check_postfilter(postfilter)
    B, Cn, n, L = _check_mix_est(who, mix_shape, est_shape)
    if Cn < 1 or Cn > BEAMFORM_MAX_CHANNELS:
        raise ValueError(f"{who}: C = {Cn} outside [1, {BEAMFORM_MAX_CHANNELS}]")
    n_fft, hop, power, eps = _check_stft(who, B, n, n_fft, hop, power, eps)
    ln = _check_item_lens(who, lens, B, L, n_fft)
    reg = _check_reg(who, reg)
    ch = _check_channels(who, channels, B, Cn)
    ref = _check_ref(who, ref, ch, Cn)
    if (isinstance(block_frames, bool) or int(block_frames) != block_frames
            or not TRACK_MIN_BLOCK <= int(block_frames) <= TRACK_MAX_BLOCK):
        raise ValueError(f"{who}: block_frames = {block_frames!r} outside [{TRACK_MIN_BLOCK}, 2^20]")
    if isinstance(context, bool) or int(context) != context or not 0 <= int(context) <= TRACK_MAX_CONTEXT:
        raise ValueError(f"{who}: context = {context!r} outside [0, {TRACK_MAX_CONTEXT}]")
    if interpolate not in (False, True):
        raise ValueError(f"{who}: interpolate = {interpolate!r} is not 0 or 1")
    Tb = int(block_frames)
    kmax = (1 + (L + hop - 1) // hop + Tb - 1) // Tb
    if kmax > TRACK_MAX_BLOCKS:
        raise ValueError(f"{who}: {kmax} blocks of block_frames = {Tb} frames at L = {L}, hop = {hop}: more than "
                         f"{TRACK_MAX_BLOCKS}")
    budget = _check_budget(who, workspace_budget, TRACK_DEFAULT_BUDGET, track_item_bytes(n_fft, hop, L, Cn, n, Tb),
                           f"C = {Cn}, n = {n}, n_fft = {n_fft}, hop = {hop}, L = {L}, block_frames = {Tb}")
    return ((B, Cn, n, L), ln, ch, ref, n_fft, hop, power, eps, reg, BEAMFORM_POSTFILTERS[postfilter], Tb, int(context),
            int(bool(interpolate)), kmax, budget)


BEAMFORM_DESIGNS = {"souden": 0, "rank1": 1, "gev": 2}                               # DSN_BEAMFORM_DESIGN_*
BEAMFORM_MAX_SWEEPS = 30
# the rank-one MVDR filter with ten Jacobi sweeps (five reach 1e-15 of the matrix where the eigenvalues are 1e-2 apart).
# These are not tuned.
DESIGN_DEFAULTS = dict(kind="rank1", sweeps=10)


def _check_design_options(opts) -> None:
    kind, sweeps = opts["kind"], opts["sweeps"]
    if not isinstance(kind, str) or kind not in BEAMFORM_DESIGNS:
        raise ValueError(f"design: kind must be one of {sorted(BEAMFORM_DESIGNS)} (got {kind!r})")
    if isinstance(sweeps, bool) or not isinstance(sweeps, int) or not 1 <= sweeps <= BEAMFORM_MAX_SWEEPS:
        raise ValueError(f"design: sweeps = {sweeps!r} outside [1, {BEAMFORM_MAX_SWEEPS}]")


def design_options(design) -> Optional[dict]:
    """The `design` keyword of the separation entry points and of Engine.beamform / beamform_spatial / beamform_track:
    None (the default: Souden's MVDR filter through today's call) -> None; "rank1", "gev" or "souden" ->
    DESIGN_DEFAULTS with that kind; a dict of kind / sweeps -> the defaults with those replaced.  Anything else, True,
    False, an unknown kind or key and sweeps outside [1, 30] included, is refused by name."""
    return _options("design", design, DESIGN_DEFAULTS, "None, 'rank1', 'gev', 'souden'",
                    lambda v: {"kind": v} if isinstance(v, str) and v in BEAMFORM_DESIGNS else None,
                    _check_design_options)


def check_design(design) -> Optional[tuple]:
    """`design` in any form design_options takes -> None (today's call) or (the DSN_BEAMFORM_DESIGN_* code, sweeps)"""
    opts = design_options(design)
    return None if opts is None else (BEAMFORM_DESIGNS[opts["kind"]], int(opts["sweeps"]))


def design_beamform_keywords(beam: Optional[dict], design: Optional[dict]) -> Optional[dict]:
    """`beam` (beamform_options) with `design` (design_options) added for whichever of Engine.beamform,
    beamform_spatial and beamform_track runs the beamforming step -- spatial_beamform_keywords and
    track_beamform_keywords hand the key on.  design= without beamform= is refused by name; without design= `beam`
    comes back as it is."""
    if design is None:
        return beam
    if beam is None:
        raise ValueError("design= picks the filter of the beamformer: it needs beamform=")
    return dict(beam, design=dict(design))


DEREVERB_MAX_CHANNELS, DEREVERB_MAX_TAPS, DEREVERB_MAX_DELAY, DEREVERB_MAX_UNKNOWNS, DEREVERB_MAX_ITERATIONS = 8, 16, 8, 80, 8
DEREVERB_DEFAULT_BUDGET = 512 << 20
# the offline recipe's usual values at 16 kHz; reg and eps are not tuned beyond the sanity runs the README names
DEREVERB_DEFAULTS = dict(taps=10, delay=3, iterations=3, n_fft=512, hop=128, reg=1e-4, eps=1e-10)


def dereverb_options(dereverb) -> Optional[dict]:
    """The `dereverb` keyword of the separation entry points as Engine.dereverb's keywords: None (off, the default)
    -> None; True -> DEREVERB_DEFAULTS; a dict of taps / delay / iterations / n_fft / hop / reg / eps -> the defaults
    with those replaced.  Anything else, False and an unknown key included, is refused by name."""
    return _options("dereverb", dereverb, DEREVERB_DEFAULTS, "None, True", lambda v: {} if v is True else None)


def dereverb_item_bytes(n_fft: int, hop: int, L: int, Cn: int, taps: int) -> int:
    """The workspace one item of a [B, C, L] batch needs in dsn_dereverb: per bin the filter (C taps x C complex
    doubles), lambda (Fs doubles), the spectra and the result (C x Fs complex floats each) and a flag, Fs = 1 +
    ceil(L / hop) frames.  The one formula: the C side computes the same number."""
    bins, Fs = n_fft // 2 + 1, 1 + (L + hop - 1) // hop
    return bins * (8 * (2 * Cn * taps * Cn + Fs + 2 * Cn * Fs) + 4)


def check_dereverb(mix_shape, lens=None, channels=None, taps=10, delay=3, iterations=3, n_fft=512, hop=128, reg=1e-4,
                   eps=1e-10, workspace_budget=0) -> tuple:
    """The refusals of dsn_dereverb (include/ditsep_hip.h), raised by name before the library is touched: mix that is
    not [B, C, L]; C outside [1, 8]; taps outside [1, 16]; delay outside [1, 8]; C taps > 80; iterations outside
    [1, 8]; what check_mask_refine refuses (n_fft, hop, eps, an item too short for one reflection); reg not finite or
    < 0; not one channel count per item, or one outside [1, C]; a negative workspace budget or one smaller than one
    item.
    -> ((B, C, L), lens or None, channels or None, taps, delay, iterations, n_fft, hop, reg, eps, workspace_budget)"""
    mix_shape = tuple(int(v) for v in mix_shape)
    if len(mix_shape) != 3:
        raise ValueError(f"dereverb: mix must be [B, C, L] (got {mix_shape})")
    B, Cn, L = mix_shape
    if Cn < 1 or Cn > DEREVERB_MAX_CHANNELS:
        raise ValueError(f"dereverb: C = {Cn} outside [1, {DEREVERB_MAX_CHANNELS}]")
    for name, v, top in (("taps", taps, DEREVERB_MAX_TAPS), ("delay", delay, DEREVERB_MAX_DELAY),
                         ("iterations", iterations, DEREVERB_MAX_ITERATIONS)):
        if isinstance(v, bool) or int(v) != v or not 1 <= int(v) <= top:
            raise ValueError(f"dereverb: {name} = {v!r} outside [1, {top}]")
    taps, delay, iterations = int(taps), int(delay), int(iterations)
    if Cn * taps > DEREVERB_MAX_UNKNOWNS:
        raise ValueError(f"dereverb: C taps = {Cn} x {taps} = {Cn * taps} unknowns per bin, more than "
                         f"{DEREVERB_MAX_UNKNOWNS}")
    n_fft, hop, _, eps = _check_stft("dereverb", B, 1, n_fft, hop, 2, eps)
    ln = _check_item_lens("dereverb", lens, B, L, n_fft)
    reg = _check_reg("dereverb", reg)
    ch = _check_channels("dereverb", channels, B, Cn)
    budget = _check_budget("dereverb", 0 if workspace_budget is None else workspace_budget, DEREVERB_DEFAULT_BUDGET,
                           dereverb_item_bytes(n_fft, hop, L, Cn, taps),
                           f"C = {Cn}, taps = {taps}, n_fft = {n_fft}, hop = {hop}, L = {L}")
    return (B, Cn, L), ln, ch, taps, delay, iterations, n_fft, hop, reg, eps, budget


ENSEMBLE_MODES = {"mean": 0, "median": 1, "best": 2, "medoid": 3}                  # DSN_ENSEMBLE_*
ENSEMBLE_MAX_K, ENSEMBLE_MAX_SRC = 16, 4


def check_samples(samples, combine="mean") -> int:
    """The `samples` / `combine` keywords of the separation entry points: samples an int in [1, 16], combine one of
    ENSEMBLE_MODES, both refused by name otherwise.  -> samples as an int"""
    if isinstance(samples, bool) or int(samples) != samples or not 1 <= int(samples) <= ENSEMBLE_MAX_K:
        raise ValueError(f"samples = {samples!r} is not an int in [1, {ENSEMBLE_MAX_K}]")
    if combine not in ENSEMBLE_MODES:
        raise ValueError(f"combine must be one of {sorted(ENSEMBLE_MODES)} (got {combine!r})")
    return int(samples)


def ensemble_checks(cands, mix=None, lens=None, mode="mean") -> tuple:
    """The refusals of dsn_ensemble_combine (include/ditsep_hip.h), raised by name before the library is touched: an
    unknown mode; cands that is not a float32 [B, K, n, L]; K outside [1, 16] or n outside [1, 4]; mix that is not a
    float32 [B, L] or [B, 1, L] of the same B and L; mode "best" without mix; not one lens entry per item, or an entry
    below 1 or above L.  -> ((B, K, n, L), lens as a list or None, the DSN_ENSEMBLE_* mode)"""
    if mode not in ENSEMBLE_MODES:
        raise ValueError(f"ensemble_combine: mode must be one of {sorted(ENSEMBLE_MODES)} (got {mode!r})")
    shape = tuple(int(v) for v in cands.shape)
    if len(shape) != 4 or cands.dtype != torch.float32 or min(shape[0], shape[3]) < 1:
        raise ValueError(f"ensemble_combine: cands must be float32 [B, K, n, L] (got {cands.dtype} {shape})")
    B, K, n, L = shape
    if K < 1 or K > ENSEMBLE_MAX_K:
        raise ValueError(f"ensemble_combine: K = {K} outside [1, {ENSEMBLE_MAX_K}]")
    if n < 1 or n > ENSEMBLE_MAX_SRC:
        raise ValueError(f"ensemble_combine: n = {n} outside [1, {ENSEMBLE_MAX_SRC}]")
    if mix is not None:
        ms = tuple(int(v) for v in mix.shape)
        if ms not in ((B, L), (B, 1, L)):
            raise ValueError(f"ensemble_combine: mix must be [B, L] or [B, 1, L] with B = {B}, L = {L} (got {ms})")
        if mix.dtype != torch.float32:
            raise ValueError(f"ensemble_combine: mix must be float32 (got {mix.dtype})")
    elif mode == "best":
        raise ValueError("ensemble_combine: mode 'best' ranks the candidates by their residual against the mixture: "
                         "mix is None")
    return shape, (None if lens is None else check_lens(lens, B, L)), ENSEMBLE_MODES[mode]


PCM_ENCODINGS = {"u8": 0, "s16": 1, "s24": 2, "s32": 3, "f32": 4, "f64": 5}        # DSN_PCM_*
PCM_SAMPLE_BYTES = {"u8": 1, "s16": 2, "s24": 3, "s32": 4, "f32": 4, "f64": 8}
PCM_OUT_ENCODINGS = ("s16", "s24", "f32")                                          # what dsn_pcm_encode writes
PCM_MAX_FRAME_BYTES = 48                                                           # DSN_PCM_MAX_FRAME_BYTES


def check_pcm_items(items, nbytes: int, downmix: bool = True) -> tuple:
    """The refusals of Engine.pcm_decode (dsn_pcm_decode's), raised by name before the library is touched.  `items` is
    one (offset, frames, channels, encoding) per payload, encoding a key of PCM_ENCODINGS: an unknown encoding;
    frames < 1 or channels < 1; a frame wider than PCM_MAX_FRAME_BYTES; a payload that leaves [0, nbytes).
    -> (offsets, frames, channels, codes, Cout, Lmax)"""
    items = [tuple(it) for it in items]
    if not items:
        raise ValueError("pcm_decode needs at least one item")
    offs, frames, chans, codes = [], [], [], []
    for b, (off, fr, ch, enc) in enumerate(items):
        if enc not in PCM_ENCODINGS:
            raise ValueError(f"item {b}: encoding must be one of {sorted(PCM_ENCODINGS)} (got {enc!r})")
        off, fr, ch = int(off), int(fr), int(ch)
        if fr < 1 or ch < 1:
            raise ValueError(f"item {b}: frames = {fr} and channels = {ch} must be at least 1")
        fb = ch * PCM_SAMPLE_BYTES[enc]
        if fb > PCM_MAX_FRAME_BYTES:
            raise ValueError(f"item {b}: frames of {fb} bytes ({ch} x {enc}) exceed PCM_MAX_FRAME_BYTES = "
                             f"{PCM_MAX_FRAME_BYTES}")
        if off < 0 or off + fb * fr > int(nbytes):
            raise ValueError(f"item {b} takes bytes [{off}, {off + fb * fr}), outside [0, {int(nbytes)})")
        offs.append(off), frames.append(fr), chans.append(ch), codes.append(PCM_ENCODINGS[enc])
    return offs, frames, chans, codes, (1 if downmix else max(chans)), max(frames)


LOUDNESS_DEFAULTS = dict(target=-23.0, peak=-1.0, link="mixture")
LOUDNESS_LINKS = ("mixture", "stem")
LOUDNESS_RATES = (8000, 192000)                                                    # LOUD_MIN_RATE, LOUD_MAX_RATE
LOUDNESS_MAX_CHANNELS = 2                                                          # LOUD_MAX_CH


def loudness_options(spec) -> Optional[dict]:
    """The `loudness` keyword of the separation entry points: None (off, the default) -> None; True ->
    LOUDNESS_DEFAULTS (-23 LUFS, a true-peak ceiling of -1 dBTP, one gain per item from the mixture); a number -> the
    defaults with that target; a dict of target / peak / link -> the defaults with those replaced (peak=None: no
    ceiling).  Anything else -- False, an unknown key or link, a target or ceiling that is not a finite number -- is
    refused by name."""
    if spec is None:
        return None
    if spec is True:
        opts = dict(LOUDNESS_DEFAULTS)
    elif isinstance(spec, (int, float)) and not isinstance(spec, bool):
        opts = dict(LOUDNESS_DEFAULTS, target=spec)
    elif isinstance(spec, Mapping):
        extra = sorted(set(spec) - set(LOUDNESS_DEFAULTS))
        if extra:
            raise ValueError(f"loudness: unknown keys {extra} (a dict of {sorted(LOUDNESS_DEFAULTS)})")
        opts = dict(LOUDNESS_DEFAULTS, **spec)
    else:
        raise ValueError(f"loudness must be None, True, a target in LUFS or a dict of {sorted(LOUDNESS_DEFAULTS)} "
                         f"(got {spec!r})")
    for key in ("target", "peak"):
        v = opts[key]
        if key == "peak" and v is None:
            continue
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v):
            raise ValueError(f"loudness: {key} = {v!r} is not a finite number"
                             + (" (or None: no ceiling)" if key == "peak" else ""))
        opts[key] = float(v)
    if opts["link"] not in LOUDNESS_LINKS:
        raise ValueError(f"loudness: link must be one of {LOUDNESS_LINKS} (got {opts['link']!r})")
    return opts


def check_loudness(shape, rates, lens=None, channels=None) -> tuple:
    """The refusals of dsn_loudness (include/ditsep_hip.h), raised by name before the library is touched: x that is
    not [L], [C, L] or [B, C, L]; B outside [1, 65535]; C outside [1, 2]; L outside [1, 2^30]; rates that is not an
    integer or one integer per item in [8000, 192000]; lens[b] outside [1, L]; channels[b] outside [1, C].
    -> ((B, C, L), rates, lens or None, channels or None) as lists"""
    if len(shape) not in (1, 2, 3):
        raise ValueError(f"loudness: x must be [L], [C, L] or [B, C, L] (got {tuple(shape)})")
    B, Cn, L = (1,) * (3 - len(shape)) + tuple(int(v) for v in shape)
    if B < 1 or B > 65535:
        raise ValueError(f"loudness: B = {B} outside [1, 65535]")
    if Cn < 1 or Cn > LOUDNESS_MAX_CHANNELS:
        raise ValueError(f"loudness: C = {Cn} outside [1, {LOUDNESS_MAX_CHANNELS}] (every channel has weight 1: no "
                         f"surround weights)")
    if L < 1 or L > 2 ** 30:
        raise ValueError(f"loudness: L = {L} outside [1, 2^30]")
    rates = [rates] * B if isinstance(rates, int) else list(rates)
    if len(rates) != B:
        raise ValueError(f"loudness: one sample rate per item is needed (B = {B}), got {len(rates)}")
    for b, r in enumerate(rates):
        if isinstance(r, bool) or int(r) != r or not LOUDNESS_RATES[0] <= int(r) <= LOUDNESS_RATES[1]:
            raise ValueError(f"loudness: rates[{b}] = {r!r} is not an integer in [{LOUDNESS_RATES[0]}, "
                             f"{LOUDNESS_RATES[1]}] Hz")
    ch = None
    if channels is not None:
        ch = [int(v) for v in channels]
        if len(ch) != B:
            raise ValueError(f"loudness: channels must hold one channel count per item (B = {B}), got {len(ch)}")
        for b, v in enumerate(ch):
            if v < 1 or v > Cn:
                raise ValueError(f"loudness: item {b} has channels = {v}, outside [1, C = {Cn}]")
    return (B, Cn, L), [int(r) for r in rates], (None if lens is None else check_lens(lens, B, L)), ch


def kweight_coeffs(fs: int):
    """The K-weighting cascade at `fs` Hz (dsn_kweight_coeffs; needs no GPU): float64 [10] = the shelf's b0 b1 b2 a1
    a2, then the high-pass's."""
    import numpy as np

    out = np.zeros(10, dtype=np.float64)
    if isinstance(fs, bool) or int(fs) != fs or load_library().dsn_kweight_coeffs(
            int(fs), out.ctypes.data_as(C.POINTER(C.c_double))) != 0:
        raise ValueError(f"kweight_coeffs: fs = {fs!r} is not an integer in [{LOUDNESS_RATES[0]}, {LOUDNESS_RATES[1]}] Hz")
    return out


def loudness_gain(stats_src, stats_rows, groups, target, peak) -> dict:
    """The gain rule of the `loudness` keyword (pure host arithmetic in float64).  Row r of the output has a gain
    source of integrated loudness stats_src[r] (LUFS) and its own true peak stats_rows[r] (linear); rows with the same
    groups[r] share one gain (groups=None: every row alone) and must share the source.
      g_dB = target - I_src;   with a ceiling (peak is not None): g_dB = min(g_dB, peak - 20 log10(TP)), TP the largest
      true peak of the group (a group of silent rows has no ceiling);   I_src = -inf (nothing passed the gates) or a
      statistic that is NaN (non-finite samples) gives 0 dB, and the row is named.
    -> {"gain_db": [R] float64, "gain": [R] 10^(g_dB / 20) rounded once to float32 (as Python floats), "limited": [R]
    bool (the ceiling set the gain), "silent": the rows whose source was -inf, "nonfinite": the rows with a NaN}"""
    import numpy as np

    src = [float(v) for v in stats_src]
    tp = [float(v) for v in stats_rows]
    R = len(src)
    if len(tp) != R:
        raise ValueError(f"loudness_gain: {R} sources but {len(tp)} rows")
    groups = list(range(R)) if groups is None else list(groups)
    if len(groups) != R:
        raise ValueError(f"loudness_gain: {R} rows but {len(groups)} group labels")
    target = float(target)
    members = {}
    for r, k in enumerate(groups):
        members.setdefault(k, []).append(r)
    gain_db, limited, silent, nonfinite = [0.0] * R, [False] * R, [], []
    for k, rows in members.items():
        I = src[rows[0]]
        if any(src[r] != I and not (math.isnan(src[r]) and math.isnan(I)) for r in rows):
            raise ValueError(f"loudness_gain: the rows of group {k!r} do not share one gain source")
        top = max(tp[r] for r in rows) if not any(math.isnan(tp[r]) for r in rows) else math.nan
        if math.isnan(I) or math.isnan(top) or I == math.inf:
            nonfinite.extend(rows)
            continue
        if I == -math.inf:
            silent.extend(rows)
            continue
        g, lim = target - I, False
        if peak is not None and top > 0.0:
            ceil_db = float(peak) - 20.0 * math.log10(top)
            if ceil_db < g:
                g, lim = ceil_db, True
        for r in rows:
            gain_db[r], limited[r] = g, lim
    gain = [float(np.float32(10.0 ** (g / 20.0))) for g in gain_db]
    return {"gain_db": gain_db, "gain": gain, "limited": limited, "silent": sorted(silent),
            "nonfinite": sorted(nonfinite)}


LIMIT_DEFAULTS = dict(ceiling=None, lookahead_ms=5.0, drive_db=6.0, iterations=4, tol=0.1)
LIMIT_MAX_HALF_WINDOW = 1024                                                       # LIM_MAX_W
LIMIT_DEFAULT_CEILING = -1.0                                                       # dBTP, when loudness= sets none


def limit_options(spec) -> Optional[dict]:
    """The `limit` keyword of the separation entry points: None (off, the default) -> None; True -> LIMIT_DEFAULTS; a
    dict of ceiling / lookahead_ms / drive_db / iterations / tol -> the defaults with those replaced.  ceiling (dBTP;
    None: the `loudness` keyword's peak, or -1 dBTP without one) is a finite number; lookahead_ms a finite number
    > 0; drive_db a finite number >= 0 (how far above the single-gain rule's gain the pre-gain may go); iterations an
    integer in [1, 16]; tol a finite number > 0 (LU).  Anything else -- False, an unknown key -- is refused by name."""
    if spec is None:
        return None
    if spec is True:
        opts = dict(LIMIT_DEFAULTS)
    elif isinstance(spec, Mapping):
        extra = sorted(set(spec) - set(LIMIT_DEFAULTS))
        if extra:
            raise ValueError(f"limit: unknown keys {extra} (a dict of {sorted(LIMIT_DEFAULTS)})")
        opts = dict(LIMIT_DEFAULTS, **spec)
    else:
        raise ValueError(f"limit must be None, True or a dict of {sorted(LIMIT_DEFAULTS)} (got {spec!r})")
    for key in ("ceiling", "lookahead_ms", "drive_db", "tol"):
        v = opts[key]
        if key == "ceiling" and v is None:
            continue
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v):
            raise ValueError(f"limit: {key} = {v!r} is not a finite number"
                             + (" (or None: the loudness keyword's peak)" if key == "ceiling" else ""))
        opts[key] = float(v)
    if opts["lookahead_ms"] <= 0.0:
        raise ValueError(f"limit: lookahead_ms = {opts['lookahead_ms']!r} is not positive")
    if opts["drive_db"] < 0.0:
        raise ValueError(f"limit: drive_db = {opts['drive_db']!r} is negative")
    if opts["tol"] <= 0.0:
        raise ValueError(f"limit: tol = {opts['tol']!r} is not positive")
    k = opts["iterations"]
    if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= 16:
        raise ValueError(f"limit: iterations = {k!r} is not an integer in [1, 16]")
    return opts


def level_options(loudness, limit) -> Optional[dict]:
    """The `loudness` and `limit` keywords of the entry points as the keywords of Engine.loudness_normalize: None when
    both are off; loudness alone is loudness_options' three keys; with a limit its options ride along as "limit", and
    limit alone is no loudness rule (target None): every item one curve against the limiter's ceiling."""
    lopts, lim = loudness_options(loudness), limit_options(limit)
    if lim is None:
        return lopts
    if lopts is None:
        lopts = dict(target=None, peak=None, link="mixture")
    return dict(lopts, limit=lim)


def limiter_half_window(lookahead_ms, fs: int) -> int:
    """W = max(1, floor(lookahead_ms fs / 1000 + 1/2)) (include/ditsep_hip.h); not yet checked against [1, 1024]"""
    return max(1, int(math.floor(float(lookahead_ms) * int(fs) / 1000.0 + 0.5)))


def limiter_window(W: int):
    """The smoothing window of the limiter: w[k] = (1/2 + 1/2 cos(pi k / (W + 1))) / (W + 1), k = -W .. W, formed in
    float64 and rounded once -> float32 [2 W + 1].  The exact sum is 1."""
    import numpy as np

    W = int(W)
    if not 1 <= W <= LIMIT_MAX_HALF_WINDOW:
        raise ValueError(f"limiter: the half-window W = {W} is outside [1, {LIMIT_MAX_HALF_WINDOW}]")
    k = np.arange(-W, W + 1, dtype=np.float64)
    return ((0.5 + 0.5 * np.cos(np.pi * k / (W + 1))) / (W + 1)).astype(np.float32)


def check_limiter(shape, rates, group, pregain, ceiling=None, lookahead_ms=None, lens=None, channels=None) -> tuple:
    """The refusals of dsn_limiter_curve and dsn_apply_curve (include/ditsep_hip.h), raised by name before the library
    is touched: what check_loudness refuses of x [R, C, L], rates, lens and channels; group that is not one integer
    per row; pregain that is not one finite number per group.  With a ceiling (the curve call; linear): group labels
    that are not 0 .. G - 1 in non-decreasing order; rows of a group that disagree on length or rate; a ceiling that
    is not finite and positive; a look-ahead that gives a half-window outside [1, 1024].  Without (apply_curve): a
    label outside [0, G).  -> ((R, C, L), rates, lens or None, channels or None, group, pregain)"""
    (R, Cn, L), rt, ln, ch = check_loudness(shape, rates, lens, channels)
    try:
        bad = any(isinstance(v, bool) or int(v) != v for v in group)
        group = [int(v) for v in group]
    except (TypeError, ValueError):
        bad = True
    if bad or len(group) != R:
        raise ValueError(f"limiter: group must hold one integer label per row (R = {R})")
    pregain = [float(v) for v in pregain]
    G = len(pregain)
    if G < 1:
        raise ValueError("limiter: pregain must hold one number per group, at least one")
    for q, v in enumerate(pregain):
        if not math.isfinite(v):
            raise ValueError(f"limiter: pregain[{q}] = {v!r} is not finite")
    if ceiling is None:
        for r, q in enumerate(group):
            if not 0 <= q < G:
                raise ValueError(f"limiter: group[{r}] = {q} outside [0, G = {G})")
        return (R, Cn, L), rt, ln, ch, group, pregain
    if isinstance(ceiling, bool) or not isinstance(ceiling, (int, float)) or not math.isfinite(ceiling) or ceiling <= 0:
        raise ValueError(f"limiter: the ceiling {ceiling!r} is not a finite positive number (linear)")
    if (isinstance(lookahead_ms, bool) or not isinstance(lookahead_ms, (int, float)) or not math.isfinite(lookahead_ms)
            or lookahead_ms < 0):
        raise ValueError(f"limiter: lookahead_ms = {lookahead_ms!r} is not a finite number >= 0")
    if group[0] != 0 or group[-1] != G - 1 or any(b - a not in (0, 1) for a, b in zip(group, group[1:])):
        raise ValueError(f"limiter: the group labels must be 0 .. G - 1 = {G - 1} in non-decreasing order")
    for r in range(R):
        W = limiter_half_window(lookahead_ms, rt[r])
        if W > LIMIT_MAX_HALF_WINDOW:
            raise ValueError(f"limiter: a look-ahead of {lookahead_ms} ms at {rt[r]} Hz is a half-window W = {W} outside "
                             f"[1, {LIMIT_MAX_HALF_WINDOW}]")
        if r and group[r] == group[r - 1]:
            a, b = (L if ln is None else ln[r - 1]), (L if ln is None else ln[r])
            if a != b or rt[r] != rt[r - 1]:
                raise ValueError(f"limiter: rows {r - 1} and {r} of group {group[r]} disagree on length or rate "
                                 f"({a} at {rt[r - 1]} Hz, {b} at {rt[r]} Hz)")
    return (R, Cn, L), rt, ln, ch, group, pregain


def limiter_drive(g_lo, i_src, target, history, drive_db=6.0, iterations=4, tol=0.1):
    """The pre-gain rule of the `limit` keyword for one group (pure host arithmetic in float64).  g_lo is the gain
    (dB) the single-gain rule native.loudness_gain gave when the ceiling set it, i_src the source's loudness, history
    the evaluations so far as (G dB, measured loudness of the limited programme) pairs.  -> the next pre-gain in dB, or
    None when the loop stops.  Every G is clamped to [g_lo, g_lo + drive_db].
      G_0 = target - i_src;   G_1 = G_0 + (target - I_0);   then the secant step G_k + (target - I_k) / s with the
      slope s = (I_k - I_{k-1}) / (G_k - G_{k-1}) clamped to [1/4, 1];
      stop when |target - I_k| <= tol, after `iterations` evaluations, when I_k is not finite, or when the clamped G
      is one that was evaluated already."""
    lo, hi = float(g_lo), float(g_lo) + float(drive_db)
    clamp = lambda v: min(max(v, lo), hi)
    target = float(target)
    if not history:
        return clamp(target - float(i_src))
    g_k, i_k = (float(v) for v in history[-1])
    if not math.isfinite(i_k) or abs(target - i_k) <= tol or len(history) >= iterations:
        return None
    if len(history) == 1:
        nxt = g_k + (target - i_k)
    else:
        g_p, i_p = (float(v) for v in history[-2])
        slope = (i_k - i_p) / (g_k - g_p) if g_k != g_p and math.isfinite(i_p) else 1.0
        nxt = g_k + (target - i_k) / min(max(slope, 0.25), 1.0)
    nxt = clamp(nxt)
    return None if any(nxt == float(g) for g, _ in history) else nxt


def limiter_best(history, target) -> int:
    """The evaluation of a limiter_drive history that is kept: the one closest to the target (the first of equals);
    evaluations that are not finite lose to any that is."""
    dist = [abs(float(target) - float(i)) if math.isfinite(float(i)) else math.inf for _, i in history]
    return dist.index(min(dist))


_lib = None


# seconds, Hz and dB at this layer; NOT tuned (sanity figures on synthetic bursts only, README "Speaker activity")
ACTIVITY_DEFAULTS = dict(gate=False, n_fft=512, hop=128, band=(100.0, 4000.0), smooth=0.04, range_db=40.0,
                         dominance_db=6.0, hysteresis_db=3.0, min_on=0.1, min_off=0.1, pad=0.0, fade_ms=5.0)
ACTIVITY_MAX_FRAMES = 1 << 22                                                      # ACTIVITY_MAX_FRAMES
ACTIVITY_MAX_HALF_WIDTH = 1024                                                     # ACTIVITY_MAX_HALF_WIDTH
ACTIVITY_MAX_FADE = 4096                                                           # ACTIVITY_MAX_FADE
ACTIVITY_MIN_HOP, ACTIVITY_MAX_HOP = 8, 65536                                       # ACTIVITY_MIN_HOP, ACTIVITY_MAX_HOP


def _number(who, key, v, lo=None) -> float:
    if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v):
        raise ValueError(f"{who}: {key} = {v!r} is not a finite number")
    if lo is not None and v < lo:
        raise ValueError(f"{who}: {key} = {v!r} < {lo}")
    return float(v)


def _check_activity_options(opts) -> None:
    if not isinstance(opts["gate"], bool):
        raise ValueError(f"activity: gate = {opts['gate']!r} is not True or False")
    for key in ("n_fft", "hop"):
        if isinstance(opts[key], bool) or not isinstance(opts[key], int):
            raise ValueError(f"activity: {key} = {opts[key]!r} is not an integer")
    band = opts["band"]
    if isinstance(band, (str, bytes)) or not hasattr(band, "__len__") or len(band) != 2:
        raise ValueError(f"activity: band = {band!r} is not a pair (low, high) in Hz")
    lo, hi = _number("activity", "band[0]", band[0], 0.0), _number("activity", "band[1]", band[1], 0.0)
    if hi < lo:
        raise ValueError(f"activity: band = ({lo}, {hi}) Hz: the high edge is below the low edge")
    opts["band"] = (lo, hi)
    for key in ("smooth", "range_db", "dominance_db", "hysteresis_db", "pad", "fade_ms"):
        opts[key] = _number("activity", key, opts[key], 0.0)
    for key in ("min_on", "min_off"):
        opts[key] = _number("activity", key, opts[key], 0.0)
        if opts[key] <= 0.0:
            raise ValueError(f"activity: {key} = {opts[key]!r} s is not positive")


def activity_options(spec) -> Optional[dict]:
    """The `activity` keyword of the separation entry points: None (off, the default) -> None; True ->
    ACTIVITY_DEFAULTS (segments only); "gate" -> the defaults with gate=True (the inactive stretches of every stem
    become digital silence); a dict of ACTIVITY_DEFAULTS' keys -> the defaults with those replaced: band a pair of
    Hz, smooth / min_on / min_off / pad seconds, range_db / dominance_db / hysteresis_db dB >= 0, fade_ms
    milliseconds.  Anything else, False included, is refused by name."""
    opts = _options("activity", spec, ACTIVITY_DEFAULTS, "None, True, 'gate'",
                    lambda v: {} if v is True else dict(gate=True) if isinstance(v, str) and v == "gate" else None,
                    _check_activity_options)
    if opts is not None and "band" in opts:
        opts["band"] = tuple(opts["band"])
    return opts


def activity_frames(opts, fs: int) -> dict:
    """The seconds of activity_options at rate fs and the options' hop as Engine.activity's frame counts and
    Engine.activity_gate's fade: a duration is max(1, int(sec fs / hop + 0.5)) frames (pad may be 0), half_width =
    int(smooth fs / hop + 0.5) // 2, fade = int(fade_ms fs / 1000 + 0.5) samples."""
    fs, hop = int(fs), int(opts["hop"])

    def frames(sec, least=1):
        return max(least, int(float(sec) * fs / hop + 0.5))

    return dict(min_on=frames(opts["min_on"]), min_off=frames(opts["min_off"]), pad=frames(opts["pad"], 0),
                half_width=int(float(opts["smooth"]) * fs / hop + 0.5) // 2,
                fade=int(float(opts["fade_ms"]) * fs / 1000.0 + 0.5))


def activity_keywords(opts, fs: int) -> dict:
    """activity_options at rate fs -> the keywords of Engine.activity (the gate's hop and fade are
    activity_frames')"""
    fr = activity_frames(opts, fs)
    return dict(fs=int(fs), n_fft=opts["n_fft"], hop=opts["hop"], band=opts["band"], half_width=fr["half_width"],
                range_db=opts["range_db"], dominance_db=opts["dominance_db"], hysteresis_db=opts["hysteresis_db"],
                min_on=fr["min_on"], min_off=fr["min_off"], pad=fr["pad"])


def activity_band(band, fs, n_fft: int) -> tuple:
    """A band in Hz as bins of an n_fft-point STFT at rate fs: j_lo = ceil(f_lo n_fft / fs), j_hi = min(n_fft / 2,
    floor(f_hi n_fft / fs)); an empty band is refused by name."""
    lo, hi = float(band[0]), float(band[1])
    j_lo, j_hi = int(math.ceil(lo * n_fft / fs)), min(n_fft // 2, int(math.floor(hi * n_fft / fs)))
    if j_lo > j_hi:
        raise ValueError(f"activity: the band ({lo}, {hi}) Hz holds no bin of an n_fft = {n_fft} transform at {fs} Hz "
                         f"(bins {j_lo} .. {j_hi})")
    return j_lo, j_hi


def activity_constants(range_db, dominance_db, hysteresis_db) -> tuple:
    """(c_r, c_d, c_r', c_d'): 10^(-dB / 10) of the range, the dominance and each with the hysteresis added, as the
    doubles the device multiplies with"""
    r, d, h = float(range_db), float(dominance_db), float(hysteresis_db)
    return 10.0 ** (-r / 10.0), 10.0 ** (-d / 10.0), 10.0 ** (-(r + h) / 10.0), 10.0 ** (-(d + h) / 10.0)


def activity_ramp(fade: int):
    """The gate's fade: ramp[d - 1] = float32(0.5 + 0.5 cos(pi d / (fade + 1))), d = 1 .. fade, formed in float64 and
    rounded once -> float32 [fade] (empty for the hard gate)."""
    import numpy as np

    fade = int(fade)
    if not 0 <= fade <= ACTIVITY_MAX_FADE:
        raise ValueError(f"activity_gate: fade = {fade} samples outside [0, {ACTIVITY_MAX_FADE}]")
    d = np.arange(1, fade + 1, dtype=np.float64)
    return (0.5 + 0.5 * np.cos(np.pi * d / (fade + 1))).astype(np.float32)


def activity_segments(act_row, F: int, hop: int, L: int) -> list:
    """The runs of set frames among act_row[:F] as sample segments [(start, end), ..]: frame t owns the samples
    [t hop - hop / 2, (t + 1) hop - hop / 2) of [0, L), so a run [s, e) is [max(0, s hop - hop / 2), min(L, e hop -
    hop / 2)); runs that own no sample of the item are dropped."""
    import numpy as np

    a = np.asarray(act_row).reshape(-1)[:int(F)] != 0
    edges = np.flatnonzero(np.diff(np.concatenate([[False], a, [False]]).astype(np.int8)))
    h2 = int(hop) // 2
    segs = []
    for s, e in zip(edges[0::2].tolist(), edges[1::2].tolist()):
        lo, hi = max(0, s * hop - h2), min(int(L), e * hop - h2)
        if hi > lo:
            segs.append((lo, hi))
    return segs


def activity_rttm(stem: str, segments, fs: int) -> list:
    """The RTTM lines of one recording: segments[i] = [(start, end), ..] in samples at rate fs of source i -> one
    "SPEAKER {stem} 1 {onset:.3f} {duration:.3f} <NA> <NA> s{i} <NA> <NA>" per segment, sorted by onset, then source"""
    rows = sorted((s, i, e) for i, row in enumerate(segments) for s, e in row)
    return [f"SPEAKER {stem} 1 {s / fs:.3f} {(e - s) / fs:.3f} <NA> <NA> s{i} <NA> <NA>" for s, i, e in rows]


def check_activity(est_shape, lens=None, fs=16000, n_fft=512, hop=128, band=(100.0, 4000.0), half_width=2,
                   range_db=40.0, dominance_db=6.0, hysteresis_db=3.0, min_on=13, min_off=13, pad=0) -> tuple:
    """The refusals of dsn_activity (include/ditsep_hip.h), raised by name before the library is touched: est that is
    not [B, n, L]; n outside [1, 4]; what check_mask_refine refuses of n_fft, hop and lens; fs that is not a positive
    integer; a band that holds no bin; half_width outside [0, 1024]; range_db, dominance_db or hysteresis_db that is
    not a finite number >= 0; min_on or min_off < 1 frame; pad < 0; more than 2^22 frames per item.
    -> ((B, n, L), lens as a list or None, n_fft, hop, (j_lo, j_hi), the four factors, Fmax)"""
    who = "activity"
    est_shape = tuple(int(v) for v in est_shape)
    if len(est_shape) != 3:
        raise ValueError(f"{who}: est must be [B, n, L] (got {est_shape})")
    B, n, L = est_shape
    n_fft, hop, _, _ = _check_stft(who, B, n, n_fft, hop, 2, 1.0)
    ln = _check_item_lens(who, lens, B, L, n_fft)
    if isinstance(fs, bool) or int(fs) != fs or int(fs) < 1:
        raise ValueError(f"{who}: fs = {fs!r} is not a positive integer")
    if isinstance(band, (str, bytes)) or not hasattr(band, "__len__") or len(band) != 2:
        raise ValueError(f"{who}: band = {band!r} is not a pair (low, high) in Hz")
    bins = activity_band((_number(who, "band[0]", band[0], 0.0), _number(who, "band[1]", band[1], 0.0)), int(fs), n_fft)
    for key, v in (("half_width", half_width), ("min_on", min_on), ("min_off", min_off), ("pad", pad)):
        if isinstance(v, bool) or int(v) != v:
            raise ValueError(f"{who}: {key} = {v!r} is not an integer number of frames")
    if not 0 <= int(half_width) <= ACTIVITY_MAX_HALF_WIDTH:
        raise ValueError(f"{who}: half_width = {half_width} outside [0, {ACTIVITY_MAX_HALF_WIDTH}]")
    for key, v in (("range_db", range_db), ("dominance_db", dominance_db), ("hysteresis_db", hysteresis_db)):
        _number(who, key, v, 0.0)
    if int(min_on) < 1 or int(min_off) < 1:
        raise ValueError(f"{who}: min_on = {min_on} or min_off = {min_off} < 1 frame")
    if int(pad) < 0:
        raise ValueError(f"{who}: pad = {pad} < 0")
    Fmax = 1 + -(-L // hop)
    if Fmax > ACTIVITY_MAX_FRAMES:
        raise ValueError(f"{who}: {Fmax} frames (L = {L}, hop = {hop}) > 2^22 per item")
    return (B, n, L), ln, n_fft, hop, bins, activity_constants(range_db, dominance_db, hysteresis_db), Fmax


def check_activity_gate(x_shape, act_shape, lens=None, hop=128, fade=80) -> tuple:
    """The refusals of dsn_activity_gate, raised by name before the library is touched: x that is not [B, n, L] with n
    in [1, 4]; act that is not [B, n, Fa] with Fa >= the frames L needs; hop outside [8, 65536]; fade outside
    [0, 4096]; lens that is not one sample count in [1, L] per item.  -> ((B, n, L), Fa, lens as a list or None)"""
    who = "activity_gate"
    x_shape, act_shape = tuple(int(v) for v in x_shape), tuple(int(v) for v in act_shape)
    if len(x_shape) != 3 or x_shape[2] < 1:
        raise ValueError(f"{who}: x must be [B, n, L] (got {x_shape})")
    B, n, L = x_shape
    if B < 1:
        raise ValueError(f"{who}: B = {B} < 1")
    if n < 1 or n > MASK_REFINE_MAX_SRC:
        raise ValueError(f"{who}: n = {n} outside [1, {MASK_REFINE_MAX_SRC}]")
    if isinstance(hop, bool) or int(hop) != hop or not ACTIVITY_MIN_HOP <= int(hop) <= ACTIVITY_MAX_HOP:
        raise ValueError(f"{who}: hop = {hop!r} outside [{ACTIVITY_MIN_HOP}, {ACTIVITY_MAX_HOP}]")
    if isinstance(fade, bool) or int(fade) != fade or not 0 <= int(fade) <= ACTIVITY_MAX_FADE:
        raise ValueError(f"{who}: fade = {fade!r} samples outside [0, {ACTIVITY_MAX_FADE}]")
    need = (L - 1 + int(hop) // 2) // int(hop) + 1
    if len(act_shape) != 3 or act_shape[:2] != (B, n) or act_shape[2] < need:
        raise ValueError(f"{who}: act must be [B, n, F] with x's B and n and F >= {need} frames (L = {L}, hop = {hop}; "
                         f"got {act_shape})")
    return (B, n, L), act_shape[2], check_lens(lens, B, L) if lens is not None else None


def load_library() -> C.CDLL:
    """dlopen the in-tree HIP library; loud failure when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} not found: the HIP extension is required (no CPU/PyTorch fallback). "
            "Build it with `python -c 'import __graft_entry__ as g; g.build()'` or `make -C ditsep_amd/csrc`.")
    lib = C.CDLL(LIB_PATH)
    vp, ci, cf, fp = C.c_void_p, C.c_int, C.c_float, C.POINTER(C.c_float)
    lib.dsn_create.restype = vp
    lib.dsn_create.argtypes = [C.POINTER(DsnConfig)]
    lib.dsn_destroy.restype = None
    lib.dsn_destroy.argtypes = [vp]
    lib.dsn_last_error.restype = C.c_char_p
    lib.dsn_last_error.argtypes = [vp]
    lib.dsn_load_tensor.argtypes = [vp, C.c_char_p, vp, C.POINTER(C.c_int64), ci, ci]
    lib.dsn_finalize_weights.argtypes = [vp]
    lib.dsn_finalize_weights_ex.argtypes = [vp, ci]
    lib.dsn_score.argtypes = [vp, vp, vp, vp, vp, ci, ci, vp]
    lib.dsn_score_ragged.argtypes = [vp, vp, vp, vp, C.POINTER(C.c_int32), vp, ci, ci, vp]
    lib.dsn_pc_sample_ragged.argtypes = [vp, vp, C.POINTER(C.c_int32), vp, C.c_uint64, vp, ci, ci, ci,
                                         C.POINTER(DsnSamplerOpts), C.POINTER(ci), vp]
    lib.dsn_decode_ragged.argtypes = [vp, vp, C.POINTER(C.c_int32), vp, ci, ci, vp]
    lib.dsn_encode_ragged.argtypes = [vp, vp, C.POINTER(C.c_int32), vp, C.c_uint64, vp, ci, ci, vp]
    lib.dsn_separate_ragged.argtypes = [vp, vp, C.POINTER(C.c_int32), vp, vp, C.c_uint64, vp, ci, ci, ci,
                                        C.POINTER(DsnSamplerOpts), C.POINTER(ci), vp]
    lib.dsn_ouve_schedule.argtypes = [vp, ci, cf, cf, fp, fp, fp, fp, fp, fp]
    lib.dsn_pc_sample.argtypes = [vp, vp, vp, C.c_uint64, vp, ci, ci, ci, ci, cf, cf, ci, C.POINTER(ci), vp]
    lib.dsn_pc_sample_sched.argtypes = [vp, vp, vp, C.c_uint64, vp, ci, ci, ci, fp, ci, cf, ci, C.POINTER(ci), vp]
    lib.dsn_pc_sample_ex.argtypes = [vp, vp, vp, C.c_uint64, vp, ci, ci, ci, C.POINTER(DsnSamplerOpts),
                                     C.POINTER(ci), vp]
    lib.dsn_pc_sample_mix.argtypes = [vp, vp, vp, C.c_uint64, vp, ci, ci, ci, C.POINTER(DsnMixOpts), C.POINTER(ci), vp]
    lib.dsn_sb_sample.argtypes = [vp, vp, vp, C.c_uint64, vp, ci, ci, ci, cf, cf, cf, cf, ci, vp]
    lib.dsn_ode_sample.argtypes = [vp, vp, vp, C.c_uint64, vp, ci, ci, C.POINTER(DsnOdeOpts), C.POINTER(DsnOdeStats),
                                   vp]
    lib.dsn_score_loss.argtypes = [vp, vp, vp, vp, vp, vp, C.c_uint64, vp, vp, vp, vp, vp, ci, ci,
                                   C.POINTER(DsnLossOpts), vp]
    lib.dsn_score_loss_ragged.argtypes = [vp, vp, vp, C.POINTER(C.c_int32), vp, vp, vp, C.c_uint64, vp, vp, vp, vp, vp,
                                          ci, ci, C.POINTER(DsnLossOpts), vp]
    lib.dsn_decode.argtypes = [vp, vp, vp, ci, ci, ci, vp]
    lib.dsn_encode.argtypes = [vp, vp, vp, C.c_uint64, vp, ci, ci, vp]
    lib.dsn_decode_chunked.argtypes = [vp, vp, vp, ci, ci, ci, ci, ci, vp]
    lib.dsn_encode_chunked.argtypes = [vp, vp, vp, C.c_uint64, vp, ci, ci, ci, ci, vp]
    lib.dsn_latent_frames.argtypes = [vp, ci]
    lib.dsn_hop_length.argtypes = [vp]
    lib.dsn_separate.argtypes = [vp, vp, vp, vp, C.c_uint64, vp, ci, ci, ci, ci, ci, cf, cf, ci,
                                 C.POINTER(ci), vp]
    lib.dsn_enable_graphs.argtypes = [vp, ci]
    lib.dsn_workspace_bytes.restype = C.c_int64
    lib.dsn_workspace_bytes.argtypes = [vp]
    lib.dsn_profile_begin.argtypes = [vp]
    lib.dsn_profile_end.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int64)]
    lib.dsn_profile_hbm.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int64)]
    lib.dsn_profile_rows.argtypes = [vp, ci, C.c_char_p, C.POINTER(C.c_double), C.POINTER(C.c_double),
                                     C.POINTER(C.c_double), C.POINTER(C.c_int64)]
    lib.dsn_test_gemm.argtypes = [vp, C.POINTER(DsnTestGemm), vp]
    lib.dsn_test_kernel.argtypes = [vp, C.POINTER(DsnTestKernel), vp]
    lib.dsn_dit_plan.argtypes = [C.POINTER(DsnConfig), ci, ci, C.POINTER(DsnDitPlan)]
    lib.dsn_si_sdr_pit.argtypes = [vp, vp, vp, ci, ci, ci, fp, C.POINTER(ci), vp]
    lib.dsn_si_bss_eval.argtypes = [vp, vp, vp, ci, ci, ci, ci, cf, fp, fp, fp, C.POINTER(ci), vp]
    lib.dsn_stoi.argtypes = [vp, vp, vp, ci, ci, ci, ci, ci, C.POINTER(ci), fp, C.POINTER(ci), vp]
    lib.dsn_composite.argtypes = [vp, vp, vp, ci, ci, ci, ci, C.POINTER(ci), fp, C.POINTER(DsnCompositeOut), vp]
    i32p = C.POINTER(C.c_int32)
    lib.dsn_si_bss_eval_ragged.argtypes = [vp, vp, vp, ci, ci, ci, i32p, ci, cf, fp, fp, fp, C.POINTER(ci), vp]
    lib.dsn_stoi_ragged.argtypes = [vp, vp, vp, ci, ci, ci, i32p, ci, ci, C.POINTER(ci), fp, C.POINTER(ci), vp]
    lib.dsn_composite_ragged.argtypes = [vp, vp, vp, ci, ci, ci, i32p, ci, C.POINTER(ci), fp,
                                         C.POINTER(DsnCompositeOut), vp]
    lib.dsn_window_stitch.argtypes = [vp, vp, ci, ci, ci, ci, ci, ci, ci, vp, i32p, C.POINTER(C.c_double), vp]
    lib.dsn_score_window_plan.argtypes = [i32p, ci, ci, ci, ci, ci, i32p, i32p, fp, C.POINTER(ci), C.POINTER(ci)]
    lib.dsn_score_windowed.argtypes = [vp, vp, vp, vp, i32p, vp, ci, ci, ci, ci, ci, ci, vp]
    lib.dsn_pc_sample_windowed.argtypes = [vp, vp, i32p, vp, C.c_uint64, vp, ci, ci, ci, ci, ci, ci, ci,
                                           C.POINTER(DsnSamplerOpts), C.POINTER(ci), vp]
    lib.dsn_separate_windowed.argtypes = [vp, vp, i32p, vp, vp, C.c_uint64, vp, ci, ci, ci, ci, ci, ci, ci,
                                          C.POINTER(DsnSamplerOpts), C.POINTER(ci), vp]
    lib.dsn_resample_plan.argtypes = [ci, ci, C.POINTER(ci), C.POINTER(ci), C.POINTER(ci), C.POINTER(ci), i32p, fp]
    lib.dsn_resample_length.argtypes = [ci, ci, ci]
    lib.dsn_resample.argtypes = [vp, vp, ci, ci, ci, i32p, ci, ci, ci, vp, ci, vp]
    i64p = C.POINTER(C.c_int64)
    lib.dsn_pcm_decode.argtypes = [vp, vp, C.c_int64, ci, i64p, i32p, i32p, i32p, ci, vp, ci, ci, vp]
    lib.dsn_pcm_encode.argtypes = [vp, vp, ci, ci, i32p, ci, vp, C.c_int64, i64p, i64p, vp]
    lib.dsn_scale_output.argtypes = [vp, vp, vp, ci, ci, ci, i32p, vp, fp, vp]
    lib.dsn_bss_eval.argtypes = [vp, vp, vp, ci, ci, ci, i32p, C.POINTER(ci), C.POINTER(DsnBssEvalOpts),
                                 C.POINTER(DsnBssEvalOut), vp]
    lib.dsn_bss_eval_plan.argtypes = [ci, ci, ci, ci, C.c_int64, C.POINTER(ci), C.POINTER(ci), C.POINTER(ci), i64p]
    lib.dsn_mask_refine.argtypes = [vp, vp, vp, ci, ci, ci, i32p, ci, ci, ci, C.c_float, vp, vp]
    f64p = C.POINTER(C.c_double)
    lib.dsn_ensemble_combine.argtypes = [vp, vp, vp, ci, ci, ci, ci, i32p, ci, vp, i32p, i32p, i32p, f64p, f64p, f64p,
                                         vp]
    lib.dsn_stems.argtypes = [vp, vp, vp, ci, ci, ci, ci, i32p, i32p, ci, ci, ci, ci, C.c_float, C.c_float, vp, f64p,
                              f64p, vp]
    lib.dsn_pcm_encode_frames.argtypes = [vp, vp, ci, ci, ci, i32p, i32p, ci, vp, C.c_int64, i64p, i64p, vp]
    lib.dsn_beamform.argtypes = [vp, vp, vp, ci, ci, ci, ci, i32p, i32p, ci, ci, ci, ci, C.c_float, C.c_float, ci,
                                 C.c_int64, vp, f64p, vp]
    lib.dsn_beamform_spatial.argtypes = [vp, vp, vp, ci, ci, ci, ci, i32p, i32p, ci, ci, ci, ci, C.c_float, C.c_float, ci,
                                         C.c_float, C.c_float, C.c_float, C.c_float, C.c_int64, vp, f64p, f64p, i32p, vp]
    lib.dsn_beamform_track.argtypes = [vp, vp, vp, ci, ci, ci, ci, i32p, i32p, ci, ci, ci, ci, C.c_float, C.c_float, ci, ci,
                                       ci, ci, C.c_int64, vp, f64p, vp]
    lib.dsn_beamform_design.argtypes = [vp, vp, vp, ci, ci, ci, ci, i32p, i32p, ci, ci, ci, ci, C.c_float, C.c_float, ci,
                                        ci, ci, C.c_int64, vp, f64p, vp]
    lib.dsn_beamform_spatial_design.argtypes = [vp, vp, vp, ci, ci, ci, ci, i32p, i32p, ci, ci, ci, ci, C.c_float,
                                                C.c_float, ci, ci, ci, C.c_float, C.c_float, C.c_float, C.c_float,
                                                C.c_int64, vp, f64p, f64p, i32p, vp]
    lib.dsn_beamform_track_design.argtypes = [vp, vp, vp, ci, ci, ci, ci, i32p, i32p, ci, ci, ci, ci, C.c_float,
                                              C.c_float, ci, ci, ci, ci, ci, ci, C.c_int64, vp, f64p, vp]
    lib.dsn_beamform_solve.argtypes = [vp, vp, i32p, ci, ci, ci, ci, ci, ci, C.c_float, C.c_float, ci, ci, vp, vp]
    lib.dsn_dereverb.argtypes = [vp, vp, ci, ci, ci, i32p, i32p, ci, ci, ci, ci, ci, C.c_float, C.c_float, C.c_int64, vp,
                                 f64p, i32p, vp]
    lib.dsn_mrstft_loss.argtypes = [vp, vp, vp, ci, ci, ci, C.POINTER(DsnMrstftConfig), C.POINTER(DsnMrstftOut), vp]
    lib.dsn_mrstft_loss_ragged.argtypes = [vp, vp, vp, C.POINTER(C.c_int32), ci, ci, ci, C.POINTER(DsnMrstftConfig),
                                           C.POINTER(DsnMrstftOut), vp]
    lib.dsn_kweight_coeffs.argtypes = [ci, f64p]
    lib.dsn_loudness.argtypes = [vp, vp, ci, ci, ci, i32p, i32p, i32p, ci, f64p, vp]
    lib.dsn_apply_gain.argtypes = [vp, vp, ci, ci, ci, i32p, i32p, fp, vp, vp]
    lib.dsn_limiter_curve.argtypes = [vp, vp, ci, ci, ci, i32p, i32p, i32p, i32p, ci, fp, cf, C.c_double, vp, vp, f64p,
                                      vp]
    lib.dsn_apply_curve.argtypes = [vp, vp, ci, ci, ci, i32p, i32p, i32p, ci, fp, vp, vp, vp]
    cd = C.c_double
    lib.dsn_activity.argtypes = [vp, vp, ci, ci, ci, i32p, ci, ci, ci, ci, ci, cd, cd, cd, cd, ci, ci, ci, vp, vp, vp, vp,
                                 vp]
    lib.dsn_activity_gate.argtypes = [vp, vp, vp, ci, ci, ci, ci, i32p, ci, ci, fp, vp, vp]
    lib.dsn_debug_read.argtypes = [vp, C.c_char_p, vp, C.c_int64]
    lib.dsn_bench_igemm.argtypes = [vp] + [ci] * 10 + [C.POINTER(C.c_double)]
    for name in EXPORTS:
        getattr(lib, name)      # every symbol include/ditsep_hip.h declares must resolve
    _lib = lib
    return lib


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else C.c_void_p(t.data_ptr())


def _host(t: Optional[torch.Tensor], ctype=C.c_double):
    """A host tensor the library writes, as a pointer to its elements"""
    return None if t is None else C.cast(C.c_void_p(t.data_ptr()), C.POINTER(ctype))


def _i32(v: Optional[list]):
    """One int32 per item, or None"""
    return None if v is None else (C.c_int32 * len(v))(*v)


def mrstft_unsupported(*, window="hann_window", w_phs=0.0, scale=None, scale_invariance=False, decay=1.0, **other):
    """Raise NotImplementedError for the options of the reference's MultiResolutionSTFTLoss / loss wrappers that have
    no native kernel (no fallback): the mel / chroma `scale`, the phase term, `scale_invariance`, a window other than
    torch.hann_window, and a `decay` other than 1 (the reference's weight decay is state carried across calls)."""
    if scale is not None:
        raise NotImplementedError(f"mrstft_loss: scale='{scale}' (mel / chroma filterbanks) is not implemented natively")
    if w_phs:
        raise NotImplementedError("mrstft_loss: the phase term (w_phs != 0) is not implemented natively")
    if scale_invariance:
        raise NotImplementedError("mrstft_loss: scale_invariance is not implemented natively")
    if window != "hann_window":
        raise NotImplementedError(f"mrstft_loss: window='{window}' (only 'hann_window' is implemented natively)")
    if float(decay) != 1.0:
        raise NotImplementedError("mrstft_loss: decay != 1.0 makes the loss weight depend on the number of earlier "
                                  "calls in the reference; only decay = 1.0 is implemented")
    if other:
        raise NotImplementedError(f"mrstft_loss: unsupported option(s) {sorted(other)}")


def mrstft_combine(tables: Mapping, *, w_sc=1.0, w_log_mag=1.0, w_lin_mag=0.0, mrstft_weight=1.0, l1_weight=0.0,
                   l2_weight=0.0, pit="batch") -> dict:
    """Pair tables (float64: "sc", "log_mag", "lin_mag" [R,B,n,n]; "l1", "l2" [B,n,n]; entry [.., b, i, j] compares
    reference source i with estimate source j) -> the reference's MultiLoss dict and the chosen permutations.

    * auraloss.py STFTLoss.forward: per resolution w_sc * sc + w_log_mag * log_mag + w_lin_mag * lin_mag, reduced by
      the mean -- the spectral convergence is one Frobenius ratio per (b, channel) and averages over B*n, the
      magnitude terms average over all elements, which for equal-sized items is again the mean over (b, channel);
      MultiResolutionSTFTLoss.forward then averages over the resolutions.  A zero weight drops the term.
    * losses.py PITLoss.forward: ONE permutation for the whole batch, the one with the smallest batch-mean loss,
      chosen independently per term (pit="batch"); a single source takes no permutation.  pit="item" (the
      smallest loss per item) and pit=None (the identity) are additions of this project, not reference behaviour.
    * ldm.py:132-152: the L1 / L2 terms exist only with a positive weight; "loss" is the sum of the terms present.
    Ties go to the first permutation in itertools.permutations order.

    Mixed lengths (Engine.mrstft_loss with lens=): the per-item tables of a ragged batch are treated exactly as those
    of a dense batch -- every item weighs the same in a batch mean, however long it is, and pit="batch" still picks
    one permutation for the whole batch by that mean.  This is this project's DEFINITION: the reference has no
    mixed-length form (its tensors hold equally long items, for which the two readings coincide)."""
    from itertools import permutations

    if pit not in ("batch", "item", None):
        raise ValueError(f"pit must be 'batch', 'item' or None (got {pit!r})")
    l1 = torch.as_tensor(tables["l1"], dtype=torch.float64)
    B, n = l1.shape[:2]
    ident = tuple(range(n))
    perms = [ident] if (n == 1 or pit is None) else list(permutations(range(n)))
    rows = torch.arange(n)

    def spectral(p):                                                    # [B]
        v = torch.zeros(B, dtype=torch.float64)
        for w, key in ((w_sc, "sc"), (w_log_mag, "log_mag"), (w_lin_mag, "lin_mag")):
            t = torch.as_tensor(tables[key], dtype=torch.float64)
            if w and t.shape[0]:
                v = v + float(w) * t[:, :, rows, list(p)].mean(-1).mean(0)
        return v

    def choose(item_values):
        vals = torch.stack([item_values(p) for p in perms])            # [P,B]
        pt = torch.tensor(perms, dtype=torch.long)
        if pit == "item":
            k = vals.argmin(0)
            return vals[k, torch.arange(B)].mean(), pt[k], vals.T
        means = vals.mean(1)
        k = int(means.argmin())
        return means[k], pt[k].expand(B, n).clone(), means

    out = {}
    loss, perm, vals = choose(spectral)
    out["pit_mrstft_loss"], out["pit_mrstft_perm"] = float(mrstft_weight) * loss, perm
    out["mrstft_values"], out["perms"] = float(mrstft_weight) * vals, perms
    total = out["pit_mrstft_loss"]
    for key, w in (("l1", l1_weight), ("l2", l2_weight)):
        if w > 0.0:
            t = torch.as_tensor(tables[key], dtype=torch.float64)
            loss, perm, _ = choose(lambda p, t=t: t[:, rows, list(p)].mean(-1))
            out[f"pit_{key}_loss"], out[f"pit_{key}_perm"] = float(w) * loss, perm
            total = total + out[f"pit_{key}_loss"]
    out["loss"] = total
    return out


def _dev32(t: torch.Tensor, device) -> torch.Tensor:
    return t.to(device=device, dtype=torch.float32).contiguous()


def downmix(x: torch.Tensor) -> torch.Tensor:
    """x [B, C, L] -> [B, 1, L]: (x_0 + .. + x_{C-1}) / C in float32 in that order, the expression of the device's
    downmix (dsn_resample, dsn_pcm_decode); one channel passes as it is"""
    s = x[:, 0]
    for c in range(1, int(x.shape[1])):
        s = s + x[:, c]
    return (s / float(x.shape[1]) if x.shape[1] > 1 else s)[:, None]


class Engine:
    """One native context on one GPU."""

    def __init__(self, *, device: int = 0, precision: int = PREC_BF16X3, n_src: int = 2, latent_dim: int = 64,
                 score_kind: int = SCORE_DIT, dit_embed_dim: int = 1024, dit_depth: int = 24,
                 dit_heads: int = 16, ncsn_nf: int = 128, ncsn_ch_mult=(1, 2, 2), ncsn_num_res_blocks: int = 2,
                 ncsn_attn_resolution: int = 16, ncsn_image_size: int = 64, ncsn_max_latent_length: int = 4,
                 vae_channels: int = 128, vae_c_mults=(1, 2, 4, 8, 16),
                 vae_strides=(2, 4, 4, 8, 8), vae_enc_latent_dim: int = 128, vae_use_snake: bool = False,
                 vae_final_tanh: bool = True, vae_has_encoder: bool = True, vae_has_decoder: bool = True,
                 sde_theta: float = 1.5, sde_sigma_min: float = 0.96, sde_sigma_max: float = 10.0):
        self.lib = load_library()
        if not torch.cuda.is_available():
            raise RuntimeError("ditsep_amd needs a ROCm GPU (torch.cuda.is_available() is False)")
        cfg = DsnConfig()
        cfg.device, cfg.precision, cfg.n_src, cfg.latent_dim = device, precision, n_src, latent_dim
        cfg.score_kind = score_kind
        cfg.dit_embed_dim, cfg.dit_depth, cfg.dit_heads = dit_embed_dim, dit_depth, dit_heads
        cfg.ncsn_nf, cfg.ncsn_n_levels = ncsn_nf, len(ncsn_ch_mult)
        for i, m in enumerate(ncsn_ch_mult):
            cfg.ncsn_ch_mult[i] = int(m)
        cfg.ncsn_num_res_blocks, cfg.ncsn_attn_resolution = ncsn_num_res_blocks, ncsn_attn_resolution
        cfg.ncsn_image_size, cfg.ncsn_max_latent_length = ncsn_image_size, ncsn_max_latent_length
        cfg.vae_channels, cfg.vae_n_blocks = vae_channels, len(vae_c_mults)
        assert len(vae_c_mults) == len(vae_strides) <= MAX_VAE_BLOCKS
        for i, (m, s) in enumerate(zip(vae_c_mults, vae_strides)):
            cfg.vae_c_mults[i], cfg.vae_strides[i] = int(m), int(s)
        cfg.vae_enc_latent_dim = vae_enc_latent_dim
        cfg.vae_use_snake, cfg.vae_final_tanh = int(vae_use_snake), int(vae_final_tanh)
        cfg.vae_has_encoder, cfg.vae_has_decoder = int(vae_has_encoder), int(vae_has_decoder)
        cfg.sde_theta, cfg.sde_sigma_min, cfg.sde_sigma_max = sde_theta, sde_sigma_min, sde_sigma_max
        self.cfg = cfg
        self.device = torch.device("cuda", device)
        self.n_src, self.latent_dim = n_src, latent_dim
        self.ctx = self.lib.dsn_create(C.byref(cfg))
        if not self.ctx:
            raise RuntimeError("dsn_create failed: " + self.lib.dsn_last_error(None).decode())

    # ------------------------------------------------------------------ plumbing
    def close(self):
        if getattr(self, "ctx", None):
            self.lib.dsn_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc: int, what: str):
        if rc != 0:
            raise RuntimeError(f"{what} failed ({rc}): {self.lib.dsn_last_error(self.ctx).decode()}")

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    # ------------------------------------------------------------------ weights
    def load_state_dict(self, sd: Mapping[str, torch.Tensor], prefix: str = ""):
        """Feed reference-named tensors (e.g. `score_model.*`, `vae.decoder.*`)."""
        for k, v in sd.items():
            if not torch.is_floating_point(v):
                continue
            t = v.detach().to(torch.float32).contiguous()
            shape = (C.c_int64 * max(t.ndim, 1))(*t.shape)
            self._check(self.lib.dsn_load_tensor(self.ctx, (prefix + k).encode(), C.c_void_p(t.data_ptr()),
                                                 shape, t.ndim, int(t.is_cuda)), f"dsn_load_tensor({prefix + k})")

    def finalize(self, strict: bool = True):
        """strict: tensors the configured network does not consume are an error (load_state_dict(strict=True))."""
        self._check(self.lib.dsn_finalize_weights_ex(self.ctx, int(strict)), "dsn_finalize_weights")

    # ------------------------------------------------------------------ path
    def score(self, xt, t, mix, frames=None, window=None, batch=0, fade="hann"):
        """frames (sequence of B ints, optional): a ragged batch padded to T frames -- item b's score over its first
        frames[b] frames is what it gets alone; the padded region of the output is unspecified (dsn_score_ragged).
        window = (Tw, To) in latent frames, with frames: the window-blended score of long latents (score_window_plan,
        dsn_score_windowed) -- the DiT runs on overlapping windows of Tw frames, at most `batch` per call (0: all), and
        the window scores are cross-faded (`fade`) back into one score per recording, zero past its end.  A definition,
        not the score of any trained model."""
        if window is not None:
            fr, Tw, To = check_windowed(self.cfg.score_kind, frames, xt.shape[0], xt.shape[-1], window)
            if fade not in FADES:
                raise ValueError(f"fade must be one of {sorted(FADES)} (got {fade!r})")
            xt, t, mix = (_dev32(a, self.device) for a in (xt, t, mix))
            R, n, D, T = xt.shape
            out = torch.empty_like(xt)
            self._check(self.lib.dsn_score_windowed(self.ctx, _ptr(xt), _ptr(t), _ptr(mix), (C.c_int32 * R)(*fr),
                                                    _ptr(out), R, T, Tw, To, FADES[fade], int(batch), self._stream()),
                        "dsn_score_windowed")
            return out
        if frames is not None:
            frames = check_ragged(self.cfg.score_kind, frames, xt.shape[0], xt.shape[-1])
        xt, t, mix = (_dev32(a, self.device) for a in (xt, t, mix))
        B, n, D, T = xt.shape
        out = torch.empty_like(xt)
        if frames is not None:
            self._check(self.lib.dsn_score_ragged(self.ctx, _ptr(xt), _ptr(t), _ptr(mix), (C.c_int32 * B)(*frames),
                                                  _ptr(out), B, T, self._stream()), "dsn_score_ragged")
            return out
        self._check(self.lib.dsn_score(self.ctx, _ptr(xt), _ptr(t), _ptr(mix), _ptr(out), B, T, self._stream()),
                    "dsn_score")
        return out

    def ouve_schedule(self, N: int, t_eps: float, snr: float):
        arr = [(C.c_float * N)() for _ in range(5)]
        stdT = C.c_float()
        self._check(self.lib.dsn_ouve_schedule(self.ctx, N, t_eps, snr, *arr, C.byref(stdT)), "dsn_ouve_schedule")
        names = ("t", "std", "step", "gain", "G")
        out = {k: torch.tensor(list(a), dtype=torch.float32) for k, a in zip(names, arr)}
        out["std_T"] = stdT.value
        return out

    def pc_sample(self, y, noise=None, *, N=30, corrector_steps=1, snr=0.5, t_eps=0.03, denoise=True, seed=0,
                  timesteps=None, predictor="reverse_diffusion", corrector="ald", prior_mean=None,
                  intermediate=False, frames=None, window=None, batch=0, fade="hann"):
        """timesteps: optional explicit schedule (>= N floats, host) -> the scheduled sampler.
        predictor / corrector: the reference's registered names (the ones with a native kernel).
        prior_mean: `true_mean` [B,n,D,T].  intermediate: also return the per-step (x, x_mean) list.
        frames (sequence of B ints, optional): a ragged batch -- y and noise keep their padded shapes, item b consumes
        noise[..., :frames[b]] and gets what it gets alone; x[b, :, :, frames[b]:] is zero (dsn_pc_sample_ragged).
        window = (Tw, To) in latent frames, with frames: the state is the whole latent of every recording and every
        score evaluation is the window-blended one of `score` (dsn_pc_sample_windowed); nfe = N (corrector_steps + 1),
        shared by all windows.  Not with timesteps, prior_mean or intermediate."""
        if predictor not in PREDICTORS or corrector not in CORRECTORS:
            raise NotImplementedError(f"no native kernel for predictor {predictor!r} / corrector {corrector!r}")
        if window is not None:
            if timesteps is not None or prior_mean is not None or intermediate:
                raise NotImplementedError("window= does not take timesteps, prior_mean or intermediate")
            if fade not in FADES:
                raise ValueError(f"fade must be one of {sorted(FADES)} (got {fade!r})")
            fr, Tw, To = check_windowed(self.cfg.score_kind, frames, y.shape[0], y.shape[-1], window, corrector)
            y = _dev32(y, self.device)
            R, _, D, T = y.shape
            draws = 1 + N * (corrector_steps + (0 if predictor == "none" else 1))
            if noise is not None:
                noise = _dev32(noise, self.device)
                if tuple(noise.shape) != (draws, R, self.n_src, D, T):
                    raise ValueError(f"noise must be {(draws, R, self.n_src, D, T)}, got {tuple(noise.shape)}")
            x = torch.empty((R, self.n_src, D, T), device=self.device, dtype=torch.float32)
            nfe = C.c_int()
            o = DsnSamplerOpts(PREDICTORS[predictor], CORRECTORS[corrector], int(corrector_steps), float(snr),
                               float(t_eps), int(denoise), None, None, None)
            self._check(self.lib.dsn_pc_sample_windowed(self.ctx, _ptr(y), (C.c_int32 * R)(*fr), _ptr(noise), seed,
                                                        _ptr(x), R, T, N, Tw, To, FADES[fade], int(batch), C.byref(o),
                                                        C.byref(nfe), self._stream()), "dsn_pc_sample_windowed")
            return x, nfe.value
        if frames is not None:
            frames = check_ragged(self.cfg.score_kind, frames, y.shape[0], y.shape[-1], corrector)
        y = _dev32(y, self.device)
        B, _, D, T = y.shape
        draws = 1 + N * (corrector_steps + (0 if predictor == "none" else 1))
        if noise is not None:
            noise = _dev32(noise, self.device)
            assert tuple(noise.shape) == (draws, B, self.n_src, D, T), noise.shape
        x = torch.empty((B, self.n_src, D, T), device=self.device, dtype=torch.float32)
        nfe = C.c_int()
        plain = (predictor == "reverse_diffusion" and corrector == "ald" and prior_mean is None and not intermediate
                 and frames is None)
        if plain and timesteps is None:
            self._check(self.lib.dsn_pc_sample(self.ctx, _ptr(y), _ptr(noise), seed, _ptr(x), B, T, N,
                                               corrector_steps, snr, t_eps, int(denoise), C.byref(nfe),
                                               self._stream()), "dsn_pc_sample")
            return x, nfe.value
        ts = None if timesteps is None else (C.c_float * N)(*[float(v) for v in list(timesteps)[:N]])
        if plain:
            self._check(self.lib.dsn_pc_sample_sched(self.ctx, _ptr(y), _ptr(noise), seed, _ptr(x), B, T, N, ts,
                                                     corrector_steps, snr, int(denoise), C.byref(nfe),
                                                     self._stream()), "dsn_pc_sample_sched")
            return x, nfe.value
        pm = None if prior_mean is None else _dev32(prior_mean, self.device)
        if pm is not None and tuple(pm.shape) != tuple(x.shape):
            raise ValueError(f"prior_mean must be {tuple(x.shape)}, got {tuple(pm.shape)}")
        im = (torch.empty((N, 2, B, self.n_src, D, T), device=self.device, dtype=torch.float32)
              if intermediate else None)
        o = DsnSamplerOpts(PREDICTORS[predictor], CORRECTORS[corrector], int(corrector_steps), float(snr),
                           float(t_eps), int(denoise), ts if ts is not None else None,
                           None if pm is None else pm.data_ptr(), None if im is None else im.data_ptr())
        if frames is not None:
            self._check(self.lib.dsn_pc_sample_ragged(self.ctx, _ptr(y), (C.c_int32 * B)(*frames), _ptr(noise), seed,
                                                      _ptr(x), B, T, N, C.byref(o), C.byref(nfe), self._stream()),
                        "dsn_pc_sample_ragged")
        else:
            self._check(self.lib.dsn_pc_sample_ex(self.ctx, _ptr(y), _ptr(noise), seed, _ptr(x), B, T, N, C.byref(o),
                                                  C.byref(nfe), self._stream()), "dsn_pc_sample_ex")
        if intermediate:
            return x, nfe.value, [(im[i, 0], im[i, 1]) for i in range(N)]
        return x, nfe.value

    def pc_sample_mix(self, y, noise=None, *, N=30, prior_mix=False, d_lambda=2.0, sigma_min=0.05, sigma_max=0.5,
                      avg_len=510, predictor="reverse_diffusion", corrector="ald2", corrector_steps=1, snr=0.5,
                      t_eps=0.03, denoise=True, seed=0):
        """MixSDE / PriorMixSDE predictor-corrector sampler (ald2 corrector) on the latent state."""
        if predictor not in PREDICTORS or corrector not in MIX_CORRECTORS:
            raise NotImplementedError(f"no native kernel for predictor {predictor!r} / corrector {corrector!r} with MixSDE")
        y = _dev32(y, self.device)
        B, _, D, T = y.shape
        c = 0 if corrector == "none" else int(corrector_steps)
        draws = 1 + N * (c + (0 if predictor == "none" else 1))
        if noise is not None:
            noise = _dev32(noise, self.device)
            assert tuple(noise.shape) == (draws, B, self.n_src, D, T), noise.shape
        x = torch.empty((B, self.n_src, D, T), device=self.device, dtype=torch.float32)
        o = DsnMixOpts(int(prior_mix), float(d_lambda), float(sigma_min), float(sigma_max), int(avg_len),
                       PREDICTORS[predictor], MIX_CORRECTORS[corrector], c, float(snr), float(t_eps), int(denoise))
        nfe = C.c_int()
        self._check(self.lib.dsn_pc_sample_mix(self.ctx, _ptr(y), _ptr(noise), seed, _ptr(x), B, T, N, C.byref(o),
                                               C.byref(nfe), self._stream()), "dsn_pc_sample_mix")
        return x, nfe.value

    def sb_sample(self, y, noise=None, *, N=50, k=2.6, c=0.4, sb_eps=1e-8, t_eps=1e-4, sampler_type="ode", seed=0):
        """Schroedinger-bridge sampler (reference get_sb_sampler + SBVESDE) on the latent state."""
        if sampler_type not in SB_TYPES:
            raise ValueError("Invalid type. Choose 'ode' or 'sde'.")
        y = _dev32(y, self.device)
        B, _, D, T = y.shape
        if noise is not None:
            noise = _dev32(noise, self.device)
            assert tuple(noise.shape) == (N, B, self.n_src, D, T), noise.shape
        x = torch.empty((B, self.n_src, D, T), device=self.device, dtype=torch.float32)
        self._check(self.lib.dsn_sb_sample(self.ctx, _ptr(y), _ptr(noise), seed, _ptr(x), B, T, N, float(k), float(c),
                                           float(sb_eps), float(t_eps), SB_TYPES[sampler_type], self._stream()),
                    "dsn_sb_sample")
        return x

    def ode_sample(self, y, noise=None, *, method="RK45", rtol=1e-5, atol=1e-5, t_eps=0.03, denoise=True, N=30,
                   first_step=None, max_step=math.inf, max_attempts=1000, seed=0, return_stats=False):
        """Probability-flow ODE sampler (reference get_ode_sampler) on the latent state: y [B,1,D,T] ->
        (x [B,n,D,T], nfev) with scipy solve_ivp's RK45 / RK23 step control on the device.  noise: the prior's
        standard normals [B,n,D,T] (or [1,B,n,D,T], draw 0 of pc_sample's layout), else the device RNG (`seed`).
        A step size underflow or more than `max_attempts` step attempts raise RuntimeError.  return_stats: also
        return {nfev, n_accepted, n_rejected, t_final, status}."""
        if method not in ODE_METHODS:
            raise NotImplementedError(f"no native ODE solver {method!r}; implemented: {sorted(ODE_METHODS)}")
        y = _dev32(y, self.device)
        B, _, D, T = y.shape
        if noise is not None:
            noise = _dev32(noise, self.device)
            if noise.dim() == 5 and noise.shape[0] == 1:
                noise = noise[0].contiguous()
            assert tuple(noise.shape) == (B, self.n_src, D, T), noise.shape
        x = torch.empty((B, self.n_src, D, T), device=self.device, dtype=torch.float32)
        o = DsnOdeOpts(ODE_METHODS[method], float(rtol), float(atol), float(t_eps), int(bool(denoise)), int(N),
                       0.0 if first_step is None else float(first_step),
                       0.0 if max_step is None or math.isinf(max_step) else float(max_step), int(max_attempts))
        st = DsnOdeStats()
        rc = self.lib.dsn_ode_sample(self.ctx, _ptr(y), _ptr(noise), seed, _ptr(x), B, T, C.byref(o), C.byref(st),
                                     self._stream())
        self._check(rc, "dsn_ode_sample")
        if return_stats:
            return x, st.nfev, {"nfev": st.nfev, "n_accepted": st.n_accepted, "n_rejected": st.n_rejected,
                                "t_final": st.t_final, "status": ODE_STATUS.get(st.status, st.status)}
        return x, st.nfev

    def score_loss(self, y, x0, *, mode="dsm", reduction="none", t_eps=0.03, time=None, noise=None, perm=None, seed=0,
                   loss=True, return_aux=False, frames=None):
        """Denoising score-matching loss with one score call (dsn_score_loss; reference sample_prior +
        compute_score_loss, or compute_score_loss_init_hack_pit for mode="init_pit").  y [B,1,D,T], x0 [B,n,D,T] ->
        loss [B,n] (reduction="none") or a scalar tensor ("mean"), float32 on the device.  time [B] in (0, 1], noise
        [B,n,D,T] and perm [B,n] (slot s of item b holds source perm[b,s]) are injected when given; otherwise t and z
        come from the device RNG for `seed`.  loss=False: the perturbation only, no score call (loss is None).
        return_aux=True: (loss, {"x_t", "t", "sigma" [B], "z"}).
        frames (B ints, optional; DiT only): a ragged batch padded to T frames, item b valid over [..., :frames[b]]
        (dsn_score_loss_ragged).  x_t there is bit for bit the dense value and zero past the item's end; x0 and noise
        are not read in the padding (y's padding goes to the score call and must be finite); loss[b, s] is the mean
        over the item's own D * frames[b] elements, and reduction="mean" the mean of the B * n row means -- a
        definition, equal to MSELoss() for equal lengths.  With the device RNG the normals are indexed by position in
        the padded tensor: a valid draw, not the one the item alone would make for that seed.  The aux tensors keep
        the padded shape."""
        if mode not in LOSS_MODES or reduction not in LOSS_REDUCTIONS:
            raise ValueError(f"mode must be one of {sorted(LOSS_MODES)} and reduction one of {sorted(LOSS_REDUCTIONS)}")
        y, x0 = _dev32(y, self.device), _dev32(x0, self.device)
        if y.dim() != 4 or x0.dim() != 4 or y.shape[1] != 1:
            raise ValueError(f"y must be [B,1,D,T] and x0 [B,n,D,T] (got {tuple(y.shape)} and {tuple(x0.shape)})")
        B, _, D, T = y.shape
        if tuple(x0.shape) != (B, self.n_src, D, T) or D != self.latent_dim:
            raise ValueError(f"x0 must be [{B},{self.n_src},{self.latent_dim},{T}], got {tuple(x0.shape)}")
        if frames is not None:
            frames = check_ragged(self.cfg.score_kind, frames, B, T)
        if time is not None:
            time = _dev32(torch.as_tensor(time), self.device).reshape(-1)
            if time.numel() != B:
                raise ValueError(f"time must hold B = {B} values")
        if noise is not None:
            noise = _dev32(noise, self.device)
            if tuple(noise.shape) != tuple(x0.shape):
                raise ValueError(f"noise must be {tuple(x0.shape)}, got {tuple(noise.shape)}")
        if perm is not None:
            perm = torch.as_tensor(perm).to(device=self.device, dtype=torch.int32).contiguous()
            if tuple(perm.shape) != (B, self.n_src):
                raise ValueError(f"perm must be [{B},{self.n_src}], got {tuple(perm.shape)}")
        out = None
        if loss:
            out = torch.empty((B, self.n_src) if reduction == "none" else (1,), device=self.device, dtype=torch.float32)
        aux = {}
        if return_aux:
            aux = {"x_t": torch.empty_like(x0), "t": torch.empty(B, device=self.device, dtype=torch.float32),
                   "sigma": torch.empty(B, device=self.device, dtype=torch.float32), "z": torch.empty_like(x0)}
        o = DsnLossOpts(LOSS_MODES[mode], LOSS_REDUCTIONS[reduction], float(t_eps))
        tail = (_ptr(time), _ptr(noise), _ptr(perm), int(seed), _ptr(out), _ptr(aux.get("x_t")), _ptr(aux.get("t")),
                _ptr(aux.get("sigma")), _ptr(aux.get("z")), B, T, C.byref(o), self._stream())
        if frames is None:
            self._check(self.lib.dsn_score_loss(self.ctx, _ptr(y), _ptr(x0), *tail), "dsn_score_loss")
        else:
            self._check(self.lib.dsn_score_loss_ragged(self.ctx, _ptr(y), _ptr(x0), (C.c_int32 * B)(*frames), *tail),
                        "dsn_score_loss_ragged")
        if out is not None and reduction == "mean":
            out = out.reshape(())
        return (out, aux) if return_aux else out

    def decode(self, est, target_len: Optional[int] = None, chunked: bool = False, overlap: int = 32,
               chunk_size: int = 128):
        """chunked / overlap / chunk_size: AudioAutoencoder.decode_audio's long-form mode (latent frames)."""
        est = _dev32(est, self.device)
        B, n, D, T = est.shape
        if n != self.n_src or D != self.latent_dim:
            raise ValueError(f"est must be [B,{self.n_src},{self.latent_dim},T], got {tuple(est.shape)}")
        L = target_len if target_len else self.hop_length * T
        wav = torch.empty((B, n, L), device=self.device, dtype=torch.float32)
        if chunked:
            self._check(self.lib.dsn_decode_chunked(self.ctx, _ptr(est), _ptr(wav), B, T, L, int(chunk_size),
                                                    int(overlap), self._stream()), "dsn_decode_chunked")
        else:
            self._check(self.lib.dsn_decode(self.ctx, _ptr(est), _ptr(wav), B, T, L, self._stream()), "dsn_decode")
        return wav

    def encode(self, mix, vae_noise=None, seed=0, chunked: bool = False, overlap: int = 32, chunk_size: int = 128):
        mix = _dev32(mix, self.device)
        B, _, L = mix.shape
        T = self.latent_frames(L)
        if vae_noise is not None:
            vae_noise = _dev32(vae_noise, self.device)
            assert tuple(vae_noise.shape) == (B, self.latent_dim, T)
        y = torch.empty((B, 1, self.latent_dim, T), device=self.device, dtype=torch.float32)
        if chunked:
            self._check(self.lib.dsn_encode_chunked(self.ctx, _ptr(mix), _ptr(vae_noise), seed, _ptr(y), B, L,
                                                    int(chunk_size), int(overlap), self._stream()),
                        "dsn_encode_chunked")
        else:
            self._check(self.lib.dsn_encode(self.ctx, _ptr(mix), _ptr(vae_noise), seed, _ptr(y), B, L,
                                            self._stream()), "dsn_encode")
        return y

    def separate(self, mix, *, vae_noise=None, noise=None, seed=0, target_len=None, N=30, corrector_steps=1,
                 snr=0.5, t_eps=0.03, denoise=True):
        mix = _dev32(mix, self.device)
        B, _, L = mix.shape
        Lt = target_len if target_len else L
        wav = torch.empty((B, self.n_src, Lt), device=self.device, dtype=torch.float32)
        nfe = C.c_int()
        vn = None if vae_noise is None else _dev32(vae_noise, self.device)
        nz = None if noise is None else _dev32(noise, self.device)
        self._check(self.lib.dsn_separate(self.ctx, _ptr(mix), _ptr(vn), _ptr(nz), seed, _ptr(wav), B, L, Lt, N,
                                          corrector_steps, snr, t_eps, int(denoise), C.byref(nfe),
                                          self._stream()), "dsn_separate")
        return wav, nfe.value

    # ------------------------------------------------------------------ ragged batches
    def _padded_mixes(self, mixes, vae_noise):
        """-> (mix [B,1,hop*Tmax] zero past each item, vae noise [B,D,Tmax] or None, frames, lengths)"""
        hop = self.hop_length
        lens = [int(m.shape[-1]) for m in mixes]
        frames = [latent_frames_of(L, hop) for L in lens]
        B, Tmax = len(mixes), max(frames)
        mix = torch.zeros((B, 1, hop * Tmax), device=self.device, dtype=torch.float32)
        for b, m in enumerate(mixes):
            mix[b, 0, :lens[b]] = _dev32(m, self.device).reshape(-1)
        vn = None
        if vae_noise is not None:
            vn = torch.zeros((B, self.latent_dim, Tmax), device=self.device, dtype=torch.float32)
            for b, v in enumerate(vae_noise):
                if tuple(v.shape) != (self.latent_dim, frames[b]):
                    raise ValueError(f"vae_noise[{b}] must be {(self.latent_dim, frames[b])}, got {tuple(v.shape)}")
                vn[b, :, :frames[b]] = _dev32(v, self.device)
        return mix, vn, frames, lens

    def encode_ragged(self, mixes, vae_noise=None, seed=0, codec="grouped"):
        """mixes: list of [1, L_b] mixtures of different lengths -> (y [B,1,D,Tmax] zero beyond each item's frames,
        frames), T_b = latent_frames(L_b).  vae_noise: list of [D, T_b] (not extended with the samples).
        codec="grouped" (default): items are grouped by T_b; each item of a group is zero-extended to T_b * hop - 1
        samples (ragged_extended_length) and the group is encoded by one `encode` call, which is what each item gets
        alone; without vae_noise group g draws with seed + g.
        codec="padded": every item is zero-extended to Tmax * hop samples and the batch is encoded in one pass
        (dsn_encode_ragged): the same result per item up to summation order; without vae_noise the draws are indexed by
        position in the padded tensor -- a valid sample, but not the one the grouped mode draws for that seed."""
        if check_codec_mode(codec) == "padded":
            mix, vn, frames, _ = self._padded_mixes(mixes, vae_noise)
            B, Tmax = len(frames), max(frames)
            y = torch.empty((B, 1, self.latent_dim, Tmax), device=self.device, dtype=torch.float32)
            self._check(self.lib.dsn_encode_ragged(self.ctx, _ptr(mix), (C.c_int32 * B)(*frames), _ptr(vn), seed,
                                                   _ptr(y), B, Tmax, self._stream()), "dsn_encode_ragged")
            return y, frames
        hop = self.hop_length
        lens = [int(m.shape[-1]) for m in mixes]
        frames = [latent_frames_of(L, hop) for L in lens]
        B, Tmax = len(mixes), max(frames)
        y = torch.zeros((B, 1, self.latent_dim, Tmax), device=self.device, dtype=torch.float32)
        for g, (Tb, idx) in enumerate(frame_groups(frames).items()):
            Lx = ragged_extended_length(lens[idx[0]], hop)
            grp = torch.zeros((len(idx), 1, Lx), device=self.device, dtype=torch.float32)
            for j, i in enumerate(idx):
                grp[j, 0, :lens[i]] = _dev32(mixes[i], self.device).reshape(-1)
            vn = None if vae_noise is None else torch.stack([_dev32(vae_noise[i], self.device) for i in idx])
            y[idx, :, :, :Tb] = self.encode(grp, vn, seed=seed + g)
        return y, frames

    def decode_ragged(self, x, frames, target_lens, codec="grouped"):
        """x [B,n,D,Tmax], frames and target_lens per item -> list of [n, L_b], each item cropped to its length.
        codec="grouped" (default): one `decode` per group of equal frame count on x[group][..., :T_b].
        codec="padded": one pass over the padded batch (dsn_decode_ragged); x's padded region may hold anything
        finite."""
        if check_codec_mode(codec) == "padded":
            B, n, D, T = x.shape
            if n != self.n_src or D != self.latent_dim:
                raise ValueError(f"x must be [B,{self.n_src},{self.latent_dim},T], got {tuple(x.shape)}")
            fr = check_ragged(self.cfg.score_kind, frames, B, T, need_dit=False)
            x = _dev32(x, self.device)
            wav = torch.empty((B, n, self.hop_length * T), device=self.device, dtype=torch.float32)
            self._check(self.lib.dsn_decode_ragged(self.ctx, _ptr(x), (C.c_int32 * B)(*fr), _ptr(wav), B, T,
                                                   self._stream()), "dsn_decode_ragged")
            return [wav[b, :, :int(target_lens[b])] for b in range(B)]
        x = _dev32(x, self.device)
        out = [None] * x.shape[0]
        for Tb, idx in frame_groups(frames).items():
            wav = self.decode(x[idx][..., :Tb].contiguous(), None)
            for j, i in enumerate(idx):
                out[i] = wav[j, :, :int(target_lens[i])]
        return out

    def separate_ragged(self, mixes, *, vae_noise=None, noise=None, seed=0, N=30, corrector_steps=1, snr=0.5,
                        t_eps=0.03, denoise=True, codec="grouped"):
        """Mixtures of different lengths in one batch: list of [1, L_b] -> (list of [n, L_b], nfe).  The sampler runs
        once on the padded batch (pc_sample with frames).  noise [draws,B,n,D,Tmax]: item b consumes
        noise[..., :frames[b]].  codec="grouped" (default): the codec runs per group of equal frame count.
        codec="padded": encoder, sampler and decoder each run once on the padded batch, in one library call
        (dsn_separate_ragged); with the device RNG the encoder draws with `seed` and the sampler with seed + 1, as
        dsn_separate does."""
        # (refused before anything is encoded)
        check_codec_mode(codec)
        check_ragged(self.cfg.score_kind, [1] * len(mixes), len(mixes), 1)
        if codec == "padded":
            mix, vn, frames, lens = self._padded_mixes(mixes, vae_noise)
            B, Tmax = len(frames), max(frames)
            nz = None if noise is None else _dev32(noise, self.device)
            draws = 1 + N * (corrector_steps + 1)
            if nz is not None and tuple(nz.shape) != (draws, B, self.n_src, self.latent_dim, Tmax):
                raise ValueError(f"noise must be {(draws, B, self.n_src, self.latent_dim, Tmax)}, got {tuple(nz.shape)}")
            wav = torch.empty((B, self.n_src, self.hop_length * Tmax), device=self.device, dtype=torch.float32)
            o = DsnSamplerOpts(PREDICTORS["reverse_diffusion"], CORRECTORS["ald"], int(corrector_steps), float(snr),
                               float(t_eps), int(denoise), None, None, None)
            nfe = C.c_int()
            self._check(self.lib.dsn_separate_ragged(self.ctx, _ptr(mix), (C.c_int32 * B)(*frames), _ptr(vn), _ptr(nz),
                                                     seed, _ptr(wav), B, Tmax, N, C.byref(o), C.byref(nfe),
                                                     self._stream()), "dsn_separate_ragged")
            return [wav[b, :, :lens[b]] for b in range(B)], nfe.value
        y, frames = self.encode_ragged(mixes, vae_noise, seed=seed)
        x, nfe = self.pc_sample(y, noise, N=N, corrector_steps=corrector_steps, snr=snr, t_eps=t_eps, denoise=denoise,
                                seed=seed, frames=frames)
        return self.decode_ragged(x, frames, [int(m.shape[-1]) for m in mixes]), nfe

    # ------------------------------------------------------------------ long recordings as batched windows
    def _stitch(self, chunks, L, overlap, fade, align, host):
        if fade not in FADES:
            raise ValueError(f"fade must be one of {sorted(FADES)} (got {fade!r})")
        chunks = _dev32(chunks, self.device)
        if chunks.dim() != 3:
            raise ValueError(f"chunks must be [W, n, Lw] (got {tuple(chunks.shape)})")
        W, n, Lw = chunks.shape
        out = torch.empty((n, int(L)), device=self.device, dtype=torch.float32)
        perms = torch.zeros((W, n), dtype=torch.int32) if host else None
        gram = torch.zeros((max(W - 1, 0), n, n), dtype=torch.float64) if host else None
        self._check(self.lib.dsn_window_stitch(
            self.ctx, _ptr(chunks), W, n, Lw, int(overlap), int(L), FADES[fade], int(bool(align)), _ptr(out),
            None if perms is None else C.cast(C.c_void_p(perms.data_ptr()), C.POINTER(C.c_int32)),
            None if gram is None else C.cast(C.c_void_p(gram.data_ptr()), C.POINTER(C.c_double)),
            self._stream()), "dsn_window_stitch")
        return out, (None if perms is None else perms.long()), gram

    def window_stitch(self, chunks, L, overlap, fade="hann", align=True):
        """The separated windows of one recording back into the recording (dsn_window_stitch): chunks [W,n,Lw], window w
        covering samples [w hop, w hop + Lw) with hop = Lw - overlap (window_plan) -> (out [n,L] on the device, perms
        [W,n] long, gram [W-1,n,n] float64, both on the host).  Slot i of `out` is slot perms[w,i] of window w: the
        order of window 0, carried from window to window by the assignment that maximises the overlap inner products
        gram[w,i,j] = <chunks[w,i,hop:], chunks[w+1,j,:overlap]> (ties go to the identity); overlaps are cross-faded
        with fade_table(overlap, fade), everything else is copied bit for bit.  align=False: no reordering -- perms is
        the identity and gram, which is not computed, is returned as zeros.  Needs no score network and no codec."""
        return self._stitch(chunks, L, overlap, fade, align, True)

    def _stitch_plans(self, sep, plans, overlap, fade, align, return_info):
        """sep [Wtot,n,window] in plan order, plans [(W, hop, L)] -> list of [n,L] (and the info dict of separate_long)"""
        outs, info, o = [], {"perms": [], "gram": [], "W": [], "hop": [], "chunks": sep}, 0
        for W, hop, L in plans:
            out, perms, gram = self._stitch(sep[o:o + W], L, overlap, fade, align, return_info)
            outs.append(out)
            for k, v in (("perms", perms), ("gram", gram), ("W", W), ("hop", hop)):
                info[k].append(v)
            o += W
        return outs, info

    def separate_long(self, mixes, *, window, overlap=None, fade="hann", align=True, batch=64, vae_noise=None,
                      noise=None, seed=0, N=30, corrector_steps=1, snr=0.5, t_eps=0.03, denoise=True,
                      return_info=False, mode="stitch"):
        """Long recordings as batched windows: `mixes` is one [1, L] tensor or a list of [1, L_r] tensors of any
        lengths -> (estimates [n, L] -- a list of [n, L_r] for a list --, the summed nfe).  Every recording is cut into
        windows of `window` samples sharing `overlap` (default window // 4) with their neighbour (window_plan; the last
        one zero-extended); the windows of all recordings are pooled in order into one [Wtot, 1, window] batch, which
        `separate` takes `batch` windows at a time (with the device RNG minibatch m draws with seed + m, the convention
        of LatentDiffSep.get_pc_sampler(minibatch=...)); each recording's windows are then put back together on the
        device by one window_stitch call.  Explicit vae_noise [Wtot, D, Tw] and noise [draws, Wtot, n, D, Tw] are
        sliced per minibatch.  return_info=True: also a dict with, per recording, the lists "perms", "gram", "W" and
        "hop", and "chunks", the separated windows [Wtot, n, window].
        The windows are sampled independently: the stitch orders and blends them, it does not make the diffusion
        samples of neighbouring windows agree.
        mode="score": every recording is ONE latent and one diffusion sample; only the score call is windowed
        (dsn_separate_windowed: one padded encoder pass, the sampler with the window-blended score of `score`, one padded
        decoder pass).  `window` and `overlap` are still in samples and must be multiples of the hop length; `batch`
        caps the windows per DiT call; `align` does not apply (there is no permutation to repair).  vae_noise: list of
        [D, T_r] (encode_ragged's), noise [draws, R, n, D, Tmax]; with the device RNG the encoder draws with `seed`, the
        sampler with seed + 1.  nfe = N (corrector_steps + 1), shared by all windows.  return_info: {"W", "windows",
        "frames", "Tw", "To"} of score_window_plan.  The blended score is a definition, not the score of any trained
        model; its separation quality against the other routes is unmeasured."""
        if mode not in LONG_MODES:
            raise ValueError(f"mode must be one of {LONG_MODES} (got {mode!r})")
        if int(batch) < 1:
            raise ValueError(f"batch = {batch} < 1")
        if mode == "score":
            return self._separate_long_score(mixes, window, overlap, fade, batch, vae_noise, noise, seed, N,
                                             corrector_steps, snr, t_eps, denoise, return_info)
        single = torch.is_tensor(mixes)
        pool, plans, overlap = cut_windows([mixes] if single else list(mixes), window, overlap, self.device)
        Wtot = pool.shape[0]
        sep = torch.empty((Wtot, self.n_src, int(window)), device=self.device, dtype=torch.float32)
        nfe = 0
        for m, lo in enumerate(range(0, Wtot, int(batch))):
            sl = slice(lo, lo + int(batch))
            wav, k = self.separate(pool[sl], vae_noise=None if vae_noise is None else vae_noise[sl],
                                   noise=None if noise is None else noise[:, sl], seed=seed + m, N=N,
                                   corrector_steps=corrector_steps, snr=snr, t_eps=t_eps, denoise=denoise)
            sep[sl] = wav
            nfe += k
        outs, info = self._stitch_plans(sep, plans, overlap, fade, align, return_info)
        res = (outs[0] if single else outs, nfe)
        return (*res, info) if return_info else res

    def _separate_long_score(self, mixes, window, overlap, fade, batch, vae_noise, noise, seed, N, corrector_steps, snr,
                             t_eps, denoise, return_info):
        hop = self.hop_length
        window = int(window)
        overlap = window // 4 if overlap is None else int(overlap)
        if window % hop or overlap % hop:
            raise ValueError(f"mode='score' windows the latent: window = {window} and overlap = {overlap} must be "
                             f"multiples of the hop length {hop}")
        if fade not in FADES:
            raise ValueError(f"fade must be one of {sorted(FADES)} (got {fade!r})")
        single = torch.is_tensor(mixes)
        mixes = [mixes] if single else list(mixes)
        for r, m in enumerate(mixes):
            if m.dim() != 2 or m.shape[0] != 1:
                raise ValueError(f"recording {r} must be [1, L] (got {tuple(m.shape)})")
        R = len(mixes)
        frames = [latent_frames_of(int(m.shape[-1]), hop) for m in mixes]
        Tmax = max(frames)
        fr, Tw, To = check_windowed(self.cfg.score_kind, frames, R, Tmax, (window // hop, overlap // hop))
        if vae_noise is not None and torch.is_tensor(vae_noise):
            vae_noise = [vae_noise[r, :, :frames[r]] for r in range(R)]
        mix, vn, _, lens = self._padded_mixes(mixes, vae_noise)
        nz = None if noise is None else _dev32(noise, self.device)
        draws = 1 + N * (corrector_steps + 1)
        if nz is not None and tuple(nz.shape) != (draws, R, self.n_src, self.latent_dim, Tmax):
            raise ValueError(f"noise must be {(draws, R, self.n_src, self.latent_dim, Tmax)}, got {tuple(nz.shape)}")
        wav = torch.empty((R, self.n_src, hop * Tmax), device=self.device, dtype=torch.float32)
        o = DsnSamplerOpts(PREDICTORS["reverse_diffusion"], CORRECTORS["ald"], int(corrector_steps), float(snr),
                           float(t_eps), int(denoise), None, None, None)
        nfe = C.c_int()
        self._check(self.lib.dsn_separate_windowed(self.ctx, _ptr(mix), (C.c_int32 * R)(*fr), _ptr(vn), _ptr(nz), seed,
                                                   _ptr(wav), R, Tmax, N, Tw, To, FADES[fade], int(batch), C.byref(o),
                                                   C.byref(nfe), self._stream()), "dsn_separate_windowed")
        outs = [wav[r, :, :lens[r]] for r in range(R)]
        res = (outs[0] if single else outs, nfe.value)
        if not return_info:
            return res
        plan = score_window_plan(fr, Tw, To, fade)
        return (*res, {"W": plan["W"], "windows": plan["windows"], "frames": fr, "Tw": Tw, "To": To})

    # ------------------------------------------------------------------ any sample rate
    def resample(self, x, fs_in: int, fs_out: int, lens=None, downmix: bool = False):
        """Sinc resampling on the device (dsn_resample; the filter of resample_plan, torchaudio.transforms.Resample's
        default): x [L], [C, L] or [B, C, L] at fs_in -> the same layout at fs_out with resample_length(L) samples.
        downmix: the channels are averaged first (in fp32, before the filter) and one channel comes back.
        lens (one sample count per item, shared by its channels): a ragged batch padded to L -- item b gets
        resample_length(lens[b]) samples, the rest of its rows is zero, and x at or past lens[b] is never read (it may
        hold NaN); the result is then (out, out_lens).  fs_in == fs_out is a copy.  Needs no score network and no
        codec; two calls give identical bits."""
        fs_in, fs_out, (B, Cn, L), ln = check_resample(fs_in, fs_out, tuple(x.shape), lens)
        nd = x.dim()
        x = _dev32(x, self.device).reshape(B, Cn, L)
        Lout = resample_length(fs_in, fs_out, L)
        Co = 1 if downmix else Cn
        out = torch.empty((B, Co, Lout), device=self.device, dtype=torch.float32)
        self._check(self.lib.dsn_resample(self.ctx, _ptr(x), B, Cn, L, None if ln is None else (C.c_int32 * B)(*ln),
                                          fs_in, fs_out, int(bool(downmix)), _ptr(out), Lout, self._stream()),
                    "dsn_resample")
        out = out.reshape((Lout,) if nd == 1 else (Co, Lout) if nd == 2 else (B, Co, Lout))
        return out if ln is None else (out, [resample_length(fs_in, fs_out, v) for v in ln])

    def _pad_items(self, mix, est=None):
        """The list form of mask_refine, stems, beamform and dereverb as one padded batch: mix a list of [C_b, L_b],
        est a list of as many [n, L_b] or None -> (mix [B, C, L], est [B, n, L] or None, lens, channels, cut), zero
        past an item's end and in the channels it does not have.  cut(res, ch_dim=None): the call's result (out, or
        (out, info)) with out as a list of the items' own samples and, ch_dim being the axis of an item's out that
        holds its channels, own channels."""
        ln, ch = [int(m.shape[-1]) for m in mix], [int(m.shape[0]) for m in mix]
        mp = torch.zeros((len(mix), max(ch), max(ln)), device=self.device, dtype=torch.float32)
        ep = None if est is None else torch.zeros((len(mix), int(est[0].shape[0]), max(ln)), device=self.device,
                                                  dtype=torch.float32)
        for b, m in enumerate(mix):
            mp[b, :ch[b], :ln[b]] = _dev32(m, self.device)
            if est is not None:
                ep[b, :, :ln[b]] = _dev32(est[b], self.device)

        def cut(res, ch_dim=None):
            out, info = res if isinstance(res, tuple) else (res, None)
            outs = [out[b, ..., :ln[b]] for b in range(len(mix))]
            if ch_dim is not None:
                outs = [o.narrow(ch_dim, 0, ch[b]) for b, o in enumerate(outs)]
            return outs if info is None else (outs, info)

        return mp, ep, ln, ch, cut

    # ------------------------------------------------------------------ mixture-consistent masks
    def mask_refine(self, mix, est, lens=None, n_fft=512, hop=128, power=2, eps=1e-10):
        """Mixture-consistent STFT masks on the device (dsn_mask_refine, csrc/maskrefine.hip; the definition is in
        include/ditsep_hip.h and tests/mask_refine_restatement.py): soft masks M_i = (|S_i|^power + eps) /
        (sum_j |S_j|^power + n eps) from the estimates' STFTs (periodic Hann of n_fft samples every hop), applied to
        the mixture's STFT and transformed back.  mix [B, L] or [B, 1, L], est [B, n, L] -> [B, n, L]: every output
        has the mixture's phase and the outputs sum to the mixture up to float32 rounding.  lens (one sample count per
        item): a ragged batch padded to L -- nothing at or past lens[b] is read (it may hold NaN), the result is zero
        there and each item gets the bits it gets alone.  Lists (mix: [1, L_b] or [L_b] each, est: [n, L_b] each) are
        padded once and a list of [n, L_b] comes back.  Not a trained step: what it does to separation quality is
        unmeasured.  Needs no score network and no codec; two calls give identical bits."""
        if isinstance(mix, (list, tuple)):
            if lens is not None or not isinstance(est, (list, tuple)) or len(est) != len(mix):
                raise ValueError("mask_refine: a list of mixtures goes with a list of as many estimates and no lens")
            ln = [int(e.shape[-1]) for e in est]
            for b, (m, e) in enumerate(zip(mix, est)):
                if e.dim() != 2 or m.numel() != ln[b] or m.dim() not in (1, 2):
                    raise ValueError(f"mask_refine: item {b} must be mix [1, L] and est [n, L] (got {tuple(m.shape)} "
                                     f"and {tuple(e.shape)})")
            mp, ep, ln, _, cut = self._pad_items([m.reshape(1, -1) for m in mix], est)
            return cut(self.mask_refine(mp, ep, lens=ln, n_fft=n_fft, hop=hop, power=power, eps=eps))
        (B, n, L), ln, n_fft, hop, power, eps = check_mask_refine(tuple(mix.shape), tuple(est.shape), lens, n_fft, hop,
                                                                  power, eps)
        mix = _dev32(mix, self.device).reshape(B, L)
        est = _dev32(est, self.device)
        out = torch.empty((B, n, L), device=self.device, dtype=torch.float32)
        self._check(self.lib.dsn_mask_refine(self.ctx, _ptr(mix), _ptr(est), B, n, L, _i32(ln), n_fft, hop, power, eps,
                                             _ptr(out), self._stream()), "dsn_mask_refine")
        return out

    # ------------------------------------------------------------------ multichannel stems from mono estimates
    def stems(self, mix, est, lens=None, channels=None, mode="wiener", n_fft=512, hop=128, power=2, eps=1e-10,
              reg=1e-3, return_info=False):
        """The mixture's channels filtered with the mono estimates (dsn_stems, csrc/maskrefine.hip; the definition is
        in include/ditsep_hip.h and tests/stems_restatement.py): mix [B, C, L], est [B, n, L] -> [B, n, C, L], every
        source with the mixture's channels.  mode "mask": the masks of `mask_refine` on every channel (C <= 8; bit for
        bit mask_refine of that channel).  mode "wiener": one expectation-maximisation pass of the multichannel Wiener
        filter (C <= 2) -- a spatial covariance per source and bin from the mixture, the per-bin solve in float64,
        lambda = reg tr(Sigma) / C + eps on the diagonal and its remainder handed out equally, so the stems of a
        channel sum to that channel up to float32 rounding.  lens / channels (one per item): a ragged batch padded to
        L and C -- nothing past an item's end or in a channel it does not have is read (it may hold NaN), the result
        is zero there and each item gets the bits it gets alone.  Lists (mix: [C_b, L_b] each, est: [n, L_b] each) are
        padded once and a list of [n, C_b, L_b] comes back.  return_info=True: (out, {"R": complex128 [B, n, bins, C,
        C], "den": float64 [B, n, bins]}) on the host, the spatial covariances and their denominators (zeros in mask
        mode).  Not a trained step: what it does to separation quality is unmeasured.  Needs no score network and no
        codec; two calls give identical bits."""
        if isinstance(mix, (list, tuple)):
            if lens is not None or channels is not None or not isinstance(est, (list, tuple)) or len(est) != len(mix):
                raise ValueError("stems: a list of mixtures goes with a list of as many estimates and no lens or "
                                 "channels")
            ln = [int(e.shape[-1]) for e in est]
            for b, (m, e) in enumerate(zip(mix, est)):
                if e.dim() != 2 or m.dim() != 2 or int(m.shape[-1]) != ln[b]:
                    raise ValueError(f"stems: item {b} must be mix [C, L] and est [n, L] (got {tuple(m.shape)} and "
                                     f"{tuple(e.shape)})")
            mp, ep, ln, ch, cut = self._pad_items(mix, est)
            return cut(self.stems(mp, ep, lens=ln, channels=ch, mode=mode, n_fft=n_fft, hop=hop, power=power, eps=eps,
                                  reg=reg, return_info=return_info), ch_dim=1)
        (B, Cn, n, L), ln, ch, code, n_fft, hop, power, eps, reg = check_stems(
            tuple(mix.shape), tuple(est.shape), lens, channels, mode, n_fft, hop, power, eps, reg)
        mix, est = _dev32(mix, self.device), _dev32(est, self.device)
        out = torch.empty((B, n, Cn, L), device=self.device, dtype=torch.float32)
        bins = n_fft // 2 + 1
        R = torch.zeros((B, n, bins, Cn, Cn), dtype=torch.complex128) if return_info else None
        den = torch.zeros((B, n, bins), dtype=torch.float64) if return_info else None
        self._check(self.lib.dsn_stems(self.ctx, _ptr(mix), _ptr(est), B, Cn, n, L, _i32(ln), _i32(ch), code, n_fft, hop,
                                       power, eps, reg, _ptr(out), _host(R), _host(den), self._stream()), "dsn_stems")
        return (out, {"R": R, "den": den}) if return_info else out

    # ------------------------------------------------------------------ mask-based MVDR beamforming
    def beamform(self, mix, est, lens=None, channels=None, ref=0, n_fft=512, hop=128, power=2, eps=1e-10, reg=1e-3,
                 postfilter=None, workspace_budget=0, return_info=False, design=None):
        """A microphone-array recording beamformed towards every source the mono estimates describe (dsn_beamform,
        csrc/beamform.hip; the definition is in include/ditsep_hip.h and tests/beamform_restatement.py): mix
        [B, C, L] (C <= 8), est [B, n, L] -> [B, n, L], every source a linear time-invariant filter of the channels.
        The masks of `mask_refine` weight the mixture's own frames into one spatial covariance per source and bin; the
        MVDR filter (Souden et al.) w = Z[:, ref] / tr Z, Z = (Q + lambda I)^-1 N_i with Q the other sources'
        covariances and lambda = reg tr(Q) / C + eps, solved per bin in float64 by Cholesky, passes source i as it is
        at channel `ref` and suppresses the others.  postfilter "mask" multiplies the beamformed spectrum with the
        source's mask.  lens / channels (one per item): a ragged batch padded to L and C -- nothing past an item's
        end or in a channel it does not have is read (it may hold NaN), the result is zero past the end and each item
        gets the bits it gets alone, under any workspace_budget (bytes, 0 = 512 MiB: the items are processed in
        chunks).  Lists (mix: [C_b, L_b] each, est: [n, L_b] each) are padded once and a list of [n, L_b] comes back.
        return_info=True: (out, {"w": complex128 [B, n, bins, C]}) on the host.  One filter per recording
        (`beamform_track` follows moving sources); not a trained step: what it does to separation quality is unmeasured.  Needs no score
        network and no codec; two calls give identical bits.
        design (default None: the call above, to the bit): "rank1", "gev", "souden" or a dict of kind / sweeps
        (native.design_options) -- the weights of dsn_beamform_design (csrc/beamform_design.hip;
        tests/beamform_design_restatement.py): with A = Q + lambda I = L L^H the principal eigenpair of
        L^-1 N_i L^-H by `sweeps` Jacobi sweeps in float64 gives the steering estimate h = L u and v = L^-H u;
        "rank1" is the MVDR filter of the rank-one model, w = v conj(h_ref); "gev" the max-SNR filter with blind
        analytic normalisation, w = v (conj(h_ref) / |h_ref|) |h| / sqrt(C), which is not distortionless.  Not
        tuned; what either does to real recordings is unmeasured."""
        if isinstance(mix, (list, tuple)):
            if lens is not None or channels is not None or not isinstance(est, (list, tuple)) or len(est) != len(mix):
                raise ValueError("beamform: a list of mixtures goes with a list of as many estimates and no lens or "
                                 "channels")
            ln = [int(e.shape[-1]) for e in est]
            for b, (m, e) in enumerate(zip(mix, est)):
                if e.dim() != 2 or m.dim() != 2 or int(m.shape[-1]) != ln[b]:
                    raise ValueError(f"beamform: item {b} must be mix [C, L] and est [n, L] (got {tuple(m.shape)} and "
                                     f"{tuple(e.shape)})")
            mp, ep, ln, ch, cut = self._pad_items(mix, est)
            return cut(self.beamform(mp, ep, lens=ln, channels=ch, ref=ref, n_fft=n_fft, hop=hop, power=power, eps=eps,
                                     reg=reg, postfilter=postfilter, workspace_budget=workspace_budget,
                                     return_info=return_info, design=design))
        (B, Cn, n, L), ln, ch, ref, n_fft, hop, power, eps, reg, post, budget = check_beamform(
            tuple(mix.shape), tuple(est.shape), lens, channels, ref, n_fft, hop, power, eps, reg, postfilter,
            workspace_budget)
        des = check_design(design)
        mix, est = _dev32(mix, self.device), _dev32(est, self.device)
        out = torch.empty((B, n, L), device=self.device, dtype=torch.float32)
        w = torch.zeros((B, n, n_fft // 2 + 1, Cn), dtype=torch.complex128) if return_info else None
        head = (self.ctx, _ptr(mix), _ptr(est), B, Cn, n, L, _i32(ln), _i32(ch), ref, n_fft, hop, power, eps, reg)
        tail = (post, budget, _ptr(out), _host(w), self._stream())
        if des is None:
            self._check(self.lib.dsn_beamform(*head, *tail), "dsn_beamform")
        else:
            self._check(self.lib.dsn_beamform_design(*head, *des, *tail), "dsn_beamform_design")
        return (out, {"w": w}) if return_info else out

    def beamform_solve(self, N, n=None, channels=None, ref=0, reg=1e-3, eps=1e-10, design="rank1"):
        """The weights launch of the beamformers alone, on the caller's own covariances (dsn_beamform_solve): N
        [items, classes, C (C + 1), bins] float64 -- per class the upper triangle of a Hermitian C x C matrix row after
        row, per entry a plane of real parts, then one of imaginary parts -- -> w [items, n, bins, C] complex128 on
        the device.  n (default: classes) sources get a filter; with classes = n + 1 the last class is noise that only
        enters the interference.  channels (one per item): entries of channels an item does not have are not read
        and their weights are zero.  design as in `beamform` (None and "souden": Souden's filter)."""
        if not torch.is_tensor(N) or N.dim() != 4 or N.dtype != torch.float64:
            raise ValueError("beamform_solve: N must be a float64 tensor [items, classes, C (C + 1), bins]")
        items, classes, T2, bins = (int(v) for v in N.shape)
        Cn = int((math.isqrt(4 * T2 + 1) - 1) // 2)
        if Cn * (Cn + 1) != T2 or Cn < 1 or Cn > BEAMFORM_MAX_CHANNELS:
            raise ValueError(f"beamform_solve: N has {T2} planes per class, not C (C + 1) for a C in [1, "
                             f"{BEAMFORM_MAX_CHANNELS}]")
        n = classes if n is None else int(n)
        if n < 1 or n > MASK_REFINE_MAX_SRC or classes not in (n, n + 1):
            raise ValueError(f"beamform_solve: n = {n} outside [1, {MASK_REFINE_MAX_SRC}] or classes = {classes} is not "
                             "n or n + 1")
        if items < 1 or bins < 1 or bins > 1025:
            raise ValueError(f"beamform_solve: items = {items} < 1 or bins = {bins} outside [1, 1025]")
        ch = _check_channels("beamform_solve", channels, items, Cn)
        ref = _check_ref("beamform_solve", ref, ch, Cn)
        reg = _check_reg("beamform_solve", reg)
        eps = float(eps)
        if not math.isfinite(eps) or not eps > 0.0:
            raise ValueError(f"beamform_solve: eps = {eps} is not a finite positive number")
        des = check_design(design) or (BEAMFORM_DESIGNS["souden"], DESIGN_DEFAULTS["sweeps"])
        N = N.to(self.device).contiguous()
        w = torch.empty((items, n, bins, Cn), device=self.device, dtype=torch.complex128)
        self._check(self.lib.dsn_beamform_solve(self.ctx, _ptr(N), _i32(ch), ref, items, Cn, n, classes, bins, reg, eps,
                                                *des, _ptr(w), self._stream()), "dsn_beamform_solve")
        return w

    # ------------------------------------------------------------------ beamforming on spatially refined masks
    def beamform_spatial(self, mix, est, lens=None, channels=None, ref=0, n_fft=512, hop=128, power=2, eps=1e-10,
                         reg=1e-3, iterations=1, noise=0.1, floor=0.1, mask_reg=1e-3, mask_eps=1e-10, workspace_budget=0,
                         return_info=False, design=None):
        """`beamform` with the masks refined by where the sources sit (dsn_beamform_spatial, csrc/spatial.hip; the
        definition is in include/ditsep_hip.h and tests/spatial_restatement.py): mix [B, C, L] (C <= 8), est
        [B, n, L] -> [B, n, L].  Per bin a complex angular central Gaussian mixture model (Ito et al. 2016) is fitted
        to the normalised channel vectors z = X / |X| in float64, one class per source and, with noise > 0, one for
        the noise, with the estimates' masks as time-frequency priors a_k = (1 - noise) ((1 - floor) M_k + floor / n)
        (guided source separation: Nakatani et al. 2017, Drude & Haeb-Umbach 2017): `iterations` times the posteriors
        gamma from the classes' covariances B_k (by Cholesky) and the covariances from the posteriors, loaded with
        mask_reg tr(B_k) / C + mask_eps.  The posteriors replace the masks in the beamformer's statistics, the noise
        class enters every source's interference, and the weights and the filter are `beamform`'s (no post-filter).
        lens / channels / workspace_budget / lists as in `beamform` (items of native.spatial_item_bytes each); each
        item gets the bits it gets alone; an item with one channel skips the model.  return_info=True: (out, {"w":
        complex128 [B, n, bins, C], "gamma": float64 [B, K, bins, F] (K = n + 1 with noise > 0; zero in frames an item
        does not have), "fail": int32 [B, bins], 1 where a pivot failed and the bin fell back to its priors}) on the
        host.  Not trained and not tuned: what it does to separation quality is unmeasured.  Needs no score network
        and no codec; two calls give identical bits.  design (default None: the call above, to the bit) as in
        `beamform`: the weights of that design on the refined statistics (dsn_beamform_spatial_design)."""
        kw = dict(ref=ref, n_fft=n_fft, hop=hop, power=power, eps=eps, reg=reg, iterations=iterations, noise=noise,
                  floor=floor, mask_reg=mask_reg, mask_eps=mask_eps, workspace_budget=workspace_budget,
                  return_info=return_info, design=design)
        if isinstance(mix, (list, tuple)):
            if lens is not None or channels is not None or not isinstance(est, (list, tuple)) or len(est) != len(mix):
                raise ValueError("beamform_spatial: a list of mixtures goes with a list of as many estimates and no lens "
                                 "or channels")
            ln = [int(e.shape[-1]) for e in est]
            for b, (m, e) in enumerate(zip(mix, est)):
                if e.dim() != 2 or m.dim() != 2 or int(m.shape[-1]) != ln[b]:
                    raise ValueError(f"beamform_spatial: item {b} must be mix [C, L] and est [n, L] (got "
                                     f"{tuple(m.shape)} and {tuple(e.shape)})")
            mp, ep, ln, ch, cut = self._pad_items(mix, est)
            return cut(self.beamform_spatial(mp, ep, lens=ln, channels=ch, **kw))
        ((B, Cn, n, L), ln, ch, ref, n_fft, hop, power, eps, reg, iterations, noise, floor, mask_reg, mask_eps,
         budget) = check_spatial(tuple(mix.shape), tuple(est.shape), lens, channels, ref, n_fft, hop, power, eps, reg,
                                 iterations, noise, floor, mask_reg, mask_eps, workspace_budget)
        des = check_design(design)
        mix, est = _dev32(mix, self.device), _dev32(est, self.device)
        out = torch.empty((B, n, L), device=self.device, dtype=torch.float32)
        bins, K, Fs = n_fft // 2 + 1, n + (C.c_float(noise).value > 0), 1 + (L + hop - 1) // hop
        w = torch.zeros((B, n, bins, Cn), dtype=torch.complex128) if return_info else None
        gamma = torch.zeros((B, K, bins, Fs), dtype=torch.float64) if return_info else None
        bad = torch.zeros((B, bins), dtype=torch.int32) if return_info else None
        head = (self.ctx, _ptr(mix), _ptr(est), B, Cn, n, L, _i32(ln), _i32(ch), ref, n_fft, hop, power, eps, reg)
        tail = (iterations, noise, floor, mask_reg, mask_eps, budget, _ptr(out), _host(w), _host(gamma),
                _host(bad, C.c_int32), self._stream())
        if des is None:
            self._check(self.lib.dsn_beamform_spatial(*head, *tail), "dsn_beamform_spatial")
        else:
            self._check(self.lib.dsn_beamform_spatial_design(*head, *des, *tail), "dsn_beamform_spatial_design")
        return (out, {"w": w, "gamma": gamma, "fail": bad}) if return_info else out

    # ------------------------------------------------------------------ block-adaptive MVDR weights
    def beamform_track(self, mix, est, lens=None, channels=None, ref=0, n_fft=512, hop=128, power=2, eps=1e-10,
                       reg=1e-3, postfilter=None, block_frames=100, context=1, interpolate=True, workspace_budget=0,
                       return_info=False, design=None):
        """`beamform` with weights that follow a moving source (dsn_beamform_track, csrc/beamform_track.hip; the
        definition is in include/ditsep_hip.h and tests/beamform_track_restatement.py): mix [B, C, L] (C <= 8), est
        [B, n, L] -> [B, n, L].  The frames are cut into blocks of `block_frames`; block k gets the MVDR filter of
        `beamform` solved on the statistics of the blocks k - context .. k + context, and frame t is filtered with the
        weights interpolated between the centres of its two nearest blocks (interpolate=False: with its own block's).
        One block is `beamform` up to the order of its sums.  lens / channels / postfilter / workspace_budget / lists as
        in `beamform` (items of native.track_item_bytes each: the weights live in the workspace too); each item gets
        the bits it gets alone.  return_info=True: (out, {"w": complex128 [B, Kmax, n, bins, C]}) on the host, zero in
        blocks and channels an item does not have.  Blocks of fixed length, not speaker-activity segments; no
        recursive or online form; not trained and not tuned: what it does to separation quality on real recordings
        is unmeasured.  Needs no score network and no codec; two calls give identical bits.  design (default None: the
        call above, to the bit) as in `beamform`: every block's weights are that design's
        (dsn_beamform_track_design)."""
        kw = dict(ref=ref, n_fft=n_fft, hop=hop, power=power, eps=eps, reg=reg, postfilter=postfilter,
                  block_frames=block_frames, context=context, interpolate=interpolate, workspace_budget=workspace_budget,
                  return_info=return_info, design=design)
        if isinstance(mix, (list, tuple)):
            if lens is not None or channels is not None or not isinstance(est, (list, tuple)) or len(est) != len(mix):
                raise ValueError("beamform_track: a list of mixtures goes with a list of as many estimates and no lens "
                                 "or channels")
            ln = [int(e.shape[-1]) for e in est]
            for b, (m, e) in enumerate(zip(mix, est)):
                if e.dim() != 2 or m.dim() != 2 or int(m.shape[-1]) != ln[b]:
                    raise ValueError(f"beamform_track: item {b} must be mix [C, L] and est [n, L] (got "
                                     f"{tuple(m.shape)} and {tuple(e.shape)})")
            mp, ep, ln, ch, cut = self._pad_items(mix, est)
            return cut(self.beamform_track(mp, ep, lens=ln, channels=ch, **kw))
        ((B, Cn, n, L), ln, ch, ref, n_fft, hop, power, eps, reg, post, Tb, context, interp, kmax,
         budget) = check_track(tuple(mix.shape), tuple(est.shape), lens, channels, ref, n_fft, hop, power, eps, reg,
                               postfilter, block_frames, context, interpolate, workspace_budget)
        des = check_design(design)
        mix, est = _dev32(mix, self.device), _dev32(est, self.device)
        out = torch.empty((B, n, L), device=self.device, dtype=torch.float32)
        w = torch.zeros((B, kmax, n, n_fft // 2 + 1, Cn), dtype=torch.complex128) if return_info else None
        head = (self.ctx, _ptr(mix), _ptr(est), B, Cn, n, L, _i32(ln), _i32(ch), ref, n_fft, hop, power, eps, reg)
        tail = (post, Tb, context, interp, budget, _ptr(out), _host(w), self._stream())
        if des is None:
            self._check(self.lib.dsn_beamform_track(*head, *tail), "dsn_beamform_track")
        else:
            self._check(self.lib.dsn_beamform_track_design(*head, *des, *tail), "dsn_beamform_track_design")
        return (out, {"w": w}) if return_info else out

    # ------------------------------------------------------------------ WPE dereverberation
    def dereverb(self, mix, lens=None, channels=None, taps=10, delay=3, iterations=3, n_fft=512, hop=128, reg=1e-4,
                 eps=1e-10, workspace_budget=None, return_info=False):
        """The channels of a reverberant recording with their late reverberation removed (dsn_dereverb,
        csrc/dereverb.hip; the definition is in include/ditsep_hip.h and tests/dereverb_restatement.py): mix [B, C, L]
        (C <= 8) -> [B, C, L].  Weighted prediction error: per bin a filter G over `taps` frames of all channels,
        `delay` frames back, is estimated in float64 against the time-varying power lambda(t) of the current estimate
        (R = sum y~ y~^H / lambda, P = sum y~ Y^H / lambda, G = (R + delta I)^-1 P by Cholesky, delta = reg tr(R) /
        (C taps) + eps) and its prediction subtracted, `iterations` times; C taps <= 80.  Analysis and synthesis are
        mask_refine's.  lens / channels (one per item): a ragged batch padded to L and C -- nothing past an item's end
        or in a channel it does not have is read (it may hold NaN), the result is zero there and each item gets the
        bits it gets alone, under any workspace_budget (bytes, None or 0 = 512 MiB: the items are processed in chunks
        of native.dereverb_item_bytes each).  A list of [C_b, L_b] is padded once and a list of [C_b, L_b] comes back.
        return_info=True: (out, {"G": complex128 [B, bins, C taps, C], the last iteration's filter, "fail": int32 [B],
        the bins that passed through because a pivot failed}) on the host.  Offline, one filter per recording; not a
        trained step: what it does to separation quality is unmeasured.  Needs no score network and no codec; two
        calls give identical bits."""
        kw = dict(taps=taps, delay=delay, iterations=iterations, n_fft=n_fft, hop=hop, reg=reg, eps=eps,
                  workspace_budget=workspace_budget, return_info=return_info)
        if isinstance(mix, (list, tuple)):
            if lens is not None or channels is not None:
                raise ValueError("dereverb: a list of mixtures goes with no lens or channels")
            for b, m in enumerate(mix):
                if m.dim() != 2:
                    raise ValueError(f"dereverb: item {b} must be [C, L] (got {tuple(m.shape)})")
            mp, _, ln, ch, cut = self._pad_items(mix)
            return cut(self.dereverb(mp, lens=ln, channels=ch, **kw), ch_dim=0)
        (B, Cn, L), ln, ch, taps, delay, iterations, n_fft, hop, reg, eps, budget = check_dereverb(
            tuple(mix.shape), lens, channels, taps, delay, iterations, n_fft, hop, reg, eps, workspace_budget)
        mix = _dev32(mix, self.device)
        out = torch.empty((B, Cn, L), device=self.device, dtype=torch.float32)
        G = torch.zeros((B, n_fft // 2 + 1, Cn * taps, Cn), dtype=torch.complex128) if return_info else None
        fail = torch.zeros((B,), dtype=torch.int32) if return_info else None
        self._check(self.lib.dsn_dereverb(self.ctx, _ptr(mix), B, Cn, L, _i32(ln), _i32(ch), n_fft, hop, taps, delay,
                                          iterations, reg, eps, budget, _ptr(out), _host(G), _host(fail, C.c_int32),
                                          self._stream()), "dsn_dereverb")
        return (out, {"G": G, "fail": fail}) if return_info else out

    # ------------------------------------------------------------------ K candidates -> one separation
    def ensemble_combine(self, cands, mix=None, lens=None, mode="mean", return_info=False):
        """K candidate separations of the same mixtures -> one (dsn_ensemble_combine, csrc/ensemble.hip; the definition
        is in include/ditsep_hip.h and tests/ensemble_restatement.py).  cands [B, K, n, L] float32 -- K draws of the
        sampler, or any rows: flattened latents [B, K, n, D T] go with mix=None --, mix [B, L] or [B, 1, L] or None ->
        out [B, n, L].  The candidates come in arbitrary source order: they are aligned to an anchor candidate (the
        one the others agree with most) by the permutations that maximise the inner products, then combined per
        sample: mode "mean" (float32 sum in candidate order, its rounding errors given back, / K), "median", "best" (the candidate with the
        smallest mixture residual |mix - sum_i cand_i|^2; needs mix) or "medoid" (the anchor).  lens: a ragged batch
        padded to L -- nothing at or past lens[b] is read, out is zero there, each item gets the bits it gets alone.
        return_info=True: (out, info) with, on the host, "perm" [B, K, n] (slot i of candidate k is its source
        perm[b, k, i]), "anchor" [B], "best" [B] (-1 without mix), "resid_db" [B, K] (the relative residual energy;
        below about L 2^-53 it is rounding), "agree_db" [B, K, n] (the SI-SDR of each aligned row against the anchor's:
        +inf for the anchor itself) and "gram" [B, R, R] float64, R = K n (+ 1, the mixture's row last).  Not a
        trained step: what it does to separation quality is unmeasured.  Needs no score network and no codec; two
        calls give identical bits."""
        (B, K, n, L), ln, code = ensemble_checks(cands, mix, lens, mode)
        cands = _dev32(cands, self.device)
        mix = None if mix is None else _dev32(mix, self.device).reshape(B, L)
        out = torch.empty((B, n, L), device=self.device, dtype=torch.float32)
        info, R = None, K * n + (mix is not None)
        if return_info:
            info = {"perm": torch.zeros((B, K, n), dtype=torch.int32), "anchor": torch.zeros(B, dtype=torch.int32),
                    "best": torch.zeros(B, dtype=torch.int32), "resid_db": torch.zeros((B, K), dtype=torch.float64),
                    "agree_db": torch.zeros((B, K, n), dtype=torch.float64),
                    "gram": torch.zeros((B, R, R), dtype=torch.float64)}
        host = lambda k, t: None if info is None else C.cast(C.c_void_p(info[k].data_ptr()), C.POINTER(t))
        self._check(self.lib.dsn_ensemble_combine(
            self.ctx, _ptr(cands), _ptr(mix), B, K, n, L, None if ln is None else (C.c_int32 * B)(*ln), code, _ptr(out),
            host("perm", C.c_int32), host("anchor", C.c_int32), host("best", C.c_int32), host("resid_db", C.c_double),
            host("agree_db", C.c_double), host("gram", C.c_double), self._stream()), "dsn_ensemble_combine")
        if info is None:
            return out
        return out, {k: (v.long() if v.dtype == torch.int32 else v) for k, v in info.items()}

    def to_model_rate(self, clips, rates, fs: int, downmix: bool = True):
        """Clips of any rate, channel count and length at the model's rate `fs`, mixed down to mono: `clips` is a list
        of [L], [C, L] or [1, C, L] tensors, `rates` an int or one rate per clip -> list of [1, L'_b] on the device.
        Clips are grouped by input rate: one resample call per distinct (rate, channel count), its clips padded to the
        group's longest; a mono clip already at `fs` is copied.  downmix=False keeps the channels: a list of
        [C_b, L'_b], every channel resampled alone (a clip already at `fs` is copied whatever its channel count)."""
        rates = [int(rates)] * len(clips) if isinstance(rates, int) else [int(r) for r in rates]
        if len(rates) != len(clips):
            raise ValueError(f"one sample rate per clip is needed ({len(clips)} clips, {len(rates)} rates)")
        norm = []
        for i, a in enumerate(clips):
            if a.dim() == 3 and a.shape[0] == 1:
                a = a[0]
            elif a.dim() == 1:
                a = a[None]
            if a.dim() != 2:
                raise ValueError(f"clip {i} must be [L], [C, L] or [1, C, L] (got {tuple(a.shape)})")
            check_resample(rates[i], fs, tuple(a.shape))
            norm.append(a)
        groups, out = {}, [None] * len(clips)
        for i, a in enumerate(norm):
            groups.setdefault((rates[i], int(a.shape[0])), []).append(i)
        for (rate, Cn), idx in groups.items():
            if rate == fs and (Cn == 1 or not downmix):
                for i in idx:
                    out[i] = _dev32(norm[i], self.device).clone()
                continue
            ln = [int(norm[i].shape[-1]) for i in idx]
            x = torch.zeros((len(idx), Cn, max(ln)), device=self.device, dtype=torch.float32)
            for j, i in enumerate(idx):
                x[j, :, :ln[j]] = _dev32(norm[i], self.device)
            y, yl = self.resample(x, rate, fs, lens=ln, downmix=bool(downmix))
            for j, i in enumerate(idx):
                out[i] = y[j, :, :yl[j]]
        return out

    def from_model_rate(self, ests, rates, fs: int, lengths):
        """The way back: `ests` is a list of [n, L'_b] estimates at the model's rate `fs` -> list of [n, lengths[b]] at
        rates[b], one resample call per distinct rate, each estimate cropped to its clip's original sample count (the
        round trip never comes back shorter: ceil(orig ceil(new L / orig) / new) >= L).  An estimate whose rate is `fs`
        is handed back as it is."""
        groups, out = {}, [None] * len(ests)
        for i, r in enumerate(rates):
            groups.setdefault(int(r), []).append(i)
        for rate, idx in groups.items():
            if rate == fs:
                for i in idx:
                    out[i] = ests[i][:, :int(lengths[i])]
                continue
            ln = [int(ests[i].shape[-1]) for i in idx]
            n = int(ests[idx[0]].shape[0])
            x = torch.zeros((len(idx), n, max(ln)), device=self.device, dtype=torch.float32)
            for j, i in enumerate(idx):
                x[j, :, :ln[j]] = ests[i]
            y, _ = self.resample(x, fs, rate, lens=ln)
            for j, i in enumerate(idx):
                out[i] = y[j, :, :int(lengths[i])]
        return out

    def stems_from_model_rate(self, stems, rates, fs: int, lengths):
        """`from_model_rate` for multichannel stems: a list of [n, C_b, L'_b] at `fs` -> list of [n, C_b, lengths[b]] at
        rates[b]; one resample call per distinct (rate, channel count)."""
        out = [None] * len(stems)
        for cn in sorted({int(s.shape[1]) for s in stems}):
            idx = [i for i, s in enumerate(stems) if int(s.shape[1]) == cn]
            back = self.from_model_rate([stems[i].reshape(-1, stems[i].shape[-1]) for i in idx],
                                        [rates[i] for i in idx], fs, [lengths[i] for i in idx])
            for i, y in zip(idx, back):
                out[i] = y.reshape(int(stems[i].shape[0]), cn, -1)
        return out

    # ------------------------------------------------------------------ WAV payloads and the output gain
    def pcm_decode(self, raw, items, downmix: bool = True):
        """The `data` payloads of WAV files to float32 on the device (dsn_pcm_decode, one launch for the whole mixed
        batch): `raw` is the payloads back to back -- a uint8 tensor (host, pinned or not, or device) or a bytes-like
        object; it goes to the device in one copy --, `items` one (offset, frames, channels, encoding) per payload with
        encoding one of PCM_ENCODINGS.  -> (x [B, Cout, Lmax] float32, zero past each item's end, and the frame counts).
        The conversions are torchaudio.load(normalize=True)'s, defined to the bit (include/ditsep_hip.h).  downmix:
        Cout = 1 and a frame is (x_0 + .. + x_{C-1}) / C in that order; else Cout is the largest channel count and an
        item's unused channels are zero.  Needs no score network and no codec."""
        if not torch.is_tensor(raw):
            raw = torch.frombuffer(bytearray(raw), dtype=torch.uint8)
        if raw.dtype != torch.uint8 or raw.dim() != 1:
            raise ValueError(f"raw must be a 1-D uint8 tensor or bytes (got {raw.dtype}, {tuple(raw.shape)})")
        offs, frames, chans, codes, Cout, Lmax = check_pcm_items(items, raw.numel(), downmix)
        raw = raw.to(self.device, non_blocking=True).contiguous()
        B = len(offs)
        out = torch.empty((B, Cout, Lmax), device=self.device, dtype=torch.float32)
        i32 = C.c_int32 * B
        self._check(self.lib.dsn_pcm_decode(self.ctx, _ptr(raw), raw.numel(), B, (C.c_int64 * B)(*offs), i32(*frames),
                                            i32(*chans), i32(*codes), int(bool(downmix)), _ptr(out), Cout, Lmax,
                                            self._stream()), "dsn_pcm_decode")
        return out, frames

    def pcm_encode(self, x, lens=None, encoding: str = "s16", offsets=None, out=None):
        """Float32 rows to mono WAV payloads on the device (dsn_pcm_encode): x [R, Lmax] (or [Lmax]), one row per
        (file, speaker) with lens[r] samples (default: Lmax each), encoding one of PCM_OUT_ENCODINGS -> (one `bytes` per
        row, the clipped counts).  s16 / s24: rint(x 2^(b-1)) with ties to even, clamped, NaN -> 0; a row's count is
        the samples that were clamped or not finite.  f32 copies the bits and counts nothing.  The rows are packed back
        to back into one device byte buffer that comes to the host in one copy; `offsets` (one byte offset per row) and
        `out` (a uint8 device tensor) place them in a buffer of the caller's instead, of which only each row's own
        bytes are written.  Needs no score network and no codec; two calls give identical bytes."""
        if encoding not in PCM_OUT_ENCODINGS:
            raise ValueError(f"encoding must be one of {PCM_OUT_ENCODINGS} (got {encoding!r})")
        x = _dev32(x, self.device)
        x = x[None] if x.dim() == 1 else x
        if x.dim() != 2 or x.shape[0] < 1 or x.shape[1] < 1:
            raise ValueError(f"x must be [R, Lmax] with at least one row and one sample (got {tuple(x.shape)})")
        R, Lmax = (int(v) for v in x.shape)
        ln = [Lmax] * R if lens is None else check_lens(lens, R, Lmax)
        w = PCM_SAMPLE_BYTES[encoding]
        if offsets is None:
            offsets, o = [], 0
            for v in ln:
                offsets.append(o)
                o += v * w
        offsets = [int(v) for v in offsets]
        if len(offsets) != R:
            raise ValueError(f"one byte offset per row is needed ({R} rows, {len(offsets)} offsets)")
        if out is None:
            out = torch.zeros(max(o + v * w for o, v in zip(offsets, ln)), device=self.device, dtype=torch.uint8)
        if out.dtype != torch.uint8 or out.dim() != 1 or not out.is_cuda or not out.is_contiguous():
            raise ValueError("out must be a contiguous 1-D uint8 tensor on the device")
        clipped = (C.c_int64 * R)()
        self._check(self.lib.dsn_pcm_encode(self.ctx, _ptr(x), R, Lmax, (C.c_int32 * R)(*ln), PCM_ENCODINGS[encoding],
                                            _ptr(out), out.numel(), (C.c_int64 * R)(*offsets), clipped, self._stream()),
                    "dsn_pcm_encode")
        host = torch.empty(out.numel(), dtype=torch.uint8, pin_memory=True)
        host.copy_(out)
        view = memoryview(host.numpy())
        return [bytes(view[o:o + v * w]) for o, v in zip(offsets, ln)], [int(c) for c in clipped]

    def pcm_encode_frames(self, x, lens=None, channels=None, encoding: str = "s16", offsets=None, out=None):
        """Float32 rows to interleaved multichannel WAV payloads on the device (dsn_pcm_encode_frames): x [R, C, Lmax],
        row r is lens[r] frames (default Lmax) of its first channels[r] channels (default C) -> (one `bytes` per row,
        channels[r] samples per frame, and the clipped counts, summed over a row's channels).  Quantisation, clamping,
        NaN handling, `offsets` and `out` as in `pcm_encode`, whose bytes these are with C = 1.  A frame wider than
        PCM_MAX_FRAME_BYTES is refused.  Needs no score network and no codec; two calls give identical bytes."""
        if encoding not in PCM_OUT_ENCODINGS:
            raise ValueError(f"encoding must be one of {PCM_OUT_ENCODINGS} (got {encoding!r})")
        x = _dev32(x, self.device)
        if x.dim() != 3 or min(x.shape) < 1:
            raise ValueError(f"x must be [R, C, Lmax] with at least one row, channel and sample (got {tuple(x.shape)})")
        R, Cn, Lmax = (int(v) for v in x.shape)
        ln = [Lmax] * R if lens is None else check_lens(lens, R, Lmax)
        ch = [Cn] * R if channels is None else [int(v) for v in channels]
        w = PCM_SAMPLE_BYTES[encoding]
        if len(ch) != R:
            raise ValueError(f"one channel count per row is needed ({R} rows, {len(ch)} counts)")
        for r, v in enumerate(ch):
            if v < 1 or v > Cn:
                raise ValueError(f"row {r}: channels = {v} outside [1, C = {Cn}]")
            if v * w > PCM_MAX_FRAME_BYTES:
                raise ValueError(f"row {r}: a frame of {v * w} bytes is wider than PCM_MAX_FRAME_BYTES = "
                                 f"{PCM_MAX_FRAME_BYTES}")
        size = [v * c * w for v, c in zip(ln, ch)]
        if offsets is None:
            offsets, o = [], 0
            for v in size:
                offsets.append(o)
                o += v
        offsets = [int(v) for v in offsets]
        if len(offsets) != R:
            raise ValueError(f"one byte offset per row is needed ({R} rows, {len(offsets)} offsets)")
        if out is None:
            out = torch.zeros(max(o + v for o, v in zip(offsets, size)), device=self.device, dtype=torch.uint8)
        if out.dtype != torch.uint8 or out.dim() != 1 or not out.is_cuda or not out.is_contiguous():
            raise ValueError("out must be a contiguous 1-D uint8 tensor on the device")
        clipped = (C.c_int64 * R)()
        i32 = C.c_int32 * R
        self._check(self.lib.dsn_pcm_encode_frames(self.ctx, _ptr(x), R, Cn, Lmax, i32(*ln), i32(*ch),
                                                   PCM_ENCODINGS[encoding], _ptr(out), out.numel(),
                                                   (C.c_int64 * R)(*offsets), clipped, self._stream()),
                    "dsn_pcm_encode_frames")
        host = torch.empty(out.numel(), dtype=torch.uint8, pin_memory=True)
        host.copy_(out)
        view = memoryview(host.numpy())
        return [bytes(view[o:o + v]) for o, v in zip(offsets, size)], [int(c) for c in clipped]

    def scale_output(self, mix, sep, lens=None):
        """The reference's output gain (src/inference/separate.py:73-78) for a ragged batch (dsn_scale_output): mix
        [B, Lmax] or [B, 1, Lmax], sep [B, n, Lmax], lens one sample count per item (default: Lmax each) ->
        (alpha sep [B, n, Lmax] on the device, zero past each item's end; alpha [B, n] float32 on the host) with
        alpha[b, i] = sum_t mix sep / sum_t (sep^2 + 1e-10) over t < lens[b], summed in float64 in a fixed order and
        rounded once.  Nothing at or past lens[b] is read; an all-zero estimate gives zeros.  Needs no score network
        and no codec; a row gives the bits it gives alone."""
        mix, sep = _dev32(mix, self.device), _dev32(sep, self.device)
        if mix.dim() == 3 and mix.shape[1] == 1:
            mix = mix[:, 0]
        if sep.dim() != 3 or mix.dim() != 2 or mix.shape[0] != sep.shape[0] or mix.shape[-1] != sep.shape[-1]:
            raise ValueError(f"mix must be [B, Lmax] or [B, 1, Lmax] and sep [B, n, Lmax] (got {tuple(mix.shape)}, "
                             f"{tuple(sep.shape)})")
        B, n, Lmax = (int(v) for v in sep.shape)
        if B < 1 or n < 1 or Lmax < 1:
            raise ValueError(f"sep must hold at least one item, source and sample (got {tuple(sep.shape)})")
        ln = None if lens is None else check_lens(lens, B, Lmax)
        mix = mix.contiguous()
        out = torch.empty_like(sep)
        alpha = torch.zeros((B, n), dtype=torch.float32)
        self._check(self.lib.dsn_scale_output(self.ctx, _ptr(mix), _ptr(sep), B, n, Lmax,
                                              None if ln is None else (C.c_int32 * B)(*ln), _ptr(out),
                                              C.cast(C.c_void_p(alpha.data_ptr()), C.POINTER(C.c_float)),
                                              self._stream()), "dsn_scale_output")
        return out, alpha

    # ------------------------------------------------------------------ loudness, true peak and one gain
    def loudness(self, x, rates, lens=None, channels=None, true_peak=True) -> dict:
        """Programme loudness by ITU-R BS.1770-4 / EBU R 128 and the peaks of a ragged batch on the device
        (dsn_loudness, csrc/loudness.hip; the definition is in include/ditsep_hip.h and tests/loudness_restatement.py):
        x [L], [C, L] or [B, C, L] with C <= 2, rates an int or one rate per item in [8000, 192000] Hz, lens /
        channels one count per item (default: L and C) -> a dict of host tensors, one entry per item:
          "loudness"     float64, integrated loudness in LUFS (K-weighting, 400 ms blocks every 100 ms, the absolute
                         gate at -70 and the relative gate 10 LU under the gated mean); -inf when no block passes
          "true_peak"    float64, linear: max |.| of the item at four times its rate (the project's resampler at 1 -> 4);
                         NaN with true_peak=False
          "sample_peak"  float64, linear: max |x|
          "blocks", "gated_blocks"  int64: complete blocks, and those that pass both gates
          "nonfinite"    int64: samples that are NaN or infinite (both peaks are then NaN)
        Nothing at or past lens[b] or in a channel an item does not have is read (it may hold NaN); an item has the
        bits it has alone, whatever the batch.  Needs no score network and no codec."""
        (B, Cn, L), rt, ln, ch = check_loudness(tuple(x.shape), rates, lens, channels)
        x = _dev32(x, self.device).reshape(B, Cn, L)
        stats = torch.zeros((B, 6), dtype=torch.float64)
        i32 = C.c_int32 * B
        self._check(self.lib.dsn_loudness(self.ctx, _ptr(x), B, Cn, L, None if ln is None else i32(*ln),
                                          None if ch is None else i32(*ch), i32(*rt), int(bool(true_peak)),
                                          C.cast(C.c_void_p(stats.data_ptr()), C.POINTER(C.c_double)),
                                          self._stream()), "dsn_loudness")
        return {"loudness": stats[:, 0].clone(), "true_peak": stats[:, 1].clone(), "sample_peak": stats[:, 2].clone(),
                "blocks": stats[:, 3].long(), "gated_blocks": stats[:, 4].long(), "nonfinite": stats[:, 5].long()}

    def apply_gain(self, x, gain, lens=None, channels=None, out=None):
        """out = gain[r] x, one float32 product per sample (dsn_apply_gain): x [R, C, L] (or [C, L], [L]) with C <= 2,
        gain one number per row (rounded to float32), lens / channels one count per row (default: L and C) -- zero
        at or past lens[r] and in the channels a row does not have, where nothing is read.  out=x works in place."""
        shape = tuple(x.shape)
        (R, Cn, L), _, ln, ch = check_loudness(shape, LOUDNESS_RATES[0], lens, channels)
        gain = [float(g) for g in (gain.tolist() if torch.is_tensor(gain) else gain)]
        if len(gain) != R:
            raise ValueError(f"apply_gain: one gain per row is needed (R = {R}), got {len(gain)}")
        x = _dev32(x, self.device)
        if out is None:
            out = torch.empty_like(x)
        elif out.shape != x.shape or out.dtype != torch.float32 or out.device != x.device or not out.is_contiguous():
            raise ValueError("apply_gain: out must be a contiguous float32 tensor of x's shape on the device")
        i32 = C.c_int32 * R
        self._check(self.lib.dsn_apply_gain(self.ctx, _ptr(x), R, Cn, L, None if ln is None else i32(*ln),
                                            None if ch is None else i32(*ch), (C.c_float * R)(*gain), _ptr(out),
                                            self._stream()), "dsn_apply_gain")
        return out

    def limiter_curve(self, x, rates, group, pregain, ceiling, lookahead_ms=5.0, lens=None, channels=None,
                      envelope=False):
        """The gain curve of the true-peak look-ahead limiter (dsn_limiter_curve, csrc/limiter.hip; the definition is
        in include/ditsep_hip.h and tests/limiter_restatement.py): x [R, C, L] (or [C, L], [L]) with C <= 2, rates an
        int or one rate per row, group one label per row (0 .. G - 1, non-decreasing; the rows of a group share one
        curve, one length and one rate), pregain one linear gain per group (rounded to float32), ceiling linear,
        lens / channels one count per row -> (curve [G, L] float32 on the device -- 1 at and past a group's length --,
        {"min_gain": float64 [G] the smallest g (NaN with non-finite samples), "limited_samples": int64 [G] the
        samples with g < 1, "nonfinite": int64 [G]}), and with envelope=True the envelope p [G, L] as a third entry
        (zero where it is not written)."""
        (R, Cn, L), rt, ln, ch, grp, pg = check_limiter(tuple(x.shape), rates, group, pregain, ceiling, lookahead_ms,
                                                        lens, channels)
        x = _dev32(x, self.device).reshape(R, Cn, L)
        G = len(pg)
        curve = torch.empty((G, L), device=x.device, dtype=torch.float32)
        env = torch.zeros((G, L), device=x.device, dtype=torch.float32) if envelope else None
        stats = torch.zeros((G, 3), dtype=torch.float64)
        i32 = C.c_int32 * R
        self._check(self.lib.dsn_limiter_curve(self.ctx, _ptr(x), R, Cn, L, None if ln is None else i32(*ln),
                                               None if ch is None else i32(*ch), i32(*rt), i32(*grp), G,
                                               (C.c_float * G)(*pg), float(ceiling), float(lookahead_ms), _ptr(curve),
                                               _ptr(env),
                                               C.cast(C.c_void_p(stats.data_ptr()), C.POINTER(C.c_double)),
                                               self._stream()), "dsn_limiter_curve")
        info = {"min_gain": stats[:, 0].clone(), "limited_samples": stats[:, 1].long(), "nonfinite": stats[:, 2].long()}
        return (curve, info, env) if envelope else (curve, info)

    def apply_curve(self, x, group, pregain, curve, lens=None, channels=None, out=None):
        """out = (pregain[group[r]] x) curve[group[r]], two float32 products per sample (dsn_apply_curve): x [R, C, L]
        (or [C, L], [L]) with C <= 2, group one label in [0, G) per row in any order, pregain [G], curve [G, L] float32
        on the device (Engine.limiter_curve's) -- zero at or past lens[r] and in the channels a row does not have, where
        nothing is read.  The rows need not be the ones the curve was formed from.  out=x works in place."""
        (R, Cn, L), _, ln, ch, grp, pg = check_limiter(tuple(x.shape), LOUDNESS_RATES[0], group, pregain, None, None,
                                                       lens, channels)
        G = len(pg)
        x = _dev32(x, self.device)
        if (not torch.is_tensor(curve) or tuple(curve.shape) != (G, L) or curve.dtype != torch.float32
                or curve.device != x.device or not curve.is_contiguous()):
            raise ValueError(f"apply_curve: curve must be a contiguous float32 tensor [G = {G}, L = {L}] on the device")
        if out is None:
            out = torch.empty_like(x)
        elif out.shape != x.shape or out.dtype != torch.float32 or out.device != x.device or not out.is_contiguous():
            raise ValueError("apply_curve: out must be a contiguous float32 tensor of x's shape on the device")
        i32 = C.c_int32 * R
        self._check(self.lib.dsn_apply_curve(self.ctx, _ptr(x), R, Cn, L, None if ln is None else i32(*ln),
                                             None if ch is None else i32(*ch), i32(*grp), G, (C.c_float * G)(*pg),
                                             _ptr(curve), _ptr(out), self._stream()), "dsn_apply_curve")
        return out

    # ------------------------------------------------------------------ speaker activity of separated stems
    def activity(self, est, lens=None, fs=16000, n_fft=512, hop=128, band=(100.0, 4000.0), half_width=2, range_db=40.0,
                 dominance_db=6.0, hysteresis_db=3.0, min_on=13, min_off=13, pad=0) -> dict:
        """Where every stem carries its speaker (dsn_activity, csrc/activity.hip; the definition is in
        include/ditsep_hip.h and tests/activity_restatement.py): est [B, n <= 4, L] separated estimates -> per item,
        source and STFT frame (mask_refine's frames, F = 1 + ceil(L / hop)) a decision from the band energy
        (`band` in Hz at rate fs) smoothed over 2 half_width + 1 frames: on where the level is within range_db of the
        item's peak and within dominance_db of the loudest stem of the frame, kept while it stays within
        hysteresis_db more of both; then gaps shorter than min_off frames between two runs are filled, runs shorter
        than min_on frames cleared and every run padded by `pad` frames.  Durations are in frames here
        (activity_frames converts seconds).  lens: a ragged batch padded to L, nothing past lens[b] is read.
        -> dict(act [B, n, Fmax] uint8, frames_on [B, n] int32, energy and level [B, n, Fmax] float64 -- on the
        device --, frames [B] the items' frame counts).  A decision rule, not a trained detector; the defaults are not
        tuned.  native.activity_segments turns a row of act into sample segments.  Two calls give identical bits."""
        (B, n, L), ln, n_fft, hop, (j_lo, j_hi), cs, Fmax = check_activity(
            tuple(est.shape), lens, fs, n_fft, hop, band, half_width, range_db, dominance_db, hysteresis_db, min_on,
            min_off, pad)
        est = _dev32(est, self.device)
        act = torch.empty((B, n, Fmax), device=self.device, dtype=torch.uint8)
        frames_on = torch.empty((B, n), device=self.device, dtype=torch.int32)
        energy = torch.empty((B, n, Fmax), device=self.device, dtype=torch.float64)
        level = torch.empty((B, n, Fmax), device=self.device, dtype=torch.float64)
        self._check(self.lib.dsn_activity(self.ctx, _ptr(est), B, n, L, _i32(ln), n_fft, hop, j_lo, j_hi, int(half_width),
                                          cs[0], cs[1], cs[2], cs[3], int(min_on), int(min_off), int(pad), _ptr(act),
                                          _ptr(frames_on), _ptr(energy), _ptr(level), self._stream()), "dsn_activity")
        return dict(act=act, frames_on=frames_on, energy=energy, level=level,
                    frames=[1 + -(-v // hop) for v in (ln if ln is not None else [L] * B)])

    def activity_gate(self, x, act, lens=None, hop=128, fade=80):
        """The stems with their inactive stretches made digital silence (dsn_activity_gate): x [B, n, L], act
        [B, n, F] (Engine.activity's) -> [B, n, L].  Sample m lies in a segment iff act[(m + hop / 2) // hop] is set:
        there the output is x bit for bit; at distance d <= fade samples from the nearest segment sample of its row it
        is activity_ramp(fade)[d - 1] x (a raised-cosine fade, one float32 product), further away +0 whatever x holds,
        and +0 at or past lens[b], where nothing is read.  fade = 0 is a hard gate."""
        (B, n, L), Fa, ln = check_activity_gate(tuple(x.shape), tuple(act.shape), lens, hop, fade)
        x = _dev32(x, self.device)
        if not torch.is_tensor(act) or act.dtype != torch.uint8:
            raise ValueError("activity_gate: act must be a uint8 tensor [B, n, F] (Engine.activity's act)")
        act = act.to(self.device).contiguous()
        ramp = activity_ramp(int(fade))
        out = torch.empty((B, n, L), device=self.device, dtype=torch.float32)
        table = (C.c_float * max(1, len(ramp)))(*ramp.tolist())
        self._check(self.lib.dsn_activity_gate(self.ctx, _ptr(x), _ptr(act), B, n, L, Fa, _i32(ln), int(hop), int(fade),
                                               table if len(ramp) else None, _ptr(out), self._stream()),
                    "dsn_activity_gate")
        return out

    def activity_of(self, est, opts, fs: int, lens=None) -> tuple:
        """The `activity` keyword on final mono estimates at rate fs: est [B, n, L] (lens: the items' own lengths),
        opts native.activity_options' dict -> (est, gated when opts["gate"] is set; per item a dict of "segments" (per
        source [(start, end), ..] in samples at fs), "seconds" (the same in seconds), "active" (seconds per source),
        "frames_on" and "options")."""
        kw, fr = activity_keywords(opts, fs), activity_frames(opts, fs)
        res = self.activity(est, lens=lens, **kw)
        out = self.activity_gate(est, res["act"], lens=lens, hop=kw["hop"], fade=fr["fade"]) if opts["gate"] else est
        act, on = res["act"].cpu().numpy(), res["frames_on"].cpu().tolist()
        B, n, L = (int(v) for v in est.shape)
        items = []
        for b in range(B):
            Lb = L if lens is None else int(lens[b])
            segs = [activity_segments(act[b, i], res["frames"][b], kw["hop"], Lb) for i in range(n)]
            items.append(dict(segments=segs, seconds=[[(s / fs, e / fs) for s, e in row] for row in segs],
                              active=[sum(e - s for s, e in row) / fs for row in segs], frames_on=on[b],
                              options=dict(opts)))
        return out, items

    def _limit_groups(self, xs, rt, ln, ch, grp, prog, g_lo, i_src, target, ceiling, lim):
        """The `limit` keyword's loop for the groups the ceiling held back: xs [R, C, L] the rows before any gain, grp
        their labels 0 .. Q - 1, prog None (a group is one row and its own programme) or (mx [Q, C', L], channels):
        one mixture per group, measured in place of the rows.  g_lo, i_src per group; target None: one evaluation at
        0 dB and no measurement.  -> (the limited rows, per group: gain_db, loudness, evaluations, min_gain,
        limited_samples, trim (linear); per row: the true peak after the trim)"""
        import numpy as np

        Q = len(g_lo)
        lin = lambda d: float(np.float32(10.0 ** (d / 20.0)))
        first = [b for b in range(len(grp)) if b == 0 or grp[b] != grp[b - 1]]   # a row of every group
        q_rt, q_ln = [rt[r] for r in first], [ln[r] for r in first]
        hist = [[] for _ in range(Q)]
        kw = dict(drive_db=lim["drive_db"], iterations=lim["iterations"], tol=lim["tol"])
        cur = [0.0 if target is None else limiter_drive(g_lo[q], i_src[q], target, [], **kw) for q in range(Q)]
        active = [] if target is None else list(range(Q))
        while active:
            pg = [lin(v) for v in cur]
            curve, _ = self.limiter_curve(xs, rt, grp, pg, ceiling, lim["lookahead_ms"], ln, ch)
            if prog is None:
                I = self.loudness(self.apply_curve(xs, grp, pg, curve, ln, ch), rt, ln, ch, true_peak=False)
            else:
                I = self.loudness(self.apply_curve(prog[0], list(range(Q)), pg, curve, q_ln, prog[1]), q_rt, q_ln,
                                  prog[1], true_peak=False)
            I = I["loudness"].tolist()
            still = []
            for q in active:
                hist[q].append((cur[q], I[q]))
                nxt = limiter_drive(g_lo[q], i_src[q], target, hist[q], **kw)
                if nxt is not None:
                    cur[q] = nxt
                    still.append(q)
            active = still
        loud = [math.nan] * Q
        for q in range(Q):
            if hist[q]:
                cur[q], loud[q] = hist[q][limiter_best(hist[q], target)]
        pg = [lin(v) for v in cur]
        curve, st = self.limiter_curve(xs, rt, grp, pg, ceiling, lim["lookahead_ms"], ln, ch)
        y = self.apply_curve(xs, grp, pg, curve, ln, ch)
        m = self.loudness(y, rt, ln, ch)
        if target is None:
            loud = [m["loudness"][r].item() for r in first]   # (a group's first row; with link "stem" its only one)
        # the trim: interpolating g y is not g times the interpolation, so the ceiling is measured, not assumed
        trim, out, tp = [1.0] * Q, y, m["true_peak"].tolist()
        for _ in range(3):
            top = [max(tp[r] for r in range(len(grp)) if grp[r] == q) for q in range(Q)]
            over = [q for q in range(Q) if top[q] > ceiling]
            if not over:
                break
            for q in over:
                trim[q] = float(np.float32(trim[q] * (ceiling / top[q])))
            out = self.apply_gain(y, [trim[q] for q in grp], ln, ch)
            tp = self.loudness(out, rt, ln, ch)["true_peak"].tolist()
        res = {"gain_db": [cur[q] + 20.0 * math.log10(trim[q]) for q in range(Q)],
               "loudness": [loud[q] + 20.0 * math.log10(trim[q]) for q in range(Q)],
               "evaluations": [max(len(h), 1) for h in hist], "min_gain": st["min_gain"].tolist(),
               "limited_samples": st["limited_samples"].tolist(), "trim": trim, "true_peak": tp}
        return out, res

    def loudness_normalize(self, sources, stems, rates, target=-23.0, peak=-1.0, link="mixture", limit=None):
        """The `loudness` keyword's last step for a list of items: `stems` is one [n, L_b] or [n, C_b, L_b] tensor per
        item at rates[b], `sources` the items' mixtures [C'_b, L'_b] (or [L'_b]) at the same rates.  link "mixture":
        every item's gain source is its mixture and its n stems share one gain; link "stem": every stem is its own
        source (sources may be None).  One Engine.loudness call on the padded mixtures, one on the padded stems, the
        gains by native.loudness_gain, one Engine.apply_gain call.  -> (list of tensors shaped like `stems`, info) with
        info = {"loudness_in", "loudness_out", "gain_db", "true_peak_db": one list of n floats per item (the source's
        loudness, that plus the gain, the gain, the stem's true peak after the gain in dBTP), "limited": likewise,
        booleans, "silent" / "nonfinite": the (item, stem) pairs left at 0 dB because their source passed no block /
        held non-finite samples}.
        limit (default None: the calls and bits above): True or a dict (native.limit_options) -- the groups whose gain
        the ceiling set ("limited") go through the true-peak look-ahead limiter instead (Engine.limiter_curve /
        apply_curve): the pre-gain starts at target - I_src, clamped to [g, g + drive_db] with g the single gain, each
        evaluation is curve -> apply -> Engine.loudness of the limited programme (the limited mixture with link
        "mixture", zero-extended or cut to the stems' length; the limited stem with link "stem"), native.limiter_drive gives the
        next pre-gain, the evaluation closest to the target is kept, and the group is trimmed by ceiling / TP where the
        measured true peak of a limited stem still exceeds the ceiling.  Other groups are untouched.  target=None
        with a limit: no loudness rule, every group one evaluation at 0 dB against the ceiling.  info gains, one list of
        n per item: "reached" (|target - loudness_out| <= tol; true where the single gain sufficed), "evaluations",
        "reduction_db" (20 log10 of the smallest g) and "limited_samples"; "loudness_out" and "true_peak_db" of a
        limited group are measured figures."""
        if link not in LOUDNESS_LINKS:
            raise ValueError(f"loudness: link must be one of {LOUDNESS_LINKS} (got {link!r})")
        lim = limit_options(limit)
        if target is None and lim is None:
            raise ValueError("loudness: target=None (no loudness rule) needs limit=")
        B = len(stems)
        rates = [int(rates)] * B if isinstance(rates, int) else [int(r) for r in rates]
        rows3 = [s[:, None] if s.dim() == 2 else s for s in stems]
        for b, s in enumerate(rows3):
            if s.dim() != 3:
                raise ValueError(f"loudness: item {b} must be [n, L] or [n, C, L] (got {tuple(stems[b].shape)})")
        n = int(rows3[0].shape[0])
        ch = [int(s.shape[1]) for s in rows3]
        ln = [int(s.shape[2]) for s in rows3]
        x = torch.zeros((B * n, max(ch), max(ln)), device=self.device, dtype=torch.float32)
        for b, s in enumerate(rows3):
            x[b * n:(b + 1) * n, :ch[b], :ln[b]] = _dev32(s, self.device)
        rep = lambda v: [a for a in v for _ in range(n)]
        rows = self.loudness(x, rep(rates), rep(ln), rep(ch))
        src = sc = sl = None
        if link == "mixture" and (target is not None or sources is not None):
            if sources is None or len(sources) != B:
                raise ValueError("loudness: link 'mixture' needs one mixture per item")
            src = [m.reshape(-1, m.shape[-1]) for m in sources]
            sc, sl = [int(m.shape[0]) for m in src], [int(m.shape[1]) for m in src]
        if target is None:
            tp = rows["true_peak"].tolist()
            groups = rep(list(range(B))) if link == "mixture" else list(range(B * n))
            nonf = sorted(r for r in range(B * n) if any(math.isnan(tp[k]) for k in range(B * n) if groups[k] == groups[r]))
            I_src = rows["loudness"].tolist()
            g = {"gain_db": [0.0] * (B * n), "gain": [1.0] * (B * n), "limited": [r not in nonf for r in range(B * n)],
                 "silent": [], "nonfinite": nonf}
        else:
            if link == "mixture":
                mx = torch.zeros((B, max(sc), max(sl)), device=self.device, dtype=torch.float32)
                for b, m in enumerate(src):
                    mx[b, :sc[b], :sl[b]] = _dev32(m, self.device)
                I_src = rep(self.loudness(mx, rates, sl, sc, true_peak=False)["loudness"].tolist())
                groups = rep(list(range(B)))
            else:
                I_src, groups = rows["loudness"].tolist(), None
            g = loudness_gain(I_src, rows["true_peak"].tolist(), groups, target, peak)
        sel = [r for r in range(B * n) if g["limited"][r]] if lim is not None else []
        held = x[sel].clone() if sel else None   # the rows of the limited groups before any gain
        if target is not None:
            self.apply_gain(x, g["gain"], rep(ln), rep(ch), out=x)
        tp = rows["true_peak"].tolist()
        tp_db = [20.0 * math.log10(v) + d if v > 0.0 else (-math.inf if v == 0.0 else math.nan)
                 for v, d in zip(tp, g["gain_db"])]
        gain_db = list(g["gain_db"])
        loud_out = [a + d for a, d in zip(I_src, gain_db)]
        extra = {}
        if lim is not None:
            R = B * n
            ok = [r not in g["silent"] and r not in g["nonfinite"] for r in range(R)]
            extra = {"reached": ok, "evaluations": [0] * R, "reduction_db": [0.0] * R, "limited_samples": [0] * R}
        if sel:
            c_db = lim["ceiling"] if lim["ceiling"] is not None else (peak if peak is not None else LIMIT_DEFAULT_CEILING)
            import numpy as np

            ceiling = float(np.float32(10.0 ** (float(c_db) / 20.0)))
            labels = groups if groups is not None else list(range(B * n))
            order = []
            for r in sel:
                if labels[r] not in order:
                    order.append(labels[r])
            grp = [order.index(labels[r]) for r in sel]
            first = [sel[grp.index(q)] for q in range(len(order))]
            prog = None
            if link == "mixture" and target is not None:
                items = [r // n for r in first]
                pm = torch.zeros((len(items), max(sc[b] for b in items), int(x.shape[-1])), device=self.device,
                                 dtype=torch.float32)
                for q, b in enumerate(items):   # (zero-extended or cut to the stems' length: one curve for both)
                    v = min(sl[b], ln[b])
                    pm[q, :sc[b], :v] = _dev32(src[b], self.device)[:, :v]
                prog = (pm, [sc[b] for b in items])
            out, res = self._limit_groups(held, [rep(rates)[r] for r in sel], [rep(ln)[r] for r in sel],
                                          [rep(ch)[r] for r in sel], grp, prog, [g["gain_db"][r] for r in first],
                                          [I_src[r] for r in first], target, ceiling, lim)
            x[sel] = out
            for k, r in enumerate(sel):
                q = grp[k]
                gain_db[r], loud_out[r] = res["gain_db"][q], res["loudness"][q]
                v = res["true_peak"][k]
                tp_db[r] = 20.0 * math.log10(v) if v > 0.0 else (-math.inf if v == 0.0 else math.nan)
                low = res["min_gain"][q]
                extra["reached"][r] = True if target is None else bool(abs(target - loud_out[r]) <= lim["tol"])
                extra["evaluations"][r] = res["evaluations"][q]
                extra["reduction_db"][r] = 20.0 * math.log10(low) if low > 0.0 else (-math.inf if low == 0.0 else math.nan)
                extra["limited_samples"][r] = int(res["limited_samples"][q])
        outs = [x[b * n:(b + 1) * n, :ch[b], :ln[b]].reshape(stems[b].shape) for b in range(B)]
        per = lambda v: [list(v[b * n:(b + 1) * n]) for b in range(B)]
        info = {"loudness_in": per(I_src), "loudness_out": per(loud_out),
                "gain_db": per(gain_db), "true_peak_db": per(tp_db), "limited": per(g["limited"]),
                "silent": [divmod(r, n) for r in g["silent"]], "nonfinite": [divmod(r, n) for r in g["nonfinite"]]}
        info.update({k: per(v) for k, v in extra.items()})
        return outs, info

    @property
    def hop_length(self) -> int:
        return self.lib.dsn_hop_length(self.ctx)

    def latent_frames(self, L: int) -> int:
        return self.lib.dsn_latent_frames(self.ctx, L)

    def enable_graphs(self, on: bool = True):
        self._check(self.lib.dsn_enable_graphs(self.ctx, int(on)), "dsn_enable_graphs")

    def workspace_bytes(self) -> int:
        return self.lib.dsn_workspace_bytes(self.ctx)

    def profile_begin(self):
        self._check(self.lib.dsn_profile_begin(self.ctx), "dsn_profile_begin")

    def profile_end(self):
        ms, fl, n = C.c_double(), C.c_double(), C.c_int64()
        self._check(self.lib.dsn_profile_end(self.ctx, C.byref(ms), C.byref(fl), C.byref(n)), "dsn_profile_end")
        hm, hb, hn = C.c_double(), C.c_double(), C.c_int64()
        self._check(self.lib.dsn_profile_hbm(self.ctx, C.byref(hm), C.byref(hb), C.byref(hn)), "dsn_profile_hbm")
        nrows = self.lib.dsn_profile_rows(self.ctx, 0, None, None, None, None, None)
        rows = []
        if nrows > 0:
            NL = 48                                     # DSN_PROFILE_NAME_LEN
            names = C.create_string_buffer(nrows * NL)
            rms, rfl, rby = ((C.c_double * nrows)() for _ in range(3))
            rn = (C.c_int64 * nrows)()
            self.lib.dsn_profile_rows(self.ctx, nrows, names, rms, rfl, rby, rn)
            for i in range(nrows):
                nm = names.raw[i * NL:(i + 1) * NL].split(b"\0", 1)[0].decode()
                rows.append({"site": nm, "ms": rms[i], "flops": rfl[i], "bytes": rby[i], "launches": int(rn[i])})
        return {"gemm_ms": ms.value, "gemm_flops": fl.value, "gemm_launches": n.value,
                "hbm_ms": hm.value, "hbm_bytes": hb.value, "hbm_launches": hn.value, "rows": rows}

    def si_sdr_pit(self, ref, est):
        """ref, est [B,n,L] -> (si_sdr [B,n] dB, perm [B,n]): est[:, perm[b,i]] matches ref[:, i]."""
        ref, est = _dev32(ref, self.device), _dev32(est, self.device)
        B, n, L = ref.shape
        sdr = (C.c_float * (B * n))()
        perm = (C.c_int * (B * n))()
        self._check(self.lib.dsn_si_sdr_pit(self.ctx, _ptr(ref), _ptr(est), B, n, L, sdr, perm, self._stream()),
                    "dsn_si_sdr_pit")
        return (torch.tensor(list(sdr), dtype=torch.float32).reshape(B, n),
                torch.tensor(list(perm), dtype=torch.long).reshape(B, n))

    def si_bss_eval(self, ref, est, perm_by: str = "sir", clamp_db: float = 100.0, lens=None):
        """ref, est [B,n,L] -> (si_sdr, si_sir, si_sar [B,n] dB, perm [B,n]) with the permutation solved on
        `perm_by` ("sir" as bss_eval / the reference's evaluate_latent.py:118-124, or "sdr").  lens (B ints, optional):
        item b holds lens[b] samples of the L-long rows and gets, bit for bit, what it gets alone; the padding is not
        read (dsn_si_bss_eval_ragged)."""
        B, n, L = ref.shape
        if lens is not None:
            lens = check_lens(lens, B, L)
        ref, est = _dev32(ref, self.device), _dev32(est, self.device)
        bufs = [(C.c_float * (B * n))() for _ in range(3)]
        perm = (C.c_int * (B * n))()
        by = {"sdr": 0, "sir": 1}[perm_by]
        if lens is None:
            self._check(self.lib.dsn_si_bss_eval(self.ctx, _ptr(ref), _ptr(est), B, n, L, by, float(clamp_db), *bufs,
                                                 perm, self._stream()), "dsn_si_bss_eval")
        else:
            self._check(self.lib.dsn_si_bss_eval_ragged(self.ctx, _ptr(ref), _ptr(est), B, n, L, (C.c_int32 * B)(*lens),
                                                        by, float(clamp_db), *bufs, perm, self._stream()),
                        "dsn_si_bss_eval_ragged")
        out = [torch.tensor(list(b), dtype=torch.float32).reshape(B, n) for b in bufs]
        return (*out, torch.tensor(list(perm), dtype=torch.long).reshape(B, n))

    def stoi(self, ref, est, fs: int, extended: bool = True, perm=None, return_frames: bool = False, lens=None):
        """ref, est [B,n,L] -> [B,n] float32 STOI (extended=False) or extended STOI (True) of est against ref, as
        pystoi.stoi(ref, est, fs, extended) defines it (restated in tests/stoi_restatement.py; parity with the pystoi
        package unpinned).  perm [B,n] (optional): est source perm[b,i] is scored against ref source i.  Items with
        fewer than 30 STFT frames left after silent-frame removal score 1e-5 with a RuntimeWarning, as in pystoi;
        return_frames=True also returns those frame counts [B,n].  lens (B ints, optional): item b holds lens[b]
        samples of the L-long rows and gets, bit for bit, what it gets alone; the padding is not read; an item shorter
        than one 10 kHz frame scores 1e-5 with 0 frames (dsn_stoi_ragged)."""
        if ref.dim() != 3 or est.shape != ref.shape:
            raise ValueError(f"ref and est must both be [B,n,L] (got {tuple(ref.shape)} and {tuple(est.shape)})")
        B, n, L = ref.shape
        if lens is not None:
            lens = check_lens(lens, B, L)
        ref, est = _dev32(ref, self.device), _dev32(est, self.device)
        out = (C.c_float * (B * n))()
        frames = (C.c_int * (B * n))()
        cperm = None
        if perm is not None:
            p = torch.as_tensor(perm, dtype=torch.int32).reshape(-1).tolist()
            if len(p) != B * n:
                raise ValueError(f"perm must hold B*n = {B * n} entries (got {len(p)})")
            cperm = (C.c_int * (B * n))(*p)
        if lens is None:
            self._check(self.lib.dsn_stoi(self.ctx, _ptr(ref), _ptr(est), B, n, L, int(fs), int(bool(extended)), cperm,
                                          out, frames, self._stream()), "dsn_stoi")
        else:
            self._check(self.lib.dsn_stoi_ragged(self.ctx, _ptr(ref), _ptr(est), B, n, L, (C.c_int32 * B)(*lens),
                                                 int(fs), int(bool(extended)), cperm, out, frames, self._stream()),
                        "dsn_stoi_ragged")
        score = torch.tensor(list(out), dtype=torch.float32).reshape(B, n)
        nfr = torch.tensor(list(frames), dtype=torch.long).reshape(B, n)
        short = (nfr < 30).nonzero().tolist()
        if short:
            warnings.warn(f"stoi: {len(short)} item(s) [b, i] {short[:8]} have fewer than 30 frames after silent-frame "
                          f"removal; their score is 1e-5", RuntimeWarning, stacklevel=2)
        return (score, nfr) if return_frames else score

    def composite(self, ref, est, fs: int, perm=None, pesq=None, lens=None) -> dict:
        """ref, est [B,n,L] -> {"llr", "wss", "segsnr", "snr": [B,n] float32, "frames": [B,n] long}: the objective
        measures of the Hu & Loizou composite scores as the reference's evaluate_covl.py computes them (restated in
        tests/composite_restatement.py, pinned by tests/golden/composite.npz).  fs is 8000 or 16000.  perm [B,n]
        (optional): est source perm[b,i] is scored against ref source i.  With pesq [B,n] (PESQ is not computed
        here) the dict also holds "csig", "cbak" and "covl", each clipped to [1, 5].  A constant estimate gives NaN
        for segsnr, snr and cbak (the reference rescales by max|est - mean| = 0); llr and wss stay defined.  lens (B
        ints, optional): item b holds lens[b] samples of the L-long rows and gets, bit for bit, what it gets alone,
        "frames" included; the padding is not read; an item shorter than one frame plus one hop is refused by name
        (dsn_composite_ragged)."""
        if ref.dim() != 3 or est.shape != ref.shape:
            raise ValueError(f"ref and est must both be [B,n,L] (got {tuple(ref.shape)} and {tuple(est.shape)})")
        B, n, L = ref.shape
        if lens is not None:
            lens = check_lens(lens, B, L, composite_min_samples(fs), f" at fs = {int(fs)}")
        ref, est = _dev32(ref, self.device), _dev32(est, self.device)
        keys = ["llr", "wss", "segsnr", "snr"] + (["csig", "cbak", "covl"] if pesq is not None else [])
        bufs = {k: (C.c_float * (B * n))() for k in keys}
        frames = (C.c_int * (B * n))()
        out = DsnCompositeOut(frames=frames, **bufs)

        def host(v, ctype, what):
            if v is None:
                return None
            flat = torch.as_tensor(v).reshape(-1).tolist()
            if len(flat) != B * n:
                raise ValueError(f"{what} must hold B*n = {B * n} entries (got {len(flat)})")
            return (ctype * (B * n))(*flat)

        cperm = host(None if perm is None else torch.as_tensor(perm, dtype=torch.int32), C.c_int, "perm")
        cpesq = host(None if pesq is None else torch.as_tensor(pesq, dtype=torch.float32), C.c_float, "pesq")
        if lens is None:
            self._check(self.lib.dsn_composite(self.ctx, _ptr(ref), _ptr(est), B, n, L, int(fs), cperm, cpesq,
                                               C.byref(out), self._stream()), "dsn_composite")
        else:
            self._check(self.lib.dsn_composite_ragged(self.ctx, _ptr(ref), _ptr(est), B, n, L, (C.c_int32 * B)(*lens),
                                                      int(fs), cperm, cpesq, C.byref(out), self._stream()),
                        "dsn_composite_ragged")
        res = {k: torch.tensor(list(b), dtype=torch.float32).reshape(B, n) for k, b in bufs.items()}
        res["frames"] = torch.tensor(list(frames), dtype=torch.long).reshape(B, n)
        return res

    def bss_eval(self, ref, est, *, filter_length: int = 512, perm_by: str = "sir", clamp_db: float = 0.0,
                 load_diag: float = 0.0, perm=None, lens=None, sir_sar: bool = True, return_pairs: bool = False,
                 workspace_budget: int = 0):
        """ref, est [B,n,L] -> (sdr, sir, sar [B,n] float64 dB, perm [B,n]): classic bss_eval (Vincent et al. 2006)
        with distortion filters of `filter_length` taps (1 .. 512), what fast_bss_eval.bss_eval_sources reports and,
        with sir_sar=False (sir and sar NaN, permutation on SDR), fast_bss_eval.sdr; restated in
        tests/bss_eval_restatement.py, parity with the fast_bss_eval / mir_eval packages unpinned.  filter_length=1 is
        si_bss_eval's decomposition.  There is no zero_mean option: subtract the means first.  The permutation is
        solved on `perm_by` ("sir", bss_eval's convention, or "sdr") unless perm [B,n] is given (est source perm[b,i]
        against ref source i).  clamp_db > 0 clamps the dB values to +-clamp_db.  lens (B ints): item b holds lens[b]
        samples and gets, bit for bit, what it gets alone; the padding is not read.  return_pairs=True appends the
        tables (sdr_pairs, sir_pairs [B,n,n]; [b,i,j]: est j against ref i).  workspace_budget (bytes, 0 = 512 MiB)
        bounds the workspace of one chunk of items (native.bss_eval_plan); it changes no bit of the result.
        An item whose Cholesky factorisation breaks down (an all-zero reference, or references so band-limited that
        the F-shift Gram matrix is numerically singular) is NaN throughout, with a RuntimeWarning that names it:
        load_diag > 0 (added to the diagonal of the unit-norm Gram matrix) regularises such items."""
        plan, by, lens, perm = check_bss_eval(ref.shape, est.shape, filter_length=filter_length, perm_by=perm_by,
                                              load_diag=load_diag, perm=perm, lens=lens,
                                              workspace_budget=workspace_budget)
        B, n, L = ref.shape
        ref, est = _dev32(ref, self.device), _dev32(est, self.device)
        vals = {k: (C.c_double * (B * n))() for k in ("sdr", "sir", "sar")}
        pairs = {k: (C.c_double * (B * n * n))() for k in ("sdr_pairs", "sir_pairs")} if return_pairs else {}
        perm_out, status = (C.c_int * (B * n))(), (C.c_int * B)()
        opts = DsnBssEvalOpts(int(filter_length), by, float(clamp_db), float(load_diag), int(bool(sir_sar)),
                              int(workspace_budget))
        out = DsnBssEvalOut(perm_out=perm_out, status=status, **vals, **pairs)
        self._check(self.lib.dsn_bss_eval(self.ctx, _ptr(ref), _ptr(est), B, n, L,
                                          None if lens is None else (C.c_int32 * B)(*lens),
                                          None if perm is None else (C.c_int * (B * n))(*perm), C.byref(opts),
                                          C.byref(out), self._stream()), "dsn_bss_eval")
        broken = [b for b in range(B) if status[b]]
        if broken:
            warnings.warn(f"bss_eval: the Cholesky factorisation broke down for {len(broken)} item(s) {broken[:8]} "
                          f"(a pivot <= 0 or not finite: an all-zero or band-limited reference); their values are NaN. "
                          f"load_diag > 0 regularises the Gram matrix", RuntimeWarning, stacklevel=2)
        res = tuple(torch.tensor(list(vals[k]), dtype=torch.float64).reshape(B, n) for k in ("sdr", "sir", "sar"))
        res += (torch.tensor(list(perm_out), dtype=torch.long).reshape(B, n),)
        if return_pairs:
            res += tuple(torch.tensor(list(pairs[k]), dtype=torch.float64).reshape(B, n, n)
                         for k in ("sdr_pairs", "sir_pairs"))
        return res

    def mrstft_loss(self, reals, decoded, fs: int, *, fft_sizes=MRSTFT_FFT_SIZES, hop_sizes=MRSTFT_HOP_SIZES,
                    win_lengths=None, perceptual_weighting: bool = True, w_sc: float = 1.0, w_log_mag: float = 1.0,
                    w_lin_mag: float = 0.0, l1_weight: float = 0.0, l2_weight: float = 0.0,
                    mrstft_weight: float = 1.0, pit="batch", lens=None, **options) -> dict:
        """reals, decoded [B,n,L] -> the forward value of the reference's LDM generator objective (src/ldm.py:100-154:
        PITLoss(AuralossLoss(MultiResolutionSTFTLoss)) plus PITLoss(L1Loss) / PITLoss(MSELoss) under MultiLoss), from
        one native call (dsn_mrstft_loss) that forms every spectrum once and returns (reference source, estimate
        source) pair tables; the combine over permutations runs on the host (mrstft_combine, which cites the reference
        behaviours it mirrors).  Returns float64 CPU tensors: the tables "sc", "log_mag", "lin_mag" [R,B,n,n], "l1",
        "l2" [B,n,n] (unweighted; a spectral table whose weight is zero is zero, as the reference skips the term);
        "pit_mrstft_loss", "pit_l1_loss", "pit_l2_loss" (weighted; the latter two only with a positive weight) and
        "loss", the reference's MultiLoss keys; "pit_*_perm" [B,n] (estimate source perm[b,i] goes with reference
        source i); "perms" and "mrstft_values", the weighted MR-STFT loss of every permutation tried ([P], or [B,P]
        with pit="item").  perceptual_weighting filters both signals with the 101-tap A-weighting FIR of `fs`
        (ditsep_amd/aweight.py).  `options` takes the reference's remaining keywords (window, w_phs, scale, n_bins,
        scale_invariance, decay, sample_rate): anything but their defaults raises NotImplementedError.
        lens (B ints, optional): a ragged batch padded to L samples, item b holding lens[b] of them
        (dsn_mrstft_loss_ragged).  Item b's rows of every table are, bit for bit, those of this call on the item alone
        -- its own frame count, reflection at its own end, its own divisors -- whatever the padding (which is not
        read) and the batch around it; every lens[b] must exceed max(fft_sizes) / 2.  The combine treats the per-item
        tables as it treats those of a dense batch (mrstft_combine: the definition for mixed lengths)."""
        options.pop("sample_rate", None)
        if options.get("n_bins") is None:
            options.pop("n_bins", None)
        mrstft_unsupported(**options)
        reals, decoded = _dev32(reals, self.device), _dev32(decoded, self.device)
        if reals.dim() != 3 or decoded.shape != reals.shape:
            raise ValueError(f"reals and decoded must both be [B,n,L] (got {tuple(reals.shape)} and "
                             f"{tuple(decoded.shape)})")
        fft_sizes, hop_sizes = [int(v) for v in fft_sizes], [int(v) for v in hop_sizes]
        win_lengths = list(fft_sizes) if win_lengths is None else [int(v) for v in win_lengths]
        if not len(fft_sizes) == len(hop_sizes) == len(win_lengths):
            raise ValueError("fft_sizes, hop_sizes and win_lengths must have the same length")   # auraloss.py:493
        if pit not in ("batch", "item", None):
            raise ValueError(f"pit must be 'batch', 'item' or None (got {pit!r})")
        B, n, L = reals.shape
        R = len(fft_sizes)
        if lens is not None:
            lens = check_lens(lens, B, L, (max(fft_sizes) // 2 + 1) if R else None,
                              " for the reflect padding of the largest FFT")
        cfg = DsnMrstftConfig(n_res=R, fft=(C.c_int * R)(*fft_sizes), hop=(C.c_int * R)(*hop_sizes),
                              win=(C.c_int * R)(*win_lengths), w_sc=float(w_sc), w_log_mag=float(w_log_mag),
                              w_lin_mag=float(w_lin_mag), taps=None, n_taps=0)
        if perceptual_weighting:
            from . import aweight
            t = aweight.taps(fs)
            ctaps = (C.c_float * len(t))(*t.tolist())
            cfg.taps, cfg.n_taps = ctaps, len(t)
        tabs = {k: torch.zeros((R, B, n, n) if k in ("sc", "log_mag", "lin_mag") else (B, n, n), dtype=torch.float64)
                for k in ("sc", "log_mag", "lin_mag", "l1", "l2")}
        out = DsnMrstftOut(**{k: C.cast(C.c_void_p(v.data_ptr()), C.POINTER(C.c_double)) for k, v in tabs.items()})
        if lens is None:
            self._check(self.lib.dsn_mrstft_loss(self.ctx, _ptr(reals), _ptr(decoded), B, n, L, C.byref(cfg),
                                                 C.byref(out), self._stream()), "dsn_mrstft_loss")
        else:
            self._check(self.lib.dsn_mrstft_loss_ragged(self.ctx, _ptr(reals), _ptr(decoded), (C.c_int32 * B)(*lens), B,
                                                        n, L, C.byref(cfg), C.byref(out), self._stream()),
                        "dsn_mrstft_loss_ragged")
        res = dict(tabs)
        res.update(mrstft_combine(tabs, w_sc=w_sc, w_log_mag=w_log_mag, w_lin_mag=w_lin_mag,
                                  mrstft_weight=mrstft_weight, l1_weight=l1_weight, l2_weight=l2_weight, pit=pit))
        return res

    def debug_read(self, name: str, shape):
        out = torch.empty(shape, dtype=torch.float32)
        self._check(self.lib.dsn_debug_read(self.ctx, name.encode(), C.c_void_p(out.data_ptr()), out.numel()),
                    f"dsn_debug_read({name})")
        return out

    def bench_igemm(self, B, Lin, Cin, N, taps=1, tap_dil=1, in_pad=0, ksplit=1, variant=2, iters=10):
        ms = C.c_double()
        self._check(self.lib.dsn_bench_igemm(self.ctx, B, Lin, Cin, N, taps, tap_dil, in_pad, ksplit, variant,
                                             iters, C.byref(ms)), "dsn_bench_igemm")
        return ms.value

    def test_igemm(self, a, w, *, taps=1, in_stride=1, tap_dil=1, in_pad=0, rows_per_b=None, panel_rows=0,
                   panel_bn=256):
        """a [B,Lin,Cin] channels-last, w [N, taps*Cin] -> [B, rows_per_b, N]: test_gemm with no epilogue, on the
        row-panel kernel (panel_bn = 128 | 256 columns) when panel_rows > 0, else on the engine's own choice."""
        a, w = _dev32(a, self.device), _dev32(w, self.device)
        B, Lin, Cin = a.shape
        N = w.shape[0]
        rpb = rows_per_b or Lin
        out = torch.empty((B, rpb, N), device=self.device, dtype=torch.float32)
        panel = dict(kernel="panel", panel_rows=panel_rows, panel_bn=panel_bn) if panel_rows > 0 else {}
        self.test_gemm(a, w, B=B, Lin=Lin, Cin=Cin, N=N, taps=taps, rows_per_b=rpb, in_stride=in_stride,
                       tap_dil=tap_dil, in_pad=in_pad, out_f32=out, **panel)
        return out

    # operand format of this context: (planes, fp16?) per precision code
    _PLANES = {PREC_BF16: (1, False), PREC_BF16X3: (2, False), PREC_FP16: (1, True), PREC_FP16X3: (2, True)}

    def test_gemm(self, a, w, *, kernel="auto", B, Lin, Cin, N, taps=1, rows_per_b=None, **kw):
        """Run one kernel of the implicit-GEMM family (dsn_test_gemm, include/ditsep_hip.h) on caller-owned fp32
        device tensors.  `a` is the whole input (a channel slice is addressed with in_row_elems / a_off), `w` is
        [N][taps*Cin].  Outputs (out_f32, out_planes as int16 [P][out_ps], slabs, gn_stats...) are written in place;
        every other keyword is the DsnTestGemm field of the same name (tensors are passed by pointer)."""
        t = DsnTestGemm()
        t.kernel = TEST_GEMM_KERNELS[kernel]
        t.B, t.Lin, t.Cin, t.N, t.taps = B, Lin, Cin, N, taps
        t.rows_per_b = Lin if rows_per_b is None else rows_per_b
        t.in_stride, t.tap_dil, t.out_scale = 1, 1, 1.0
        keep = [a, w]
        for name, tensor_like in (("a", a), ("w", w)):
            assert tensor_like.is_cuda and tensor_like.dtype == torch.float32 and tensor_like.is_contiguous(), name
        t.a, t.a_numel, t.w = a.data_ptr(), a.numel(), w.data_ptr()
        if w.numel() != N * taps * Cin:
            raise ValueError(f"w has {w.numel()} elements, N*taps*Cin = {N * taps * Cin}")
        for k, v in kw.items():
            if isinstance(v, torch.Tensor):
                assert v.is_cuda and v.is_contiguous(), k
                assert v.dtype == (torch.int16 if k == "out_planes" else torch.float32), k
                keep.append(v)
                setattr(t, k, v.data_ptr())
                if k == "sc_a":
                    t.sc_a_numel = v.numel()
                if k == "out_planes" and "out_ps" not in kw:
                    t.out_ps = v.shape[-1] if v.dim() > 1 else v.numel()
            elif v is not None:
                setattr(t, k, v)
        self._check(self.lib.dsn_test_gemm(self.ctx, C.byref(t), self._stream()), f"dsn_test_gemm({kernel})")

    def test_kernel(self, kind, **kw):
        """Run one launch wrapper of the non-GEMM kernels (dsn_test_kernel, include/ditsep_hip.h) on caller-owned device
        tensors.  Every keyword is the DsnTestKernel field of the same name; tensors are passed by pointer (fp32, but
        out_planes / in_planes int16 [P][out_ps / in_ps], out_fp8 / out_fp8_scale / in_fp8 / in_fp8_scale uint8 and lens,
        wtab and ftab int32), `a` / `w` / `w2` also set their _numel field."""
        t = DsnTestKernel()
        t.kind = TEST_KERNEL_KINDS[kind]
        keep = []
        dtypes = {"out_planes": torch.int16, "out_fp8": torch.uint8, "out_fp8_scale": torch.uint8, "lens": torch.int32,
                  "in_planes": torch.int16, "in_fp8": torch.uint8, "in_fp8_scale": torch.uint8, "wtab": torch.int32,
                  "ftab": torch.int32}
        for k, v in kw.items():
            if isinstance(v, torch.Tensor):
                assert v.is_cuda and v.dtype == dtypes.get(k, torch.float32), k
                assert v.is_contiguous() or k == "x", k      # (x may be a view into a wider buffer: its base pointer)
                keep.append(v)
                setattr(t, k, v.data_ptr())
                if k in ("a", "w", "w2"):
                    setattr(t, k + "_numel", v.numel())
                if k == "out_planes" and "out_ps" not in kw:
                    t.out_ps = v.shape[-1] if v.dim() > 1 else v.numel()
                if k == "in_planes" and "in_ps" not in kw:
                    t.in_ps = v.shape[-1] if v.dim() > 1 else v.numel()
            elif v is not None:
                setattr(t, k, v)
        self._check(self.lib.dsn_test_kernel(self.ctx, C.byref(t), self._stream()), f"dsn_test_kernel({kind})")

    def decode_planes(self, raw):
        """int16 operand planes [P][n] as written by a GEMM epilogue -> float64 values (hi, or hi + lo)."""
        P, f16 = self._PLANES[self.cfg.precision]
        raw = raw.reshape(P, -1)
        planes = [(raw[p].view(torch.float16) if f16 else raw[p].view(torch.bfloat16)).double() for p in range(P)]
        return planes[0] if P == 1 else planes[0] + planes[1]
