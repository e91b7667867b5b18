"""`LatentDiffSep`-shaped facade over the HIP engine (the drop-in boundary).

Mirrors the inference surface of the reference Lightning module
(reference src/diffsep_latent.py): `encode` :107-118, `decode` :120-128, `forward` :147-148,
`get_pc_sampler` :406-469, `separate` :471-487, and the forward half of its loss code -- `sample_time`,
`sample_prior`, `compute_score_loss`, `compute_score_loss_init_hack_pit`, `train_step_init_5` :130-208 and
`validation_step` :251-273 -- with the same config keys (`model.score_model`, `model.vae`, `model.sde`,
`model.t_eps`, `model.sampler`, `model.n_speakers`, `model.loss`, `model.init_hack`, `model.init_hack_p`,
`model.valid_max_sep_batches`) and the same state_dict naming (`score_model.*`, `vae.*`).
Gradients, training, EMA updates and logging are out of scope.
"""
from __future__ import annotations

import json
import math
from typing import Any, Mapping, Optional

import torch

from . import checkpoint, native, sdes


def _get(cfg: Any, path: str, default=None):
    cur = cfg
    for key in path.split("."):
        if cur is None:
            return default
        if isinstance(cur, Mapping):
            cur = cur.get(key, None)
        else:
            cur = getattr(cur, key, None)
    return default if cur is None else cur


def _vae_arch(vae_cfg) -> dict:
    """Read the Oobleck architecture from a stable-audio-tools model config (dict or JSON path;
    reference src/utils/load_stable_model.py:9-35, autoencoders.py:866-909)."""
    cfg = vae_cfg
    path = _get(vae_cfg, "config_path")
    if path is not None and _get(vae_cfg, "model") is None:
        with open(path) as fh:
            cfg = json.load(fh)
    enc = _get(cfg, "model.encoder.config")
    dec = _get(cfg, "model.decoder.config")
    if _get(cfg, "model.encoder.type", "oobleck") != "oobleck" or _get(cfg, "model.decoder.type", "oobleck") != "oobleck":
        raise NotImplementedError("only Oobleck encoders/decoders are implemented natively")
    if _get(cfg, "model.bottleneck.type", "vae") != "vae":
        raise NotImplementedError("only the VAE bottleneck is implemented natively")
    src = dec if dec is not None else enc
    return dict(vae_channels=int(_get(src, "channels", 128)), vae_c_mults=tuple(_get(src, "c_mults", (1, 2, 4, 8))),
                vae_strides=tuple(_get(src, "strides", (2, 4, 8, 8))),
                latent_dim=int(_get(cfg, "model.latent_dim", _get(dec, "latent_dim", 64))),
                vae_enc_latent_dim=int(_get(enc, "latent_dim", 128)) if enc is not None else 128,
                vae_use_snake=bool(_get(src, "use_snake", False)), vae_final_tanh=bool(_get(dec, "final_tanh", True)),
                vae_has_encoder=enc is not None, vae_has_decoder=dec is not None)


def loss_config(config, sde_N: int) -> dict:
    """The reference's reading of `model.loss`, `model.init_hack` and `model.init_hack_p`
    (src/diffsep_latent.py:66-67, :79-85) -> {"init_hack", "init_hack_p", "reduction"}.  Only torch.nn.MSELoss has a
    native reduction kernel: any other `_target_` raises NotImplementedError (no fallback).  A missing `model.loss`
    reads as MSELoss()."""
    init_hack = _get(config, "model.init_hack", False)
    init_hack_p = float(_get(config, "model.init_hack_p", 1.0 / sde_N))
    loss = _get(config, "model.loss")
    target = str(_get(loss, "_target_", "torch.nn.MSELoss"))
    if target not in ("torch.nn.MSELoss", "torch.nn.modules.loss.MSELoss"):
        raise NotImplementedError(f"model.loss._target_ = '{target}': the native score loss implements "
                                  "torch.nn.MSELoss only (no PyTorch fallback)")
    reduction = _get(loss, "reduction")
    if init_hack in (5, 6, 7):
        if reduction is None:
            reduction = "none"
        elif reduction != "none":
            raise ValueError("Reduction should 'none' for loss with init_hack == 5")     # reference :83
    elif reduction is None:
        reduction = "mean"
    if reduction not in ("none", "mean"):
        raise NotImplementedError(f"MSELoss(reduction='{reduction}') has no native kernel (none | mean)")
    return {"init_hack": init_hack, "init_hack_p": init_hack_p, "reduction": reduction}


_PRECISIONS = {"bf16": native.PREC_BF16, "bf16x3": native.PREC_BF16X3, "fp16": native.PREC_FP16,
               "fp16x3": native.PREC_FP16X3, "fp8": native.PREC_FP8}


class LatentDiffSep:
    """Native latent-diffusion separator.  `config` is the reference's Hydra tree (a nested dict or an
    OmegaConf object); `config.model.score_model._target_` selects the score network:
      * `...DiTScoreModel` / `...DiffusionTransformer`  DiT over latent tokens (kwargs embed_dim, depth,
        num_heads; io = n_speakers*latent, input_concat = latent)
      * `...LatentScoreModelNCSNpp`                      the NCSN++ latent U-Net the reference wires in
    """

    last_activity = None   # what the last call with activity= decided: one dict per item (Engine.activity_of)

    def __init__(self, config, device: int = 0, precision: str = "fp16"):
        self.config = config
        self.device_index = device
        n_src = int(_get(config, "model.n_speakers", 2))
        sm = _get(config, "model.score_model")
        target = str(_get(sm, "_target_", ""))
        args = dict(device=device, precision=_PRECISIONS[precision], n_src=n_src)
        if target.endswith("DiTScoreModel") or target.endswith("DiffusionTransformer"):
            args.update(score_kind=native.SCORE_DIT, dit_embed_dim=int(_get(sm, "embed_dim", 1024)),
                        dit_depth=int(_get(sm, "depth", 24)), dit_heads=int(_get(sm, "num_heads", 16)))
        elif target.endswith("LatentScoreModelNCSNpp"):
            ba = _get(sm, "backbone_args")
            attn = tuple(_get(ba, "attn_resolutions", (16,)))
            if len(attn) != 1:
                raise NotImplementedError("NCSN++: exactly one attention resolution is implemented natively")
            args.update(score_kind=native.SCORE_NCSNPP, ncsn_nf=int(_get(ba, "nf", 128)),
                        ncsn_ch_mult=tuple(_get(ba, "ch_mult", (1, 2, 2))),
                        ncsn_num_res_blocks=int(_get(ba, "num_res_blocks", 2)), ncsn_attn_resolution=int(attn[0]),
                        ncsn_image_size=int(_get(ba, "image_size", 64)),
                        ncsn_max_latent_length=int(_get(sm, "max_latent_length", 16)))
        elif target == "":
            args.update(score_kind=native.SCORE_NONE)
        else:
            raise ValueError(f"unknown score_model _target_ '{target}'")
        args.update(_vae_arch(_get(config, "model.vae")))
        self.sde = sdes.OUVESDE(theta=_get(config, "model.sde.theta", 1.5),
                                sigma_min=_get(config, "model.sde.sigma_min", 0.96),
                                sigma_max=_get(config, "model.sde.sigma_max", 10.0),
                                N=_get(config, "model.sde.N", 30))
        args.update(sde_theta=self.sde.theta, sde_sigma_min=self.sde.sigma_min, sde_sigma_max=self.sde.sigma_max)
        self.t_eps = float(_get(config, "model.t_eps", 0.03))
        self.t_max = self.sde.T
        self.n_src = n_src
        fs = _get(config, "model.fs")                   # the key the reference's CLI reads (src/inference/separate.py:141)
        self.fs = None if fs is None else int(fs)
        self.engine = native.Engine(**args)
        # the object `config.model.score_model._target_` names (reference diffsep_latent.py:39), bound to the engine
        from . import score_models
        if args["score_kind"] == native.SCORE_DIT:
            self.score_model = score_models.DiTScoreModel(embed_dim=args["dit_embed_dim"], depth=args["dit_depth"],
                                                          num_heads=args["dit_heads"]).bind(self.engine)
        elif args["score_kind"] == native.SCORE_NCSNPP:
            self.score_model = score_models.LatentScoreModelNCSNpp(
                num_sources=n_src, backbone_args=dict(_get(sm, "backbone_args", {}) or {}),
                max_latent_length=args["ncsn_max_latent_length"]).bind(self.engine)
        else:
            self.score_model = None
        self.max_len_lat = 0
        self._finalized = False
        lc = loss_config(config, self.sde.N)
        self.init_hack, self.init_hack_p, self.loss_reduction = lc["init_hack"], lc["init_hack_p"], lc["reduction"]
        self.valid_max_sep_batches = int(_get(config, "model.valid_max_sep_batches", 1))
        self.n_batches_est_done = 0

    # ------------------------------------------------------------------ weights
    def load_state_dict(self, state_dict, strict: bool = True):
        """Reference checkpoint naming: `score_model.*`, `vae.encoder.*`, `vae.decoder.*`
        (non-EMA parameters, as evaluate_latent.py:203-208 uses them)."""
        self.engine.load_state_dict(state_dict)
        # a missing tensor always raises; with strict (nn.Module's default, and what the reference's loaders use) so
        # does a tensor the configured network does not consume -- e.g. cross-attention / global-conditioning /
        # qk-norm weights of a DiT trained with other options, which would otherwise be silently ignored
        self.engine.finalize(strict=strict)
        self._finalized = True
        return self

    def load_checkpoint(self, ckpt, use_ema: bool = False):
        """Load a checkpoint written by the reference's training loop (reference src/diffsep_latent.py:341-392):
        `ckpt["state_dict"]` (`score_model.*`, `vae.*`, weight-norm `weight_g/weight_v`), `ckpt["ema"]`
        (torch_ema state: `shadow_params` in `parameters()` order -- of the whole module when
        `ckpt["trainable_vae"]`, else of `score_model` only) and `ckpt["trainable_vae"]`.
        `ckpt` is that dict or a path; a path is read with `torch.load(..., weights_only=True)` only (nothing
        in the file is executed; a checkpoint that loader refuses must be re-saved as plain tensors).
        `use_ema` selects the EMA weights now; `eval(no_ema=...)` switches later (reference :356-388)."""
        if not isinstance(ckpt, dict):
            ckpt = torch.load(str(ckpt), map_location="cpu", weights_only=True)
        if "state_dict" not in ckpt:
            raise KeyError("checkpoint has no 'state_dict'")
        raw = dict(ckpt["state_dict"])
        self._raw_state, self._ema_state = raw, None
        ema = ckpt.get("ema")
        if ema is not None:
            scope = "" if ckpt.get("trainable_vae", False) else "score_model."
            # by position in parameters() order, checked by count AND by the shape of every pair
            self._ema_state = {**raw, **checkpoint.match_ema(list(ema["shadow_params"]), raw, scope)}
        if use_ema and self._ema_state is None:
            raise ValueError("use_ema=True but the checkpoint has no 'ema' entry")   # reference: _error_loading_ema
        self._using_ema = bool(use_ema)
        return self.load_state_dict(self._ema_state if use_ema else raw)

    def to(self, device=None, *args, **kwargs):
        """nn.Module.to for the one thing it can mean here: the engine lives on the GPU it was created on.  The
        same device (or a dtype-only / no-op call) returns self; another device is refused loudly rather than
        silently ignored -- build a new LatentDiffSep(config, device=i) there instead."""
        if device is None or isinstance(device, torch.dtype):
            return self
        dev = torch.device(device)
        if dev.type == "cuda" and (dev.index is None or dev.index == self.device_index):
            return self
        raise RuntimeError(f"LatentDiffSep lives on cuda:{self.device_index}; cannot move it to {dev} "
                           "(create a new instance with device=<index>)")

    def train(self, mode: bool = True, no_ema: bool = False):
        """Reference semantics (src/diffsep_latent.py:356-388): eval mode swaps the EMA weights in unless
        `no_ema`; train mode restores the raw parameters.  Only meaningful after `load_checkpoint` with an
        'ema' entry; otherwise a no-op (as the reference behaves when the EMA failed to load)."""
        ema_state = getattr(self, "_ema_state", None)
        if ema_state is None:
            return self
        want = (not mode) and (not no_ema)
        if want != self._using_ema:
            self._using_ema = want
            self.load_state_dict(ema_state if want else self._raw_state)
        return self

    def eval(self, no_ema: bool = False):
        return self.train(False, no_ema=no_ema)

    @property
    def hop_length(self) -> int:
        return self.engine.hop_length

    # ------------------------------------------------------------------ reference surface
    @torch.no_grad()
    def encode(self, mix, target=None, vae_noise=None, seed=None, chunked=False, overlap=32, chunk_size=128):
        """reference src/diffsep_latent.py:107-118.  `seed=None` draws fresh posterior noise per call (as the
        reference's randn does); an int makes the draw reproducible."""
        if seed is None:
            seed = int(torch.randint(0, 2**31 - 2, (1,)).item())
        y = self.engine.encode(mix, vae_noise, seed=seed, chunked=chunked, overlap=overlap, chunk_size=chunk_size)
        self.max_len_lat = max(self.max_len_lat, y.shape[-1])
        if target is None:
            return y, None
        B, n, L = target.shape
        t = self.engine.encode(target.reshape(B * n, 1, L), None, seed=seed + 1)
        return y, t.reshape(B, n, *t.shape[2:])

    @torch.no_grad()
    def decode(self, est, target_dim=None, chunked=False, overlap=32, chunk_size=128):
        """reference src/diffsep_latent.py:120-128.  `chunked` / `overlap` / `chunk_size` (latent frames) select
        the VAE's long-form mode, AudioAutoencoder.decode_audio(..., chunked=True) (autoencoders.py:665-731)."""
        return self.engine.decode(est, target_dim, chunked=chunked, overlap=overlap, chunk_size=chunk_size)

    def forward(self, xt, time, mix):
        return self.engine.score(xt, time, mix)

    __call__ = forward

    def get_pc_sampler(self, predictor_name, corrector_name, y, N=None, minibatch=None, schedule=None, **kwargs):
        N = self.sde.N if N is None else N
        sde = self.sde.copy()
        sde.N = N
        kwargs = {"eps": self.t_eps, "n_spkrs": self.n_src, **kwargs}
        if schedule is not None:
            if minibatch is not None:
                raise NotImplementedError("minibatch + schedule")
            return sdes.get_pc_scheduled_sampler(predictor_name, corrector_name, sde=sde, score_fn=self, y=y,
                                                 schedule=schedule, **kwargs)
        if minibatch is None:
            return sdes.get_pc_sampler(predictor_name, corrector_name, sde=sde, score_fn=self, y=y, **kwargs)
        M = y.shape[0]
        noise = kwargs.pop("noise", None)
        seed = kwargs.pop("seed", None)

        def batched_sampling_fn():
            samples, ns = [], []
            for i in range(int(math.ceil(M / minibatch))):
                sl = slice(i * minibatch, (i + 1) * minibatch)
                nz = None if noise is None else noise[:, sl]
                # independent draws per minibatch, as the reference's successive randn calls give: an explicit seed
                # is offset by the minibatch index (the same seed would repeat one Philox stream in every minibatch)
                sampler = sdes.get_pc_sampler(predictor_name, corrector_name, sde=sde, score_fn=self, y=y[sl],
                                              noise=nz, seed=None if seed is None else int(seed) + i, **kwargs)
                s, n = sampler()
                samples.append(s)
                ns.append(n)
            return torch.cat(samples, dim=0), ns

        return batched_sampling_fn

    def get_ode_sampler(self, y, N=None, minibatch=1, **kwargs):
        """reference src/diffsep.py:697-725: the probability-flow ODE sampler (sdes.get_ode_sampler) with this model's
        SDE (N: the denoising step's dt = 1/N) and t_eps.  minibatch=None: the whole batch under one step-size
        controller; an integer splits the batch into independently integrated minibatches and returns
        (x, [nfe per minibatch]).  An explicit `seed` is offset by the minibatch index, as in get_pc_sampler;
        `noise` [B,n,D,T] is sliced per minibatch."""
        N = self.sde.N if N is None else N
        sde = self.sde.copy()
        sde.N = N
        kwargs = {"eps": self.t_eps, "n_spkrs": self.n_src, **kwargs}
        if minibatch is None:
            return sdes.get_ode_sampler(sde, self, y=y, **kwargs)
        M = y.shape[0]
        noise = kwargs.pop("noise", None)
        if noise is not None and noise.dim() == 5:
            noise = noise[0]
        seed = kwargs.pop("seed", None)

        def batched_sampling_fn():
            samples, ns = [], []
            for i in range(int(math.ceil(M / minibatch))):
                sl = slice(i * minibatch, (i + 1) * minibatch)
                sampler = sdes.get_ode_sampler(sde, self, y=y[sl], noise=None if noise is None else noise[sl],
                                               seed=None if seed is None else int(seed) + i, **kwargs)
                s, n = sampler()
                samples.append(s)
                ns.append(n)
            return torch.cat(samples, dim=0), ns

        return batched_sampling_fn

    # ------------------------------------------------------------------ audio at any sample rate
    def _model_rate(self, what: str) -> int:
        if self.fs is None:
            raise ValueError(f"{what} needs the model's sample rate: config.model.fs is missing")
        return self.fs

    @torch.no_grad()
    def preprocess_audio_for_encoder(self, audio, in_sr):
        """AudioAutoencoder.preprocess_audio_for_encoder (autoencoders.py:543-551): one clip -> [1, 1, Lpad]."""
        return self.preprocess_audio_list_for_encoder([audio], [in_sr])

    @torch.no_grad()
    def preprocess_audio_list_for_encoder(self, audio_list, in_sr_list):
        """AudioAutoencoder.preprocess_audio_list_for_encoder (autoencoders.py:553-594) for this mono model: a list of
        clips of different lengths, channel counts ([L], [C, L] or [1, C, L]) and sample rates (`in_sr_list`: an int
        or one rate per clip) -> [B, 1, Lpad] at `config.model.fs`, ready for `encode`.  Every clip is resampled on the
        device (Engine.resample: torchaudio.transforms.Resample's default filter; one call per distinct input rate and
        channel count, a mono clip already at the model's rate is copied), mixed down to mono, and zero-padded to
        Lpad = max_len + (hop - max_len % hop) % hop -- that function's rule, not utils.pad's.  The reference
        resamples every channel and then takes their mean; the mean is taken first here, which is the same sum."""
        fs = self._model_rate("preprocess_audio_list_for_encoder")
        if isinstance(in_sr_list, int):
            in_sr_list = [in_sr_list] * len(audio_list)
        if len(in_sr_list) != len(audio_list):
            raise ValueError("list of sample rates must be the same length of audio_list")      # reference :566
        rows = self.engine.to_model_rate(list(audio_list), list(in_sr_list), fs)
        hop = self.hop_length
        max_len = max(int(r.shape[-1]) for r in rows)
        out = torch.zeros((len(rows), 1, max_len + (hop - max_len % hop) % hop), device=self.engine.device,
                          dtype=torch.float32)
        for b, r in enumerate(rows):
            out[b, :, :r.shape[-1]] = r
        return out

    @torch.no_grad()
    def _separate_at_rate(self, mix, sample_rate, target_dim, kwargs, refine=None, activity=None, **ens):
        """`separate` of mix [B, C, L] (or [B, L]) at `sample_rate`: to the model's rate (mixed down), the existing
        call (with `refine` and the `samples` keywords `ens`, there), every estimate back to `sample_rate` and cropped
        to L."""
        fs, eng = self._model_rate("sample_rate="), self.engine
        mix = mix[:, None] if mix.dim() == 2 else mix
        L = int(mix.shape[-1])
        m = eng.resample(mix, sample_rate, fs, downmix=True)
        est, *others = self.separate(m, target_dim, refine=refine, activity=activity, **ens, **kwargs)
        return (eng.resample(est, fs, sample_rate)[..., :L], *others)

    # ------------------------------------------------------------------ multichannel stems (the `stems` keyword)
    @staticmethod
    def _fit(x, L):
        """x [..., L0] zero-extended or cut to L samples"""
        return torch.nn.functional.pad(x, (0, L - int(x.shape[-1]))) if int(x.shape[-1]) < L else x[..., :L]

    def _stems_refusals(self, sopts, channels, latent=False, intermediate=None):
        """What the `stems` keyword refuses, before any device work"""
        if latent:
            raise ValueError("stems= filters waveforms: with latent=True there is no mixture to filter")
        if intermediate:
            raise ValueError("stems= does not go with intermediate: the per-step states are not filtered")
        most = native.STEMS_MAX_CHANNELS[sopts["mode"]]
        for b, c in enumerate(channels):
            if c < 1 or c > most:
                raise ValueError(f"stems: item {b} has {c} channels, outside [1, {most}] for mode {sopts['mode']!r}")

    @torch.no_grad()
    def _separate_stems(self, mix, target_dim, sample_rate, sopts, mono_kw, kwargs):
        """`separate` with stems=: mix [B, C, L] -> the mono call on the downmix, Engine.stems against the channels at
        the model's rate (zero-extended or cut to the estimates' length), back to `sample_rate`"""
        eng = self.engine
        if not torch.is_tensor(mix) or mix.dim() != 3:
            raise ValueError(f"stems= takes mix [B, C, L] (got {tuple(getattr(mix, 'shape', ()))})")
        B, Cn, L = (int(v) for v in mix.shape)
        self._stems_refusals(sopts, [Cn], intermediate=kwargs.get("intermediate"))
        if sample_rate is None:
            mc = native._dev32(mix, eng.device)
            mono = native.downmix(mc)
        else:
            fs = self._model_rate("sample_rate=")
            mc, mono = eng.resample(mix, sample_rate, fs), eng.resample(mix, sample_rate, fs, downmix=True)
        est, *others = self.separate(mono, target_dim, **mono_kw, **kwargs)
        out = eng.stems(self._fit(mc, int(est.shape[-1])), est, **sopts)
        if sample_rate is not None:
            n, Le = int(out.shape[1]), int(out.shape[-1])
            out = eng.resample(out.reshape(B, n * Cn, Le), fs, sample_rate)[..., :L].reshape(B, n, Cn, L)
        return (out, *others)

    @torch.no_grad()
    def _stems_of_lists(self, clips, rates, sopts, run):
        """The list entry points with stems=: `clips` [C_b, L_b] each (or [L_b], [1, C_b, L_b]) at `rates` (None: the
        model's rate); run(list of mono [1, L'_b]) -> (list of [n, Le_b] estimates at the model's rate, *others).
        -> (list of [n, C_b, L_b] at each clip's own rate, *others)"""
        eng = self.engine
        clips = [c[None] if c.dim() == 1 else c[0] if c.dim() == 3 and c.shape[0] == 1 else c for c in clips]
        for b, c in enumerate(clips):
            if c.dim() != 2:
                raise ValueError(f"stems=: clip {b} must be [L], [C, L] or [1, C, L] (got {tuple(c.shape)})")
        self._stems_refusals(sopts, [int(c.shape[0]) for c in clips])
        if rates is None:
            mc = [native._dev32(c, eng.device) for c in clips]
            mono = [native.downmix(c[None])[0] for c in mc]
        else:
            fs = self._model_rate("sample_rates=")
            mc, mono = eng.to_model_rate(clips, rates, fs, downmix=False), eng.to_model_rate(clips, rates, fs)
        est, *others = run(mono)
        out = eng.stems([self._fit(m, int(e.shape[-1])) for m, e in zip(mc, est)], list(est), **sopts)
        if rates is not None:
            out = eng.stems_from_model_rate(out, rates, fs, [int(c.shape[-1]) for c in clips])
        return (out, *others)

    # ------------------------------------------------------------------ beamforming (the `beamform` keyword)
    def _beamform_refusals(self, bopts, channels, stems=None, latent=False, intermediate=None):
        """What the `beamform` keyword refuses, before any device work"""
        if stems is not None:
            raise ValueError("beamform= does not go with stems=: the beamformer returns one mono signal per source, "
                             "stems= the mixture's channels")
        if latent:
            raise ValueError("beamform= filters waveforms: with latent=True there is no mixture to filter")
        if intermediate:
            raise ValueError("beamform= does not go with intermediate: the per-step states are not filtered")
        ref, most = bopts["ref"], native.BEAMFORM_MAX_CHANNELS
        for b, c in enumerate(channels):
            if c < 1 or c > most:
                raise ValueError(f"beamform: item {b} has {c} channels, outside [1, {most}]")
            if isinstance(ref, bool) or int(ref) != ref or not 0 <= ref < c:
                raise ValueError(f"beamform: ref = {ref!r} outside [0, {c}): item {b} has {c} channels")

    @staticmethod
    def _spatial_refusals(spopts, bopts, stems=None, latent=False, intermediate=None):
        """What the `spatial` keyword refuses, before any device work -> the keywords of the beamforming step"""
        if stems is not None:
            raise ValueError("spatial= does not go with stems=: it refines the masks of the beamformer, which stems= "
                             "does not run")
        if latent:
            raise ValueError("spatial= refines the masks of waveforms: with latent=True there is no mixture to filter")
        if intermediate:
            raise ValueError("spatial= does not go with intermediate: the per-step states are not filtered")
        return native.spatial_beamform_keywords(bopts, spopts)

    @staticmethod
    def _track_refusals(tropts, bopts, spopts, stems=None, latent=False, intermediate=None):
        """What the `track` keyword refuses, before any device work"""
        if stems is not None:
            raise ValueError("track= does not go with stems=: it adapts the weights of the beamformer, which stems= "
                             "does not run")
        if latent:
            raise ValueError("track= adapts the filter of waveforms: with latent=True there is no mixture to filter")
        if intermediate:
            raise ValueError("track= does not go with intermediate: the per-step states are not filtered")
        native.track_beamform_keywords(bopts, tropts, None, spopts)

    def _beamform_step(self, mix, est, bopts, spopts, tropts=None):
        """The beamforming step of the entry points: Engine.beamform, with spatial= Engine.beamform_spatial, with track=
        Engine.beamform_track on blocks of tropts["block"] seconds at the model's rate"""
        if tropts is not None:
            return self.engine.beamform_track(mix, est, **native.track_beamform_keywords(
                bopts, tropts, self._model_rate("track="), spopts))
        if spopts is None:
            return self.engine.beamform(mix, est, **bopts)
        return self.engine.beamform_spatial(mix, est, **native.spatial_beamform_keywords(bopts, spopts))

    @staticmethod
    def _reference_channel(clips, ref):
        """clips [C_b, L_b] each -> channel `ref` of each as [1, L_b]"""
        return [c[ref:ref + 1].contiguous() for c in clips]

    @torch.no_grad()
    def _separate_beamform(self, mix, target_dim, sample_rate, bopts, mono_kw, kwargs, spopts=None, tropts=None,
                           aopts=None):
        """`separate` with beamform=: mix [B, C, L] -> the mono call on channel `ref`, Engine.beamform against all
        channels at the model's rate (zero-extended or cut to the estimates' length), back to `sample_rate`"""
        eng = self.engine
        if not torch.is_tensor(mix) or mix.dim() != 3:
            raise ValueError(f"beamform= takes mix [B, C, L] (got {tuple(getattr(mix, 'shape', ()))})")
        B, Cn, L = (int(v) for v in mix.shape)
        self._beamform_refusals(bopts, [Cn], intermediate=kwargs.get("intermediate"))
        if tropts is not None:
            self._model_rate("track=")
        if sample_rate is None:
            mc = native._dev32(mix, eng.device)
        else:
            fs = self._model_rate("sample_rate=")
            mc = eng.resample(mix, sample_rate, fs)
        one = mc[:, bopts["ref"]:bopts["ref"] + 1].contiguous()
        est, *others = self.separate(one, target_dim, **mono_kw, **kwargs)
        out = self._beamform_step(self._fit(mc, int(est.shape[-1])), est, bopts, spopts, tropts)
        if aopts is not None:
            out = self._activity_step(out, aopts)
        if sample_rate is not None:
            out = eng.resample(out, fs, sample_rate)[..., :L]
        return (out, *others)

    @staticmethod
    def _as_channel_clips(clips, what):
        clips = [c[None] if c.dim() == 1 else c[0] if c.dim() == 3 and c.shape[0] == 1 else c for c in clips]
        for b, c in enumerate(clips):
            if c.dim() != 2:
                raise ValueError(f"{what}=: clip {b} must be [L], [C, L] or [1, C, L] (got {tuple(c.shape)})")
        return clips

    @torch.no_grad()
    def _beamform_of_lists(self, clips, rates, bopts, run, spopts=None, tropts=None, aopts=None):
        """The list entry points with beamform=: `clips` [C_b, L_b] each (or [L_b], [1, C_b, L_b]) at `rates` (None:
        the model's rate); run(list of [1, L'_b], channel `ref` of each) -> (list of [n, Le_b] estimates at the model's
        rate, *others).  -> (list of [n, L_b] at each clip's own rate, *others)"""
        eng = self.engine
        clips = self._as_channel_clips(clips, "beamform")
        self._beamform_refusals(bopts, [int(c.shape[0]) for c in clips])
        if tropts is not None:
            self._model_rate("track=")
        if rates is None:
            mc = [native._dev32(c, eng.device) for c in clips]
        else:
            fs = self._model_rate("sample_rates=")
            mc = eng.to_model_rate(clips, rates, fs, downmix=False)
        est, *others = run(self._reference_channel(mc, bopts["ref"]))
        out = self._beamform_step([self._fit(m, int(e.shape[-1])) for m, e in zip(mc, est)], list(est), bopts, spopts,
                                  tropts)
        if aopts is not None:
            out = self._activity_step(out, aopts)
        if rates is not None:
            out = eng.from_model_rate(out, rates, fs, [int(c.shape[-1]) for c in clips])
        return (out, *others)

    # ------------------------------------------------------------------ dereverberation (the `dereverb` keyword)
    def _dereverb_refusals(self, dopts, shapes, rates=None, latent=False, intermediate=None):
        """What the `dereverb` keyword refuses, before any device work: `shapes` is one (channels, samples) per item,
        `rates` None (the model's rate) or one rate per item"""
        if latent:
            raise ValueError("dereverb= filters waveforms: with latent=True there is no mixture to filter")
        if intermediate:
            raise ValueError("dereverb= does not go with intermediate: the per-step states are not filtered")
        most, need = native.DEREVERB_MAX_CHANNELS, int(dopts["n_fft"]) // 2 + 1
        fs = None if rates is None else self._model_rate("dereverb=")
        for b, (c, v) in enumerate(shapes):
            if c < 1 or c > most:
                raise ValueError(f"dereverb: item {b} has {c} channels, outside [1, {most}]")
            at = v if rates is None else native.resample_length(int(rates[b]), fs, v)
            if at < need:
                raise ValueError(f"dereverb: item {b} has {at} samples at the model's rate; dereverb= needs at least "
                                 f"n_fft / 2 + 1 = {need}")

    @torch.no_grad()
    def _separate_dereverb(self, mix, target_dim, sample_rate, dopts, inner_kw, kwargs):
        """`separate` with dereverb=: mix [B, C, L] (or mono [B, L]) to the model's rate with its channels kept,
        Engine.dereverb, the existing call there -- on native.downmix of the result, or on its channels with stems= or
        beamform= --, the outputs back to `sample_rate`"""
        eng = self.engine
        if not torch.is_tensor(mix) or mix.dim() not in (2, 3):
            raise ValueError(f"dereverb= takes mix [B, C, L] or [B, L] (got {tuple(getattr(mix, 'shape', ()))})")
        m3 = mix[:, None] if mix.dim() == 2 else mix
        B, Cn, L = (int(v) for v in m3.shape)
        self._dereverb_refusals(dopts, [(Cn, L)], None if sample_rate is None else [sample_rate],
                                intermediate=kwargs.get("intermediate"))
        if sample_rate is None:
            mc = native._dev32(m3, eng.device)
        else:
            fs = self._model_rate("sample_rate=")
            mc = eng.resample(m3, sample_rate, fs)
        dry = eng.dereverb(mc, **dopts)
        keep = inner_kw.get("stems") is not None or inner_kw.get("beamform") is not None
        est, *others = self.separate(dry if keep else native.downmix(dry), target_dim, **inner_kw, **kwargs)
        if sample_rate is not None:
            lead = tuple(est.shape[:-1])
            est = eng.resample(est.reshape(B, -1, int(est.shape[-1])), fs, sample_rate)[..., :L].reshape(*lead, L)
        return (est, *others)

    @torch.no_grad()
    def _dereverb_of_lists(self, clips, rates, dopts, keep, run):
        """The list entry points with dereverb=: `clips` [C_b, L_b] each (or [L_b], [1, C_b, L_b]) at `rates` (None:
        the model's rate); every clip is dereverberated whole at the model's rate (one Engine.dereverb call), and
        run(list) -- of the results' downmixes [1, L'_b], or with `keep` (stems=, beamform=) of their channels
        [C_b, L'_b] -- gives (the list of outputs at the model's rate, *others).  -> (the outputs at each clip's own
        rate and sample count, *others)"""
        eng = self.engine
        clips = self._as_channel_clips(clips, "dereverb")
        self._dereverb_refusals(dopts, [(int(c.shape[0]), int(c.shape[-1])) for c in clips], rates)
        if rates is None:
            mc = [native._dev32(c, eng.device) for c in clips]
        else:
            fs = self._model_rate("sample_rates=")
            mc = eng.to_model_rate(clips, rates, fs, downmix=False)
        dry = eng.dereverb(mc, **dopts)
        out, *others = run(list(dry) if keep else [native.downmix(d[None])[0] for d in dry])
        if rates is not None:
            back = eng.stems_from_model_rate if out[0].dim() == 3 else eng.from_model_rate
            out = back(list(out), rates, fs, [int(c.shape[-1]) for c in clips])
        return (out, *others)

    # ------------------------------------------------------------------ speaker activity (the `activity` keyword)
    @staticmethod
    def _activity_refusals(aopts, stems=None, latent=False, intermediate=None):
        """What the `activity` keyword refuses, before any device work"""
        if stems is not None:
            raise ValueError("activity= does not go with stems=: it decides on mono estimates, stems= returns the "
                             "mixture's channels (no gate for stems)")
        if latent:
            raise ValueError("activity= decides on waveforms: with latent=True there is nothing to frame")
        if intermediate:
            raise ValueError("activity= does not go with intermediate: the per-step states are not decided on")

    def _activity_step(self, est, aopts):
        """The activity step of the entry points, on the final mono estimates at the model's rate: est [B, n, L] or a
        list of [n, L_b] (one padded Engine.activity call with the items' lengths) -> the same, gated when the options
        say so; leaves self.last_activity, one dict per item (Engine.activity_of)"""
        eng, fs = self.engine, self._model_rate("activity=")
        if torch.is_tensor(est):
            out, self.last_activity = eng.activity_of(est, aopts, fs)
            return out
        ln = [int(e.shape[-1]) for e in est]
        ep = torch.zeros((len(est), int(est[0].shape[0]), max(ln)), device=eng.device, dtype=torch.float32)
        for b, e in enumerate(est):
            ep[b, :, :ln[b]] = e
        out, self.last_activity = eng.activity_of(ep, aopts, fs, lens=ln)
        return list(est) if out is ep else [out[b, :, :ln[b]] for b in range(len(est))]

    # ------------------------------------------------------------------ loudness (the `loudness` keyword)
    def _loudness_refusals(self, lopts, channels, latent=False, intermediate=None):
        """What the `loudness` keyword refuses, before any device work"""
        if latent:
            raise ValueError("loudness= measures waveforms: with latent=True there is nothing to measure")
        if intermediate:
            raise ValueError("loudness= does not go with intermediate: the per-step states are not normalised")
        most = native.LOUDNESS_MAX_CHANNELS
        for b, c in enumerate(channels):
            if lopts["link"] == "mixture" and lopts["target"] is not None and (c < 1 or c > most):
                raise ValueError(f"loudness: mixture {b} has {c} channels, outside [1, {most}] (every channel has "
                                 f"weight 1: no surround weights; link='stem' measures the stems instead)")

    @staticmethod
    def _clip_channels(c):
        """channel count of a clip given as [L], [C, L] or [1, C, L]"""
        return 1 if c.dim() == 1 else int(c.shape[-2])

    def _normalise(self, lopts, sources, ests, rates, others, return_info, inner_info):
        """The last step of the entry points with loudness=: Engine.loudness_normalize on the lists, and the info dict
        merged into the combine's (inner_info) or appended (return_info alone)"""
        src = None
        if lopts["link"] == "mixture" and lopts["target"] is not None:
            src = [m[None] if m.dim() == 1 else m.reshape(-1, m.shape[-1]) for m in sources]
        outs, info = self.engine.loudness_normalize(src, list(ests), rates, **lopts)
        others = list(others)
        if inner_info:
            others[-1] = dict(others[-1], **info)
        elif return_info:
            others.append(info)
        return outs, others

    @torch.no_grad()
    def separate(self, mix, target_dim=None, latent=False, sample_rate=None, refine=None, samples=None, combine="mean",
                 return_info=False, stems=None, loudness=None, limit=None, beamform=None, dereverb=None, spatial=None,
                 track=None, activity=None, design=None, **kwargs):
        """reference src/diffsep_latent.py:471-487.  sample_rate (default None: mix is mono at the model's rate, the
        call is what it was): the rate of `mix` [B, C, L] -- it is resampled to config.model.fs on the device and mixed
        down, separated (target_dim keeps its meaning at the model's rate), and the estimates come back at
        `sample_rate`, cropped to L.
        refine (default None: the decoder's output is returned as it is): None, True or "mask" (Engine.mask_refine
        with native.MASK_REFINE_DEFAULTS) or a dict of n_fft / hop / power / eps -- the estimates are refined against
        the mono mixture at the model's rate after the decoder and before any resampling back.  Where the estimates
        are longer than the mixture (without target_dim the codec hands back whole hops) the mixture is zero-extended
        to their length, which is what the encoder saw; shorter estimates are refused.  Refused with latent=True:
        there is no waveform mixture.
        samples (default None: one draw, the call is what it was): K in [1, 16] -- every mixture is repeated K times
        item-major (row b K + k) and goes through this call once under the one seed (the device generator gives every
        batch row its own draws; explicit vae_noise / noise then have B K rows), and the K candidates of each mixture
        are aligned and combined on the device (Engine.ensemble_combine, combine = "mean", "median", "best" or
        "medoid") against the mono mixture at the model's rate, zero-extended or cut to the estimates' length --
        after the decoder and before refine and any resampling back.  return_info=True appends the info dict of
        Engine.ensemble_combine to what is returned.  Refused with latent=True and with intermediate.
        stems (default None: the call is what it was): "mask", "wiener" or a dict of mode / n_fft / hop / power / eps /
        reg (native.stems_options) -- mix is then [B, C, L] and [B, n, C, L] comes back: the call above runs on the
        downmix ((x_0 + .. + x_{C-1}) / C), and Engine.stems filters the mixture's channels at the model's rate (the
        channels resampled without downmix, zero-extended or cut to the estimates' length) with the mono estimates,
        after combine and refine and before the resampling back.  The stems of a channel sum to that channel; nothing
        above the model's Nyquist frequency comes back.  Refused with latent=True and with intermediate.
        loudness (default None: the call returns the bits it returned before): True, a target in LUFS or a dict of
        target / peak / link (native.loudness_options; -23 LUFS, a true-peak ceiling of -1 dBTP, link "mixture") --
        the last step, after combine, refine, stems and the resampling back, at the rate the estimates come back at:
        the programme loudness (ITU-R BS.1770-4 / EBU R 128) and the true peak are measured on the device
        (Engine.loudness) and every estimate is multiplied by one gain (Engine.apply_gain; a gain, not a limiter).
        link "mixture": the gain source is the mixture as it was given, all its channels (at most two) at its own
        rate, and all stems of an item share the gain g that brings the mixture to the target -- held back so that no
        stem's true peak passes the ceiling --, so stems that summed to the mixture sum to g mixture.  link "stem":
        every stem is brought to the target by itself.  A source that passes no gating block stays at 0 dB.
        return_info=True (allowed without samples= then) appends, or merges into the combine's info, "loudness_in",
        "loudness_out", "gain_db", "true_peak_db" (one list of n per item), "limited", "silent", "nonfinite".  Refused
        with latent=True and with intermediate.
        limit (default None: the call returns the bits it returned before): True or a dict of ceiling / lookahead_ms /
        drive_db / iterations / tol (native.limit_options) -- the true-peak look-ahead limiter (Engine.limiter_curve /
        apply_curve) as part of that last step: an item whose target the ceiling forbids to a single gain is driven
        harder and only the neighbourhood of its peaks is lowered, until the limited programme measures the target
        within tol (Engine.loudness_normalize states the loop); an item the single gain brings to the target keeps
        its bits.  With link "mixture" the stems share the curve g[t], so stems that summed to the mixture sum to
        g[t] G mixture[t].  Without loudness= every item goes once
        through the limiter at 0 dB against the ceiling (default -1 dBTP).  The info gains "reached", "evaluations",
        "reduction_db" and "limited_samples".  Refused where loudness= is.
        beamform (default None: the call returns the bits it returned before): True, an int (the reference channel) or
        a dict of ref / n_fft / hop / power / eps / reg / postfilter (native.beamform_options) -- mix is then a
        microphone-array recording [B, C, L] (C <= 8) and [B, n, L] comes back: the call above runs on channel `ref`
        (not on the downmix), and Engine.beamform filters all channels at the model's rate (resampled with the
        channels kept, zero-extended or cut to the estimates' length) towards every source with a mask-based MVDR
        beamformer, after combine and refine and before the resampling back, loudness and limit, which see mono
        estimates as they do without the keyword; loudness with link "mixture" measures channel `ref`.  One filter
        per recording; not a trained step.  Refused together with stems=, with latent=True and with intermediate.
        dereverb (default None: the call returns the bits it returned before): True or a dict of taps / delay /
        iterations / n_fft / hop / reg / eps (native.dereverb_options) -- the first waveform step: mix [B, C, L]
        (C <= 8; mono [B, L] is one channel) goes to the model's rate with its channels kept, Engine.dereverb removes
        the late reverberation (WPE, one filter per recording), and the call above runs on the result at the model's
        rate with every other keyword: on native.downmix of the dereverberated channels, or -- with stems= or
        beamform= -- on the channels themselves; the outputs go back to `sample_rate`.  loudness / limit stay the
        last step and link "mixture" keeps measuring `mix` as given.  Not a trained step; its effect on separation
        quality is unmeasured.  Refused with latent=True, with intermediate, with more than 8 channels and with an
        item shorter than n_fft / 2 + 1 samples at the model's rate.
        spatial (default None: the call returns the bits it returned before): True or a dict of iterations / noise /
        floor / reg / eps (native.spatial_options) -- only together with beamform=: the beamforming step is then
        Engine.beamform_spatial, whose guided cACGMM refines the masks that weight the beamformer's statistics, in the
        same place and on the same inputs.  Not trained and not tuned.  Refused without beamform=, with its
        postfilter "mask", with stems=, with latent=True and with intermediate.
        track (default None: the call returns the bits it returned before): True, a block length in seconds or a dict
        of block / context / interpolate (native.track_options; 0.8 s, 1, True -- not tuned) -- only together with
        beamform=: the beamforming step is then Engine.beamform_track, in the same place and on the same inputs: one
        MVDR filter per block of max(4, round(block fs / hop)) frames at the model's rate, solved on the blocks within
        `context` of it and interpolated between the blocks' centres, so the filter follows a speaker who moves.
        Blocks of fixed length; not a trained step.  Refused without beamform=, with spatial= (the cACGMM sums its
        statistics inside its solve workgroup; cutting those per block is a separate piece of work), with stems=, with
        latent=True and with intermediate.
        activity (default None: the call is what it was): None, True (segments only), "gate" or a dict of
        native.ACTIVITY_DEFAULTS' keys (native.activity_options; seconds, Hz and dB, not tuned) -- Engine.activity decides
        per source and STFT frame where a stem carries its speaker, on the final mono estimates at the model's rate:
        after samples / combine, refine and beamform (with or without spatial / track) and before the resampling back,
        loudness and limit.  What is returned is what was returned, with gate=True after Engine.activity_gate (the
        stretches outside a stem's segments become digital silence); self.last_activity holds per item the segments
        per source in samples at the model's rate and in seconds, the active seconds, frames_on and the options.  A
        decision rule, not a trained detector.  Refused with stems=, latent=True and with intermediate.
        design (default None: the call returns the bits it returned before): "rank1", "gev", "souden" or a dict of
        kind / sweeps (native.design_options; "rank1", 10 -- not tuned) -- only together with beamform=: whichever of
        Engine.beamform, beamform_spatial and beamform_track runs the beamforming step gets design=, in the same place
        and on the same inputs: the rank-one MVDR filter from the principal generalised eigenvector of (N_i, Q_i +
        lambda I), or the GEV (max-SNR) filter with blind analytic normalisation, which is not distortionless.
        Combines with spatial=, track=, dereverb=, activity=, loudness= and limit= as beamform= does.  Refused without
        beamform= and wherever beamform= is (stems=, latent=True, intermediate)."""
        dopts = native.dereverb_options(dereverb)
        if dopts is not None and (latent or kwargs.get("intermediate")):
            self._dereverb_refusals(dopts, [], latent=latent, intermediate=kwargs.get("intermediate"))
        bopts, spopts = native.beamform_options(beamform), native.spatial_options(spatial)
        bopts = native.design_beamform_keywords(bopts, native.design_options(design))
        if spopts is not None:
            self._spatial_refusals(spopts, bopts, stems=stems, latent=latent, intermediate=kwargs.get("intermediate"))
        tropts = native.track_options(track)
        if tropts is not None:
            self._track_refusals(tropts, bopts, spopts, stems=stems, latent=latent,
                                 intermediate=kwargs.get("intermediate"))
        if bopts is not None:
            chans = [int(mix.shape[1])] if torch.is_tensor(mix) and mix.dim() == 3 else []
            self._beamform_refusals(bopts, chans, stems=stems, latent=latent, intermediate=kwargs.get("intermediate"))
        aopts = native.activity_options(activity)
        if aopts is not None:
            self._activity_refusals(aopts, stems=stems, latent=latent, intermediate=kwargs.get("intermediate"))
        lopts = native.level_options(loudness, limit)
        if lopts is not None:
            chans = [int(mix.shape[1])] if torch.is_tensor(mix) and mix.dim() == 3 and bopts is None else [1]
            self._loudness_refusals(lopts, chans, latent=latent, intermediate=kwargs.get("intermediate"))
            rate = self._model_rate("loudness=") if sample_rate is None else int(sample_rate)
            inner = bool(return_info) and samples is not None
            est, *others = self.separate(mix, target_dim, sample_rate=sample_rate, refine=refine, samples=samples,
                                         combine=combine, return_info=inner, stems=stems, beamform=beamform,
                                         dereverb=dereverb, spatial=spatial, track=track, activity=activity,
                                         design=design, **kwargs)
            B = int(est.shape[0])
            m3 = mix[:, None] if mix.dim() == 2 else mix
            if bopts is not None:
                m3 = m3[:, bopts["ref"]:bopts["ref"] + 1]
            outs, others = self._normalise(lopts, [m3[b] for b in range(B)], [est[b] for b in range(B)], rate, others,
                                           return_info, inner)
            return (torch.stack(outs), *others)
        if dopts is not None:
            inner_kw = dict(refine=refine, samples=samples, combine=combine, return_info=return_info, stems=stems,
                            beamform=beamform, spatial=spatial, track=track, activity=activity, design=design)
            return self._separate_dereverb(mix, target_dim, sample_rate, dopts, inner_kw, kwargs)
        sopts = native.stems_options(stems)
        if sopts is not None:
            self._stems_refusals(sopts, [], latent=latent, intermediate=kwargs.get("intermediate"))
            mono_kw = dict(refine=refine, samples=samples, combine=combine, return_info=return_info)
            return self._separate_stems(mix, target_dim, sample_rate, sopts, mono_kw, kwargs)
        if bopts is not None:
            mono_kw = dict(refine=refine, samples=samples, combine=combine, return_info=return_info)
            return self._separate_beamform(mix, target_dim, sample_rate, bopts, mono_kw, kwargs, spopts, tropts, aopts)
        ens = {}
        if samples is not None:
            ens = dict(samples=native.check_samples(samples, combine), combine=combine, return_info=return_info)
            if latent:
                raise ValueError("samples= combines waveforms: with latent=True there is nothing to decode (combine "
                                 "flattened latents with Engine.ensemble_combine)")
            if kwargs.get("intermediate"):
                raise ValueError("samples= does not go with intermediate: the per-step states are not combined")
        elif return_info:
            raise ValueError("return_info=True hands back the info of the combine: it needs samples=")
        opts = native.refine_options(refine)
        if opts is not None and latent:
            raise ValueError("refine= applies to waveforms: with latent=True there is no waveform mixture to refine "
                             "against")
        if sample_rate is not None:
            if latent:
                raise ValueError("sample_rate= applies to waveforms: a latent has no sample rate to convert")
            return self._separate_at_rate(mix, sample_rate, target_dim, kwargs, refine=refine, activity=activity, **ens)
        if aopts is not None:
            est, *others = self.separate(mix, target_dim, refine=refine, **ens, **kwargs)
            return (self._activity_step(est, aopts), *others)
        if opts is not None:
            est, *others = self.separate(mix, target_dim, **ens, **kwargs)
            short = int(est.shape[-1]) - int(mix.shape[-1])
            if short < 0:
                raise ValueError(f"refine=: the estimates ({est.shape[-1]} samples) are shorter than the mixture "
                                 f"({mix.shape[-1]}); target_dim must not cut the mixture")
            return (self.engine.mask_refine(torch.nn.functional.pad(mix, (0, short)), est, **opts), *others)
        if ens:
            B, K = int(mix.shape[0]), ens["samples"]
            est, *others = self.separate(mix.repeat_interleave(K, 0), target_dim, **kwargs)
            Le = int(est.shape[-1])
            m = mix.reshape(B, -1)[:, :Le].to(device=est.device, dtype=torch.float32)
            m = torch.nn.functional.pad(m, (0, Le - int(m.shape[-1])))
            res = self.engine.ensemble_combine(est.reshape(B, K, -1, Le), m, mode=combine, return_info=return_info)
            return (res[0], *others, res[1]) if return_info else (res, *others)
        if not latent:
            # the reference draws fresh VAE posterior noise on every call (bottleneck.py:57-83): without an explicit
            # seed, so does this (an explicit seed makes the whole call reproducible)
            seed = kwargs.get("seed")
            enc_seed = int(torch.randint(0, 2**31 - 1, (1,)).item()) if seed is None else int(seed)
            mix, _ = self.encode(mix, None, vae_noise=kwargs.pop("vae_noise", None), seed=enc_seed)
        sampler_kwargs = dict(_get(self.config, "model.sampler", {}) or {})
        sampler_kwargs.update(kwargs)
        sampler = self.get_pc_sampler("reverse_diffusion", "ald", mix, **sampler_kwargs)
        est, *others = sampler()
        est = self.decode(est, target_dim)
        return (est, *others)

    @torch.no_grad()
    def separate_batch(self, mixes, target_dims=None, codec="grouped", sample_rates=None, refine=None, samples=None,
                       combine="mean", return_info=False, stems=None, loudness=None, limit=None, beamform=None,
                       dereverb=None, spatial=None, track=None, activity=None, design=None, **sampler_kwargs):
        """Mixtures of different lengths in one batch (DiT score network): `mixes` is a list of [1, L_b] tensors ->
        (list of [n, target_dims[b] or L_b] estimates, *what the sampler returns besides).  Every item gets what
        `separate` gives it alone: the codec runs per group of equal latent frame count, the sampler once on the
        batch padded to the longest item with the score network masking each item's keys at its own length.
        Keywords as `separate` (seed, vae_noise: list of [D, T_b], noise [draws,B,n,D,Tmax], N, snr, ...).
        codec="padded": encoder and decoder run once on the padded batch as well (Engine.encode_ragged /
        decode_ragged); per item the same result up to summation order, other device-RNG VAE draws.
        sample_rates (default None: every mixture is mono at the model's rate, the call is what it was): an int or one
        rate per item; the mixtures may then be [L], [C, L] or [1, C, L].  They are resampled to config.model.fs on the
        device (Engine.to_model_rate: mixed down, one call per distinct rate), separated as above -- target_dims,
        vae_noise and noise keep their meaning at the model's rate -- and every estimate comes back at its item's own
        rate, cropped to the item's sample count (Engine.from_model_rate).
        refine (default None: off), as in `separate`: one Engine.mask_refine call on the padded batch with the items'
        lengths, at the model's rate, before any resampling back; each item gets the bits it gets alone.
        samples (default None: one draw), combine, return_info as in `separate`: every mixture is repeated K times
        item-major, the B K rows go through this call once, and one Engine.ensemble_combine call on the padded
        candidates with the items' lengths combines them against the mixtures, before refine and resampling back.
        stems (default None: off), as in `separate`: the mixtures are [C_b, L_b] (mixed channel counts are fine), the
        call runs on their downmixes, one Engine.stems call on the padded batch filters every item's own channels at
        the model's rate, and a list of [n, C_b, L_b] comes back, each item with the bits it gets alone.
        loudness (default None: off), as in `separate`: the last step, one Engine.loudness call on the padded mixtures
        as they were given (each at its own rate, with its own channels), one on the padded estimates, one
        Engine.apply_gain call; each item gets the gain it gets alone.
        limit (default None: off), as in `separate`: the items the ceiling holds back go through the limiter's loop
        together, each with the pre-gains and the curve it gets alone.
        beamform (default None: off), as in `separate`: the mixtures are array recordings [C_b, L_b] (mixed channel
        counts are fine), the call runs on channel `ref` of each, one Engine.beamform call on the padded batch filters
        every item's own channels at the model's rate, and a list of [n, L_b] comes back, each item with the bits it
        gets alone.
        dereverb (default None: off), as in `separate`: the mixtures are [C_b, L_b] (or [L_b]; mixed channel counts
        are fine), one Engine.dereverb call on the padded batch dereverberates every item at the model's rate, the
        call above runs on the results there, and the outputs go back to every item's own rate and sample count.
        spatial (default None: off), as in `separate`: with beamform=, one Engine.beamform_spatial call on the padded
        batch in place of Engine.beamform.
        track (default None: off), as in `separate`: with beamform=, one Engine.beamform_track call on the padded batch
        in place of Engine.beamform; every item has its own number of blocks.
        activity (default None: off), as in `separate`: one Engine.activity call (and with gate=True one
        Engine.activity_gate call) on the padded batch with the items' lengths at the model's rate; each item gets the
        bits it gets alone, and last_activity holds one entry per item.
        design (default None: off), as in `separate`: with beamform=, the one beamforming call on the padded batch gets
        design=."""
        eng = self.engine
        dopts = native.dereverb_options(dereverb)
        if dopts is not None and sampler_kwargs.get("intermediate"):
            self._dereverb_refusals(dopts, [], intermediate=sampler_kwargs.get("intermediate"))
        bopts, spopts = native.beamform_options(beamform), native.spatial_options(spatial)
        bopts = native.design_beamform_keywords(bopts, native.design_options(design))
        if spopts is not None:
            self._spatial_refusals(spopts, bopts, stems=stems, intermediate=sampler_kwargs.get("intermediate"))
        tropts = native.track_options(track)
        if tropts is not None:
            self._track_refusals(tropts, bopts, spopts, stems=stems, intermediate=sampler_kwargs.get("intermediate"))
        if bopts is not None:
            mixes = self._as_channel_clips(list(mixes), "beamform")
            self._beamform_refusals(bopts, [int(m.shape[0]) for m in mixes], stems=stems,
                                    intermediate=sampler_kwargs.get("intermediate"))
        aopts = native.activity_options(activity)
        if aopts is not None:
            self._activity_refusals(aopts, stems=stems, intermediate=sampler_kwargs.get("intermediate"))
        lopts = native.level_options(loudness, limit)
        if lopts is not None:
            mixes = list(mixes)
            sources = mixes if bopts is None else self._reference_channel(mixes, bopts["ref"])
            self._loudness_refusals(lopts, [self._clip_channels(m) for m in sources],
                                    intermediate=sampler_kwargs.get("intermediate"))
            rates = self._model_rate("loudness=") if sample_rates is None else sample_rates
            inner = bool(return_info) and samples is not None
            est, *others = self.separate_batch(mixes, target_dims, codec, sample_rates=sample_rates, refine=refine,
                                               samples=samples, combine=combine, return_info=inner, stems=stems,
                                               beamform=beamform, dereverb=dereverb, spatial=spatial, track=track,
                                               activity=activity, design=design, **sampler_kwargs)
            outs, others = self._normalise(lopts, sources, est, rates, others, return_info, inner)
            return (outs, *others)
        if dopts is not None:
            rates = sample_rates
            if rates is not None:
                rates = [int(rates)] * len(mixes) if isinstance(rates, int) else [int(r) for r in rates]
            return self._dereverb_of_lists(list(mixes), rates, dopts, stems is not None or bopts is not None,
                                           lambda at_fs: self.separate_batch(
                at_fs, target_dims, codec, refine=refine, samples=samples, combine=combine, return_info=return_info,
                stems=stems, beamform=beamform, spatial=spatial, track=track, activity=activity, design=design,
                **sampler_kwargs))
        sopts = native.stems_options(stems)
        if sopts is not None:
            self._stems_refusals(sopts, [], intermediate=sampler_kwargs.get("intermediate"))
            rates = sample_rates
            if rates is not None:
                rates = [int(rates)] * len(mixes) if isinstance(rates, int) else [int(r) for r in rates]
            return self._stems_of_lists(list(mixes), rates, sopts, lambda mono: self.separate_batch(
                mono, target_dims, codec, refine=refine, samples=samples, combine=combine, return_info=return_info,
                **sampler_kwargs))
        if bopts is not None:
            rates = sample_rates
            if rates is not None:
                rates = [int(rates)] * len(mixes) if isinstance(rates, int) else [int(r) for r in rates]
            return self._beamform_of_lists(mixes, rates, bopts, lambda one: self.separate_batch(
                one, target_dims, codec, refine=refine, samples=samples, combine=combine, return_info=return_info,
                **sampler_kwargs), spopts, tropts, aopts)
        ens = {}
        if samples is not None:
            ens = dict(samples=native.check_samples(samples, combine), combine=combine, return_info=return_info)
            if sampler_kwargs.get("intermediate"):
                raise ValueError("samples= does not go with intermediate: the per-step states are not combined")
        elif return_info:
            raise ValueError("return_info=True hands back the info of the combine: it needs samples=")
        opts = native.refine_options(refine)
        if sample_rates is not None:
            fs = self._model_rate("sample_rates=")
            rates = [int(sample_rates)] * len(mixes) if isinstance(sample_rates, int) else [int(r) for r in sample_rates]
            at_fs = eng.to_model_rate(list(mixes), rates, fs)
            est, *others = self.separate_batch(at_fs, target_dims, codec, refine=refine, activity=activity, **ens,
                                               **sampler_kwargs)
            return (eng.from_model_rate(est, rates, fs, [int(m.shape[-1]) for m in mixes]), *others)
        if aopts is not None:
            est, *others = self.separate_batch(mixes, target_dims, codec, refine=refine, **ens, **sampler_kwargs)
            return (self._activity_step(est, aopts), *others)
        if opts is not None:
            est, *others = self.separate_batch(mixes, target_dims, codec, **ens, **sampler_kwargs)
            return (eng.mask_refine(list(mixes), est, **opts), *others)
        if ens:
            B, K = len(mixes), ens["samples"]
            dims = None if target_dims is None else [d for d in target_dims for _ in range(K)]
            est, *others = self.separate_batch([m for m in mixes for _ in range(K)], dims, codec, **sampler_kwargs)
            ln = [int(est[b * K].shape[-1]) for b in range(B)]
            cands = torch.zeros((B, K, int(est[0].shape[0]), max(ln)), device=eng.device, dtype=torch.float32)
            mp = torch.zeros((B, max(ln)), device=eng.device, dtype=torch.float32)
            for b, m in enumerate(mixes):
                v = min(ln[b], int(m.shape[-1]))
                mp[b, :v] = m.reshape(-1)[:v]
                for k in range(K):
                    cands[b, k, :, :ln[b]] = est[b * K + k]
            res = eng.ensemble_combine(cands, mp, lens=ln, mode=combine, return_info=return_info)
            out = res[0] if return_info else res
            outs = [out[b, :, :ln[b]] for b in range(B)]
            return (outs, *others, res[1]) if return_info else (outs, *others)
        native.check_codec_mode(codec)
        native.check_ragged(eng.cfg.score_kind, [1] * len(mixes), len(mixes), 1)
        kwargs = dict(sampler_kwargs)
        seed = kwargs.get("seed")
        enc_seed = int(torch.randint(0, 2**31 - 1, (1,)).item()) if seed is None else int(seed)
        y, frames = eng.encode_ragged(mixes, kwargs.pop("vae_noise", None), seed=enc_seed, codec=codec)
        self.max_len_lat = max(self.max_len_lat, y.shape[-1])
        skw = dict(_get(self.config, "model.sampler", {}) or {})
        skw.update(kwargs)
        sampler = self.get_pc_sampler("reverse_diffusion", "ald", y, frames=frames, **skw)
        est, *others = sampler()
        dims = [int(m.shape[-1]) for m in mixes] if target_dims is None else list(target_dims)
        return (eng.decode_ragged(est, frames, dims, codec=codec), *others)

    @torch.no_grad()
    def separate_long(self, mixes, window, overlap=None, fade="hann", align=True, batch=64, return_info=False,
                      mode="stitch", sample_rates=None, refine=None, stems=None, loudness=None, limit=None,
                      beamform=None, dereverb=None, spatial=None, track=None, activity=None, design=None,
                      **sampler_kwargs):
        """Long recordings as batched windows (Engine.separate_long's plan and stitch): `mixes` is one [1, L] tensor
        or a list of [1, L_r] tensors -> (estimates [n, L] or a list of [n, L_r], the summed nfe).  The windows of all
        recordings are pooled and go `batch` at a time through encode -> get_pc_sampler with the configured sampler
        keywords -> decode(..., window), exactly as `separate` does, so the model's own SDE and sampler are used; an
        explicit seed is offset by the minibatch index, vae_noise [Wtot, D, Tw] and noise [draws, Wtot, n, D, Tw] are
        sliced per minibatch.  Each recording is put back together by one Engine.window_stitch call (overlap default
        window // 4).  The windows are sampled independently: the stitch orders and blends them only.
        mode="score": Engine.separate_long(mode="score") with the model's SDE steps, t_eps and the configured sampler
        keywords (N, snr, corrector_steps, denoise, eps) -- every recording one latent and one diffusion sample, the
        score window-blended; vae_noise is then a list of [D, T_r] and noise [draws, R, n, D, Tmax].
        sample_rates (default None: the recordings are mono at the model's rate, the call is what it was): an int or
        one rate per recording, as in separate_batch -- the recordings are resampled to config.model.fs and mixed down,
        `window` and `overlap` stay in samples at the model's rate, and every estimate comes back at its recording's
        own rate and sample count.
        refine (default None: off), as in `separate`: every recording is refined whole against its mono mixture at
        the model's rate, after the stitch (or the single decode of mode="score") and before any resampling back.
        stems (default None: off), as in `separate_batch`: the recordings are [C, L_r], the call runs on their
        downmixes, and every recording's channels are filtered whole (Engine.stems) at the model's rate after the
        stitch and refine: [n, C, L] or a list of [n, C_r, L_r] comes back.
        loudness (default None: off), as in `separate_batch`: every recording is measured whole and gets one gain,
        the last step; with return_info=True its entries join the stitch's info dict.
        limit (default None: off), as in `separate_batch`: every recording is limited whole.
        beamform (default None: off), as in `separate_batch`, in both modes: the recordings are [C, L_r], the call runs
        on channel `ref` of each, and every recording's channels are beamformed whole (Engine.beamform: one filter per
        recording) at the model's rate after the stitch and refine: [n, L] or a list of [n, L_r] comes back.
        dereverb (default None: off), as in `separate_batch`, in both modes: every recording [C, L_r] (or [1, L_r]) is
        dereverberated whole at the model's rate, before any windowing, and the call above runs on the result.
        spatial (default None: off), as in `separate_batch`, in both modes: with beamform=, every recording's channels
        are beamformed whole by Engine.beamform_spatial.
        track (default None: off), as in `separate_batch`, in both modes: with beamform=, every recording's channels are
        beamformed whole by Engine.beamform_track -- a filter per block of the recording, not one for all of it.
        activity (default None: off), as in `separate`: decided over every whole recording after the stitch, refine and
        the beamforming step, at the model's rate.
        design (default None: off), as in `separate_batch`, in both modes: with beamform=, every recording's beamforming
        call gets design=."""
        eng = self.engine
        dopts = native.dereverb_options(dereverb)
        if dopts is not None and sampler_kwargs.get("intermediate"):
            self._dereverb_refusals(dopts, [], intermediate=sampler_kwargs.get("intermediate"))
        bopts, spopts = native.beamform_options(beamform), native.spatial_options(spatial)
        bopts = native.design_beamform_keywords(bopts, native.design_options(design))
        if spopts is not None:
            self._spatial_refusals(spopts, bopts, stems=stems, intermediate=sampler_kwargs.get("intermediate"))
        tropts = native.track_options(track)
        if tropts is not None:
            self._track_refusals(tropts, bopts, spopts, stems=stems, intermediate=sampler_kwargs.get("intermediate"))
        if bopts is not None:
            bclips = self._as_channel_clips([mixes] if torch.is_tensor(mixes) else list(mixes), "beamform")
            self._beamform_refusals(bopts, [int(m.shape[0]) for m in bclips], stems=stems,
                                    intermediate=sampler_kwargs.get("intermediate"))
        aopts = native.activity_options(activity)
        if aopts is not None:
            self._activity_refusals(aopts, stems=stems, intermediate=sampler_kwargs.get("intermediate"))
        lopts = native.level_options(loudness, limit)
        if lopts is not None:
            single = torch.is_tensor(mixes)
            clips = [mixes] if single else list(mixes)
            if bopts is not None:
                clips = self._reference_channel(bclips, bopts["ref"])
            self._loudness_refusals(lopts, [self._clip_channels(m) for m in clips],
                                    intermediate=sampler_kwargs.get("intermediate"))
            rates = self._model_rate("loudness=") if sample_rates is None else sample_rates
            est, *others = self.separate_long(mixes, window, overlap=overlap, fade=fade, align=align, batch=batch,
                                              return_info=return_info, mode=mode, sample_rates=sample_rates,
                                              refine=refine, stems=stems, beamform=beamform, dereverb=dereverb,
                                              spatial=spatial, track=track, activity=activity, design=design,
                                              **sampler_kwargs)
            outs, others = self._normalise(lopts, clips, [est] if single else est, rates, others, return_info,
                                           bool(return_info))
            return (outs[0] if single else outs, *others)
        if dopts is not None:
            single = torch.is_tensor(mixes)
            clips = [mixes] if single else list(mixes)
            rates = sample_rates
            if rates is not None:
                rates = [int(rates)] * len(clips) if isinstance(rates, int) else [int(r) for r in rates]
            out, *others = self._dereverb_of_lists(clips, rates, dopts, stems is not None or bopts is not None,
                                                   lambda at_fs: self.separate_long(
                at_fs, window, overlap=overlap, fade=fade, align=align, batch=batch, return_info=return_info, mode=mode,
                refine=refine, stems=stems, beamform=beamform, spatial=spatial, track=track, activity=activity,
                design=design, **sampler_kwargs))
            return (out[0] if single else out, *others)
        sopts = native.stems_options(stems)
        if sopts is not None:
            self._stems_refusals(sopts, [], intermediate=sampler_kwargs.get("intermediate"))
            single = torch.is_tensor(mixes)
            clips = [mixes] if single else list(mixes)
            rates = sample_rates
            if rates is not None:
                rates = [int(rates)] * len(clips) if isinstance(rates, int) else [int(r) for r in rates]
            out, *others = self._stems_of_lists(clips, rates, sopts, lambda mono: self.separate_long(
                mono, window, overlap=overlap, fade=fade, align=align, batch=batch, return_info=return_info, mode=mode,
                refine=refine, **sampler_kwargs))
            return (out[0] if single else out, *others)
        if bopts is not None:
            single = torch.is_tensor(mixes)
            rates = sample_rates
            if rates is not None:
                rates = [int(rates)] * len(bclips) if isinstance(rates, int) else [int(r) for r in rates]
            out, *others = self._beamform_of_lists(bclips, rates, bopts, lambda one: self.separate_long(
                one, window, overlap=overlap, fade=fade, align=align, batch=batch, return_info=return_info, mode=mode,
                refine=refine, **sampler_kwargs), spopts, tropts, aopts)
            return (out[0] if single else out, *others)
        opts = native.refine_options(refine)
        if sample_rates is not None:
            fs = self._model_rate("sample_rates=")
            single = torch.is_tensor(mixes)
            clips = [mixes] if single else list(mixes)
            rates = [int(sample_rates)] * len(clips) if isinstance(sample_rates, int) else [int(r) for r in sample_rates]
            at_fs = eng.to_model_rate(clips, rates, fs)
            est, *others = self.separate_long(at_fs[0] if single else at_fs, window, overlap=overlap, fade=fade,
                                              align=align, batch=batch, return_info=return_info, mode=mode,
                                              refine=refine, activity=activity, **sampler_kwargs)
            back = eng.from_model_rate([est] if single else est, rates, fs, [int(m.shape[-1]) for m in clips])
            return (back[0] if single else back, *others)
        if aopts is not None:
            single = torch.is_tensor(mixes)
            est, *others = self.separate_long(mixes, window, overlap=overlap, fade=fade, align=align, batch=batch,
                                              return_info=return_info, mode=mode, refine=refine, **sampler_kwargs)
            out = self._activity_step([est] if single else list(est), aopts)
            return (out[0] if single else out, *others)
        if opts is not None:
            single = torch.is_tensor(mixes)
            est, *others = self.separate_long(mixes, window, overlap=overlap, fade=fade, align=align, batch=batch,
                                              return_info=return_info, mode=mode, **sampler_kwargs)
            ref = eng.mask_refine([mixes] if single else list(mixes), [est] if single else est, **opts)
            return (ref[0] if single else ref, *others)
        if mode not in native.LONG_MODES:
            raise ValueError(f"mode must be one of {native.LONG_MODES} (got {mode!r})")
        if int(batch) < 1:
            raise ValueError(f"batch = {batch} < 1")
        if mode == "score":
            kwargs = dict(_get(self.config, "model.sampler", {}) or {})
            kwargs.update(sampler_kwargs)
            seed = kwargs.pop("seed", None)
            call = dict(vae_noise=kwargs.pop("vae_noise", None), noise=kwargs.pop("noise", None), seed=self._seed(seed),
                        N=int(kwargs.pop("N", None) or self.sde.N), snr=float(kwargs.pop("snr", 0.1)),
                        corrector_steps=int(kwargs.pop("corrector_steps", 1)), denoise=bool(kwargs.pop("denoise", True)),
                        t_eps=float(kwargs.pop("eps", self.t_eps)))
            kwargs.pop("n_spkrs", None)
            if kwargs:
                raise NotImplementedError(f"mode='score' runs the OUVE predictor-corrector sampler (reverse_diffusion + "
                                          f"ald); unsupported sampler keywords: {sorted(kwargs)}")
            return eng.separate_long(mixes, window=window, overlap=overlap, fade=fade, batch=batch,
                                     return_info=return_info, mode="score", **call)
        single = torch.is_tensor(mixes)
        pool, plans, overlap = native.cut_windows([mixes] if single else list(mixes), window, overlap, eng.device)
        kwargs = dict(sampler_kwargs)
        seed, vae_noise, noise = kwargs.pop("seed", None), kwargs.pop("vae_noise", None), kwargs.pop("noise", None)
        skw = dict(_get(self.config, "model.sampler", {}) or {})
        skw.update(kwargs)
        Wtot = pool.shape[0]
        sep = torch.empty((Wtot, self.n_src, int(window)), device=eng.device, dtype=torch.float32)
        nfe = 0
        for m, lo in enumerate(range(0, Wtot, int(batch))):
            sl = slice(lo, lo + int(batch))
            s = self._seed(None) if seed is None else int(seed) + m
            y, _ = self.encode(pool[sl], None, vae_noise=None if vae_noise is None else vae_noise[sl], seed=s)
            sampler = self.get_pc_sampler("reverse_diffusion", "ald", y, seed=None if seed is None else s,
                                          noise=None if noise is None else noise[:, sl], **skw)
            est, k = sampler()
            sep[sl] = self.decode(est, int(window))
            nfe += k
        outs, info = eng._stitch_plans(sep, plans, overlap, fade, align, return_info)
        res = (outs[0] if single else outs, nfe)
        return (*res, info) if return_info else res

    @torch.no_grad()
    def separate_files(self, paths, out_dir, *, batch=64, codec="padded", encoding="s16", rescale=False,
                       long_after=None, window=None, overlap=None, long_mode="stitch", seed=None, refine=None,
                       samples=None, combine="mean", stems=None, loudness=None, limit=None, beamform=None,
                       dereverb=None, spatial=None, track=None, activity=None, design=None, **sampler_kwargs):
        """WAV files in, one mono WAV per speaker out: `out_dir/s{i}/{stem}.wav` at each input's own rate and frame
        count (what the reference's src/inference/separate.py does one file per call; a file at another rate is
        resampled, not "skipped").  All headers are parsed first (wavio.read_header): a file that is refused, or two
        inputs with the same stem, raises ValueError before any device work.  The files are cut into batches of
        similar length at the model's rate (files.plan_files); per batch the payloads are read into one pinned buffer
        and copied once, decoded and mixed down on the device (Engine.pcm_decode), taken to config.model.fs
        (Engine.to_model_rate), separated by `separate_batch(codec=codec)` -- batch k with seed + k when a seed is
        given --, optionally scaled by the reference's output gain against the mono mixture at the model's rate
        (rescale: Engine.scale_output), taken back to each file's rate and frame count (Engine.from_model_rate),
        quantised on the device (Engine.pcm_encode: "s16", "s24" or "f32"; no dither), copied back once and written.
        long_after (seconds; default None: nothing is set aside): longer files go together through
        `separate_long(window, overlap=overlap, mode=long_mode, batch=batch, seed=seed)` -- window and overlap in
        samples at the model's rate, window defaulting to long_after seconds rounded down to a multiple of 4 hops --
        and the same way out.  -> one dict per input, in input order: "path", "rate", "channels", "frames", "outputs"
        (the files written), "clipped" (per speaker, the samples that were clamped), "alpha" (per speaker, with
        rescale), "batch" (the batch index, or "long").  DiT score network only (separate_batch's restriction).
        refine (default None: off), as in `separate`: per batch the order is separate -> refine (Engine.mask_refine
        against the mono mixtures at the model's rate) -> rescale -> back to each file's rate -> quantise.
        samples (default None: one draw), combine as in `separate_batch`, which gets them: a batch then holds
        batch // samples files, and a file that would go through separate_long (long_after) is refused before any
        device work -- candidate windows are a different problem.
        stems (default None: off), as in `separate`: the files are decoded with their channels, the separation runs
        on the downmix as above, and after refine every file's own channels are filtered at the model's rate
        (Engine.stems), taken back to the file's rate and frame count, interleaved and quantised on the device
        (Engine.pcm_encode_frames) and written with the input's channel count: a stereo file gives stereo stems that
        sum to it, a mono file in the same batch comes out mono.  Each dict gains "stems" (the mode).  Refused with
        rescale (the stems already sum to the mixture) before any device work.
        loudness (default None: off, the files are the bytes they were), as in `separate`: the last step before the
        quantiser, at each file's own rate -- after refine, stems, rescale and the resampling back.  link "mixture"
        measures the file as it was decoded, with its channels (at most two; refused before any device work
        otherwise), and all its speakers share one gain; link "stem" brings every speaker's file to the target.  Each
        dict gains "loudness_in", "loudness_out", "gain_db" and "true_peak_db", one entry per speaker.  A single
        gain, not a limiter, and no dither.
        limit (default None: off, the files are the bytes they were), as in `separate`: the true-peak look-ahead limiter
        in that last step, immediately before the quantiser; a file the single gain brings to the target keeps its
        bytes.  Each dict gains "reached", "evaluations", "reduction_db" and "limited_samples", one entry per speaker
        (and, without loudness=, the four entries above).
        beamform (default None: off, the files are the bytes they were), as in `separate`: array recordings of up to 8
        channels are decoded with their channels (Engine.pcm_decode, downmix=False), the separation runs on channel
        `ref` at the model's rate, and after refine every file's own channels are beamformed (Engine.beamform); then
        rescale (against channel `ref`), the resampling back, loudness (link "mixture" measures channel `ref` of the
        file) and limit as without the keyword.  The outputs stay mono `out_dir/s{i}/{stem}.wav`.  Each dict gains
        "beamform" (the reference channel).  A file with too few channels for `ref`, more than 8, or too short for one
        reflection is refused before any device work; so is stems= together with it.
        dereverb (default None: off, the files are the bytes they were), as in `separate`: the files are decoded with
        their channels kept (up to 8), taken to the model's rate and dereverberated whole (Engine.dereverb, one call
        per batch of files) before anything else; the separation runs on native.downmix of the result, stems= and
        beamform= on its channels.  loudness with link "mixture" keeps measuring the file as given.  Each dict gains
        "dereverb" (the options).  A file with more than 8 channels or too short for one reflection is refused
        before any device work.
        spatial (default None: off, the files are the bytes they were), as in `separate`: with beamform=, every file's
        channels are beamformed by Engine.beamform_spatial.  Each dict gains "spatial" (the options).  Refused before
        any device work without beamform=, with its postfilter "mask" and with stems=.
        track (default None: off, the files are the bytes they were), as in `separate`: with beamform=, every file's
        channels are beamformed by Engine.beamform_track.  Each dict gains "track" (the options).  Refused before any
        device work without beamform=, with spatial= and with stems=.
        activity (default None: off), as in `separate`: per batch Engine.activity on the final mono estimates at the
        model's rate (after refine and the beamforming step, before rescale, the resampling back and loudness), with
        gate=True Engine.activity_gate; every record gains "activity" (segments in seconds and active seconds per
        source) and every input an `out_dir/{stem}.rttm`, one "SPEAKER {stem} 1 {onset:.3f} {duration:.3f} <NA> <NA>
        s{i} <NA> <NA>" line per segment sorted by onset, then source (empty when nobody is active).  Refused with
        stems=.
        design (default None: off, the files are the bytes they were), as in `separate`: with beamform=, every file's
        beamforming call gets design=.  Each dict gains "design" (the options).  Refused before any device work
        without beamform=."""
        from . import files

        return files.separate_files(self, paths, out_dir, batch=batch, codec=codec, encoding=encoding, rescale=rescale,
                                    long_after=long_after, window=window, overlap=overlap, long_mode=long_mode,
                                    seed=seed, refine=refine, samples=samples, combine=combine, stems=stems,
                                    loudness=loudness, limit=limit, beamform=beamform, dereverb=dereverb,
                                    spatial=spatial, track=track, activity=activity, design=design, **sampler_kwargs)

    # ------------------------------------------------------------------ score-matching loss (forward only)
    @staticmethod
    def _seed(seed):
        return int(torch.randint(0, 2**31 - 1, (1,)).item()) if seed is None else int(seed)

    def _loss_chunks(self, B, minibatch):
        mb = B if minibatch is None else int(minibatch)
        return [slice(i, min(i + mb, B)) for i in range(0, B, mb)]

    def encode_lists(self, mixes, targets, seed=None, codec="grouped"):
        """A mixed-length batch as lists -- mixtures [1, L_b] and targets [n, L_b] -> (y [B,1,D,Tmax], x [B,n,D,Tmax],
        frames): Engine.encode_ragged under `codec` on the mixtures (seed) and on the B * n target rows (seed + 1, as
        `encode` does), zero past each item's frames."""
        mixes, targets = list(mixes), list(targets)
        if len(mixes) != len(targets) or not mixes:
            raise ValueError(f"a list batch needs as many mixtures as targets, at least one (got {len(mixes)} and "
                             f"{len(targets)})")
        n = int(targets[0].shape[0])
        for b, (m, t) in enumerate(zip(mixes, targets)):
            if m.dim() != 2 or t.dim() != 2 or m.shape[0] != 1 or t.shape[0] != n or m.shape[-1] != t.shape[-1]:
                raise ValueError(f"item {b}: the mixture must be [1, L_b] and the target [{n}, L_b] (got "
                                 f"{tuple(m.shape)} and {tuple(t.shape)})")
        native.check_codec_mode(codec)
        seed = self._seed(seed)
        y, frames = self.engine.encode_ragged(mixes, None, seed=seed, codec=codec)
        x, _ = self.engine.encode_ragged([t[i:i + 1] for t in targets for i in range(n)], None, seed=seed + 1,
                                         codec=codec)
        self.max_len_lat = max(self.max_len_lat, y.shape[-1])
        return y, x.reshape(len(mixes), n, *x.shape[2:]), frames

    def _score_loss(self, mode, reduction, y, x, time, noise, perm, seed, minibatch, frames=None):
        """One engine call per minibatch; an explicit seed is offset by the minibatch index (as get_pc_sampler).
        frames: a ragged batch, which is one call (Engine.score_loss with frames=)."""
        seed = self._seed(seed)
        if frames is not None:
            if minibatch is not None:
                raise ValueError("a mixed-length batch is one score_loss call: minibatch= does not go with lists")
            return self.engine.score_loss(y, x, mode=mode, reduction=reduction, t_eps=self.t_eps, seed=seed, time=time,
                                          noise=noise, perm=perm, frames=frames)
        outs, sizes = [], []
        for i, sl in enumerate(self._loss_chunks(y.shape[0], minibatch)):
            outs.append(self.engine.score_loss(
                y[sl], x[sl], mode=mode, reduction=reduction, t_eps=self.t_eps, seed=seed + i,
                time=None if time is None else time[sl], noise=None if noise is None else noise[sl],
                perm=None if perm is None else perm[sl]))
            sizes.append(outs[-1].shape[0] if reduction == "none" else sl.stop - sl.start)
        if len(outs) == 1:
            return outs[0]
        if reduction == "none":
            return torch.cat(outs, dim=0)
        w = torch.tensor(sizes, device=outs[0].device, dtype=torch.float32)
        return (torch.stack(outs) * w).sum() / w.sum()

    @torch.no_grad()
    def sample_time(self, x, seed=None):
        """reference :130-132: t ~ U(t_eps, T) per item of x [B,n,D,T], from the device stream of `seed` (the t that
        sample_prior / compute_score_loss draw for the same seed)."""
        _, aux = self.engine.score_loss(x[:, :1], x, t_eps=self.t_eps, seed=self._seed(seed), loss=False,
                                        return_aux=True)
        return aux["t"]

    @torch.no_grad()
    def sample_prior(self, mix, target, time=None, noise=None, seed=None, perm=None):
        """reference :134-145 -> (x_t, time, sigma [B,1,1,1], z).  time / noise: injected t [B] and z [B,n,D,T];
        perm [B,n]: per-item source order of `target` (utils.shuffle_sources' indices)."""
        _, aux = self.engine.score_loss(mix, target, t_eps=self.t_eps, time=time, noise=noise, perm=perm,
                                        seed=self._seed(seed), loss=False, return_aux=True)
        return aux["x_t"], aux["t"], aux["sigma"].reshape(-1, 1, 1, 1), aux["z"]

    @torch.no_grad()
    def compute_score_loss(self, y, x, time=None, noise=None, seed=None, perm=None, minibatch=None, codec="grouped"):
        """reference :154-160 with ONE native call (dsn_score_loss): `loss(score(x_t, t, y) sigma, -z)` followed by
        the reference's mean over the trailing axes -- a scalar for MSELoss(), **[B, n]** for
        MSELoss(reduction="none") (the mean runs over (D, T) only; kept as the reference has it).
        Lists (an addition of this project): y a list of mixture waveforms [1, L_b] and x a list of target waveforms
        [n, L_b] of different lengths.  They are encoded by `encode_lists` under `codec` (seed, seed + 1) and scored by
        one Engine.score_loss call with the items' frame counts: each row is the mean over the item's own frames, and
        MSELoss() becomes the mean of the B * n row means.  noise, when given, is [B,n,D,Tmax]."""
        y, x, frames = self._maybe_lists(y, x, seed, codec)
        return self._score_loss("dsm", self.loss_reduction, y, x, time, noise, perm, seed, minibatch, frames)

    def _maybe_lists(self, y, x, seed, codec):
        if isinstance(y, (list, tuple)) != isinstance(x, (list, tuple)):
            raise ValueError("mixtures and targets must both be tensors (latents) or both be lists (waveforms)")
        if not isinstance(y, (list, tuple)):
            return y, x, None
        return self.encode_lists(y, x, seed=seed, codec=codec)

    @torch.no_grad()
    def compute_score_loss_init_hack_pit(self, mix, target, noise=None, seed=None, minibatch=None, codec="grouped"):
        """reference :162-187 -> [B, n]: t = T, x_t = mix + sigma z0 and the minimum over all source permutations
        **per (item, source slot)** (the reference's stack(dim=1).min(dim=1) on [B,n] losses).  The reference calls
        the network n! times on identical inputs; this makes one call.  With MSELoss() the reference's stack of
        scalars raises IndexError, and so does this.  Lists of waveforms as in compute_score_loss."""
        if self.loss_reduction != "none":
            raise IndexError("Dimension out of range: compute_score_loss_init_hack_pit needs "
                             "MSELoss(reduction='none'), as in the reference")
        mix, target, frames = self._maybe_lists(mix, target, seed, codec)
        return self._score_loss("init_pit", "none", mix, target, None, noise, None, seed, minibatch, frames)

    @torch.no_grad()
    def train_step_init_5(self, mix, target, pit_mask=None, perm=None, time=None, noise=None, seed=None,
                          minibatch=None, codec="grouped", frames=None):
        """reference :189-208 (forward value only): items with pit_mask go through the PIT variant, the rest through
        shuffle_sources + compute_score_loss; torch.cat(losses).mean().  pit_mask [B] bool (default: a
        Bernoulli(init_hack_p) draw), perm [B - n_pit, n] (default: argsort of a uniform draw per item) -- both host
        draws from torch's generator, seeded by `seed` when given; time [B - n_pit] / noise [B,n,D,T] (z0 of the PIT
        items, z of the rest) are injected into the engine calls.
        Lists of waveforms as in compute_score_loss (encoded once, then split by pit_mask), or padded latents with
        frames= (B ints): each of the two groups is then one ragged Engine.score_loss call."""
        if self.loss_reduction != "none":
            raise ValueError("Reduction should 'none' for loss with init_hack == 5")
        seed = self._seed(seed)
        if isinstance(mix, (list, tuple)) or isinstance(target, (list, tuple)):
            if frames is not None:
                raise ValueError("frames= goes with padded latents; lists of waveforms carry their own lengths")
            mix, target, frames = self._maybe_lists(mix, target, seed, codec)
        B, n = target.shape[:2]
        if frames is not None:
            frames = native.check_ragged(self.engine.cfg.score_kind, frames, B, target.shape[-1])
        g = torch.Generator().manual_seed(seed)
        if pit_mask is None:
            pit_mask = torch.rand(B, generator=g) < self.init_hack_p
        pit = torch.as_tensor(pit_mask).bool().cpu()
        n_pit = int(pit.sum())

        def take(a, mask):
            return None if a is None else a[mask.to(a.device)]

        def take_frames(mask):
            return None if frames is None else [f for f, m in zip(frames, mask.tolist()) if m]

        losses = []
        if n_pit > 0:
            losses.append(self._score_loss("init_pit", "none", take(mix, pit), take(target, pit), None,
                                           take(noise, pit), None, seed, minibatch, take_frames(pit)))
        if n_pit != B:
            if perm is None:
                perm = torch.argsort(torch.rand((B - n_pit, n), generator=g), dim=1)
            losses.append(self._score_loss("dsm", "none", take(mix, ~pit), take(target, ~pit), time,
                                           take(noise, ~pit), perm, seed + 7919, minibatch, take_frames(~pit)))
        return torch.cat(losses).mean()

    def on_validation_epoch_start(self):
        self.n_batches_est_done = 0

    @torch.no_grad()
    def validation_step(self, batch, batch_idx=0, dataset_i=0, seed=None, codec="grouped", **loss_kwargs):
        """reference :251-273 as a dict instead of Lightning log calls: encode mix and targets, then
        "val/score_loss" (train_step_init_5 when init_hack == 5, else compute_score_loss; loss_kwargs are passed
        on) and, for the first `valid_max_sep_batches` calls since on_validation_epoch_start, "val/si_sdr": the
        reference's SISDRLoss(zero_mean=false, clamp_db=30, sign_flip=true, reduction=mean) of separate()'s estimate,
        from the device SI-SDR (dsn_si_sdr_pit).  That number is unpinned, like the other SI-SDR figures of this
        build: the reference computes it with fast_bss_eval.si_sdr_pit_loss, which is not available to compare with.
        "val/pesq" is not computed.
        A batch of lists (mixtures [1, L_b], targets [n, L_b] of different lengths): encode_lists under `codec`, one
        ragged score-loss call (or train_step_init_5's two), separate_batch for the estimates and the SI-SDR of every
        item over its own samples under its best SI-SDR permutation (Engine.si_bss_eval with lens=)."""
        mix, target = batch
        seed = self._seed(seed)
        if isinstance(mix, (list, tuple)):
            return self._validation_step_lists(list(mix), list(target), seed, codec, loss_kwargs)
        y, x = self.encode(mix, target, seed=seed)
        if self.init_hack == 5:
            loss = self.train_step_init_5(y, x, seed=seed, **loss_kwargs)
        else:
            loss = self.compute_score_loss(y, x, seed=seed, **loss_kwargs)
        out = {"val/score_loss": loss}
        if self.n_batches_est_done < self.valid_max_sep_batches:
            self.n_batches_est_done += 1
            est, *_ = self.separate(y, latent=True, target_dim=target.shape[-1], seed=seed)
            si_sdr, _ = self.engine.si_sdr_pit(target, est)
            out["val/si_sdr"] = si_sdr.clamp(-30.0, 30.0).mean()
        return out

    def _validation_step_lists(self, mixes, targets, seed, codec, loss_kwargs):
        y, x, frames = self.encode_lists(mixes, targets, seed=seed, codec=codec)
        if self.init_hack == 5:
            loss = self.train_step_init_5(y, x, seed=seed, frames=frames, **loss_kwargs)
        else:
            loss = self._score_loss("dsm", self.loss_reduction, y, x, loss_kwargs.get("time"), loss_kwargs.get("noise"),
                                    loss_kwargs.get("perm"), seed, loss_kwargs.get("minibatch"), frames)
        out = {"val/score_loss": loss}
        if self.n_batches_est_done < self.valid_max_sep_batches:
            self.n_batches_est_done += 1
            est, *_ = self.separate_batch(mixes, codec=codec, seed=seed)
            lens = [int(t.shape[-1]) for t in targets]
            dev = self.engine.device
            pad = lambda items: torch.stack([torch.nn.functional.pad(t.to(dev, torch.float32), (0, max(lens) - t.shape[-1]))
                                             for t in items])
            si_sdr = self.engine.si_bss_eval(pad(targets), pad(est), perm_by="sdr", clamp_db=30.0, lens=lens)[0]
            out["val/si_sdr"] = si_sdr.clamp(-30.0, 30.0).mean()
        return out

    def test_step(self, batch, batch_idx=0, dataset_i=None, **kwargs):
        return self.validation_step(batch, batch_idx, dataset_i=dataset_i, **kwargs)

    def close(self):
        self.engine.close()


def reconstruction_loss_config(config) -> dict:
    """The reference's reading of `training.loss` in LDM.__init__ (src/ldm.py:92-154) -> the keyword arguments of
    Engine.mrstft_loss (without `fs`-independent defaults changed): `spectral.config` (the MultiResolutionSTFTLoss
    keywords; `sample_rate` becomes "fs"), `spectral.weights.mrstft`, `spectral.decay`, `time.weights.l1` / `l2`.
    A discriminator (`training.discriminator` together with `training.loss.discriminator`, :92) raises
    NotImplementedError, as does any MultiResolutionSTFTLoss option without a native kernel."""
    tr = _get(config, "training")
    loss = _get(tr, "loss")
    if loss is None or _get(loss, "spectral") is None:
        raise ValueError("training.loss.spectral is missing: LDM needs the reference's loss section (src/ldm.py:100-130)")
    if _get(tr, "discriminator") is not None and _get(loss, "discriminator") is not None:
        raise NotImplementedError("training.discriminator: the adversarial and feature-matching terms are not "
                                  "implemented natively (forward value of the reconstruction terms only)")
    spec = dict(_get(loss, "spectral.config", {}) or {})
    target = str(spec.pop("_target_", "stable_audio_tools.training.losses.auraloss.MultiResolutionSTFTLoss"))
    if not target.endswith("MultiResolutionSTFTLoss"):
        raise NotImplementedError(f"training.loss.spectral.config._target_ = '{target}': only "
                                  "MultiResolutionSTFTLoss is implemented natively")
    kw = dict(fs=spec.pop("sample_rate", None),
              # auraloss.py:475-491, the constructor's defaults
              fft_sizes=tuple(spec.pop("fft_sizes", (1024, 2048, 512))),
              hop_sizes=tuple(spec.pop("hop_sizes", (120, 240, 50))),
              win_lengths=tuple(spec.pop("win_lengths", (600, 1200, 240))),
              perceptual_weighting=bool(spec.pop("perceptual_weighting", False)),
              w_sc=float(spec.pop("w_sc", 1.0)), w_log_mag=float(spec.pop("w_log_mag", 1.0)),
              w_lin_mag=float(spec.pop("w_lin_mag", 0.0)),
              mrstft_weight=float(_get(loss, "spectral.weights.mrstft", 1.0)),
              l1_weight=float(_get(loss, "time.weights.l1", 0.0)), l2_weight=float(_get(loss, "time.weights.l2", 0.0)))
    if spec.get("n_bins") is None:
        spec.pop("n_bins", None)
    native.mrstft_unsupported(decay=_get(loss, "spectral.decay", 1.0), **spec)
    if kw["perceptual_weighting"] and kw["fs"] is None:
        raise ValueError("`sample_rate` must be supplied when `perceptual_weighting = True`.")      # auraloss.py:362
    return kw


def padded_pair(decoded, reals, lens, device):
    """losses_gen's arguments -> (decoded, reals, lens): tensors pass as they are; two lists of [n, L_b] whose items
    agree in shape are zero-padded once to [B, n, Lmax] and lens becomes their lengths."""
    dl, rl = isinstance(decoded, (list, tuple)), isinstance(reals, (list, tuple))
    if dl != rl:
        raise ValueError("decoded and reals must both be tensors or both be lists of [n, L_b]")
    if not dl:
        return decoded, reals, lens
    if lens is not None:
        raise ValueError("lens= goes with padded tensors; lists carry their own lengths")
    if len(decoded) != len(reals) or not reals:
        raise ValueError(f"decoded and reals must hold the same number of items, at least one (got {len(decoded)} and "
                         f"{len(reals)})")
    for b, (d, r) in enumerate(zip(decoded, reals)):
        if d.dim() != 2 or tuple(d.shape) != tuple(r.shape) or d.shape[0] != reals[0].shape[0]:
            raise ValueError(f"item {b}: decoded and reals must both be [n, L_b] (got {tuple(d.shape)} and "
                             f"{tuple(r.shape)})")
    lens = [int(r.shape[-1]) for r in reals]
    pad = lambda items: torch.stack([torch.nn.functional.pad(t.to(device=device, dtype=torch.float32),
                                                             (0, max(lens) - t.shape[-1])) for t in items])
    return pad(decoded), pad(reals), lens


class LDM(LatentDiffSep):
    """The reference's second latent module (src/ldm.py), which fine-tunes the decoder through the frozen sampler:
    the inference surface is LatentDiffSep's (`LDM.separate` is the same code), and `losses_gen` is the forward value
    of its generator objective, read from `config.training.loss` as LDM.__init__ reads it (ldm.py:100-154).
    Gradients, the discriminator terms, warm-up and training are out of scope."""

    def __init__(self, config, device: int = 0, precision: str = "fp16", pit="batch"):
        self.loss_kwargs = reconstruction_loss_config(config)       # before the engine exists: a bad section fails early
        self.loss_fs = self.loss_kwargs.pop("fs")
        self.pit = pit
        super().__init__(config, device=device, precision=precision)

    @torch.no_grad()
    def losses_gen(self, decoded, reals, lens=None):
        """reference ldm.py:154 `self.losses_gen({"reals": reals, "decoded": decoded})` -> (loss, losses) with the
        MultiLoss keys "pit_mrstft_loss", "pit_l1_loss", "pit_l2_loss" (the latter two with a positive weight only).
        `self.last_loss_tables` keeps the whole Engine.mrstft_loss result (pair tables, chosen permutations).
        Mixed lengths (an addition of this project): decoded and reals as lists of [n, L_b] -- padded once and scored
        by one call with the items' lengths -- or as padded tensors with lens=; every item's tables are those it gets
        alone, combined as a dense batch's are (native.mrstft_combine)."""
        decoded, reals, lens = padded_pair(decoded, reals, lens, self.engine.device)
        res = self.engine.mrstft_loss(reals, decoded, self.loss_fs if self.loss_fs is not None else 0,
                                      pit=self.pit, lens=lens, **self.loss_kwargs)
        self.last_loss_tables = res
        losses = {k: res[k] for k in ("pit_mrstft_loss", "pit_l1_loss", "pit_l2_loss") if k in res}
        return res["loss"], losses

    @torch.no_grad()
    def generator_loss(self, mix, reals, **sampler_kwargs):
        """separate(mix) followed by losses_gen against `reals` [B,n,L] -> (loss, losses, decoded)."""
        decoded, *_ = self.separate(mix, target_dim=reals.shape[-1], **sampler_kwargs)
        loss, losses = self.losses_gen(decoded, reals)
        return loss, losses, decoded
