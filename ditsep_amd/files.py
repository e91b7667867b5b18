"""WAV files in, one WAV per speaker out: the file layer over LatentDiffSep.separate_batch / separate_long.

The host parses headers and moves raw bytes (wavio); every sample conversion runs on the device (Engine.pcm_decode /
pcm_encode), so a batch costs one host-to-device copy of the payloads as the files hold them and one device-to-host
copy of the payloads as they are written."""
from __future__ import annotations

import os
from typing import Optional

from . import native, wavio


def plan_files(headers, fs: int, hop: int, batch: int = 64, long_after: Optional[float] = None) -> dict:
    """How a set of files goes through the engine (pure: no GPU, no file is opened).  `headers` is one
    wavio.WavHeader per file, `fs` the model's rate, `hop` its hop length ->
      "lengths"  every file's sample count at the model's rate (native.resample_length of its frame count)
      "frames"   .. and its latent frames
      "batches"  index lists of at most `batch` files of similar length (evaluate.length_batches on "lengths":
                 sorted by length, ties by index), over the files that are not set aside
      "long"     the files longer than `long_after` seconds (default None: none), in input order
    Every file appears exactly once, in one batch or in "long"."""
    from .evaluate import length_batches

    if int(batch) < 1:
        raise ValueError(f"batch = {batch} < 1")
    if long_after is not None and not float(long_after) > 0:
        raise ValueError(f"long_after = {long_after!r} must be a positive number of seconds")
    lengths = [native.resample_length(h.rate, fs, h.frames) for h in headers]
    long = [i for i, h in enumerate(headers) if long_after is not None and h.frames > float(long_after) * h.rate]
    short = [i for i in range(len(headers)) if i not in set(long)]
    batches = [[short[j] for j in b] for b in length_batches([lengths[i] for i in short], int(batch))]
    return {"lengths": lengths, "frames": [native.latent_frames_of(v, hop) for v in lengths], "batches": batches,
            "long": long}


def files_per_batch(batch: int, samples: Optional[int] = None) -> int:
    """Files of one separate_batch call of `batch` rows when every file is drawn `samples` times: batch // samples
    (default None: one draw, `batch` files).  A batch too small for one file is refused."""
    if samples is None:
        return int(batch)
    if int(batch) < int(samples):
        raise ValueError(f"batch = {batch} < samples = {samples}: a batch holds batch // samples files")
    return int(batch) // int(samples)


def parse_inputs(paths) -> list:
    """Every header, before any device work: a file wavio refuses raises its ValueError, and so do two inputs with the
    same stem (they would be written to the same output files)."""
    paths = [os.fspath(p) for p in paths]
    if not paths:
        raise ValueError("no input files")
    stems = {}
    for p in paths:
        stem = os.path.splitext(os.path.basename(p))[0]
        if stem in stems:
            raise ValueError(f"{p} and {stems[stem]} have the same stem {stem!r}: their outputs would collide")
        stems[stem] = p
    return [wavio.read_header(p) for p in paths]


def load_batch(engine, paths, headers, downmix: bool = True):
    """The payloads of `paths` back to back in one pinned buffer, one host-to-device copy, one decode launch ->
    (list of mono [1, frames_b] clips at each file's own rate, on the device; downmix=False: [channels_b, frames_b],
    every file with its own channels)"""
    import torch

    offsets, total = [], 0
    for h in headers:
        offsets.append(total)
        total += h.data_bytes
    raw = torch.empty(total, dtype=torch.uint8, pin_memory=True)
    view = raw.numpy()
    for p, h, o in zip(paths, headers, offsets):
        wavio.read_payload(p, h, out=view[o:o + h.data_bytes])
    items = [(o, h.frames, h.channels, h.encoding) for o, h in zip(offsets, headers)]
    x, frames = engine.pcm_decode(raw, items, downmix=downmix)
    return [x[b, :1 if downmix else h.channels, :frames[b]] for b, h in enumerate(headers)]


def _padded(rows, device):
    import torch

    lens = [int(r.shape[-1]) for r in rows]
    out = torch.zeros((len(rows), int(rows[0].shape[0]), max(lens)), device=device, dtype=torch.float32)
    for b, r in enumerate(rows):
        out[b, :, :lens[b]] = r
    return out, lens


def separate_files(model, paths, out_dir, *, batch=64, codec="padded", encoding="s16", rescale=False, long_after=None,
                   window=None, overlap=None, long_mode="stitch", seed=None, refine=None, samples=None, combine="mean",
                   stems=None, loudness=None, limit=None, beamform=None, dereverb=None, spatial=None, track=None,
                   activity=None, design=None, **sampler_kwargs) -> list:
    """LatentDiffSep.separate_files (see there)."""
    import torch

    eng = model.engine
    fs = model._model_rate("separate_files")
    if encoding not in native.PCM_OUT_ENCODINGS:
        raise ValueError(f"encoding must be one of {native.PCM_OUT_ENCODINGS} (got {encoding!r})")
    native.check_codec_mode(codec)
    refine = native.refine_options(refine)
    stems = native.stems_options(stems)
    if stems is not None and rescale:
        raise ValueError("stems= does not go with rescale: the stems of a channel already sum to that channel of the "
                         "mixture")
    des = native.design_options(design)
    beam = native.design_beamform_keywords(native.beamform_options(beamform), des)
    spat = native.spatial_options(spatial)
    if spat is not None:
        if stems is not None:
            raise ValueError("spatial= does not go with stems=: it refines the masks of the beamformer, which stems= "
                             "does not run")
        native.spatial_beamform_keywords(beam, spat)
    trk = native.track_options(track)
    if trk is not None:
        if stems is not None:
            raise ValueError("track= does not go with stems=: it adapts the weights of the beamformer, which stems= "
                             "does not run")
        native.track_beamform_keywords(beam, trk, fs, spat)
    if beam is not None and stems is not None:
        raise ValueError("beamform= does not go with stems=: the beamformer returns one mono signal per source, stems= "
                         "the mixture's channels")
    dere = native.dereverb_options(dereverb)
    act = native.activity_options(activity)
    if act is not None and stems is not None:
        raise ValueError("activity= does not go with stems=: it decides on mono estimates, stems= returns the mixture's "
                         "channels (no gate for stems)")
    loud = native.level_options(loudness, limit)
    linked = loud is not None and loud["link"] == "mixture" and loud["target"] is not None   # the file is the source
    if long_mode not in native.LONG_MODES:
        raise ValueError(f"long_mode must be one of {native.LONG_MODES} (got {long_mode!r})")
    paths = [os.fspath(p) for p in paths]
    headers = parse_inputs(paths)
    if loud is not None:
        for p, h in zip(paths, headers):
            if not native.LOUDNESS_RATES[0] <= h.rate <= native.LOUDNESS_RATES[1]:
                raise ValueError(f"{p}: {h.rate} Hz; loudness= measures rates in [{native.LOUDNESS_RATES[0]}, "
                                 f"{native.LOUDNESS_RATES[1]}] Hz")
            if linked and beam is None and h.channels > native.LOUDNESS_MAX_CHANNELS:
                raise ValueError(f"{p}: {h.channels} channels; loudness= with link 'mixture' measures at most "
                                 f"{native.LOUDNESS_MAX_CHANNELS} (no surround weights; link 'stem' measures the outputs)")
    # the files' own channels are needed by the stems filter, by the beamformer, by the dereverberation and as the gain
    # source of a mixture-linked loudness
    keep_channels = stems is not None or beam is not None or dere is not None or linked
    hop = model.hop_length
    ens = {} if samples is None else dict(samples=native.check_samples(samples, combine), combine=combine)
    plan = plan_files(headers, fs, hop, files_per_batch(batch, samples), long_after)
    if ens and plan["long"]:
        raise ValueError(f"{paths[plan['long'][0]]} is longer than long_after = {long_after} s and would be separated as "
                         f"windows: samples= has no separate_long form")
    if plan["long"] and window is None:
        window = max(4 * hop, int(float(long_after) * fs) // (4 * hop) * (4 * hop))
    out_dir = os.fspath(out_dir)
    n = model.n_src
    if refine is not None:
        # its refusals before any device work (checked on a stand-in item long enough for every n_fft), a file too
        # short for one reflection included
        need = native.check_mask_refine((1, 2049), (1, n, 2049), None, **refine)[2] // 2 + 1
        for p, v in zip(paths, plan["lengths"]):
            if v < need:
                raise ValueError(f"{p}: {v} samples at the model's rate; refine= needs at least n_fft / 2 + 1 = {need}")
    if stems is not None:
        # .. and those of the stems: the parameters on a stand-in item, every file's channel count and length
        need = native.check_stems((1, 1, 2049), (1, n, 2049), None, None, **stems)[4] // 2 + 1
        for p, h, v in zip(paths, headers, plan["lengths"]):
            if h.channels > native.STEMS_MAX_CHANNELS[stems["mode"]]:
                raise ValueError(f"{p}: {h.channels} channels; stems mode {stems['mode']!r} takes at most "
                                 f"{native.STEMS_MAX_CHANNELS[stems['mode']]}")
            if v < need:
                raise ValueError(f"{p}: {v} samples at the model's rate; stems= needs at least n_fft / 2 + 1 = {need}")
    if beam is not None:
        # .. and those of the beamformer: the parameters on a stand-in item, every file's channel count and length
        # (design= was checked by design_options and is no argument of check_beamform)
        plain = {k: v for k, v in beam.items() if k != "design"}
        need = native.check_beamform((1, 8, 2049), (1, n, 2049), None, None, **dict(plain, ref=0))[4] // 2 + 1
        ref = beam["ref"]
        for p, h, v in zip(paths, headers, plan["lengths"]):
            if h.channels > native.BEAMFORM_MAX_CHANNELS:
                raise ValueError(f"{p}: {h.channels} channels; beamform= takes at most {native.BEAMFORM_MAX_CHANNELS}")
            if isinstance(ref, bool) or int(ref) != ref or not 0 <= ref < h.channels:
                raise ValueError(f"{p}: {h.channels} channels; beamform= has ref = {ref!r} outside [0, {h.channels})")
            if v < need:
                raise ValueError(f"{p}: {v} samples at the model's rate; beamform= needs at least n_fft / 2 + 1 = {need}")
    if dere is not None:
        # .. and those of the dereverberation: the parameters on a stand-in item, every file's channel count and length
        need = native.check_dereverb((1, 1, 2049), None, None, **dere)[6] // 2 + 1
        for p, h, v in zip(paths, headers, plan["lengths"]):
            if h.channels > native.DEREVERB_MAX_CHANNELS:
                raise ValueError(f"{p}: {h.channels} channels; dereverb= takes at most {native.DEREVERB_MAX_CHANNELS}")
            native.check_dereverb((1, h.channels, 2049), None, None, **dere)
            if v < need:
                raise ValueError(f"{p}: {v} samples at the model's rate; dereverb= needs at least n_fft / 2 + 1 = {need}")
    if act is not None:
        # .. and those of the activity decision: the parameters on a stand-in item, every file's length
        need = native.check_activity((1, n, 2049), None, **native.activity_keywords(act, fs))[2] // 2 + 1
        native.activity_ramp(native.activity_frames(act, fs)["fade"])
        for p, v in zip(paths, plan["lengths"]):
            if v < need:
                raise ValueError(f"{p}: {v} samples at the model's rate; activity= needs at least n_fft / 2 + 1 = {need}")
    records = [None] * len(paths)

    def reference(clips):
        """channel `ref` of every clip [C, L] as [1, L]: what the model separates and loudness measures with beamform="""
        return [c[beam["ref"]:beam["ref"] + 1].contiguous() for c in clips]

    def level(idx, clips, back):
        """the `loudness` step: rows at the files' own rates -> (the rows with their gains applied, the record entries)"""
        if loud is None:
            return back, [{} for _ in idx]
        sources = None if not linked else clips if beam is None else reference(clips)
        back, info = eng.loudness_normalize(sources, back, [headers[i].rate for i in idx], **loud)
        keys = ("loudness_in", "loudness_out", "gain_db", "true_peak_db")
        if loud.get("limit") is not None:
            keys += ("reached", "evaluations", "reduction_db", "limited_samples")
        return back, [{k: info[k][j] for k in keys} for j in range(len(idx))]

    def finish_stems(idx, clips, est, label, channels_fs=None):
        """mono estimates at the model's rate -> multichannel files; `clips` the files' own channels at their own rates
        (with dereverb=: `channels_fs` the dereverberated channels at the model's rate, which the filter then sees)"""
        hs = [headers[i] for i in idx]
        at_fs = channels_fs if dere is not None else eng.to_model_rate(clips, [h.rate for h in hs], fs, downmix=False)
        back = eng.stems_from_model_rate(eng.stems(at_fs, est, **stems), [h.rate for h in hs], fs,
                                         [h.frames for h in hs])
        back, levels = level(idx, clips, back)
        rows = torch.zeros((len(idx), n, max(h.channels for h in hs), max(h.frames for h in hs)), device=eng.device,
                           dtype=torch.float32)
        for j, y in enumerate(back):
            rows[j, :, :hs[j].channels, :hs[j].frames] = y
        payloads, clipped = eng.pcm_encode_frames(rows.reshape(len(idx) * n, *rows.shape[2:]),
                                                  [h.frames for h in hs for _ in range(n)],
                                                  [h.channels for h in hs for _ in range(n)], encoding)
        for j, i in enumerate(idx):
            stem = os.path.splitext(os.path.basename(paths[i]))[0]
            outs = []
            for s in range(n):
                d = os.path.join(out_dir, f"s{s}")
                os.makedirs(d, exist_ok=True)
                outs.append(os.path.join(d, stem + ".wav"))
                wavio.write_wav(outs[-1], payloads[j * n + s], hs[j].rate, hs[j].channels, encoding)
            records[i] = {"path": paths[i], "rate": hs[j].rate, "channels": hs[j].channels, "frames": hs[j].frames,
                          "outputs": outs, "clipped": clipped[j * n:(j + 1) * n], "batch": label,
                          "stems": stems["mode"], **levels[j]}
            if dere is not None:
                records[i]["dereverb"] = dict(dere)

    def finish(idx, at_fs, est, label, clips=None, channels_fs=None):
        """estimates at the model's rate -> files; `at_fs` the mono mixtures there (with beamform=: channel `ref`, and
        `channels_fs` all channels)"""
        alpha = None
        if refine is not None:
            est = eng.mask_refine(at_fs, est, **refine)
        if stems is not None:
            return finish_stems(idx, clips, est, label, channels_fs)
        if beam is not None:
            est = model._beamform_step([model._fit(m, int(e.shape[-1])) for m, e in zip(channels_fs, est)], list(est),
                                       beam, spat, trk)
        decided = None
        if act is not None:
            # on the final mono estimates at the model's rate, before rescale, the resampling back and loudness
            est = model._activity_step(list(est), act)
            decided = model.last_activity
        if rescale:
            sep, lens = _padded(est, eng.device)
            mix, _ = _padded(at_fs, eng.device)
            scaled, alpha = eng.scale_output(mix, sep, lens)
            est = [scaled[j, :, :lens[j]] for j in range(len(idx))]
        hs = [headers[i] for i in idx]
        back = eng.from_model_rate(est, [h.rate for h in hs], fs, [h.frames for h in hs])
        back, levels = level(idx, clips, back)
        rows, lens = _padded(back, eng.device)
        payloads, clipped = eng.pcm_encode(rows.reshape(len(idx) * n, -1), [v for v in lens for _ in range(n)],
                                           encoding)
        for j, i in enumerate(idx):
            stem = os.path.splitext(os.path.basename(paths[i]))[0]
            outs = []
            for s in range(n):
                d = os.path.join(out_dir, f"s{s}")
                os.makedirs(d, exist_ok=True)
                outs.append(os.path.join(d, stem + ".wav"))
                wavio.write_wav(outs[-1], payloads[j * n + s], hs[j].rate, 1, encoding)
            rec = {"path": paths[i], "rate": hs[j].rate, "channels": hs[j].channels, "frames": hs[j].frames,
                   "outputs": outs, "clipped": clipped[j * n:(j + 1) * n], "batch": label}
            if alpha is not None:
                rec["alpha"] = [float(a) for a in alpha[j]]
            if beam is not None:
                rec["beamform"] = beam["ref"]
            if spat is not None:
                rec["spatial"] = dict(spat)
            if trk is not None:
                rec["track"] = dict(trk)
            if des is not None:
                rec["design"] = dict(des)
            if dere is not None:
                rec["dereverb"] = dict(dere)
            if decided is not None:
                rec["activity"] = dict(segments=decided[j]["seconds"], active=decided[j]["active"])
                os.makedirs(out_dir, exist_ok=True)
                with open(os.path.join(out_dir, stem + ".rttm"), "w") as f:
                    f.write("".join(line + "\n" for line in native.activity_rttm(stem, decided[j]["segments"], fs)))
            records[i] = dict(rec, **levels[j])

    def mono_at_model_rate(idx, clips):
        """what the model separates, at its rate: the downmix -- or, with beamform=, channel `ref` of all channels taken
        there with the channels kept, which come back as well"""
        rates = [headers[i].rate for i in idx]
        if beam is None and dere is None:
            return eng.to_model_rate(clips, rates, fs), None
        channels_fs = eng.to_model_rate(clips, rates, fs, downmix=False)
        if dere is not None:
            # the first waveform step: every file dereverberated whole with its channels kept; the model separates
            # native.downmix of the result (or, with beamform=, its channel `ref`)
            channels_fs = eng.dereverb(list(channels_fs), **dere)
            if beam is None:
                return [native.downmix(c[None])[0] for c in channels_fs], channels_fs
        return reference(channels_fs), channels_fs

    for k, idx in enumerate(plan["batches"]):
        clips = load_batch(eng, [paths[i] for i in idx], [headers[i] for i in idx], downmix=not keep_channels)
        at_fs, channels_fs = mono_at_model_rate(idx, clips)
        kw = dict(sampler_kwargs) if seed is None else dict(sampler_kwargs, seed=int(seed) + k)
        est, *_ = model.separate_batch(at_fs, codec=codec, **ens, **kw)
        finish(idx, at_fs, est, k, clips, channels_fs)
    if plan["long"]:
        idx = plan["long"]
        clips = load_batch(eng, [paths[i] for i in idx], [headers[i] for i in idx], downmix=not keep_channels)
        at_fs, channels_fs = mono_at_model_rate(idx, clips)
        kw = dict(sampler_kwargs) if seed is None else dict(sampler_kwargs, seed=int(seed))
        est, *_ = model.separate_long(at_fs, window, overlap=overlap, mode=long_mode, batch=batch, **kw)
        finish(idx, at_fs, est, "long", clips, channels_fs)
    return records
