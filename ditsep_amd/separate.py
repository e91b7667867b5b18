"""python -m ditsep_amd.separate input_dir output_dir --config CONFIG --checkpoint CKPT

Separate every .wav file of a folder (the reference's src/inference/separate.py, with its sampler arguments): the files
go through LatentDiffSep.separate_files in batches of similar length, and `output_dir/s{i}/{stem}.wav` is written at
each input's own sample rate and frame count.  A file at another rate than the model's is resampled on the device (the
reference prints "Skipping" for it and separates it at the wrong rate anyway)."""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path


def str_or_int(x):
    try:
        return int(x)
    except ValueError:
        return x


def _bool(x):
    if str(x).lower() in ("1", "true", "yes", "on"):
        return True
    if str(x).lower() in ("0", "false", "no", "off"):
        return False
    raise argparse.ArgumentTypeError(f"expected a boolean, got {x!r}")


def _dbtp(x):
    if str(x).lower() == "none":
        return None
    try:
        return float(x)
    except ValueError:
        raise argparse.ArgumentTypeError(f"expected a level in dBTP or 'none', got {x!r}") from None


def build_parser() -> argparse.ArgumentParser:
    """The command line (importing and calling this needs neither the HIP library nor a GPU)."""
    p = argparse.ArgumentParser(prog="python -m ditsep_amd.separate",
                                description="Separate all the wav files in a specified folder")
    p.add_argument("input_dir", type=Path, help="Path to the input folder")
    p.add_argument("output_dir", type=Path, help="Path to the output folder")
    # the reference's arguments
    p.add_argument("-d", "--device", type=str_or_int, default="cuda:0", help="Device to use (default: cuda:0)")
    p.add_argument("-N", type=int, default=None, help="Number of steps (default: config.model.sampler.N)")
    p.add_argument("--snr", type=float, default=None, help="Step size of corrector")
    p.add_argument("--corrector-steps", type=int, default=None, help="Number of corrector steps")
    p.add_argument("--denoise", type=_bool, default=True, help="Use denoising in solver")
    p.add_argument("-s", "--schedule", type=str, default=None, help="Pick a different schedule for the inference")
    # the model
    p.add_argument("--config", type=Path, required=True,
                   help="The model's configuration tree: JSON, or YAML when the yaml package is installed")
    p.add_argument("--checkpoint", type=Path, default=None, help="Checkpoint written by the reference's training loop")
    p.add_argument("--ema", action="store_true", help="Use the checkpoint's EMA weights")
    p.add_argument("--precision", default="fp16", choices=["bf16", "bf16x3", "fp16", "fp16x3", "fp8"])
    # the file layer
    p.add_argument("--batch", type=int, default=64, help="Files per batch (and windows per batch of long files)")
    p.add_argument("--encoding", default="s16", choices=["s16", "s24", "f32"], help="Sample format of the outputs")
    p.add_argument("--rescale", action="store_true",
                   help="Scale every output by the reference's gain (the mixture projected onto it)")
    p.add_argument("--long-after", type=float, default=None,
                   help="Seconds; longer files are separated as windows (default: none are)")
    p.add_argument("--window", type=int, default=None, help="Window of long files, samples at the model's rate")
    p.add_argument("--overlap", type=int, default=None, help="Overlap of neighbouring windows (default window / 4)")
    p.add_argument("--long-mode", default="stitch", choices=["stitch", "score"])
    p.add_argument("--seed", type=int, default=None, help="Makes the run reproducible")
    p.add_argument("--refine", action="store_true",
                   help="Refine the estimates with mixture-consistent STFT masks before they are written (not a "
                        "trained step; off by default)")
    p.add_argument("--refine-nfft", type=int, default=512, help="Window of the masks, samples at the model's rate")
    p.add_argument("--refine-hop", type=int, default=128, help="Hop of the masks (window / 2, / 4 or / 8)")
    p.add_argument("--refine-power", type=int, default=2, choices=[1, 2], help="Exponent of the mask magnitudes")
    p.add_argument("--samples", type=int, default=None,
                   help="Draw this many candidate separations per file (1 to 16) and combine them on the device "
                        "(default: one draw)")
    p.add_argument("--combine", default="mean", choices=["mean", "median", "best", "medoid"],
                   help="How the candidates of --samples are combined")
    p.add_argument("--stems", default=None, choices=["mask", "wiener"],
                   help="Write every speaker with the input's own channels: the mixture's channels filtered with the "
                        "mono estimates (mask: the masks on every channel; wiener: multichannel Wiener filter, up to "
                        "two channels; not a trained step; off by default)")
    p.add_argument("--stems-nfft", type=int, default=512, help="Window of the stems filter, samples at the model's rate")
    p.add_argument("--stems-hop", type=int, default=128, help="Hop of the stems filter (window / 2, / 4 or / 8)")
    p.add_argument("--stems-power", type=int, default=2, choices=[1, 2], help="Exponent of the mask magnitudes")
    p.add_argument("--stems-reg", type=float, default=1e-3,
                   help="Diagonal loading of the Wiener solve, relative to the mean channel variance")
    p.add_argument("--beamform", action="store_true",
                   help="Microphone-array input (up to 8 channels): separate the reference channel and beamform all "
                        "channels towards every speaker with a mask-based MVDR filter; the outputs stay mono (not a "
                        "trained step; off by default)")
    p.add_argument("--beamform-ref", type=int, default=0, help="Reference channel of the beamformer")
    p.add_argument("--beamform-nfft", type=int, default=512, help="Window of the beamformer, samples at the model's rate")
    p.add_argument("--beamform-hop", type=int, default=128, help="Hop of the beamformer (window / 2, / 4 or / 8)")
    p.add_argument("--beamform-reg", type=float, default=1e-3,
                   help="Diagonal loading of the beamformer's solve, relative to the mean interference power")
    p.add_argument("--beamform-post", default="none", choices=["none", "mask"],
                   help="Post-filter of the beamformed spectrum: the speaker's own mask, or none")
    p.add_argument("--beamform-design", default=None, choices=["rank1", "gev"],
                   help="With --beamform: the filter -- rank1, the MVDR filter of a rank-one steering estimate (the "
                        "principal generalised eigenvector), or gev, the max-SNR filter with blind analytic "
                        "normalisation, which is not distortionless (not tuned; without the flag the filter is Souden's "
                        "MVDR, which is why 'souden' is no choice here)")
    p.add_argument("--beamform-sweeps", type=int, default=10, metavar="N",
                   help="Jacobi sweeps of the eigen-solver behind --beamform-design (1 .. 30); without "
                        "--beamform-design there is no eigen-solver and the value is not used")
    p.add_argument("--spatial", action="store_true",
                   help="With --beamform: refine the masks that steer the beamformer with a spatial mixture model "
                        "(guided cACGMM) fitted to the recording's own channels (not a trained step; not tuned; off by "
                        "default)")
    p.add_argument("--spatial-iterations", type=int, default=1, help="Expectation-maximisation passes of the model")
    p.add_argument("--spatial-noise", type=float, default=0.1, help="Prior mass of the noise class (0: no noise class)")
    p.add_argument("--spatial-floor", type=float, default=0.1,
                   help="Share of the prior spread equally over the speakers, whatever the estimates say")
    p.add_argument("--spatial-reg", type=float, default=1e-3,
                   help="Diagonal loading of the classes' covariances, relative to their mean diagonal")
    p.add_argument("--track", action="store_true",
                   help="With --beamform: follow moving speakers -- one MVDR filter per block of the recording, solved on "
                        "the blocks around it and interpolated from frame to frame (not a trained step; not tuned; off "
                        "by default)")
    p.add_argument("--track-block", type=float, default=0.8, metavar="SECONDS", help="Length of a block")
    p.add_argument("--track-context", type=int, default=1, metavar="N",
                   help="Blocks each side of a block whose statistics enter its filter")
    p.add_argument("--track-hold", action="store_true",
                   help="Hold a block's filter over the whole block (no interpolation between the blocks' centres)")
    p.add_argument("--activity", action="store_true",
                   help="Decide where every stem carries its speaker (a level floor and a dominance test between the "
                        "stems, with hysteresis and minimum durations) and write the segments to OUT/{name}.rttm (a "
                        "decision rule, not a trained detector; not tuned; off by default)")
    p.add_argument("--activity-gate", action="store_true",
                   help="--activity, and the stretches of a stem outside its segments become digital silence")
    p.add_argument("--activity-range", type=float, default=40.0, metavar="DB",
                   help="A frame is active within this many dB of the recording's loudest frame")
    p.add_argument("--activity-dominance", type=float, default=6.0, metavar="DB",
                   help=".. and within this many dB of the loudest stem of the same frame")
    p.add_argument("--activity-hysteresis", type=float, default=3.0, metavar="DB",
                   help="An active stem stays active this many dB below both thresholds")
    p.add_argument("--activity-min-on", type=float, default=0.1, metavar="SECONDS", help="Shorter segments are dropped")
    p.add_argument("--activity-min-off", type=float, default=0.1, metavar="SECONDS",
                   help="Shorter gaps between two segments are closed")
    p.add_argument("--activity-pad", type=float, default=0.0, metavar="SECONDS", help="Every segment grows by this at both ends")
    p.add_argument("--activity-smooth", type=float, default=0.04, metavar="SECONDS", help="Length of the level's box window")
    p.add_argument("--activity-band", type=float, nargs=2, default=(100.0, 4000.0), metavar=("LO", "HI"),
                   help="The band of the level in Hz")
    p.add_argument("--activity-fade", type=float, default=5.0, metavar="MS",
                   help="With --activity-gate: raised-cosine fade at the segments' edges in milliseconds (0: hard gate)")
    p.add_argument("--dereverb", action="store_true",
                   help="Dereverberate every recording first (weighted prediction error on up to 8 channels, kept for "
                        "the steps that use them; not a trained step; off by default)")
    p.add_argument("--dereverb-taps", type=int, default=10, help="Frames of the prediction filter")
    p.add_argument("--dereverb-delay", type=int, default=3, help="Frames between the predicted frame and the filter's first")
    p.add_argument("--dereverb-iterations", type=int, default=3, help="Re-estimations of the variance and the filter")
    p.add_argument("--dereverb-nfft", type=int, default=512, help="Window of the dereverberation, samples at the model's rate")
    p.add_argument("--dereverb-hop", type=int, default=128, help="Hop of the dereverberation (window / 2, / 4 or / 8)")
    p.add_argument("--dereverb-reg", type=float, default=1e-4,
                   help="Diagonal loading of the filter's solve, relative to the mean diagonal of the correlation matrix")
    p.add_argument("--loudness", type=float, default=None, metavar="LUFS",
                   help="Bring every file's stems to this programme loudness (ITU-R BS.1770 / EBU R 128, measured on "
                        "the device) with one gain, e.g. -23; a gain, not a limiter (off by default)")
    p.add_argument("--true-peak", type=_dbtp, default=-1.0, metavar="DBTP",
                   help="With --loudness: the gain is held back so that no stem's true peak exceeds this (default -1; "
                        "'none': no ceiling)")
    p.add_argument("--loudness-link", default="mixture", choices=["mixture", "stem"],
                   help="With --loudness: measure the input file and give all its stems one gain (mixture), or bring "
                        "every stem to the target by itself (stem)")
    p.add_argument("--limit", action="store_true",
                   help="True-peak look-ahead limiter as the last step: where the ceiling forbids the --loudness target "
                        "to a single gain, only the neighbourhood of the peaks is lowered so that the rest can reach it; "
                        "without --loudness, every file once against a ceiling of -1 dBTP (off by default)")
    p.add_argument("--limit-lookahead", type=float, default=5.0, metavar="MS",
                   help="With --limit: the look-ahead (and hold) time in milliseconds")
    p.add_argument("--limit-drive", type=float, default=6.0, metavar="DB",
                   help="With --limit: how far above the single gain the pre-gain may go")
    p.add_argument("--limit-iterations", type=int, default=4, metavar="K",
                   help="With --limit: at most this many evaluations of the limited programme's loudness")
    return p


def load_config(path: Path):
    text = Path(path).read_text()
    if Path(path).suffix.lower() in (".yaml", ".yml"):
        try:
            import yaml
        except ImportError as e:
            raise ValueError(f"{path}: a YAML configuration needs the yaml package; convert it to JSON") from e
        return yaml.safe_load(text)
    return json.loads(text)


def device_index(device) -> int:
    if isinstance(device, int):
        return device
    if device == "cuda":
        return 0
    if str(device).startswith("cuda:"):
        return int(str(device)[5:])
    raise ValueError(f"the engine runs on a GPU: --device must be cuda:<index> or an index (got {device!r})")


def refine_of(args):
    """The `refine` keyword of separate_files from the parsed flags: None unless --refine is given."""
    if not args.refine:
        return None
    return dict(n_fft=args.refine_nfft, hop=args.refine_hop, power=args.refine_power)


def stems_of(args):
    """The `stems` keyword of separate_files from the parsed flags: None unless --stems is given."""
    if args.stems is None:
        return None
    return dict(mode=args.stems, n_fft=args.stems_nfft, hop=args.stems_hop, power=args.stems_power,
                reg=args.stems_reg)


def beamform_of(args):
    """The `beamform` keyword of separate_files from the parsed flags: None unless --beamform is given."""
    if not args.beamform:
        return None
    return dict(ref=args.beamform_ref, n_fft=args.beamform_nfft, hop=args.beamform_hop, reg=args.beamform_reg,
                postfilter=None if args.beamform_post == "none" else args.beamform_post)


def design_of(args):
    """The `design` keyword of separate_files from the parsed flags: None unless --beamform-design is given."""
    if args.beamform_design is None:
        return None
    return dict(kind=args.beamform_design, sweeps=args.beamform_sweeps)


def spatial_of(args):
    """The `spatial` keyword of separate_files from the parsed flags: None unless --spatial is given."""
    if not args.spatial:
        return None
    return dict(iterations=args.spatial_iterations, noise=args.spatial_noise, floor=args.spatial_floor,
                reg=args.spatial_reg)


def track_of(args):
    """The `track` keyword of separate_files from the parsed flags: None unless --track is given."""
    if not args.track:
        return None
    return dict(block=args.track_block, context=args.track_context, interpolate=not args.track_hold)


def activity_of(args):
    """The `activity` keyword of separate_files from the parsed flags: None unless --activity or --activity-gate is
    given."""
    if not (args.activity or args.activity_gate):
        return None
    return dict(gate=bool(args.activity_gate), band=tuple(args.activity_band), smooth=args.activity_smooth,
                range_db=args.activity_range, dominance_db=args.activity_dominance,
                hysteresis_db=args.activity_hysteresis, min_on=args.activity_min_on, min_off=args.activity_min_off,
                pad=args.activity_pad, fade_ms=args.activity_fade)


def dereverb_of(args):
    """The `dereverb` keyword of separate_files from the parsed flags: None unless --dereverb is given."""
    if not args.dereverb:
        return None
    return dict(taps=args.dereverb_taps, delay=args.dereverb_delay, iterations=args.dereverb_iterations,
                n_fft=args.dereverb_nfft, hop=args.dereverb_hop, reg=args.dereverb_reg)


def loudness_of(args):
    """The `loudness` keyword of separate_files from the parsed flags: None unless --loudness is given."""
    if args.loudness is None:
        return None
    return dict(target=args.loudness, peak=args.true_peak, link=args.loudness_link)


def limit_of(args):
    """The `limit` keyword of separate_files from the parsed flags: None unless --limit is given."""
    if not args.limit:
        return None
    return dict(lookahead_ms=args.limit_lookahead, drive_db=args.limit_drive, iterations=args.limit_iterations)


def main(argv=None) -> int:
    args = build_parser().parse_args(argv)
    try:
        if not args.input_dir.is_dir():
            raise ValueError(f"{args.input_dir} is not a folder")
        if args.output_dir.is_file():
            raise ValueError("Output directory is a file")
        paths = sorted(args.input_dir.glob("*.wav"))
        if not paths:
            raise ValueError(f"no .wav files in {args.input_dir}")
        config = load_config(args.config)
        dev = device_index(args.device)
    except ValueError as e:
        print(f"error: {e}", file=sys.stderr)
        return 2

    from .latent import LatentDiffSep

    model = LatentDiffSep(config, device=dev, precision=args.precision)
    try:
        if args.checkpoint is not None:
            model.load_checkpoint(args.checkpoint, use_ema=args.ema)
        kw = {k: v for k, v in (("N", args.N), ("snr", args.snr), ("corrector_steps", args.corrector_steps),
                                ("schedule", args.schedule)) if v is not None}
        try:
            records = model.separate_files(paths, args.output_dir, batch=args.batch, encoding=args.encoding,
                                           rescale=args.rescale, long_after=args.long_after, window=args.window,
                                           overlap=args.overlap, long_mode=args.long_mode, seed=args.seed,
                                           refine=refine_of(args), samples=args.samples, combine=args.combine,
                                           stems=stems_of(args), beamform=beamform_of(args),
                                           dereverb=dereverb_of(args), spatial=spatial_of(args), track=track_of(args),
                                           loudness=loudness_of(args), limit=limit_of(args), activity=activity_of(args),
                                           design=design_of(args), denoise=args.denoise, **kw)
        except ValueError as e:
            print(f"error: {e}", file=sys.stderr)
            return 2
        for r in records:
            clipped = sum(r["clipped"])
            print(f"{r['path']}: {r['frames']} frames at {r['rate']} Hz, {r['channels']} ch -> {len(r['outputs'])} files"
                  + (f", {clipped} samples clipped" if clipped else "")
                  + (f", gain {', '.join(f'{g:+.2f}' for g in r['gain_db'])} dB" if "gain_db" in r else "")
                  + (f", limiter down to {min(r['reduction_db']):+.2f} dB"
                     + ("" if all(r["reached"]) else ", target not reached") if "reduction_db" in r else ""))
        return 0
    finally:
        model.close()


if __name__ == "__main__":
    sys.exit(main())
