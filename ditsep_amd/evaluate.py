"""Evaluation harness with the semantics of the reference's `evaluate_process`
(reference src/evaluate_latent.py:159-338): per utterance (or batch) encode, then the TIMED region
sampler + decode (with a device sync, which the reference lacks :273-277), then permutation-solved
SI-SDR / SI-SIR / SI-SAR on the device (dsn_si_bss_eval: the bss_eval decomposition with a one-tap filter, the
permutation chosen on SIR as the reference's `fast_bss_eval.si_bss_eval_sources(..., compute_permutation=True)`
does, :118-124), one result record per utterance with the reference's JSON fields (:294-304) and the mean
summary (:139-156).  With stoi=True the "stoi" field holds extended STOI (the reference calls pystoi.stoi(...,
extended=True); stoi_extended=False gives classic STOI, its stoi_no_extended) from the device (dsn_stoi), scored on
the SIR permutation as the reference orders the estimates by perm before calling stoi; parity with the pystoi package
is unpinned (the float64 restatement in tests/stoi_restatement.py is the contract).  By default, and always for PESQ
(ITU-T P.862, not implemented), the field is null.

composite=True adds the measures of the reference's second evaluation stage (src/evaluate/evaluate_covl.py): "llr",
"wss" and "segsnr" per source from the device (dsn_composite), scored on the SIR permutation like STOI.  PESQ is the
caller's: with pesq_fn(fs, ref_1d, est_1d) -> float the "pesq" field is filled and the composite scores "csig", "cbak"
and "covl" are added.  pesq_fn sees what the reference's PESQ call sees: eval_composite runs it after SSNR has, in
place and in float32, removed both means and rescaled the estimate to the reference's peak (condition_for_pesq).

mrstft=True adds "mrstft" and "l1" per source from the device (dsn_mrstft_loss): the A-weighted multi-resolution STFT
distance (the reference's LDM objective, src/config/ldm/training/default.yaml, unweighted) and the mean absolute
waveform error of each reference source against the estimate the SIR permutation assigns to it.

Utterances of different lengths (the reference evaluates them one at a time, :238): a batch whose `mix` and `target`
are lists of differently long tensors takes the ragged route -- `length_batches` cuts a data set into such batches
with little padding -- in which every utterance gets what it gets alone (LatentDiffSep.separate_batch) and every
metric above is one call on the padded batch with the utterances' lengths.  mrstft and score_loss are refused there
(NotImplementedError) unless the caller passes ragged_losses=True: they then run as one call each too, under this
project's definitions for mixed lengths (Engine.score_loss with frames=, Engine.mrstft_loss with lens=).

bss_eval=True adds "sdr", "sir" and "sar" per source from the device (dsn_bss_eval): classic bss_eval (Vincent et al.
2006) with distortion filters of bss_filter_length taps (512, the bss_eval default, behind the SDRi column of a
WSJ0-2mix table), scored on the record's SI-SIR permutation as stoi and composite are; dense and ragged batches alike.
Parity with fast_bss_eval / mir_eval is unpinned (tests/bss_eval_restatement.py is the contract)."""
from __future__ import annotations

import json
import time
from typing import Iterable, Optional

import numpy as np
import torch


def length_batches(lengths, batch_size: int) -> list:
    """Index lists that cut a data set into batches of `batch_size` utterances of similar length: the indices sorted by
    length (ties by index), then cut in order, so a batch's padding stays small.  Every index appears exactly once."""
    if batch_size < 1:
        raise ValueError("batch_size must be at least 1")
    order = sorted(range(len(lengths)), key=lambda i: (int(lengths[i]), i))
    return [order[i:i + batch_size] for i in range(0, len(order), batch_size)]


def _pad_items(items, Lmax: int, device) -> torch.Tensor:
    """list of [n, L_b] -> [B, n, Lmax] float32 on `device`, zero past each item's end (the ragged metric calls read
    nothing there)."""
    out = torch.zeros((len(items), items[0].shape[0], Lmax), dtype=torch.float32, device=device)
    for b, t in enumerate(items):
        out[b, :, :t.shape[-1]] = t.to(device=device, dtype=torch.float32)
    return out


def _evaluate_ragged(model, mixes, targets, fs, idx, seed, N, corrector_steps, snr, denoise, stoi, stoi_extended,
                     codec="grouped", composite=False, pesq_fn=None, bss_eval=False, bss_filter_length=512,
                     score_loss=False, mrstft=False) -> dict:
    """One batch of differently long utterances: mixes list of [1, L_b], targets list of [n, L_b].  The timed region is
    sampler + decode as in the dense route; every requested metric then runs once on the padded [B, n, Lmax] pair with
    the items' lengths (Engine.si_bss_eval / stoi / composite / mrstft_loss with lens=), each item scored as it is alone.
    score_loss: the targets are encoded as B * n rows (seed + idx + 1) and scored by one Engine.score_loss call with the
    items' frame counts (seed + idx), as the dense route seeds them.  codec: how the encoder and the decoder take the
    batch (Engine.encode_ragged)."""
    eng, dev = model.engine, model.engine.device
    B = len(mixes)
    y, frames = eng.encode_ragged(mixes, None, seed=seed + idx, codec=codec)
    sampler = model.get_pc_sampler("reverse_diffusion", "ald", y, N=N, denoise=denoise, corrector_steps=corrector_steps,
                                   snr=snr, seed=seed + idx, frames=frames)
    lens = [int(t.shape[-1]) for t in targets]
    sl = None
    if score_loss:
        n0 = targets[0].shape[0]
        tgt_lat, _ = eng.encode_ragged([t[i:i + 1] for t in targets for i in range(n0)], None, seed=seed + idx + 1,
                                       codec=codec)
        sl = eng.score_loss(y, tgt_lat.reshape(B, n0, *tgt_lat.shape[2:]), reduction="none", t_eps=model.t_eps,
                            seed=seed + idx, frames=frames).cpu()
    torch.cuda.synchronize(dev)
    t_s = time.perf_counter()
    x_result, nfe = sampler()
    est = eng.decode_ragged(x_result, frames, lens, codec=codec)
    torch.cuda.synchronize(dev)
    t_proc = time.perf_counter() - t_s
    Lmax, n_src = max(lens), targets[0].shape[0]
    tgt, xr = _pad_items(targets, Lmax, dev), _pad_items(est, Lmax, dev)
    si_sdr, si_sir, si_sar, perm = eng.si_bss_eval(tgt, xr, perm_by="sir", clamp_db=100.0, lens=lens)
    st = eng.stoi(tgt, xr, fs, extended=stoi_extended, perm=perm, lens=lens) if stoi else None
    comp = pq = None
    if composite:
        if pesq_fn is not None:
            pq = torch.tensor([[float(pesq_fn(fs, *condition_for_pesq(targets[b][i].cpu().numpy(),
                                                                       est[b][int(perm[b, i])].cpu().numpy())))
                                for i in range(n_src)] for b in range(B)], dtype=torch.float32)
        comp = eng.composite(tgt, xr, fs, perm=perm, pesq=pq, lens=lens)
    mr = None
    if mrstft:
        tabs = eng.mrstft_loss(tgt, xr, fs, pit=None, lens=lens)
        rows = torch.arange(n_src)
        spec = (tabs["sc"] + tabs["log_mag"]).mean(0)                        # [B,n,n]: mean over the resolutions
        mr = {"mrstft": torch.stack([spec[b, rows, perm[b]] for b in range(B)]),
              "l1": torch.stack([tabs["l1"][b, rows, perm[b]] for b in range(B)])}
    bss = eng.bss_eval(tgt, xr, filter_length=bss_filter_length, perm=perm, lens=lens)[:3] if bss_eval else None
    records = {}
    for b in range(B):
        rec = {"batch_idx": idx + b, "si_sdr": si_sdr[b].tolist(), "si_sir": si_sir[b].tolist(),
               "si_sar": si_sar[b].tolist(), "pesq": None, "stoi": None if st is None else st[b].tolist(),
               "nfe": nfe, "runtime": t_proc / B, "len_s": lens[b] / fs, "perm": perm[b].tolist()}
        if sl is not None:
            rec["score_loss"] = sl[b].tolist()
        if comp is not None:
            for k in ("llr", "wss", "segsnr") + (("csig", "cbak", "covl") if pq is not None else ()):
                rec[k] = comp[k][b].tolist()
            if pq is not None:
                rec["pesq"] = pq[b].tolist()
        if mr is not None:
            for k in ("mrstft", "l1"):
                rec[k] = mr[k][b].tolist()
        if bss is not None:
            for k, v in zip(("sdr", "sir", "sar"), bss):
                rec[k] = v[b].tolist()
        records[idx + b] = rec
    return records


def evaluate_batches(model, batches: Iterable, fs: int, *, N: Optional[int] = None, corrector_steps: Optional[int] = None,
                     snr: Optional[float] = None, denoise: bool = True, start_idx: int = 0, seed: int = 0,
                     stoi: bool = False, stoi_extended: bool = True, score_loss: bool = False,
                     composite: bool = False, pesq_fn=None, mrstft: bool = False, codec: str = "grouped",
                     bss_eval: bool = False, bss_filter_length: int = 512, ragged_losses: bool = False) -> dict:
    """`batches` yields (mix [B,1,L], target [B,n,L]); returns {utterance index: record}.  stoi=True fills "stoi"
    with n floats per record (ESTOI, or STOI with stoi_extended=False); it stays null otherwise.  score_loss=True
    adds "score_loss": the denoising score-matching loss of the utterance per source slot (n floats; one score
    call per batch on the encoded targets, t and z from the device stream of the utterance's seed).  composite=True
    adds "llr", "wss" and "segsnr" (n floats each); with pesq_fn(fs, ref_1d, est_1d) -> float as well, "pesq" is filled
    and "csig", "cbak" and "covl" are added.  mrstft=True adds "mrstft" and "l1" (n floats each, unweighted): the
    diagonal, under the SIR permutation, of the pair tables of Engine.mrstft_loss at its defaults (seven resolutions,
    A-weighting of `fs`, spectral convergence plus log magnitude).  bss_eval=True adds "sdr", "sir" and "sar" (n floats
    each, last in the record): Engine.bss_eval with bss_filter_length taps on the record's "perm".

    A batch may also be (list of mix [1,L_b], list of target [n,L_b]) with differing L_b: it takes the ragged route
    (one sampler call on the padded batch, the codec per group of equal length, every metric once on the padded batch
    with the items' lengths); each record carries its own "len_s", "runtime" stays the batch time divided by B, and
    stoi, composite and pesq_fn work as above, pesq_fn on each utterance's own unpadded signals.  score_loss and mrstft
    on a list batch need ragged_losses=True (NotImplementedError without it, as before they had a ragged form): the
    keyword is the caller's consent to what the mixed-length forms are -- score_loss on each utterance's own latent
    frames with device draws indexed by position in the padded batch (Engine.score_loss with frames=: a valid draw,
    not the one the utterance alone makes for that seed), mrstft on its own samples (Engine.mrstft_loss with lens=) --
    with the record keys and seeds of the dense branch; dense batches ignore it.  codec="padded" runs the codec of a ragged batch once on the padded batch
    instead of once per group (Engine.encode_ragged / decode_ragged); dense batches ignore it."""
    from .native import check_codec_mode
    check_codec_mode(codec)
    if pesq_fn is not None and not composite:
        raise ValueError("pesq_fn is used by composite=True only")
    cfg_s = dict(getattr(model, "config", {}).get("model", {}).get("sampler", {})) if isinstance(getattr(model, "config", None), dict) else {}
    N = N if N is not None else cfg_s.get("N", model.sde.N)
    corrector_steps = corrector_steps if corrector_steps is not None else cfg_s.get("corrector_steps", 1)
    snr = snr if snr is not None else cfg_s.get("snr", 0.5)
    results, idx = {}, start_idx
    dev = model.engine.device
    for mix, target in batches:
        if isinstance(mix, (list, tuple)):
            if (score_loss or mrstft) and not ragged_losses:
                raise NotImplementedError("score_loss / mrstft are not implemented for ragged batches unless "
                                          "ragged_losses=True asks for their mixed-length forms")
            results.update(_evaluate_ragged(model, list(mix), list(target), fs, idx, seed, N, corrector_steps, snr,
                                            denoise, stoi, stoi_extended, codec=codec, composite=composite,
                                            pesq_fn=pesq_fn, bss_eval=bss_eval,
                                            bss_filter_length=bss_filter_length, score_loss=score_loss,
                                            mrstft=mrstft))
            idx += len(mix)
            continue
        mix, target = mix.to(dev), target.to(dev)
        L = target.shape[-1]
        mix_latent, _ = model.encode(mix, None, seed=seed + idx)
        sampler = model.get_pc_sampler("reverse_diffusion", "ald", mix_latent, N=N, denoise=denoise,
                                       corrector_steps=corrector_steps, snr=snr, seed=seed + idx)
        sl = None
        if score_loss:
            B0, n0 = target.shape[:2]
            tgt = model.engine.encode(target.reshape(B0 * n0, 1, L), None, seed=seed + idx + 1)
            sl = model.engine.score_loss(mix_latent, tgt.reshape(B0, n0, *tgt.shape[2:]), reduction="none",
                                         t_eps=model.t_eps, seed=seed + idx).cpu()
        torch.cuda.synchronize(dev)
        t_s = time.perf_counter()
        x_result, nfe = sampler()
        x_result = model.decode(x_result, L)
        torch.cuda.synchronize(dev)
        t_proc = time.perf_counter() - t_s
        si_sdr, si_sir, si_sar, perm = model.engine.si_bss_eval(target, x_result, perm_by="sir", clamp_db=100.0)
        st = model.engine.stoi(target, x_result, fs, extended=stoi_extended, perm=perm) if stoi else None
        B = mix.shape[0]
        comp = pq = None
        if composite:
            if pesq_fn is not None:
                tgt_h, est_h = target.cpu().numpy(), x_result.cpu().numpy()
                pq = torch.tensor([[float(pesq_fn(fs, *condition_for_pesq(tgt_h[b, i], est_h[b, int(perm[b, i])])))
                                    for i in range(target.shape[1])] for b in range(B)], dtype=torch.float32)
            comp = model.engine.composite(target, x_result, fs, perm=perm, pesq=pq)
        mr = None
        if mrstft:
            tabs = model.engine.mrstft_loss(target, x_result, fs, pit=None)
            n_src = target.shape[1]
            rows = torch.arange(n_src)
            spec = (tabs["sc"] + tabs["log_mag"]).mean(0)                        # [B,n,n]: mean over the resolutions
            mr = {"mrstft": torch.stack([spec[b, rows, perm[b]] for b in range(B)]),
                  "l1": torch.stack([tabs["l1"][b, rows, perm[b]] for b in range(B)])}
        bss = (model.engine.bss_eval(target, x_result, filter_length=bss_filter_length, perm=perm)[:3]
               if bss_eval else None)
        for b in range(B):
            results[idx] = {"batch_idx": idx, "si_sdr": si_sdr[b].tolist(), "si_sir": si_sir[b].tolist(),
                            "si_sar": si_sar[b].tolist(),
                            "pesq": None, "stoi": None if st is None else st[b].tolist(),
                            "nfe": nfe, "runtime": t_proc / B, "len_s": L / fs, "perm": perm[b].tolist()}
            if sl is not None:
                results[idx]["score_loss"] = sl[b].tolist()
            if comp is not None:
                for k in ("llr", "wss", "segsnr") + (("csig", "cbak", "covl") if pq is not None else ()):
                    results[idx][k] = comp[k][b].tolist()
                if pq is not None:
                    results[idx]["pesq"] = pq[b].tolist()
            if mr is not None:
                for k in ("mrstft", "l1"):
                    results[idx][k] = mr[k][b].tolist()
            if bss is not None:
                for k, v in zip(("sdr", "sir", "sar"), bss):
                    results[idx][k] = v[b].tolist()
            idx += 1
    return results


def condition_for_pesq(ref: np.ndarray, est: np.ndarray):
    """The (ref, est) pair the reference hands to PESQ in eval_composite: its SSNR has by then, in place and in
    float32, removed both means and scaled the estimate by max|ref| / max|est| of the mean-removed signals."""
    r = np.array(ref, dtype=np.float32).reshape(-1)
    e = np.array(est, dtype=np.float32).reshape(-1)
    r -= r.mean()
    e -= e.mean()
    with np.errstate(all="ignore"):
        e *= np.max(np.abs(r)) / np.max(np.abs(e))
    return r, e


def summarize(results: dict, ignore_inf: bool = True) -> dict:
    """Mean over utterances of every numeric field (reference summarize(), evaluate_latent.py:139-156)."""
    summary = {"number": 0}
    acc = {}
    for rec in results.values():
        summary["number"] += 1
        for k, v in rec.items():
            if k in ("batch_idx", "perm") or v is None:
                continue
            a = np.atleast_1d(np.asarray(v, dtype=np.float64))
            if ignore_inf:
                a = a[np.isfinite(a)]
            if a.size:
                s, c = acc.get(k, (0.0, 0))
                acc[k] = (s + float(a.mean()), c + 1)
    for k, (s, c) in acc.items():
        summary[k] = s / c
    return summary


def write_results(path: str, results: dict):
    with open(path, "w") as fh:
        json.dump({str(k): v for k, v in results.items()}, fh, indent=2)
    summary = summarize(results)
    # the per-utterance records keep exactly the reference's fields; provenance of the metric arithmetic goes into the
    # summary: SI-SDR / SI-SIR / SI-SAR are this build's own device kernels (dsn_si_bss_eval), checked against the
    # definition-level CPU restatement only -- fast_bss_eval, which the reference calls, is not installed here
    summary["si_bss_impl"] = "native (dsn_si_bss_eval); parity unpinned vs fast_bss_eval"
    if any(rec.get("stoi") is not None for rec in results.values()):
        summary["stoi_impl"] = "native (dsn_stoi); parity unpinned vs pystoi"
    if any("llr" in rec for rec in results.values()):
        summary["composite_impl"] = ("native (dsn_composite): llr, wss, segsnr pinned to the reference's evaluate_covl.py; "
                                     "pesq, where given, is the caller's")
    if any("mrstft" in rec for rec in results.values()):
        summary["mrstft_impl"] = ("native (dsn_mrstft_loss): pinned to the reference's auraloss.MultiResolutionSTFTLoss "
                                  "(A-weighted, 7 resolutions) and L1; per source under the SIR permutation")
    if any("sdr" in rec for rec in results.values()):
        summary["bss_eval_impl"] = ("native (dsn_bss_eval): bss_eval SDR / SIR / SAR with a 512-tap distortion filter "
                                    "unless bss_filter_length says otherwise, pinned to the float64 restatement in "
                                    "tests/bss_eval_restatement.py; parity unpinned vs fast_bss_eval / mir_eval "
                                    "(neither is installed)")
    summary["nfe_note"] = "nfe = N * (corrector_steps + 1), the reference's bookkeeping (not a count of score calls)"
    with open(path.replace(".json", "_summary.json"), "w") as fh:
        json.dump(summary, fh, indent=2)
