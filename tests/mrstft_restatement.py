"""float64 restatement of the generator objective of the reference's LDM (src/ldm.py: a permutation-invariant
multi-resolution STFT loss plus permutation-invariant L1 / L2 waveform losses) in the pair-table formulation of
dsn_mrstft_loss: every term of every source permutation is a mean of values of one (item b, reference source i,
estimate source j) pair.  numpy (torch only for the reference's float32 window); pinned to the reference's own modules by tests/golden/mrstft.npz
(scripts/make_golden_mrstft.py, tests/test_mrstft_host.py)."""
from itertools import permutations

import numpy as np

FFT_SIZES = (2048, 1024, 512, 256, 128, 64, 32)
HOP_SIZES = (512, 256, 128, 64, 32, 16, 8)
EPS = 1e-8
# name: (fs, B, n, L, seed)
CASES = {"fs8k": (8000, 2, 2, 4000, 11), "fs16k": (16000, 2, 3, 6000, 12)}


def make_case(name):
    """(reals, decoded) float32 [B,n,L]: amplitude-modulated tones plus noise; the estimates are the references in
    another source order plus noise."""
    fs, B, n, L, seed = CASES[name]
    return make_signals(fs, B, n, L, seed)


def make_signals(fs, B, n, L, seed, est_noise=0.05):
    rng = np.random.default_rng(seed)
    t = np.arange(L) / fs
    reals = np.zeros((B, n, L))
    for b in range(B):
        for i in range(n):
            f0 = rng.uniform(150.0, 0.35 * fs)
            fm = rng.uniform(2.0, 9.0)
            reals[b, i] = (0.25 * (1.0 + 0.8 * np.sin(2 * np.pi * fm * t + rng.uniform(0, 6.28)))
                           * np.sin(2 * np.pi * f0 * t + rng.uniform(0, 6.28)) + 0.02 * rng.standard_normal(L))
    # item b's estimates are its references rolled by 1 + b mod (n - 1): never the identity order, and with n > 2
    # not the same order for every item
    order = np.array([np.roll(np.arange(n), 1 + b % max(n - 1, 1)) for b in range(B)])
    decoded = np.stack([reals[b, order[b]] for b in range(B)]) + est_noise * rng.standard_normal((B, n, L))
    return reals.astype(np.float32), decoded.astype(np.float32)


def prefilter(x, taps):
    """zero-padded "same" cross-correlation of every row of x [..., L] with taps (odd count)"""
    taps = np.asarray(taps, dtype=np.float64)
    half = len(taps) // 2
    flat = np.asarray(x, dtype=np.float64).reshape(-1, x.shape[-1])
    out = np.stack([np.correlate(np.pad(row, half), taps, mode="valid") for row in flat])
    return out.reshape(x.shape)


def padded_window(fft, win):
    """the reference's window, torch.hann_window(win) as the float32 tensor it is (periodic Hann), centred in `fft`
    (the left pad is (fft - win) // 2).  Its float32 rounding matters: the leakage floor of a spectrum follows it."""
    import torch

    w = np.zeros(fft)
    left = (fft - win) // 2
    w[left:left + win] = torch.hann_window(win).double().numpy()
    return w


def magnitudes(x, fft, hop, win):
    """x [..., L] -> [..., frames, fft // 2 + 1]: sqrt(max(|STFT|^2, 1e-8)); frame f starts at f * hop of the signal
    reflect-padded by fft // 2, frames = 1 + L // hop"""
    L = x.shape[-1]
    if L <= fft // 2:
        raise ValueError(f"L = {L} is too short for reflect padding of {fft // 2}")
    xp = np.pad(np.asarray(x, dtype=np.float64), [(0, 0)] * (x.ndim - 1) + [(fft // 2, fft // 2)], mode="reflect")
    F = 1 + L // hop
    idx = np.arange(F)[:, None] * hop + np.arange(fft)[None, :]
    spec = np.fft.rfft(xp[..., idx] * padded_window(fft, win), axis=-1)
    return np.sqrt(np.maximum(spec.real ** 2 + spec.imag ** 2, EPS))


def pair_tables(reals, decoded, fft_sizes=FFT_SIZES, hop_sizes=HOP_SIZES, win_lengths=None, taps=None):
    """{"sc", "log_mag", "lin_mag": [R,B,n,n], "l1", "l2": [B,n,n]}; entry [.., b, i, j] compares reference source i
    with estimate source j of item b.  The spectral-convergence norm in the denominator is the estimate's."""
    win_lengths = fft_sizes if win_lengths is None else win_lengths
    r64, d64 = np.asarray(reals, dtype=np.float64), np.asarray(decoded, dtype=np.float64)
    diff = r64[:, :, None, :] - d64[:, None, :, :]
    out = {"l1": np.abs(diff).mean(-1), "l2": (diff ** 2).mean(-1)}
    if taps is not None:
        r64, d64 = prefilter(r64, taps), prefilter(d64, taps)
    sc, lg, lin = [], [], []
    for fft, hop, win in zip(fft_sizes, hop_sizes, win_lengths):
        mr, md = magnitudes(r64, fft, hop, win), magnitudes(d64, fft, hop, win)        # [B,n,F,K]
        dm = md[:, None, :, :, :] - mr[:, :, None, :, :]                                 # [B,i,j,F,K]
        sc.append(np.sqrt((dm ** 2).sum((-1, -2))) / np.sqrt((md ** 2).sum((-1, -2)))[:, None, :])
        lg.append(np.abs(np.log(mr)[:, :, None] - np.log(md)[:, None, :]).mean((-1, -2)))
        lin.append(np.abs(dm).mean((-1, -2)))
    B, n = r64.shape[:2]
    empty = np.zeros((0, B, n, n))
    out.update(sc=np.array(sc) if sc else empty, log_mag=np.array(lg) if lg else empty,
               lin_mag=np.array(lin) if lin else empty)
    return out


def spectral_item_values(tab, perm, w_sc=1.0, w_log_mag=1.0, w_lin_mag=0.0):
    """[B]: the MR-STFT loss of each item with estimate source perm[i] assigned to reference source i; the batch
    loss is the mean of these"""
    i = np.arange(len(perm))
    per_res = 0.0
    for w, key in ((w_sc, "sc"), (w_log_mag, "log_mag"), (w_lin_mag, "lin_mag")):
        if w:
            per_res = per_res + w * tab[key][:, :, i, list(perm)].mean(-1)              # [R,B]
    return np.zeros(tab["l1"].shape[0]) if np.isscalar(per_res) else per_res.mean(0)


def time_item_values(tab, key, perm):
    i = np.arange(len(perm))
    return tab[key][:, i, list(perm)].mean(-1)


def pit(item_values_of, n, mode="batch"):
    """item_values_of(perm) -> [B].  mode "batch": the one permutation with the smallest batch mean (the reference's
    PITLoss); "item": the smallest per item; None: the identity.  -> (loss, perms [B,n], values)"""
    ident = tuple(range(n))
    B = len(item_values_of(ident))
    if n == 1 or mode is None:
        v = item_values_of(ident)
        return float(v.mean()), np.tile(np.array(ident), (B, 1)), np.array([v.mean()])
    perms = list(permutations(range(n)))
    vals = np.array([item_values_of(p) for p in perms])                                # [P,B]
    if mode == "batch":
        means = vals.mean(1)
        k = int(np.argmin(means))
        return float(means[k]), np.tile(np.array(perms[k]), (B, 1)), means
    if mode == "item":
        k = np.argmin(vals, axis=0)
        return float(vals[k, np.arange(B)].mean()), np.array([perms[q] for q in k]), vals.T
    raise ValueError(mode)


def objective(tab, n, *, w_sc=1.0, w_log_mag=1.0, w_lin_mag=0.0, mrstft_weight=1.0, l1_weight=0.0, l2_weight=0.0,
              mode="batch"):
    """The reference's MultiLoss over its PITLoss modules: each term picks its own permutation; the L1 / L2 terms
    exist only with a positive weight."""
    out = {}
    loss, perm, vals = pit(lambda p: spectral_item_values(tab, p, w_sc, w_log_mag, w_lin_mag), n, mode)
    out["pit_mrstft_loss"], out["pit_mrstft_perm"], out["mrstft_values"] = mrstft_weight * loss, perm, mrstft_weight * vals
    total = out["pit_mrstft_loss"]
    for key, w in (("l1", l1_weight), ("l2", l2_weight)):
        if w > 0.0:
            loss, perm, _ = pit(lambda p, key=key: time_item_values(tab, key, p), n, mode)
            out[f"pit_{key}_loss"], out[f"pit_{key}_perm"] = w * loss, perm
            total = total + w * loss
    out["loss"] = total
    return out
