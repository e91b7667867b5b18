"""float64 yardstick of the two losses on mixed-length batches.

The DEFINITION is per item: item b of a ragged batch gets what the dense restatement (tests/mrstft_restatement.py,
tests/score_loss_restatement.py) gives it alone, cut to its own length -- `mrstft_items`, `score_loss_items`.  The
device does not loop; it works on the padded tensors with the lengths as data.  `mrstft_masked` and `score_loss_masked`
restate THAT formulation (index arithmetic on the padded rows, masks, per-item divisors) without ever touching a value
at or past an item's end, and tests/test_ragged_losses_host.py checks that the two formulations agree in float64.
Nothing here imports the engine."""
import numpy as np
import torch

from tests import mrstft_restatement as M
from tests import score_loss_restatement as S

F64 = torch.float64
KEYS = ("sc", "log_mag", "lin_mag", "l1", "l2")


# ---------------------------------------------------------------------------------------------- MR-STFT
def mrstft_items(reals, decoded, lens, fft_sizes=M.FFT_SIZES, hop_sizes=M.HOP_SIZES, win_lengths=None, taps=None):
    """reals, decoded [B,n,Lmax] (anything past lens[b]) -> the pair tables, item b's rows being M.pair_tables of
    the item alone: [R,B,n,n] and [B,n,n]"""
    per = [M.pair_tables(reals[b:b + 1, :, :v], decoded[b:b + 1, :, :v], fft_sizes, hop_sizes, win_lengths, taps)
           for b, v in enumerate(lens)]
    return {k: np.concatenate([p[k] for p in per], axis=1 if k in ("sc", "log_mag", "lin_mag") else 0) for k in KEYS}


def _take(x, idx, ok):
    """x [B,n,L], idx / ok [B,...] -> x[b, :, idx[b]] where ok, 0 elsewhere; nothing else is read"""
    B, n = x.shape[:2]
    out = np.zeros((B, n) + idx.shape[1:])
    for b in range(B):
        out[b][:, ok[b]] = x[b][:, idx[b][ok[b]]]
    return out


def mrstft_masked(reals, decoded, lens, fft_sizes=M.FFT_SIZES, hop_sizes=M.HOP_SIZES, win_lengths=None, taps=None):
    """The same tables from the padded tensors: every frame index of the longest item, the sample index
    f hop - fft / 2 + t folded at 0 and at the item's own last sample, frames at or past 1 + lens[b] / hop masked, the
    prefilter's reads past lens[b] replaced by zero, and the sums divided by the item's own counts."""
    lens = np.asarray(lens)
    B, n, Lmax = reals.shape
    win_lengths = fft_sizes if win_lengths is None else win_lengths
    pos = np.arange(Lmax)[None, :]
    valid = pos < lens[:, None]                                                       # [B,Lmax]
    r64 = _take(reals.astype(np.float64), np.broadcast_to(pos, (B, Lmax)), valid)
    d64 = _take(decoded.astype(np.float64), np.broadcast_to(pos, (B, Lmax)), valid)
    diff = r64[:, :, None, :] - d64[:, None, :, :]                                     # zero in the padding
    out = {"l1": np.abs(diff).sum(-1) / lens[:, None, None], "l2": (diff ** 2).sum(-1) / lens[:, None, None]}
    if taps is not None:
        tp, half = np.asarray(taps, dtype=np.float64), len(taps) // 2

        def fir(x):                                                                    # reads zero past the item's end
            k = pos[:, :, None] - half + np.arange(len(tp))[None, None, :]            # [1,Lmax,taps]
            k = np.broadcast_to(k, (B, Lmax, len(tp)))
            ok = (k >= 0) & (k < lens[:, None, None]) & valid[:, :, None]
            return (_take(x, np.where(ok, k, 0), ok) * tp).sum(-1)

        r64, d64 = fir(r64), fir(d64)
    sc, lg, lin = [], [], []
    for fft, hop, win in zip(fft_sizes, hop_sizes, win_lengths):
        if np.any(lens <= fft // 2):
            raise ValueError(f"an item is too short for reflect padding of {fft // 2}")
        Fb = 1 + lens // hop
        f = np.arange(Fb.max())
        idx = f[None, :, None] * hop - fft // 2 + np.arange(fft)[None, None, :]       # [1,F,fft]
        idx = np.abs(idx)
        last = (lens - 1)[:, None, None]
        idx = np.where(idx > last, 2 * last - idx, idx)                               # [B,F,fft]
        ok = np.broadcast_to((f[None, :] < Fb[:, None])[:, :, None], idx.shape)

        def mags(x):
            spec = np.fft.rfft(_take(x, np.where(ok, idx, 0), ok) * M.padded_window(fft, win), axis=-1)
            return np.sqrt(np.maximum(spec.real ** 2 + spec.imag ** 2, M.EPS))         # [B,n,F,K]

        mr, md = mags(r64), mags(d64)
        fm = ok[:, None, None, :, :1]                                                  # [B,1,1,F,1]
        cnt = ((fft // 2 + 1) * Fb)[:, None, None]
        dm = (md[:, None] - mr[:, :, None]) * fm                                       # [B,i,j,F,K]
        den = ((md ** 2) * ok[:, None, :, :1]).sum((-1, -2))
        sc.append(np.sqrt((dm ** 2).sum((-1, -2))) / np.sqrt(den)[:, None, :])
        lg.append((np.abs(np.log(mr)[:, :, None] - np.log(md)[:, None]) * fm).sum((-1, -2)) / cnt)
        lin.append(np.abs(dm).sum((-1, -2)) / cnt)
    empty = np.zeros((0, B, n, n))
    out.update(sc=np.array(sc) if sc else empty, log_mag=np.array(lg) if lg else empty,
               lin_mag=np.array(lin) if lin else empty)
    return out


def sum_terms(key, fft, hop, length):
    """N of the summation-order bound 2 N 2^-53: the terms of one table entry of an item of `length` samples"""
    return length if key in ("l1", "l2") else (fft // 2 + 1) * (1 + length // hop)


# ---------------------------------------------------------------------------------------------- score loss
def _item(a, b, f):
    return None if a is None else a[b:b + 1, ..., :f]


def score_loss_items(sde, score_of_item, y, x, t, z, frames, mode="dsm", x_t=None, score_dtype=None):
    """[B,n] float64: item b's row is the dense restatement on the item alone, cut to frames[b] frames.
    score_of_item(b) -> the callable score(x_t, t, y) of that item ([1,n,D,frames[b]]).  mode "dsm" (t, z injected; x
    already in slot order) or "init_pit" (z is z0, t ignored).  x_t [B,n,D,T]: optional override (the device's own)."""
    rows = []
    for b, f in enumerate(frames):
        args = (sde, score_of_item(b), _item(y, b, f), _item(x, b, f))
        if mode == "dsm":
            rows.append(S.compute_score_loss(*args, t[b:b + 1], _item(z, b, f), x_t=_item(x_t, b, f),
                                             score_dtype=score_dtype))
        else:
            rows.append(S.compute_score_loss_init_hack_pit(*args, _item(z, b, f), x_t=_item(x_t, b, f),
                                                           score_dtype=score_dtype))
    return torch.cat(rows)


def score_loss_masked(sde, score_padded, y, x, t, z, frames, mode="dsm"):
    """The same rows from the padded tensors: the terms (sigma score + z_j)^2 formed everywhere a finite stand-in
    allows, masked to [..., :frames[b]], summed and divided by D frames[b]; "init_pit" takes the per-slot minimum
    over the source j in the slot.  score_padded [B,n,D,T] float64: the score on the padded batch (only its valid
    region is used).  x, z may hold NaN in the padding."""
    B, n, D, T = x.shape
    fr = torch.as_tensor(frames)
    mask = (torch.arange(T)[None, :] < fr[:, None]).reshape(B, 1, 1, T)
    clean = lambda a: torch.where(mask, a.to(F64), torch.zeros((), dtype=F64))
    y, x, z, sc = clean(y), clean(x), clean(z), clean(score_padded)
    cnt = (D * fr).to(F64).reshape(B, 1)
    if mode == "dsm":
        sigma = sde.std(t.to(F64)).reshape(B, 1, 1, 1)
        return (((sigma * sc + z) ** 2) * mask).sum((-1, -2)) / cnt
    ones = torch.ones(B, dtype=F64)
    sigma = sde.std(ones).reshape(B, 1, 1, 1)
    tab = []
    for j in range(n):
        mean, _ = sde.marginal_prob(x[:, j:j + 1], ones, y)
        tab.append((((sigma * sc + z + (y - mean) / sigma) ** 2) * mask).sum((-1, -2)) / cnt)
    return torch.stack(tab, dim=-1).min(dim=-1).values


def reduce_mean(rows):
    """DSN_LOSS_REDUCE_MEAN on a ragged batch, by definition: the mean of the B n row means"""
    return rows.mean()
