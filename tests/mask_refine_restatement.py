"""Restatement of dsn_mask_refine (include/ditsep_hip.h): mixture-consistent STFT masks, written twice.

Per item: mixture m [L], estimates s [n, L], parameters n_fft, hop, power in {1, 2}, eps > 0.
  Lp = hop ceil(L / hop); every signal is zero-extended to Lp
  STFT: centred frames of n_fft samples every hop samples over the signal reflect-padded by n_fft / 2 on both sides
        (F = 1 + Lp / hop frames, bins 0 .. n_fft / 2), periodic Hann window computed in float64 and rounded once to
        float32
  a_i = |S_i|^power,  M_i = (a_i + eps) / (sum_j a_j + n eps),  Y_i = M_i X            (X: the mixture's STFT)
  y_i = the overlap-add of the windowed inverse frames of Y_i divided, per sample, by the sum of w^2 over the frames
        that cover it; cropped to L

(a) `refine_torch`: torch.stft / torch.istft (center = True, pad_mode = "reflect").
(b) `refine_numpy`: explicit framing with numpy.fft.rfft / irfft.

Both take the working dtype (float64: the reference; float32: the yardstick of the device's rounding error) and return
[n, L] in that dtype."""
import numpy as np
import torch

DEFAULTS = dict(n_fft=512, hop=128, power=2, eps=1e-10)


def padded_length(L: int, hop: int) -> int:
    return hop * (-(-int(L) // hop))


def window(n_fft: int, dtype=np.float64) -> np.ndarray:
    """periodic Hann in float64, rounded once to float32, then held in `dtype`"""
    w = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n_fft, dtype=np.float64) / n_fft)
    return w.astype(np.float32).astype(dtype)


def masks(S, power=2, eps=1e-10):
    """S [n, ...] complex -> M [n, ...] real, sums to 1 over the first axis"""
    a = np.abs(S) if power == 1 else S.real ** 2 + S.imag ** 2
    return (a + a.dtype.type(eps)) / (a.sum(axis=0) + a.dtype.type(S.shape[0]) * a.dtype.type(eps))


def refine_torch(mix, est, n_fft=512, hop=128, power=2, eps=1e-10, dtype=np.float64):
    mix = np.asarray(mix, dtype=dtype)
    est = np.asarray(est, dtype=dtype)
    n, L = est.shape
    Lp = padded_length(L, hop)
    tdt = torch.float64 if dtype == np.float64 else torch.float32
    x = torch.zeros((n + 1, Lp), dtype=tdt)
    x[0, :L] = torch.from_numpy(mix)
    x[1:, :L] = torch.from_numpy(est)
    w = torch.from_numpy(window(n_fft, dtype))
    Z = torch.stft(x, n_fft, hop_length=hop, win_length=n_fft, window=w, center=True, pad_mode="reflect",
                   return_complex=True)                                          # [n + 1, n_fft / 2 + 1, F]
    assert Z.shape[-1] == 1 + Lp // hop
    X, S = Z[0], Z[1:]
    a = S.abs() if power == 1 else S.real ** 2 + S.imag ** 2
    e = torch.tensor(eps, dtype=tdt)
    M = (a + e) / (a.sum(dim=0) + torch.tensor(float(n), dtype=tdt) * e)
    y = torch.istft(M * X, n_fft, hop_length=hop, win_length=n_fft, window=w, center=True, length=Lp)
    return y[:, :L].numpy()


def frames_of(x, n_fft, hop, w):
    """x [Lp] -> the windowed frames [F, n_fft] of the reflect-padded signal"""
    half = n_fft // 2
    xp = np.concatenate([x[1:half + 1][::-1], x, x[-half - 1:-1][::-1]])
    F = 1 + len(x) // hop
    return np.stack([xp[f * hop:f * hop + n_fft] for f in range(F)]) * w


def refine_numpy(mix, est, n_fft=512, hop=128, power=2, eps=1e-10, dtype=np.float64):
    mix = np.asarray(mix, dtype=dtype)
    est = np.asarray(est, dtype=dtype)
    n, L = est.shape
    Lp = padded_length(L, hop)
    half = n_fft // 2
    cdt = np.complex128 if dtype == np.float64 else np.complex64
    w = window(n_fft, dtype)
    x = np.zeros((n + 1, Lp), dtype=dtype)
    x[0, :L] = mix
    x[1:, :L] = est
    Z = np.stack([np.fft.rfft(frames_of(r, n_fft, hop, w), axis=-1).astype(cdt) for r in x])   # [n + 1, F, bins]
    M = masks(Z[1:], power=power, eps=eps)
    Y = M * Z[0]
    F = Z.shape[1]
    out = np.zeros((n, Lp + n_fft), dtype=dtype)
    env = np.zeros(Lp + n_fft, dtype=dtype)
    for f in range(F):                                                           # frame order
        out[:, f * hop:f * hop + n_fft] += np.fft.irfft(Y[:, f], n=n_fft, axis=-1).astype(dtype) * w
        env[f * hop:f * hop + n_fft] += w * w
    return (out[:, half:half + Lp] / env[half:half + Lp])[:, :L].astype(dtype)


def make_case(seed, n, L, noise=0.3):
    """seeded Gaussian sources with noisy estimates -> (mix [L], est [n, L]) float32"""
    g = np.random.default_rng(seed)
    src = g.standard_normal((n, L)) * 0.1
    mix = src.sum(axis=0)
    est = src + noise * 0.1 * g.standard_normal((n, L))
    return mix.astype(np.float32), est.astype(np.float32)


def rel_err(a, b, mix):
    return float(np.max(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))) / np.max(np.abs(mix)))
