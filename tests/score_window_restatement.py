"""The window-blended DiT score restated on the CPU (numpy / torch float64), independently of
ditsep_amd.native.score_window_plan and of the device:

  plan_one(T, Tw, To)       the windows of one recording and, per frame, the one or two (window, offset, weight) that
                            serve it -- written from the seams outwards (seam j = frames [(j+1) hop, (j+1) hop + To);
                            a frame outside every seam takes the window whose index is the number of seams to its left),
                            not from the frame's quotient by the hop as the product's plan is
  plan(frames, Tw, To)      the same for several recordings, window indices running through the pool
  blend64(ws, pl, T)        window scores [Wtot, n, D, Twin] -> [R, n, D, T] float64, zero past each recording's end
  windowed(score_fn, ...)   any oracle score function (oracle.dit.DiTScore) as the long-latent score, so that
                            oracle.sampler.pc_sample and oracle.pipeline.separate take it unchanged

The fade weights are ditsep_amd.native.fade_table's float32 values (the product's tables, as they stand), used as
float64 numbers: a result of this file differs from the device's by the blend's own fp32 rounding only."""
import math

import numpy as np
import torch

from ditsep_amd import native


def plan_one(T, Tw, To, fade="hann"):
    """-> (windows [(start, length)], serve): serve[f] = [(w, offset, weight)], one or two entries"""
    if 2 * To > Tw or To < 0 or Tw < 1 or T < 1:
        raise ValueError("bad window plan")
    if T <= Tw:
        return [(0, T)], [[(0, f, 1.0)] for f in range(T)]
    hop = Tw - To
    W = 1 + math.ceil((T - Tw) / hop)
    starts = [min(w * hop, T - Tw) for w in range(W)]
    fall, rise = native.fade_table(To, fade)
    serve = [None] * T
    for j in range(W - 1):
        for k in range(To):
            f = (j + 1) * hop + k
            serve[f] = [(j, f - starts[j], float(fall[k])), (j + 1, f - starts[j + 1], float(rise[k]))]
    for f in range(T):
        if serve[f] is None:
            j = sum(1 for s in range(W - 1) if f >= (s + 1) * hop + To)
            serve[f] = [(j, f - starts[j], 1.0)]
    return [(s, Tw) for s in starts], serve


def plan(frames, Tw, To, fade="hann"):
    """-> (windows [(recording, start, length)], serve[r][f] with pool-wide window indices)"""
    windows, serve = [], []
    for r, T in enumerate(frames):
        win, sv = plan_one(int(T), Tw, To, fade)
        base = len(windows)
        windows += [(r, s, l) for s, l in win]
        serve.append([[(base + w, o, wt) for w, o, wt in e] for e in sv])
    return windows, serve


def blend64(ws, serve, T):
    """ws [Wtot, n, D, Twin] (any float dtype) -> float64 [R, n, D, T]: out[r, :, :, f] = sum of weight * ws[w, :, :, o]"""
    ws = np.asarray(ws, dtype=np.float64)
    out = np.zeros((len(serve),) + ws.shape[1:3] + (T,), dtype=np.float64)
    for r, sv in enumerate(serve):
        for f, e in enumerate(sv):
            if len(e) == 1:
                out[r, :, :, f] = ws[e[0][0], :, :, e[0][1]]
            else:
                out[r, :, :, f] = sum(wt * ws[w, :, :, o] for w, o, wt in e)
    return out


def cut(x, windows, Twin):
    """x [R, C.., T] torch -> [Wtot, C.., Twin]: the windows cut on the host, zero past a short window's length"""
    out = torch.zeros((len(windows),) + tuple(x.shape[1:-1]) + (Twin,), dtype=x.dtype)
    for i, (r, s, l) in enumerate(windows):
        out[i, ..., :l] = x[r, ..., s:s + l]
    return out


def window_scores(score_fn, xt, t, y, windows):
    """every window through score_fn at ITS OWN length, the windows of one length in one batch -> list of
    [n, D, length] tensors"""
    out = [None] * len(windows)
    for l in sorted({w[2] for w in windows}):
        idx = [i for i, w in enumerate(windows) if w[2] == l]
        xw = torch.stack([xt[windows[i][0], ..., windows[i][1]:windows[i][1] + l] for i in idx])
        yw = torch.stack([y[windows[i][0], ..., windows[i][1]:windows[i][1] + l] for i in idx])
        tw = torch.stack([t[windows[i][0]] for i in idx])
        sc = score_fn(xw.contiguous(), tw, yw.contiguous())
        for j, i in enumerate(idx):
            out[i] = sc[j]
    return out


def windowed(score_fn, Tw, To, frames, fade="hann"):
    """score_fn(xt [B,n,D,T'], t [B], y [B,1,D,T']) -> the long-latent score fn(xt [R,n,D,T], t [R], y [R,1,D,T]) ->
    [R,n,D,T] float32, blended in float64, zero past each recording's frames[r]"""
    windows, serve = plan(frames, Tw, To, fade)
    Twin = max(w[2] for w in windows)

    def fn(xt, t, y):
        assert xt.shape[0] == len(frames) and xt.shape[-1] >= max(frames)
        sc = window_scores(score_fn, xt, t, y, windows)
        ws = np.zeros((len(windows),) + tuple(xt.shape[1:3]) + (Twin,), dtype=np.float64)
        for i, s in enumerate(sc):
            ws[i, :, :, :s.shape[-1]] = s.double().numpy()
        return torch.from_numpy(blend64(ws, serve, xt.shape[-1])).to(torch.float32)

    fn.windows, fn.serve, fn.Twin = windows, serve, Twin
    return fn
