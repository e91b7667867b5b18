"""Float64 restatement of the score-matching loss methods of the reference's LatentDiffSep
(src/diffsep_latent.py:130-208) with every random draw injected.

sample_prior :134-145, compute_score_loss :154-160, compute_score_loss_init_hack_pit :162-187 (the reference's
own enumeration of all n! permutations, one score evaluation each), train_step_init_5 :189-208 with
utils.shuffle_sources (utils/separate.py:3-21) replaced by its gather on injected indices, and OUVESDE.marginal_prob
(sdes/sdes.py:662-685).  `score(x_t, t, y)` is any callable returning [B,n,D,T]; it is evaluated on float64 tensors
unless `score_dtype` says otherwise.  Nothing here imports the engine.
"""
from __future__ import annotations

import itertools

import torch

F64 = torch.float64


def toy_score(x, t, y):
    """Closed-form stand-in score whose value depends on the source slot (so that a permuted target matters).
    Its slope is small on purpose: sigma^2 reaches 61 at t = 1, and with the samplers' toy slope of 0.05 the term
    sigma * score comes to cancel z at some t (the toy turns into a nearly exact score there).  The loss is then a
    small difference of O(1) terms and the reference's OWN fp32 rounding is amplified by |z| / |sigma s + z|: the
    captured fp32 loss of such an item sat 1.5e-6 from the float64 value, i.e. the fixture, not the restatement,
    left the 1e-6 the fixture comparison allows."""
    tt = t.reshape(-1, 1, 1, 1)
    slot = 1.0 + 0.5 * torch.arange(x.shape[1], dtype=x.dtype, device=x.device).reshape(1, -1, 1, 1)
    return -(x - y) * 0.005 / (1 + tt) + 0.01 * slot * torch.tanh(x)


class SDE:
    """OUVESDE closed forms (reference sdes/sdes.py:625-685) in the dtype of `t`."""

    def __init__(self, theta=1.5, sigma_min=0.96, sigma_max=10.0, N=30):
        self.theta, self.sigma_min, self.sigma_max, self.N = float(theta), float(sigma_min), float(sigma_max), int(N)
        self.logsig = float(torch.log(torch.tensor(self.sigma_max / self.sigma_min, dtype=F64)))
        self.T = 1

    def mean(self, x0, t, y):
        e = torch.exp(-self.theta * t)
        e = e.reshape(e.shape + (1,) * (x0.ndim - e.ndim))
        return e * x0 + (1 - e) * y

    def std(self, t):
        smin, th, ls = self.sigma_min, self.theta, self.logsig
        return torch.sqrt(smin ** 2 * torch.exp(-2 * th * t) * (torch.exp(2 * (th + ls) * t) - 1) * ls / (th + ls))

    def marginal_prob(self, x0, t, y):
        return self.mean(x0, t, y), self.std(t)


def _call(score, x_t, t, y, score_dtype):
    if score_dtype is None:
        return score(x_t, t, y).to(F64)
    return score(x_t.to(score_dtype), t.to(score_dtype), y.to(score_dtype)).to(F64)


def mse(a, b, reduction):
    """torch.nn.MSELoss(reduction=...)"""
    d = (a - b) ** 2
    return d.mean() if reduction == "mean" else d


def trailing_mean(loss):
    """`loss.mean(dim=tuple(range(2 - loss.ndim, 0)))`: the last ndim - 2 axes ([B,n,D,T] -> [B,n]); a scalar stays."""
    dims = tuple(range(2 - loss.ndim, 0))
    return loss.mean(dim=dims) if dims else loss


def sample_prior(sde, mix, target, t, z):
    """-> (x_t, t, sigma [B,1,1,1], z) from injected t [B] and z [B,n,D,T]."""
    mix, target, t, z = (a.to(F64) for a in (mix, target, t, z))
    mean, std = sde.marginal_prob(target, t, mix)
    sigma = std.reshape(std.shape + (1,) * (mean.ndim - std.ndim))
    return mean + sigma * z, t, sigma, z


def compute_score_loss(sde, score, y, x, t, z, reduction="none", score_dtype=None, x_t=None):
    """x_t: optional override of the perturbed state fed to the score (e.g. the device's own fp32 x_t)."""
    xt, t, sigma, z = sample_prior(sde, y, x, t, z)
    if x_t is not None:
        xt = x_t.to(F64)
    pred = _call(score, xt, t, y.to(F64), score_dtype)
    return trailing_mean(mse(pred * sigma, -z, reduction))


def compute_score_loss_init_hack_pit(sde, score, mix, target, z0, reduction="none", score_dtype=None, x_t=None,
                                     count=None):
    """The reference's loop over all permutations, one score evaluation per permutation (count["calls"] counts
    them), then stack(dim=1).min(dim=1)."""
    mix, target, z0 = (a.to(F64) for a in (mix, target, z0))
    time = torch.ones(mix.shape[0], dtype=F64) * sde.T
    losses = []
    for perm in itertools.permutations(range(target.shape[1])):
        mean, std = sde.marginal_prob(target[:, list(perm)], time, mix)
        sigma = std.reshape(std.shape + (1,) * (mix.ndim - std.ndim))
        z = z0 + (mix - mean) / sigma
        xt = mix + sigma * z0 if x_t is None else x_t.to(F64)
        pred = _call(score, xt, time, mix, score_dtype)
        if count is not None:
            count["calls"] = count.get("calls", 0) + 1
        losses.append(trailing_mean(mse(pred * sigma, -z, reduction)))
    return torch.stack(losses, dim=1).min(dim=1).values


def shuffle_sources(x, idx):
    """utils.shuffle_sources with its argsort result injected: out[b, s] = x[b, idx[b, s]]."""
    idx = idx.reshape(idx.shape + (1,) * (x.ndim - 2)).expand(x.shape)
    return torch.gather(x, 1, idx)


def train_step_init_5(sde, score, mix, target, pit_mask, z0_pit, perm, t, z, score_dtype=None):
    """pit_mask [B] bool; z0_pit [n_pit,n,D,T]; perm [B - n_pit, n] (shuffle indices), t [B - n_pit], z for the
    rest.  reduction is "none" here (the reference forces it for init_hack == 5)."""
    pit_mask = pit_mask.bool()
    losses = []
    if int(pit_mask.sum()) > 0:
        losses.append(compute_score_loss_init_hack_pit(sde, score, mix[pit_mask], target[pit_mask], z0_pit,
                                                       score_dtype=score_dtype))
    if int(pit_mask.sum()) != mix.shape[0]:
        tgt = shuffle_sources(target[~pit_mask], perm.long())
        losses.append(compute_score_loss(sde, score, mix[~pit_mask], tgt, t, z, score_dtype=score_dtype))
    return torch.cat(losses).mean()
