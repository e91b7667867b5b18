"""Capture tests/golden/score_loss.npz from the reference's own LatentDiffSep methods (build container only).

Run:  python scripts/make_golden_score_loss.py     (exits cleanly when the reference tree is absent)

The reference module (src/diffsep_latent.py) is imported as it is, with `sys.modules` stubs for the third-party
packages it names at import time that are not installed here (pytorch_lightning, omegaconf, torch_ema,
fast_bss_eval -- on top of what oracle/reference_loader.py already stubs).  Its methods sample_prior,
compute_score_loss, compute_score_loss_init_hack_pit and train_step_init_5 are then called on an instance made with
object.__new__ whose attributes (sde, loss, t_eps, t_max, init_hack_p, score_model) are set by hand; the score model
is the closed-form toy of tests/score_loss_restatement.py.  The methods draw from torch's global generator: every
case is run under torch.manual_seed(seed), and the draws (t, z, the PIT mask, the shuffle's argsort) are recorded by
replaying that seed with the same calls in the same order; the replay is checked against the (x_t, t) the reference
handed to the score model.  Only arrays are stored.
"""
from __future__ import annotations

import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import reference_loader as rl  # noqa: E402
from tests.score_loss_restatement import toy_score  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "score_loss.npz")
SDE = dict(theta=1.5, sigma_min=0.96, sigma_max=10.0, N=30)
T_EPS = 0.03
D, T = 8, 6


def _stub(name, **attrs):
    m = types.ModuleType(name)
    for k, v in attrs.items():
        setattr(m, k, v)
    sys.modules[name] = m
    return m


def load_reference_module():
    ns = rl.load()
    import importlib

    class _Ctx:
        def __init__(self, *a, **k):
            pass

        def __enter__(self):
            return self

        def __exit__(self, *a):
            return False

    if "pytorch_lightning" not in sys.modules:
        _stub("pytorch_lightning", LightningModule=torch.nn.Module)
    if "omegaconf" not in sys.modules:
        oc = _stub("omegaconf", DictConfig=dict)
        oc.omegaconf = _stub("omegaconf.omegaconf", open_dict=_Ctx)
    if "torch_ema" not in sys.modules:
        _stub("torch_ema", ExponentialMovingAverage=_Ctx)
    if "fast_bss_eval" not in sys.modules:
        _stub("fast_bss_eval")
    utils = sys.modules["utils"]          # bare namespace set up by reference_loader (skips utils/__init__.py)
    sep = importlib.import_module("utils.separate")
    utils.shuffle_sources = sep.shuffle_sources
    mod = importlib.import_module("diffsep_latent")
    return ns, mod


class _Recorder(torch.nn.Module):
    """score_model: the toy score, remembering what it was called with"""

    def __init__(self):
        super().__init__()
        self.calls = []

    def forward(self, xt, time, mix):
        self.calls.append((xt.clone(), time.clone()))
        return toy_score(xt, time, mix)


def make_model(mod, ns, reduction):
    m = object.__new__(mod.LatentDiffSep)
    torch.nn.Module.__init__(m)
    m.sde = ns.OUVESDE(**SDE)
    m.loss = torch.nn.MSELoss() if reduction == "mean" else torch.nn.MSELoss(reduction="none")
    m.t_eps, m.t_max = T_EPS, m.sde.T
    m.init_hack_p = 0.5
    m.score_model = _Recorder()
    return m


def inputs(B, n, seed):
    g = torch.Generator().manual_seed(seed)
    mix = torch.randn((B, 1, D, T), generator=g)
    target = 0.7 * torch.randn((B, n, D, T), generator=g)
    return mix, target


def main():
    if not rl.available():
        print("reference tree not present: nothing captured")
        return 0
    ns, mod = load_reference_module()
    out = {"D": D, "T": T, "t_eps": T_EPS, **{f"sde_{k}": v for k, v in SDE.items()}}
    for n in (2, 3):
        B = 4
        mix, target = inputs(B, n, 200 + n)
        out[f"mix_n{n}"], out[f"target_n{n}"] = mix, target
        for red in ("none", "mean"):
            tag = f"n{n}_{red}"
            # ---- sample_prior + compute_score_loss
            m = make_model(mod, ns, red)
            seed = 300 + n
            torch.manual_seed(seed)
            loss = m.compute_score_loss(mix, target)
            torch.manual_seed(seed)
            t = target.new_zeros(B).uniform_(T_EPS, 1)
            z = torch.randn_like(target)
            (xt, tt), = m.score_model.calls
            assert torch.equal(tt, t)
            torch.manual_seed(seed)
            x_t, t2, sigma, z2 = m.sample_prior(mix, target)
            assert torch.equal(x_t, xt) and torch.equal(z2, z) and torch.equal(t2, t)
            mean, _ = m.sde.marginal_prob(x0=target, t=t, y=mix)
            out.update({f"dsm_t_{tag}": t, f"dsm_z_{tag}": z, f"dsm_xt_{tag}": x_t, f"dsm_sigma_{tag}": sigma,
                        f"dsm_mean_{tag}": mean, f"dsm_loss_{tag}": loss})
            # ---- compute_score_loss_init_hack_pit (reduction "none" only: with MSELoss() the reference's
            # torch.stack(losses, dim=1) of scalars raises IndexError)
            m = make_model(mod, ns, red)
            if red == "mean":
                try:
                    m.compute_score_loss_init_hack_pit(mix, target)
                    raise AssertionError("expected the reference to fail")
                except IndexError:
                    continue
            seed = 400 + n
            torch.manual_seed(seed)
            loss = m.compute_score_loss_init_hack_pit(mix, target)
            torch.manual_seed(seed)
            z0 = torch.randn_like(target)
            assert len(m.score_model.calls) == int(np.prod(range(1, n + 1)))
            std1 = m.sde._std(torch.ones(B))
            for xt, tt in m.score_model.calls:     # every permutation sees the same x_t and t
                assert torch.equal(xt, mix + std1[:, None, None, None] * z0) and torch.equal(tt, torch.ones(B))
            out.update({f"pit_z0_{tag}": z0, f"pit_xt_{tag}": m.score_model.calls[0][0], f"pit_loss_{tag}": loss,
                        f"pit_sigma_{tag}": std1})
        # ---- train_step_init_5 (reduction "none"), a seed whose mask hits both branches
        B5 = 6
        mix5, target5 = inputs(B5, n, 500 + n)
        for seed in range(600, 700):
            torch.manual_seed(seed)
            pit = mix5.new_zeros(B5).uniform_() < 0.5
            if 0 < int(pit.sum()) < B5:
                break
        m = make_model(mod, ns, "none")
        torch.manual_seed(seed)
        loss = m.train_step_init_5(mix5, target5)
        torch.manual_seed(seed)
        pit = mix5.new_zeros(B5).uniform_() < m.init_hack_p
        z0 = torch.randn_like(target5[pit])
        c = target5[~pit].new_zeros(target5[~pit].shape[:2]).uniform_()
        idx = torch.argsort(c, dim=1)
        t = target5[~pit].new_zeros(int((~pit).sum())).uniform_(T_EPS, 1)
        z = torch.randn_like(target5[~pit])
        xt_last, t_last = m.score_model.calls[-1]
        assert torch.equal(t_last, t)
        out.update({f"ts5_mix_n{n}": mix5, f"ts5_target_n{n}": target5, f"ts5_mask_n{n}": pit, f"ts5_z0_n{n}": z0,
                    f"ts5_perm_n{n}": idx, f"ts5_t_n{n}": t, f"ts5_z_n{n}": z, f"ts5_xt_n{n}": xt_last,
                    f"ts5_loss_n{n}": loss, f"ts5_p_n{n}": m.init_hack_p})
    conv = {k: (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)) for k, v in out.items()}
    np.savez_compressed(OUT, **conv)
    print(f"wrote {OUT} ({os.path.getsize(OUT) / 1024:.1f} KiB, {len(conv)} arrays)")
    return 0


if __name__ == "__main__":
    sys.exit(main())
