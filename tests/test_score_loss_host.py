"""Host checks of the score-matching loss: the float64 restatement (tests/score_loss_restatement.py) against the
arrays captured from the reference's own methods (tests/golden/score_loss.npz, scripts/make_golden_score_loss.py),
the reference's shape quirks, and the config handling of ditsep_amd.latent.loss_config.

Bound: 1e-6 relative.  The fixture is the reference's fp32 arithmetic, the restatement float64: a few ulp (6e-8)
per element, and the losses are averages of non-negative terms, so nothing is amplified.  Element-wise arrays
(x_t, mean) are compared against the largest magnitude of the array (x_t = mean + sigma z cancels per element)."""
import os

import numpy as np
import pytest
import torch

from ditsep_amd import latent, native, sdes
from tests import score_loss_restatement as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "score_loss.npz")
TOL = 1e-6


@pytest.fixture(scope="module")
def g():
    z = np.load(GOLDEN)
    return {k: torch.from_numpy(np.asarray(z[k])) for k in z.files}


def sde_of(g):
    return R.SDE(float(g["sde_theta"]), float(g["sde_sigma_min"]), float(g["sde_sigma_max"]), int(g["sde_N"]))


def rel_max(a, b):
    a, b = a.double(), b.double()
    return float((a - b).abs().max() / b.abs().max())


def rel_each(a, b):
    a, b = a.double(), b.double()
    return float(((a - b).abs() / b.abs()).max())


@pytest.mark.parametrize("n", [2, 3])
@pytest.mark.parametrize("red", ["none", "mean"])
def test_restatement_reproduces_sample_prior_and_dsm_loss(g, n, red):
    sde, tag = sde_of(g), f"n{n}_{red}"
    mix, target, t, z = g[f"mix_n{n}"], g[f"target_n{n}"], g[f"dsm_t_{tag}"], g[f"dsm_z_{tag}"]
    x_t, t64, sigma, _ = R.sample_prior(sde, mix, target, t, z)
    assert sigma.shape == (mix.shape[0], 1, 1, 1)
    assert rel_each(sigma, g[f"dsm_sigma_{tag}"]) <= TOL
    assert rel_max(x_t, g[f"dsm_xt_{tag}"]) <= TOL
    assert rel_max(sde.mean(target.double(), t.double(), mix.double()), g[f"dsm_mean_{tag}"]) <= TOL
    loss = R.compute_score_loss(sde, R.toy_score, mix, target, t, z, reduction=red)
    want = g[f"dsm_loss_{tag}"]
    # MSELoss(reduction="none") leaves [B, n]: the reference's mean runs over (D, T) only
    assert tuple(want.shape) == ((mix.shape[0], n) if red == "none" else ())
    assert loss.shape == want.shape
    assert rel_each(loss, want) <= TOL


@pytest.mark.parametrize("n", [2, 3])
def test_restatement_reproduces_pit_loss_and_slot_minimum(g, n):
    sde, tag = sde_of(g), f"n{n}_none"
    mix, target, z0 = g[f"mix_n{n}"], g[f"target_n{n}"], g[f"pit_z0_{tag}"]
    count = {}
    loss = R.compute_score_loss_init_hack_pit(sde, R.toy_score, mix, target, z0, count=count)
    want = g[f"pit_loss_{tag}"]
    assert count["calls"] == {2: 2, 3: 6}[n]
    assert tuple(want.shape) == (mix.shape[0], n) and loss.shape == want.shape
    assert rel_each(loss, want) <= TOL
    assert rel_each(sde.std(torch.ones(mix.shape[0], dtype=torch.float64)), g[f"pit_sigma_{tag}"]) <= TOL
    # the minimum is taken per (item, slot): it equals min_j of the n x n table of "source j in slot s" losses, and is
    # in general below the best whole-assignment loss
    sigma = sde.std(torch.ones(1, dtype=torch.float64))
    m, tg, z = mix.double(), target.double(), z0.double()
    xt = m + sigma * z
    pred = R.toy_score(xt, torch.ones(mix.shape[0], dtype=torch.float64), m)
    table = torch.stack([torch.stack([
        ((pred[:, s] * sigma + z[:, s] + (m[:, 0] - sde.mean(tg[:, j], torch.ones(mix.shape[0], dtype=torch.float64),
                                                              m[:, 0])) / sigma) ** 2).mean(dim=(-2, -1))
        for j in range(n)], dim=1) for s in range(n)], dim=1)          # [B, slot, source]
    assert rel_each(table.min(dim=2).values, want) <= TOL


@pytest.mark.parametrize("n", [2, 3])
def test_restatement_reproduces_train_step_init_5(g, n):
    sde = sde_of(g)
    mask = g[f"ts5_mask_n{n}"].bool()
    assert 0 < int(mask.sum()) < mask.numel()          # both branches
    loss = R.train_step_init_5(sde, R.toy_score, g[f"ts5_mix_n{n}"], g[f"ts5_target_n{n}"], mask, g[f"ts5_z0_n{n}"],
                               g[f"ts5_perm_n{n}"], g[f"ts5_t_n{n}"], g[f"ts5_z_n{n}"])
    want = g[f"ts5_loss_n{n}"]
    assert loss.shape == want.shape == ()
    assert rel_each(loss, want) <= TOL
    # the shuffled non-PIT branch's x_t, as the reference handed it to the score model
    tgt = R.shuffle_sources(g[f"ts5_target_n{n}"][~mask], g[f"ts5_perm_n{n}"].long())
    x_t, *_ = R.sample_prior(sde, g[f"ts5_mix_n{n}"][~mask], tgt, g[f"ts5_t_n{n}"], g[f"ts5_z_n{n}"])
    assert rel_max(x_t, g[f"ts5_xt_n{n}"]) <= TOL


def test_host_marginal_prob_matches_fixture_and_restatement(g):
    """ditsep_amd.sdes.OUVESDE.marginal_prob (host torch forms) against the reference's arrays."""
    sde = sdes.OUVESDE(float(g["sde_theta"]), float(g["sde_sigma_min"]), float(g["sde_sigma_max"]), N=int(g["sde_N"]))
    for n in (2, 3):
        tag = f"n{n}_none"
        t = g[f"dsm_t_{tag}"]
        mean, std = sde.marginal_prob(g[f"target_n{n}"].double(), t.double(), g[f"mix_n{n}"].double())
        assert rel_max(mean, g[f"dsm_mean_{tag}"]) <= TOL
        assert rel_each(std, g[f"dsm_sigma_{tag}"].reshape(-1)) <= TOL
        assert rel_each(std, sde_of(g).std(t.double())) <= 1e-12


def test_loss_config_follows_the_reference():
    lc = latent.loss_config
    assert lc({"model": {}}, 30) == {"init_hack": False, "init_hack_p": 1.0 / 30, "reduction": "mean"}
    assert lc({"model": {"loss": {"_target_": "torch.nn.MSELoss"}, "init_hack": 5}}, 50) == {
        "init_hack": 5, "init_hack_p": 1.0 / 50, "reduction": "none"}
    assert lc({"model": {"loss": {"_target_": "torch.nn.MSELoss", "reduction": "none"}, "init_hack": 5,
                         "init_hack_p": 0.25}}, 30)["init_hack_p"] == 0.25
    assert lc({"model": {"loss": {"_target_": "torch.nn.MSELoss", "reduction": "none"}}}, 30)["reduction"] == "none"
    with pytest.raises(ValueError, match="Reduction should 'none'"):
        lc({"model": {"loss": {"_target_": "torch.nn.MSELoss", "reduction": "mean"}, "init_hack": 5}}, 30)
    with pytest.raises(NotImplementedError, match="L1Loss"):
        lc({"model": {"loss": {"_target_": "torch.nn.L1Loss"}}}, 30)
    with pytest.raises(NotImplementedError, match="sum"):
        lc({"model": {"loss": {"_target_": "torch.nn.MSELoss", "reduction": "sum"}}}, 30)


def test_binding_declares_the_entry_point_and_its_enums():
    lib = native.load_library()
    assert hasattr(lib, "dsn_score_loss") and "dsn_score_loss" in native.EXPORTS
    hdr = open(os.path.join(os.path.dirname(GOLDEN), "..", "..", "include", "ditsep_hip.h")).read()
    for name, val in (("DSN_LOSS_DSM", native.LOSS_MODES["dsm"]), ("DSN_LOSS_INIT_PIT", native.LOSS_MODES["init_pit"]),
                      ("DSN_LOSS_REDUCE_NONE", native.LOSS_REDUCTIONS["none"]),
                      ("DSN_LOSS_REDUCE_MEAN", native.LOSS_REDUCTIONS["mean"])):
        assert f"{name} = {val}" in hdr
    assert [f[0] for f in native.DsnLossOpts._fields_] == ["mode", "reduction", "t_eps"]
    for m in ("sample_time", "sample_prior", "compute_score_loss", "compute_score_loss_init_hack_pit",
              "train_step_init_5", "validation_step"):
        assert callable(getattr(latent.LatentDiffSep, m))
