"""GPU: the native probability-flow ODE sampler (dsn_ode_sample, ditsep_amd/csrc/ode.hip) against the float64
restatement of scipy's solve_ivp (tests/ode_restatement.py) driven by the CPU oracle networks.

Expected: the same nfev (every accept / reject decision and step size the same) and rel-L2(x) <= 1e-4 in the bf16x3
parity mode.  Measured: the error estimator works at the score network's own rounding level, and bf16x3 (~1e-5
relative) moves step sizes.  Tiny DiT, RK45, seed 9, rtol = atol = 1e-5: 44 evaluations on the device against 38 in
the restatement (one more accepted step, no decision flipped), rel-L2 8.2e-6; the restatement alone goes from 38 to 44
when its score is perturbed by 1e-5 relative noise (1e-6: unchanged).  RK23, and RK45 at 1e-4: identical counts.
Tiny NCSN++, RK45, which rejects 8-10 steps at 1e-5: there the count moves with a 1-ulp change of x_T alone (two
builds differing only in whether the prior was computed with an FMA: T = 8 422 then 404 evaluations against 422, T = 6
428 then 422 against 434, i.e. 0 to 3 of ~70 attempts); rel-L2 5.6e-5 ... 7.2e-5.  At 1e-4 (1 rejection): 158 and 170
or 176 against 158 and 176, rel-L2 1.1e-4 ... 1.8e-4.  Full-size DiT at 1e-4: identical counts (38), rel-L2 2.1e-6.
So the tests assert equal counts where they were measured equal in every run (tiny DiT at 1e-4, the forced-rejection
case), allow elsewhere a difference of at most 10 % of the restatement's attempts (at least 2; measured at most 4 %),
and hold rel-L2 to 1e-4 except tiny NCSN++ at 1e-4 (3e-4) and the full-size DiT (1e-3).  Each test prints its margins,
the attempt difference included ("ode-margin ...", visible with -s)."""
import json

import numpy as np
import pytest
import torch

from oracle import dit as odit
from oracle import oobleck as ovae
from oracle.make_golden import tiny_vae_weights
from tests import ode_restatement as ode
from tests.util import make_engine, rel_l2

pytestmark = pytest.mark.gpu

X3 = 2
THETA, SMIN, SMAX = 1.5, float(np.float32(0.96)), 10.0   # the engine holds the SDE parameters as float32


def _oracle_score(net, ymix):
    def score(x, t):
        B = x.shape[0]
        with torch.no_grad():
            return net(torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)), torch.full((B,), float(t)),
                       ymix).double().numpy()
    return score


def _restated(net, ymix, z, n_src, **kw):
    return ode.ode_sample(_oracle_score(net, ymix), ymix.numpy(), z.numpy(), n_src=n_src, theta=THETA,
                          sigma_min=SMIN, sigma_max=SMAX, **kw)


def _attempt_diff(nfe, sol, method):
    return (nfe - sol["nfev"]) / ode.TABLEAUX[method]["n_stages"]


def _report(name, nfe, st, sol, err, method="RK45"):
    print("ode-margin " + json.dumps({"test": name, "nfev": nfe, "ref_nfev": sol["nfev"],
                                      "attempt_diff": _attempt_diff(nfe, sol, method), "accepted": st["n_accepted"],
                                      "rejected": st["n_rejected"], "ref_accepted": sol["n_accepted"],
                                      "ref_rejected": sol["n_rejected"], "rel_l2": err}))


def _check_nfev(nfe, sol, st, exact, method):
    if exact:
        assert nfe == sol["nfev"] and st["n_accepted"] == sol["n_accepted"] and st["n_rejected"] == sol["n_rejected"]
    else:   # the estimator at the score network's rounding level (module docstring): measured <= 4 %, bound 10 %
        assert abs(_attempt_diff(nfe, sol, method)) <= max(2, 0.1 * sol["attempts"])


def _tiny_dit():
    cfg = odit.DiTConfig(n_src=2, embed_dim=128, depth=2, num_heads=2)
    sd = odit.random_dit_weights(cfg, 32, out_gain=0.005)
    return cfg, sd


@pytest.fixture(scope="module")
def tiny_dit_engine():
    cfg, sd = _tiny_dit()
    eng = make_engine(cfg, sd, precision=X3)
    yield cfg, sd, eng
    eng.close()


@pytest.mark.parametrize("method", ["RK45", "RK23"])
@pytest.mark.parametrize("denoise", [True, False])
@pytest.mark.parametrize("tol", [1e-5, 1e-4])
def test_ode_tiny_dit_matches_restatement(tiny_dit_engine, method, denoise, tol):
    torch.set_num_threads(16)
    cfg, sd, eng = tiny_dit_engine
    g = torch.Generator().manual_seed(9)
    B, T = 3, 4
    ymix = torch.randn((B, 1, 64, T), generator=g)
    z = torch.randn((B, 2, 64, T), generator=g)
    x, nfe, st = eng.ode_sample(ymix, z, method=method, denoise=denoise, N=30, rtol=tol, atol=tol, return_stats=True)
    ref, sol = _restated(odit.DiTScore(sd, cfg), ymix, z, 2, method=method, denoise=denoise, N=30, rtol=tol, atol=tol)
    err = rel_l2(x, torch.from_numpy(ref))
    _report(f"tiny_dit/{method}/denoise={denoise}/tol={tol}", nfe, st, sol, err, method)
    assert st["status"] == "finished" and st["t_final"] == 0.03
    _check_nfev(nfe, sol, st, tol >= 1e-4, method)
    assert err <= 1e-4


@pytest.mark.parametrize("T", [8, 6])   # T = 6: the score net pads the frames to a multiple of max_latent_length
@pytest.mark.parametrize("tol", [1e-5, 1e-4])
def test_ode_tiny_ncsnpp_matches_restatement(T, tol):
    from oracle import ncsnpp as oncs

    torch.set_num_threads(16)
    cfg = oncs.NCSNppConfig(n_src=2, nf=32)
    sd = oncs.random_ncsnpp_weights(cfg, 41)
    eng = make_engine(ncfg=cfg, nsd=sd, precision=X3)
    g = torch.Generator().manual_seed(10 + T)
    B = 2
    ymix = torch.randn((B, 1, 64, T), generator=g)
    z = torch.randn((B, 2, 64, T), generator=g)
    x, nfe, st = eng.ode_sample(ymix, z, method="RK45", denoise=True, N=30, rtol=tol, atol=tol, return_stats=True)
    ref, sol = _restated(oncs.NCSNppScore(sd, cfg), ymix, z, 2, method="RK45", denoise=True, N=30, rtol=tol, atol=tol)
    err = rel_l2(x, torch.from_numpy(ref))
    _report(f"tiny_ncsnpp/T={T}/tol={tol}", nfe, st, sol, err)
    _check_nfev(nfe, sol, st, False, "RK45")
    assert err <= (1e-4 if tol < 1e-4 else 3e-4)
    eng.close()


def test_ode_full_size_dit_matches_restatement():
    """default DiT dimensions (1024 wide, 24 layers) at B = 2, rtol = atol = 1e-4.  Loose bounds (measured: equal
    counts, rel-L2 2.1e-6): rel-L2 <= 1e-3 and the count slack of the other cases."""
    torch.set_num_threads(16)
    cfg = odit.DiTConfig(n_src=2)
    sd = odit.random_dit_weights(cfg, 5, out_gain=0.005)   # unit out_gain makes the flow stiff (step underflow)
    eng = make_engine(cfg, sd, precision=X3)
    g = torch.Generator().manual_seed(6)
    B, T = 2, 8
    ymix = torch.randn((B, 1, 64, T), generator=g)
    z = torch.randn((B, 2, 64, T), generator=g)
    x, nfe, st = eng.ode_sample(ymix, z, rtol=1e-4, atol=1e-4, return_stats=True)
    ref, sol = _restated(odit.DiTScore(sd, cfg), ymix, z, 2, rtol=1e-4, atol=1e-4)
    err = rel_l2(x, torch.from_numpy(ref))
    _report("full_dit/B=2/tol=1e-4", nfe, st, sol, err)
    _check_nfev(nfe, sol, st, False, "RK45")
    assert err <= 1e-3
    eng.close()


@pytest.mark.parametrize("method", ["RK45", "RK23"])
def test_ode_forced_rejection_first_and_max_step(tiny_dit_engine, method):
    """The caller's first step (0.9, clamped to max_step = 0.5) is too large: the controller rejects, caps the next
    factor at 1 and shrinks the step, exactly as the restatement (2 rejections there); the select_initial_step launches
    are skipped (nfev = 1 + stages x attempts)."""
    cfg, sd, eng = tiny_dit_engine
    g = torch.Generator().manual_seed(9)
    ymix = torch.randn((3, 1, 64, 4), generator=g)
    z = torch.randn((3, 2, 64, 4), generator=g)
    kw = dict(method=method, rtol=1e-4, atol=1e-4, first_step=0.9, max_step=0.5)
    runs = []
    for graphs in (False, True, True, True):      # eager, then the first_step init graph's warm-up, capture, replay
        eng.enable_graphs(graphs)
        runs.append(eng.ode_sample(ymix, z, return_stats=True, **kw))
    eng.enable_graphs(False)
    x, nfe, st = runs[0]
    assert all(torch.equal(r[0], x) and r[2] == st for r in runs[1:])
    ref, sol = _restated(odit.DiTScore(sd, cfg), ymix, z, 2, **kw)
    err = rel_l2(x, torch.from_numpy(ref))
    _report(f"forced_rejection/{method}", nfe, st, sol, err, method)
    assert sol["n_rejected"] > 0 and st["n_rejected"] > 0
    _check_nfev(nfe, sol, st, True, method)
    assert nfe == 1 + ode.TABLEAUX[method]["n_stages"] * (st["n_accepted"] + st["n_rejected"])
    assert err <= 1e-4


@pytest.mark.parametrize("seeded", [False, True])
def test_ode_prior_is_the_pc_prior(tiny_dit_engine, seeded):
    """x_T is bit for bit the PC sampler's prior for the same noise or seed.  The PC side: one step of predictor 'none'
    without corrector steps returns its prior; the ODE side: after a call stopped by max_attempts = 1 the fp64 state
    buffer still holds y0 = x_T (an accepted step is applied at the start of the next attempt)."""
    _, _, eng = tiny_dit_engine
    g = torch.Generator().manual_seed(21)
    B, T = 3, 4
    ymix = torch.randn((B, 1, 64, T), generator=g)
    z = None if seeded else torch.randn((B, 2, 64, T), generator=g)
    pc_x, _ = eng.pc_sample(ymix, None if z is None else z[None], N=1, corrector_steps=0, predictor="none",
                            denoise=False, seed=77)
    with pytest.raises(RuntimeError, match="max_attempts"):
        eng.ode_sample(ymix, z, max_attempts=1, seed=77)
    n = B * 2 * 64 * T
    y0 = eng.debug_read("ode_y", (2 * n,)).view(torch.float64).reshape(B, 2, 64, T)
    assert torch.equal(y0, pc_x.cpu().double())


def test_ode_invalid_options_rejected_by_the_engine(tiny_dit_engine):
    """The C-ABI refuses what the Python layer refuses too: NaN or out-of-range first_step, NaN max_step."""
    _, _, eng = tiny_dit_engine
    y = torch.zeros((1, 1, 64, 4))
    for kw in (dict(first_step=float("nan")), dict(first_step=-0.1), dict(first_step=0.98),
               dict(max_step=float("nan")), dict(t_eps=1.0), dict(max_attempts=0)):
        with pytest.raises(RuntimeError, match="dsn_ode_sample"):
            eng.ode_sample(y, **kw)


def test_ode_graph_replay_bit_identical(tiny_dit_engine):
    """Eager and hipGraph replay (init, one step attempt, output captured once each) give bit-identical x and stats;
    so do two runs, with injected noise and with the device RNG."""
    _, _, eng = tiny_dit_engine
    g = torch.Generator().manual_seed(3)
    ymix = torch.randn((3, 1, 64, 4), generator=g)
    z = torch.randn((3, 2, 64, 4), generator=g)
    for method in ("RK45", "RK23"):
        eng.enable_graphs(False)
        x0, n0, s0 = eng.ode_sample(ymix, z, method=method, return_stats=True)
        x1, n1, s1 = eng.ode_sample(ymix, z, method=method, return_stats=True)
        assert torch.equal(x0, x1) and s0 == s1
        eng.enable_graphs(True)
        for _ in range(3):                    # eager warm-up, capture, replay
            xg, ng, sg = eng.ode_sample(ymix, z, method=method, return_stats=True)
            assert torch.equal(x0, xg) and sg == s0
        # a different input through the captured graphs
        xe2 = eng.ode_sample(ymix * 0.5, z, method=method)[0]
        eng.enable_graphs(False)
        assert torch.equal(xe2, eng.ode_sample(ymix * 0.5, z, method=method)[0])
    xs = eng.ode_sample(ymix, None, seed=123)[0]
    assert torch.equal(xs, eng.ode_sample(ymix, None, seed=123)[0])
    assert not torch.equal(xs, eng.ode_sample(ymix, None, seed=124)[0])


def test_ode_max_attempts_raises_and_engine_recovers(tiny_dit_engine):
    _, _, eng = tiny_dit_engine
    g = torch.Generator().manual_seed(4)
    ymix = torch.randn((3, 1, 64, 4), generator=g)
    z = torch.randn((3, 2, 64, 4), generator=g)
    ok, _ = eng.ode_sample(ymix, z)
    with pytest.raises(RuntimeError, match="max_attempts"):
        eng.ode_sample(ymix, z, max_attempts=3)
    again, _ = eng.ode_sample(ymix, z)
    assert torch.equal(ok, again)
    torch.cuda.synchronize()


def _tiny_config(tmp_path):
    vae_json = {"model_type": "autoencoder", "sample_rate": 16000,
                "model": {"encoder": {"type": "oobleck", "config": {"in_channels": 1, "channels": 32,
                                                                     "c_mults": [1, 2, 4, 8, 16],
                                                                     "strides": [2, 4, 4, 8, 8], "latent_dim": 128}},
                          "decoder": {"type": "oobleck", "config": {"out_channels": 1, "channels": 32,
                                                                     "c_mults": [1, 2, 4, 8, 16],
                                                                     "strides": [2, 4, 4, 8, 8], "latent_dim": 64}},
                          "bottleneck": {"type": "vae"}, "latent_dim": 64, "downsampling_ratio": 2048,
                          "io_channels": 1}}
    p = tmp_path / "vae.json"
    p.write_text(json.dumps(vae_json))
    return {"model": {"n_speakers": 2, "t_eps": 0.03,
                      "score_model": {"_target_": "ditsep_amd.score_models.DiTScoreModel", "embed_dim": 128,
                                      "depth": 2, "num_heads": 2},
                      "vae": {"config_path": str(p), "ckpt_path": None, "trainable_vae": False},
                      "sde": {"_target_": "sdes.sdes.OUVESDE", "theta": 1.5, "sigma_min": 0.96, "sigma_max": 10.0,
                              "N": 4}}}


def test_latentdiffsep_get_ode_sampler_minibatches(tmp_path):
    """minibatch=1 equals per-item calls (noise sliced, explicit seed offset per minibatch); minibatch=None runs the
    batch under one controller; the error path of the sampler reaches the facade."""
    from ditsep_amd import LatentDiffSep, sdes

    vcfg = ovae.OobleckConfig(channels=32)
    vsd = tiny_vae_weights(vcfg, 31)
    _, dsd = _tiny_dit()
    model = LatentDiffSep(_tiny_config(tmp_path), precision="bf16x3")
    sd = {"score_model." + k: v for k, v in dsd.items()}
    sd.update({"vae." + k: v for k, v in vsd.items()})
    model.load_state_dict(sd)
    g = torch.Generator().manual_seed(12)
    y = torch.randn((3, 1, 64, 4), generator=g)
    z = torch.randn((3, 2, 64, 4), generator=g)
    x, ns = model.get_ode_sampler(y, minibatch=1, noise=z)()
    assert len(ns) == 3
    for i in range(3):
        xi, ni = sdes.get_ode_sampler(model.sde, model, y[i:i + 1], eps=0.03, noise=z[i:i + 1])()
        assert ni == ns[i] and torch.equal(xi, x[i:i + 1])
    xs, nss = model.get_ode_sampler(y, minibatch=2, seed=7)()
    x0, _ = sdes.get_ode_sampler(model.sde, model, y[0:2], eps=0.03, seed=7)()
    x1, _ = sdes.get_ode_sampler(model.sde, model, y[2:3], eps=0.03, seed=8)()
    assert torch.equal(xs, torch.cat([x0, x1]))
    xb, nb = model.get_ode_sampler(y, minibatch=None, noise=z)()
    assert isinstance(nb, int) and xb.shape == x.shape
    with pytest.raises(RuntimeError, match="max_attempts"):
        model.get_ode_sampler(y, minibatch=1, noise=z, max_attempts=3)()
    model.close()
