"""CPU-only: the float64 restatement of the probability-flow ODE solver (tests/ode_restatement.py) against scipy's
solve_ivp and against the closed-form flow, the host-side error paths of sdes.get_ode_sampler, and the C-ABI symbol."""
import math
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from ditsep_amd import native, sdes
from tests import ode_restatement as ode

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
THETA, SMIN, SMAX = 1.5, 0.96, 10.0


def _point_mass_problem(seed, shape=(2, 2, 8, 5)):
    """OUVE data distribution = a point mass at x0 (per element): the score of p_t is -(x - m_t)/std_t^2."""
    rng = np.random.default_rng(seed)
    x0 = rng.standard_normal(shape)
    y = np.broadcast_to(rng.standard_normal((shape[0], 1) + shape[2:]), shape).copy()

    def score(x, t):
        m, s = ode.ouve_mean_std(x0.reshape(-1), y.reshape(-1), t, THETA, SMIN, SMAX)
        return -(x - m) / (s * s)

    _, std_T = ode.ouve_mean_std(0.0, 0.0, 1.0, THETA, SMIN, SMAX)
    x_T = y + std_T * rng.standard_normal(shape)
    return x0, y, score, x_T.reshape(-1)


def _solve_ivp_equal(fun, x_T, method, rtol, atol, eps=0.03):
    integrate = pytest.importorskip("scipy.integrate")
    ref = integrate.solve_ivp(fun, (1.0, eps), x_T, rtol=rtol, atol=atol, method=method)
    assert ref.success
    got = ode.solve(fun, 1.0, eps, x_T, method=method, rtol=rtol, atol=atol)
    np.testing.assert_array_equal(got["t"], ref.t)
    assert got["nfev"] == ref.nfev
    assert np.max(np.abs(got["y"] - ref.y[:, -1])) <= 1e-12
    n = ode.TABLEAUX[method]["n_stages"]
    assert got["nfev"] == 2 + n * got["attempts"]
    return got


@pytest.mark.parametrize("method", ["RK45", "RK23"])
@pytest.mark.parametrize("tol", [1e-5, 1e-3])
def test_restatement_equals_solve_ivp_analytic_score(method, tol):
    _, y, score, x_T = _point_mass_problem(3)
    fun = ode.ouve_pf_drift(score, y, THETA, SMIN, SMAX)
    got = _solve_ivp_equal(fun, x_T, method, tol, tol)
    assert got["n_accepted"] == len(got["t"]) - 1


def test_restatement_rejects_like_solve_ivp():
    """A forced too-large first step makes the controller reject (the factor capped at 1 after a rejection)."""
    integrate = pytest.importorskip("scipy.integrate")
    _, y, score, x_T = _point_mass_problem(5)
    fun = ode.ouve_pf_drift(score, y, THETA, SMIN, SMAX)
    ref = integrate.solve_ivp(fun, (1.0, 0.03), x_T, rtol=1e-6, atol=1e-6, method="RK45", first_step=0.9,
                              max_step=0.5)
    got = ode.solve(fun, 1.0, 0.03, x_T, method="RK45", rtol=1e-6, atol=1e-6, first_step=0.9, max_step=0.5)
    np.testing.assert_array_equal(got["t"], ref.t)
    assert got["nfev"] == ref.nfev and got["n_rejected"] > 0
    assert got["nfev"] == 1 + 6 * got["attempts"]
    assert np.max(np.abs(got["y"] - ref.y[:, -1])) <= 1e-12


@pytest.mark.parametrize("method", ["RK45", "RK23"])
def test_restatement_equals_solve_ivp_tiny_dit(method):
    """The CPU oracle's tiny DiT as the score network, the state in float64, the network fed its float32 cast."""
    pytest.importorskip("scipy.integrate")
    from oracle import dit as odit

    cfg = odit.DiTConfig(n_src=2, embed_dim=128, depth=2, num_heads=2)
    sd = odit.random_dit_weights(cfg, 32, out_gain=0.005)
    net = odit.DiTScore(sd, cfg)
    g = torch.Generator().manual_seed(9)
    shape = (2, 2, 64, 4)
    ymix = torch.randn((2, 1, 64, 4), generator=g)
    z = torch.randn(shape, generator=g)
    yb = ymix.expand(shape).double().numpy()

    def score(x, t):
        with torch.no_grad():
            xt = torch.from_numpy(np.asarray(x).astype(np.float32).reshape(shape))
            return net(xt, torch.full((2,), float(np.float32(t))), ymix).double().numpy()

    std_T = ode.ouve_std_f32(1.0, THETA, SMIN, SMAX)
    x_T = (ymix.expand(shape) + z * std_T).double().numpy().reshape(-1)
    fun = ode.ouve_pf_drift(score, yb, THETA, SMIN, SMAX)
    _solve_ivp_equal(fun, x_T, method, 1e-5, 1e-5)


@pytest.mark.parametrize("method,tol", [("RK45", 1e-5), ("RK45", 1e-7), ("RK23", 1e-5)])
def test_restatement_matches_closed_form_flow(method, tol):
    """Point-mass data: the probability-flow ODE maps x_T to x(t) = m_t + std_t/std_T (x_T - m_T) exactly.  The
    global error is held to the tolerance the solver ran at, measured in its own norm: RMS of
    err / (atol + rtol |x|) <= 1 (measured 0.38, 0.13 and 0.20 for the three cases)."""
    x0, y, score, x_T = _point_mass_problem(7)
    fun = ode.ouve_pf_drift(score, y, THETA, SMIN, SMAX)
    eps = 0.03
    got = ode.solve(fun, 1.0, eps, x_T, method=method, rtol=tol, atol=tol)
    mT, sT = ode.ouve_mean_std(x0.reshape(-1), y.reshape(-1), 1.0, THETA, SMIN, SMAX)
    me, se = ode.ouve_mean_std(x0.reshape(-1), y.reshape(-1), eps, THETA, SMIN, SMAX)
    exact = me + se / sT * (x_T - mT)
    assert ode.norm((got["y"] - exact) / (tol + tol * np.abs(exact))) <= 1.0


def test_restatement_failure_paths():
    _, y, score, x_T = _point_mass_problem(11)
    fun = ode.ouve_pf_drift(score, y, THETA, SMIN, SMAX)
    with pytest.raises(ode.SolverFailed):
        ode.solve(fun, 1.0, 0.03, x_T, method="RK45", rtol=1e-5, atol=1e-5, max_attempts=3)


def _fake_model(n_src=2):
    cfg = SimpleNamespace(sde_theta=THETA, sde_sigma_min=SMIN, sde_sigma_max=SMAX)
    return SimpleNamespace(engine=SimpleNamespace(n_src=n_src, cfg=cfg))


def test_get_ode_sampler_error_behaviour():
    sde = sdes.OUVESDE(THETA, SMIN, SMAX, N=30)
    y = torch.zeros(1, 1, 64, 2)
    model = _fake_model()
    with pytest.raises(ValueError, match="method"):                 # a name solve_ivp does not know
        sdes.get_ode_sampler(sde, model, y, method="nope")
    for m in ("DOP853", "Radau", "BDF", "LSODA"):                     # solve_ivp methods not built natively
        with pytest.raises(NotImplementedError, match="RK45, RK23"):
            sdes.get_ode_sampler(sde, model, y, method=m)
    with pytest.raises(NotImplementedError, match="native score model"):
        sdes.get_ode_sampler(sde, lambda x, t, y: x, y)
    with pytest.raises(NotImplementedError, match="OUVESDE"):
        sdes.get_ode_sampler(sdes.MixSDE(2, 2.0, 0.05, 0.5), model, y)
    with pytest.raises(NotImplementedError, match="OUVESDE"):
        sdes.get_ode_sampler(sdes.SBVESDE(2.6, 0.4), model, y)
    for opt in ("dense_output", "events", "vectorized", "t_eval"):
        with pytest.raises(NotImplementedError, match="first_step, max_step, max_attempts"):
            sdes.get_ode_sampler(sde, model, y, **{opt: None})
    with pytest.raises(ValueError, match="n_spkrs"):
        sdes.get_ode_sampler(sde, model, y, n_spkrs=3)
    with pytest.raises(ValueError, match="sde parameters"):
        sdes.get_ode_sampler(sdes.OUVESDE(1.0, SMIN, SMAX), model, y)
    with pytest.raises(ValueError, match="first_step"):
        sdes.get_ode_sampler(sde, model, y, first_step=2.0)
    with pytest.raises(ValueError, match="max_step"):
        sdes.get_ode_sampler(sde, model, y, max_step=0.0)
    with pytest.raises(ValueError, match="max_attempts"):
        sdes.get_ode_sampler(sde, model, y, max_attempts=0)
    # accepted options build a sampler without touching the GPU
    assert callable(sdes.get_ode_sampler(sde, model, y, method="RK23", first_step=0.1, max_step=0.5, max_attempts=9))


def test_ode_symbol_declared_and_exported():
    with open(os.path.join(ROOT, "include", "ditsep_hip.h")) as fh:
        header = fh.read()
    assert re.search(r"\bint dsn_ode_sample\(dsn_ctx\* ctx, const float\* y, const float\* noise, uint64_t seed, "
                     r"float\* x_out, int B, int T,\s+const DsnOdeOpts\* o, DsnOdeStats\* stats, void\* stream\);",
                     header)
    assert "dsn_ode_sample" in native.EXPORTS
    for name in ("DsnOdeOpts", "DsnOdeStats", "DSN_ODE_RK45", "DSN_ODE_RK23", "DSN_ESOLVER"):
        assert name in header
    # the ctypes mirrors have the C field order
    assert [f[0] for f in native.DsnOdeOpts._fields_] == ["method", "rtol", "atol", "t_eps", "denoise", "N",
                                                          "first_step", "max_step", "max_attempts"]
    assert [f[0] for f in native.DsnOdeStats._fields_] == ["nfev", "n_accepted", "n_rejected", "t_final", "status"]
    if os.path.exists(native.LIB_PATH):
        assert hasattr(native.load_library(), "dsn_ode_sample")
    # the engine's float32 std(1) (prior scale) agrees with the float64 closed form
    assert math.isclose(ode.ouve_std_f32(1.0, THETA, SMIN, SMAX), ode.ouve_mean_std(0, 0, 1.0, THETA, SMIN, SMAX)[1],
                        rel_tol=1e-6)
