"""Float64 restatement of the probability-flow ODE solver of ditsep_amd (ditsep_amd/csrc/ode.hip).

scipy 1.15's solve_ivp(method="RK45" | "RK23") as the reference's get_ode_sampler calls it
(src/sdes/__init__.py:196-281): RungeKutta._step_impl, rk_step and _estimate_error_norm
(scipy/integrate/_ivp/rk.py), select_initial_step and norm (common.py), and the OdeSolver.step /
solve_ivp loop around them, over one flattened float64 state vector.  It takes any drift callable
`fun(t, y) -> dy/dt` and does not import scipy (the GPU machines need not have it).
"""
from __future__ import annotations

import math

import numpy as np

EPS = np.finfo(float).eps
SAFETY = 0.9
MIN_FACTOR = 0.2
MAX_FACTOR = 10

TABLEAUX = {
    # Dormand-Prince 5(4): 6 stages + FSAL, error-estimator order 4
    "RK45": dict(
        order=4, n_stages=6,
        C=np.array([0, 1 / 5, 3 / 10, 4 / 5, 8 / 9, 1]),
        A=np.array([
            [0, 0, 0, 0, 0],
            [1 / 5, 0, 0, 0, 0],
            [3 / 40, 9 / 40, 0, 0, 0],
            [44 / 45, -56 / 15, 32 / 9, 0, 0],
            [19372 / 6561, -25360 / 2187, 64448 / 6561, -212 / 729, 0],
            [9017 / 3168, -355 / 33, 46732 / 5247, 49 / 176, -5103 / 18656],
        ]),
        B=np.array([35 / 384, 0, 500 / 1113, 125 / 192, -2187 / 6784, 11 / 84]),
        E=np.array([-71 / 57600, 0, 71 / 16695, -71 / 1920, 17253 / 339200, -22 / 525, 1 / 40]),
    ),
    # Bogacki-Shampine 3(2): 3 stages + FSAL, error-estimator order 2
    "RK23": dict(
        order=2, n_stages=3,
        C=np.array([0, 1 / 2, 3 / 4]),
        A=np.array([[0, 0, 0], [1 / 2, 0, 0], [0, 3 / 4, 0]]),
        B=np.array([2 / 9, 1 / 3, 4 / 9]),
        E=np.array([5 / 72, -1 / 12, -1 / 9, 1 / 8]),
    ),
}


class SolverFailed(RuntimeError):
    """A step size below 10 ulp of t (solve_ivp: success=False) or more than max_attempts step attempts."""


def norm(x):
    """RMS norm (scipy common.norm)."""
    return np.linalg.norm(x) / x.size ** 0.5


def select_initial_step(fun, t0, y0, t_bound, max_step, f0, direction, order, rtol, atol):
    interval_length = abs(t_bound - t0)
    if interval_length == 0.0:
        return 0.0
    scale = atol + np.abs(y0) * rtol
    d0 = norm(y0 / scale)
    d1 = norm(f0 / scale)
    if d0 < 1e-5 or d1 < 1e-5:
        h0 = 1e-6
    else:
        h0 = 0.01 * d0 / d1
    h0 = min(h0, interval_length)
    y1 = y0 + h0 * direction * f0
    f1 = fun(t0 + h0 * direction, y1)
    d2 = norm((f1 - f0) / scale) / h0
    if d1 <= 1e-15 and d2 <= 1e-15:
        h1 = max(1e-6, h0 * 1e-3)
    else:
        h1 = (0.01 / max(d1, d2)) ** (1 / (order + 1))
    return min(100 * h0, h1, interval_length, max_step)


def rk_step(fun, t, y, f, h, A, B, C, K):
    K[0] = f
    for s, (a, c) in enumerate(zip(A[1:], C[1:]), start=1):
        dy = np.dot(K[:s].T, a[:s]) * h
        K[s] = fun(t + c * h, y + dy)
    y_new = y + h * np.dot(K[:-1].T, B)
    f_new = fun(t + h, y_new)
    K[-1] = f_new
    return y_new, f_new


def solve(fun, t0, t_bound, y0, method="RK45", rtol=1e-3, atol=1e-6, first_step=None, max_step=np.inf,
          max_attempts=None):
    """solve_ivp(fun, (t0, t_bound), y0, method, rtol, atol, first_step, max_step) restated.  Returns a dict with
    y (final state), t (accepted times, t0 first), nfev, n_accepted, n_rejected, attempts.  Raises SolverFailed where
    solve_ivp reports success=False, and after max_attempts step attempts (no scipy twin)."""
    tab = TABLEAUX[method]
    A, B, C, E = tab["A"], tab["B"], tab["C"], tab["E"]
    order, n_stages = tab["order"], tab["n_stages"]
    nfev = [0]

    def f_(t, y):
        nfev[0] += 1
        return np.asarray(fun(t, y), dtype=np.float64)

    t0, t_bound = float(t0), float(t_bound)
    y = np.array(y0, dtype=np.float64).reshape(-1).copy()
    rtol = max(rtol, 100 * EPS)
    direction = np.sign(t_bound - t0) if t_bound != t0 else 1
    t = t0
    f = f_(t, y)
    if first_step is None:
        h_abs = select_initial_step(f_, t, y, t_bound, max_step, f, direction, order, rtol, atol)
    else:
        if first_step <= 0 or first_step > abs(t_bound - t0):
            raise ValueError("first_step out of range")
        h_abs = first_step
    K = np.empty((n_stages + 1, y.size), dtype=np.float64)
    exponent = -1 / (order + 1)
    ts = [t]
    accepted = rejected = attempts = 0
    while not (t == t_bound):
        min_step = 10 * np.abs(np.nextafter(t, direction * np.inf) - t)
        if h_abs > max_step:
            h_abs = max_step
        elif h_abs < min_step:
            h_abs = min_step
        step_accepted = False
        step_rejected = False
        while not step_accepted:
            if h_abs < min_step:
                raise SolverFailed(f"step size {h_abs} below {min_step} at t={t}")
            if max_attempts is not None and attempts >= max_attempts:
                raise SolverFailed(f"t_bound not reached in {max_attempts} attempts")
            h = h_abs * direction
            t_new = t + h
            if direction * (t_new - t_bound) > 0:
                t_new = t_bound
            h = t_new - t
            h_abs = np.abs(h)
            y_new, f_new = rk_step(f_, t, y, f, h, A, B, C, K)
            attempts += 1
            scale = atol + np.maximum(np.abs(y), np.abs(y_new)) * rtol
            error_norm = norm(np.dot(K.T, E) * h / scale)
            if error_norm < 1:
                if error_norm == 0:
                    factor = MAX_FACTOR
                else:
                    factor = min(MAX_FACTOR, SAFETY * error_norm ** exponent)
                if step_rejected:
                    factor = min(1, factor)
                h_abs *= factor
                step_accepted = True
            else:
                h_abs *= max(MIN_FACTOR, SAFETY * error_norm ** exponent)
                step_rejected = True
                rejected += 1
        t, y, f = t_new, y_new, f_new
        accepted += 1
        ts.append(t)
        if direction * (t - t_bound) >= 0:
            break
    return dict(y=y, t=np.array(ts), nfev=nfev[0], n_accepted=accepted, n_rejected=rejected, attempts=attempts)


# ---------------------------------------------------------------- the OUVE probability-flow ODE
def ouve_g2(t, sigma_min, sigma_max):
    """g(t)^2 = (sigma_min (sigma_max/sigma_min)^t)^2 2 log(sigma_max/sigma_min)."""
    ratio = sigma_max / sigma_min
    sigma = sigma_min * ratio ** t
    return sigma * sigma * (2.0 * math.log(ratio))


def ouve_mean_std(x0, y, t, theta, sigma_min, sigma_max):
    """Marginal mean and std of the OUVE SDE (reference sdes.py:595-698) in float64."""
    ls = math.log(sigma_max / sigma_min)
    e = math.exp(-theta * t)
    std = math.sqrt(sigma_min ** 2 * math.exp(-2 * theta * t) * (math.exp(2 * (theta + ls) * t) - 1) * ls
                    / (theta + ls))
    return e * x0 + (1 - e) * y, std


def ouve_pf_drift(score, y, theta, sigma_min, sigma_max):
    """fun(t, x) of the flattened state x: theta (y - x) - 1/2 g(t)^2 score(x, t).  `score(x_flat, t)` returns the
    score (float64 or float32, x's size); `y` is the mixture broadcast to the state's shape."""
    y = np.asarray(y, dtype=np.float64).reshape(-1)

    def fun(t, x):
        s = np.asarray(score(x, t), dtype=np.float64).reshape(-1)
        return theta * (y - x) - 0.5 * ouve_g2(t, sigma_min, sigma_max) * s

    return fun


def ouve_std_f32(t, theta, sigma_min, sigma_max):
    """std(t) with the engine's float32 rounding (csrc/engine.hip ouve_std)."""
    f = np.float32
    th, smin = float(f(theta)), float(f(sigma_min))
    ls = math.log(float(f(sigma_max)) / smin)
    a = np.exp(f(-2.0 * th) * f(t), dtype=np.float32)
    b = np.exp(f(2.0 * (th + ls)) * f(t), dtype=np.float32) - f(1)
    num = f(smin * smin) * a * b * f(ls)
    return float(np.sqrt(num / f(th + ls), dtype=np.float32))


def reverse_diffusion_mean(x, y, s, eps, N, theta, sigma_min, sigma_max):
    """x_mean of the reverse-diffusion predictor at t = eps, dt = 1/N, in float32 (the engine's arithmetic)."""
    f = np.float32
    smin, smax = float(f(sigma_min)), float(f(sigma_max))
    ls = math.log(smax / smin)
    sigma = f(smin) * np.power(f(smax / smin), f(eps), dtype=np.float32)
    dt = f(1.0 / N)
    G = sigma * f(math.sqrt(2.0 * ls)) * np.sqrt(dt, dtype=np.float32)
    fdrift = f(theta) * (np.asarray(y, np.float32) - x) * dt
    return (x - (fdrift - (G * G) * np.asarray(s, np.float32))).astype(np.float32)


def ode_sample(score, ymix, z, *, n_src, theta, sigma_min, sigma_max, method="RK45", rtol=1e-5, atol=1e-5, eps=3e-2,
               denoise=True, N=30, first_step=None, max_step=np.inf, max_attempts=None):
    """The native sampler's contract: ymix [B,1,D,T], z [B,n,D,T] (numpy); score(x [B,n,D,T] float32, t float32)
    -> [B,n,D,T].  Prior x_T = y + std(1) z in float32 with one rounding (as the engine draws it), ODE state float64 with the network
    fed the float32 cast of each stage point, optional noise-free reverse-diffusion step at eps (float32, dt = 1/N).
    Returns (x float32 [B,n,D,T], solver dict)."""
    ymix = np.asarray(ymix, dtype=np.float32)
    B, _, D, T = ymix.shape
    shape = (B, n_src, D, T)
    yb = np.broadcast_to(ymix, shape)
    std_T = np.float32(ouve_std_f32(1.0, theta, sigma_min, sigma_max))
    # one rounding, as the engine's prior kernel computes it (fma(z, std_T, y); the float32 product is exact in float64)
    x_T = (np.asarray(z, dtype=np.float32).astype(np.float64) * np.float64(std_T) + yb.astype(np.float64)).astype(
        np.float32)

    def net(x, t):
        return score(np.asarray(x, dtype=np.float64).astype(np.float32).reshape(shape), np.float32(t))

    fun = ouve_pf_drift(net, yb.astype(np.float64), theta, sigma_min, sigma_max)
    sol = solve(fun, 1.0, eps, x_T.astype(np.float64).reshape(-1), method=method, rtol=rtol, atol=atol,
                first_step=first_step, max_step=max_step, max_attempts=max_attempts)
    x = sol["y"].astype(np.float32).reshape(shape)
    if denoise:
        x = reverse_diffusion_mean(x, yb, score(x, np.float32(eps)), eps, N, theta, sigma_min, sigma_max)
    return x, sol
