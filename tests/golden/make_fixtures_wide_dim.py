#!/usr/bin/env python3
"""Generate tests/golden/ref_wide_dim.npz by RUNNING THE REFERENCE (gpmp v0.9.37) on inputs of dimension d > 64.

Run where the reference is importable, in two passes (values with the NumPy backend, then the autograd gradients with the
torch-CPU backend, which adds its keys to the same file):

    cd /tmp && PYTHONDONTWRITEBYTECODE=1 MPLBACKEND=Agg PYTHONPATH=<reference checkout> \\
        python3 <repo>/tests/golden/make_fixtures_wide_dim.py numpy
    cd /tmp && PYTHONDONTWRITEBYTECODE=1 MPLBACKEND=Agg PYTHONPATH=<reference checkout> \\
        python3 <repo>/tests/golden/make_fixtures_wide_dim.py torch

Length scales grow like sqrt(d) (rho_j = sqrt(d) (1 + j / d) / 4), so that scaled distances stay of order
one whatever d: with the plain anisotropic guess of the other fixtures every entry of K would underflow at d = 1000.
Only inputs and outputs (plain arrays) are stored; the point sets as uint8 grid indices (x = (q + 1/2) / 256), which keeps the file
small (fp64 random inputs do not compress).
"""
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, "ref_wide_dim.npz")
backend = sys.argv[1] if len(sys.argv) > 1 else "numpy"
os.environ["GPMP_BACKEND"] = backend
os.environ.setdefault("GPMP_LOG_LEVEL", "WARNING")

import gpmp as gp  # noqa: E402  (the reference)
import gpmp.num as gnp  # noqa: E402

assert gnp._gpmp_backend_ == backend, (gnp._gpmp_backend_, backend)


def make_xz(n, d, seed, noise=0.0):
    """Points on the grid (q + 1/2) / 256 (exact in fp64; stored as the uint8 q, decoded by tests/wide_dim_inputs.py)."""
    rng = np.random.default_rng(seed)
    q = rng.integers(0, 256, size=(n, d), dtype=np.uint8)
    x = (q.astype(np.float64) + 0.5) / 256.0
    z = np.sin(2 * np.pi * x[:, 0]) + x[:, 1:].sum(axis=1) / np.sqrt(d)
    if noise:
        z = z + noise * rng.standard_normal(n)
    return x, z, q


def theta_wide(d, sigma2=1.0):
    rho = 0.5 * np.sqrt(d) * 0.5 * (1.0 + np.arange(d) / d)
    return np.concatenate(([np.log(sigma2)], -np.log(rho)))


def linear_mean(x, param):
    # linear in the first three coordinates: q = 4 (a mean linear in all d > 64 coordinates has more columns than the library's
    # mean-space limit, GPMP_MAX_RANK - 1)
    return gnp.hstack((gnp.ones((x.shape[0], 1)), gnp.asarray(x)[:, :3]))


def constant_mean(x, param):
    return gnp.ones((x.shape[0], 1))


def make_kernel(p):
    def kernel(x, y, covparam, pairwise=False):
        return gp.kernel.maternp_covariance(x, y, p, covparam, pairwise)

    return kernel


def make_noisy_kernel(p):
    # examples/gpmp_example07_nd_regression.py:95-131 construction: theta = [log s2, log s2_noise, log 1/rho ...]
    def kernel(x, y, param, pairwise=False):
        sigma2 = gnp.exp(param[0])
        noise_variance = gnp.exp(param[1])
        loginvrho = param[2:]
        if y is x or y is None:
            if pairwise:
                return sigma2 * gnp.ones((x.shape[0],))
            K = gnp.scaled_distance(loginvrho, x, x)
            return sigma2 * gp.kernel.maternp_kernel(p, K) + noise_variance * gnp.eye(K.shape[0])
        K = gnp.scaled_distance_elementwise(loginvrho, x, y) if pairwise else gnp.scaled_distance(loginvrho, x, y)
        return sigma2 * gp.kernel.maternp_kernel(p, K)

    return kernel


def tonp(a):
    return np.asarray(gnp.to_np(a) if backend == "numpy" else a.detach().cpu().numpy(), dtype=np.float64)


def noisy_theta(d):
    return np.concatenate(([0.0, np.log(0.05 ** 2)], theta_wide(d)[1:]))


def numpy_pass():
    out = {}
    # ---- Gram matrices ii / it, scaled distance: odd sizes (ragged tiles on the device)
    for d in (65, 200, 1000):
        x, _, xq = make_xz(21, d, 100 + d)
        y, _, yq = make_xz(13, d, 200 + d)
        th = theta_wide(d, sigma2=1.3)
        thn = noisy_theta(d)
        out[f"gram_d{d}_x_q"], out[f"gram_d{d}_y_q"], out[f"gram_d{d}_theta"], out[f"gram_d{d}_theta_noise"] = xq, yq, th, thn
        out[f"dist_d{d}"] = tonp(gnp.scaled_distance(th[1:], x, y))
        for p in (0, 2, 5):
            out[f"gram_d{d}_p{p}_ii"] = tonp(gp.kernel.maternp_covariance(x, x, p, th))
            out[f"gram_d{d}_p{p}_it"] = tonp(gp.kernel.maternp_covariance(x, y, p, th))
            out[f"gram_d{d}_p{p}_pw"] = tonp(gp.kernel.maternp_covariance(x[:13], y, p, th, True))
            k = make_noisy_kernel(p)
            out[f"gram_d{d}_p{p}_noise_ii"] = tonp(k(x, x, thn))
            out[f"gram_d{d}_p{p}_noise_it"] = tonp(k(x, y, thn))
    # ---- NLL / REML values at n = 300, d = 200 (gradients: torch pass)
    n, d = 300, 200
    xi, zi, xiq = make_xz(n, d, 300)
    th = theta_wide(d)
    out["crit_xi_q"], out["crit_zi"], out["crit_theta"] = xiq, zi, th
    k = make_kernel(2)
    mz = gp.core.Model(None, k, None, th, "zero")
    mc = gp.core.Model(constant_mean, k, None, th, "linear_predictor")
    out["crit_nll"] = np.array(float(gp.kernel.negative_log_likelihood_zero_mean(mz, th, xi, zi)))
    out["crit_reml_const"] = np.array(float(gp.kernel.negative_log_restricted_likelihood(mc, th, xi, zi)))
    # ---- predictions: zero mean and linear predictor (constant and linear-in-x means), d = 200
    xt, _, xtq = make_xz(51, d, 301)
    out["pred_xt_q"] = xtq
    ml = gp.core.Model(linear_mean, k, None, th, "linear_predictor")
    for tag, model in (("zero", mz), ("const", mc), ("lin", ml)):
        zpm, zpv = model.predict(xi, zi, xt)
        out[f"pred_{tag}_zpm"], out[f"pred_{tag}_zpv"] = tonp(zpm), tonp(zpv)
    # ---- LOO at d = 150
    xl, zl, xlq = make_xz(180, 150, 400)
    thl = theta_wide(150)
    out["loo_xi_q"], out["loo_zi"], out["loo_theta"] = xlq, zl, thl
    for tag, model in (("zero", gp.core.Model(None, k, None, thl, "zero")),
                       ("const", gp.core.Model(constant_mean, k, None, thl, "linear_predictor"))):
        zloo, s2, eloo = model.loo(xl, zl)
        out[f"loo_{tag}_zloo"], out[f"loo_{tag}_s2"], out[f"loo_{tag}_eloo"] = tonp(zloo), tonp(s2), tonp(eloo)
    # ---- near-duplicate points at d = 200: pairs 1e-6 apart, the nugget decides positive definiteness
    xd, zd, xdq = make_xz(60, 200, 500)
    rng = np.random.default_rng(501)
    delta = 1e-6 * rng.standard_normal((10, 200))
    xd = np.vstack((xd, xd[:10] + delta))
    zd = np.concatenate((zd, zd[:10]))
    thd = theta_wide(200)
    out["dup_base_q"], out["dup_delta"], out["dup_zi"], out["dup_theta"] = xdq, delta, zd, thd
    out["dup_K"] = tonp(gp.kernel.maternp_covariance(xd, xd, 2, thd))
    mdup = gp.core.Model(None, k, None, thd, "zero")
    out["dup_nll"] = np.array(float(gp.kernel.negative_log_likelihood_zero_mean(mdup, thd, xd, zd)))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        zpm, zpv = mdup.predict(xd, zd, xt[:20])
    out["dup_zpm"], out["dup_zpv"] = tonp(zpm), tonp(zpv)
    np.savez_compressed(PATH, **{k: np.asarray(v) for k, v in out.items()})
    print("wrote", PATH, len(out), "arrays")


def torch_pass():
    import torch

    g = dict(np.load(PATH, allow_pickle=False))
    xi, zi, th = (g["crit_xi_q"].astype(np.float64) + 0.5) / 256.0, g["crit_zi"], g["crit_theta"]
    k = make_kernel(2)
    mz = gp.core.Model(None, k, None, None, "zero")
    mc = gp.core.Model(constant_mean, k, None, None, "linear_predictor")
    for name, model, crit_fn in (("nll", mz, gp.kernel.negative_log_likelihood_zero_mean),
                                 ("reml_const", mc, gp.kernel.negative_log_restricted_likelihood)):
        _, pre, _, grad = gp.kernel.make_selection_criterion_with_gradient(model, crit_fn, xi, zi)
        tt = torch.as_tensor(th, dtype=torch.float64)
        g[f"crit_{name}_torch"] = np.array(float(pre(tt)))
        g[f"crit_{name}_grad"] = tonp(grad(tt))
    # noisy kernel at p = 0 (subgradient convention at coincident points is exercised on the diagonal)
    xn, zn, xnq = make_xz(150, 100, 302, noise=0.05)
    thn = noisy_theta(100)
    mn = gp.core.Model(None, make_noisy_kernel(0), None, None, "zero")
    _, pre, _, grad = gp.kernel.make_selection_criterion_with_gradient(mn, gp.kernel.negative_log_likelihood_zero_mean, xn, zn)
    tt = torch.as_tensor(thn, dtype=torch.float64)
    g["critn_xi_q"], g["critn_zi"], g["critn_theta"] = xnq, zn, thn
    g["critn_nll"], g["critn_nll_grad"] = np.array(float(pre(tt))), tonp(grad(tt))
    np.savez_compressed(PATH, **g)
    print("updated", PATH, len(g), "arrays")


if __name__ == "__main__":
    numpy_pass() if backend == "numpy" else torch_pass()
