#!/usr/bin/env python3
"""Maximise expected improvement on a 2-D test function with SciPy L-BFGS-B, the EI gradient from Model.predict_gradient
(analytic gradients of the posterior mean and variance with respect to the prediction point) -- what a GPmp user writes with
``xt.requires_grad_()`` + autograd on the reference's torch backend.

    python examples/example_ei_gradient.py            # needs a MI355X
"""
import math
import os
import sys

import numpy as np
from scipy.optimize import minimize
from scipy.stats import norm

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gpmp_amd as gp          # noqa: E402
import gpmp_amd.num as gnp     # noqa: E402
from gpmp_amd.kernel import MaternCovariance  # noqa: E402


def branin(x):
    x1, x2 = 15.0 * x[:, 0] - 5.0, 15.0 * x[:, 1]
    return (x2 - 5.1 / (4 * math.pi ** 2) * x1 ** 2 + 5 / math.pi * x1 - 6) ** 2 + 10 * (1 - 1 / (8 * math.pi)) * np.cos(x1) + 10


def constant_mean(x, param):
    return gnp.ones((x.shape[0], 1))


def neg_ei_and_grad(x, model, xi, zi, zmin):
    """-EI(x) and its gradient (minimisation of the improvement over zmin)."""
    zpm, zpv, dm, dv = model.predict_gradient(xi, zi, x.reshape(1, -1))
    s = math.sqrt(max(zpv[0], 1e-300))
    u = (zmin - zpm[0]) / s
    ei = s * (u * norm.cdf(u) + norm.pdf(u))
    # dEI = -Phi(u) dmean + phi(u) ds,  ds = dvar / (2 s)
    g = -norm.cdf(u) * dm[0] + norm.pdf(u) * dv[0] / (2.0 * s)
    return -ei, -g


def main():
    rng = np.random.default_rng(0)
    xi = rng.random((20, 2))
    zi = branin(xi)
    model = gp.Model(constant_mean, MaternCovariance(2), None, None, "linear_predictor")
    model, info = gp.kernel.select_parameters_with_reml(model, xi, zi, info=True)
    zmin = float(zi.min())
    # the analytic gradient against central differences at one point
    x0 = np.array([0.3, 0.6])
    f0, g0 = neg_ei_and_grad(x0, model, xi, zi, zmin)
    h, fd = 1e-6, np.zeros(2)
    for j in range(2):
        e = np.zeros(2)
        e[j] = h
        fd[j] = (neg_ei_and_grad(x0 + e, model, xi, zi, zmin)[0] - neg_ei_and_grad(x0 - e, model, xi, zi, zmin)[0]) / (2 * h)
    rel = np.max(np.abs(g0 - fd)) / max(np.max(np.abs(fd)), 1e-12)
    print(f"EI gradient check: analytic {g0} central differences {fd} (relative difference {rel:.1e})")
    assert rel < 1e-4, rel
    best = None
    for start in rng.random((8, 2)):
        r = minimize(neg_ei_and_grad, start, args=(model, xi, zi, zmin), jac=True, method="L-BFGS-B", bounds=[(0, 1), (0, 1)])
        if best is None or r.fun < best.fun:
            best = r
    print(f"max EI {-best.fun:.4g} at x = {best.x} (f = {branin(best.x.reshape(1, -1))[0]:.4g}, best observed {zmin:.4g})")


if __name__ == "__main__":
    main()
