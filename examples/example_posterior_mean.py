#!/usr/bin/env python3
"""Fit a posterior mean once, evaluate it many times: ``Model.posterior_mean`` returns an object that holds the weights
alpha = K^-1 (z - P beta) and beta, and every evaluation after that -- values on three batches, then a few steps of multi-start
gradient ascent with ``mean_and_gradient`` -- is one matrix-free pass over the (observation, point) pairs instead of a new
factorisation and an n^2 m solve per call (``Model.predict`` / ``Model.predict_gradient``).

    python examples/example_posterior_mean.py            # needs a MI355X
"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gpmp_amd as gp          # noqa: E402
import gpmp_amd.num as gnp     # noqa: E402
from gpmp_amd.kernel import MaternCovariance  # noqa: E402


def f(x):
    return np.sin(2 * np.pi * x[:, 0]) * np.cos(np.pi * x[:, 1]) + x[:, 2] - (x[:, 3] - 0.3) ** 2


def constant_mean(x, param):
    return gnp.ones((x.shape[0], 1))


def main():
    rng = np.random.default_rng(0)
    n, d = 2000, 4
    xi = rng.random((n, d))
    zi = f(xi)
    theta = np.concatenate(([0.0], -np.log(0.5 * (1.0 + np.arange(d) / d))))
    model = gp.Model(constant_mean, MaternCovariance(2), None, theta, "linear_predictor")

    t0 = time.perf_counter()
    post = model.posterior_mean(xi, zi)
    t_fit = time.perf_counter() - t0

    # agreement with the full predictors: the two routes round differently in proportion to cond(K)
    K = gnp.to_np(model.covariance(gnp.asarray(xi), None, theta))
    tol = max(1e-9, 100 * 1e-16 * np.linalg.cond(K))
    worst = 0.0
    for m in (1, 300, 5000):
        xt = rng.random((m, d))
        zpm = post(xt)
        ref, _ = model.predict(xi, zi, xt)
        err = np.max(np.abs(zpm - ref)) / max(1.0, np.max(np.abs(ref)))
        worst = max(worst, err)
        assert err <= tol, (m, err, tol)
    xt = rng.random((64, d))
    zpm, dzpm = post.mean_and_gradient(xt)
    rz, _, rg, _ = model.predict_gradient(xi, zi, xt, variance=False)
    eg = np.max(np.abs(dzpm - rg)) / max(1.0, np.max(np.abs(rg)))
    assert np.max(np.abs(zpm - rz)) <= tol * max(1.0, np.max(np.abs(rz))) and eg <= tol, (eg, tol)
    print(f"posterior mean check: fit {1e3 * t_fit:.1f} ms, worst relative difference to Model.predict {worst:.1e}, "
          f"gradient to Model.predict_gradient {eg:.1e} (bound {tol:.1e})")

    # multi-start projected gradient ascent on the posterior mean: 64 starts at once, one pass per step
    x = xt.copy()
    start = post(x)
    best_v, best_x = start.copy(), x.copy()
    step = 0.05
    t0 = time.perf_counter()
    for _ in range(25):
        v, g = post.mean_and_gradient(x)
        better = v > best_v
        best_v[better], best_x[better] = v[better], x[better]
        x = np.clip(x + step * g / np.maximum(np.linalg.norm(g, axis=1, keepdims=True), 1e-12), 0.0, 1.0)
    t_steps = time.perf_counter() - t0
    assert np.all(np.isfinite(best_v)) and np.all(best_v >= start)
    k = int(np.argmax(best_v))
    print(f"25 ascent steps from 64 starts in {1e3 * t_steps:.1f} ms: best mean {start.max():.4f} -> {best_v.max():.4f} "
          f"at x = {np.round(best_x[k], 3)}")


if __name__ == "__main__":
    main()
