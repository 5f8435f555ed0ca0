#!/usr/bin/env python3
"""Conditional sample paths without kriging weights: ``Model.conditional_sample_paths_from_data`` conditions all paths through
``Model.posterior_means`` -- one factorisation, weights of shape (n, paths) and one matrix-free pass over the (observation, point)
pairs -- where the lambda-based route solves for an n x m weight matrix first.  Both are run and compared here.

    python examples/example_conditional_paths_matrix_free.py            # needs a MI355X
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gpmp_amd as gp          # noqa: E402
import gpmp_amd.num as gnp     # noqa: E402
from gpmp_amd.kernel import MaternCovariance  # noqa: E402


def main():
    rng = np.random.default_rng(0)
    n, m, d, paths = 400, 1500, 2, 32
    xi, xt = rng.random((n, d)), rng.random((m, d))
    zi = np.sin(2 * np.pi * xi[:, 0]) + xi[:, 1]
    theta = np.concatenate(([0.0], -np.log([0.3, 0.5])))
    model = gp.Model(lambda x, param: gnp.ones((x.shape[0], 1)), MaternCovariance(2), None, theta, "linear_predictor")

    # unconditional paths on the stacked points (SVD route: the stacked covariance is only semi-definite to rounding)
    ztsim = gnp.to_np(model.sample_paths(np.vstack((xi, xt)), paths, method="svd"))
    xi_ind, xt_ind = np.arange(n), n + np.arange(m)
    cond = model.conditional_sample_paths_from_data(ztsim, xi, xi_ind, zi, xt, xt_ind)

    _, _, lam = model.predict(xi, zi, xt, return_lambdas=True)
    ref = model.conditional_sample_paths(ztsim, xi_ind, zi, xt_ind, lam)
    err = np.max(np.abs(cond - ref)) / max(1.0, np.max(np.abs(ref)))
    K = gnp.to_np(model.covariance(gnp.asarray(xi), None, theta))
    tol = max(1e-9, 100 * 1e-16 * np.linalg.cond(K))
    assert cond.shape == (m, paths) and err <= tol, (err, tol)

    # several responses on one design: the same object, column c is the posterior mean of Z[:, c]
    Z = np.stack((zi, np.cos(2 * np.pi * xi[:, 0]), xi[:, 0] * xi[:, 1]), axis=1)
    means = model.posterior_means(xi, Z)(xt)
    one = model.posterior_mean(xi, Z[:, 1])(xt)
    assert means.shape == (m, 3) and np.max(np.abs(means[:, 1] - one)) <= tol * max(1.0, np.max(np.abs(one)))
    print(f"matrix-free conditional paths check: {paths} paths at {m} points, relative difference to the lambda route {err:.1e} "
          f"(bound {tol:.1e})")


if __name__ == "__main__":
    main()
