"""NumPy restatement of the fitted posterior mean (include/gpmp_hip.h, gpmp_posterior_weights / gpmp_posterior_mean), independent of
the library: the dual form by the Cholesky route

    K = L L^T,  W = L^-1 [z | P] = [w | Wp],  beta = (Wp^T Wp)^-1 Wp^T w,  alpha = L^-T (w - Wp beta)
    mean_t = sum_i alpha_i k(x_t, x_i) + Pt[t] . beta
    d mean_t / d x_tj = sigma^2 rho_j^-2 sum_i alpha_i S(h_it) (x_tj - x_ij) + sum_a beta_a J[t, a, j]

on the covariance pieces of tests/predict_grad_numpy.py."""
import math

import numpy as np
import scipy.linalg as sla

from . import predict_grad_numpy as pgn


def gram(xi, p, theta, noise):
    """K(xi, xi) with the nugget (or the noise variance) on its diagonal."""
    K, _, _ = pgn.cov_parts(xi, xi, p, theta, noise)
    sigma2 = math.exp(theta[0])
    return K + (math.exp(theta[1]) if noise else 10.0 * sigma2 * np.finfo(float).eps) * np.eye(xi.shape[0])


def weights(xi, zi, p, theta, noise, Pi=None):
    """(alpha, beta); beta has length 0 without a mean design."""
    L = np.linalg.cholesky(gram(xi, p, theta, noise))
    w = sla.solve_triangular(L, zi, lower=True)
    beta = np.zeros(0)
    y = w
    if Pi is not None and Pi.shape[1] > 0:
        Wp = sla.solve_triangular(L, Pi, lower=True)
        beta = np.linalg.solve(Wp.T @ Wp, Wp.T @ w)
        y = w - Wp @ beta
    return sla.solve_triangular(L, y, lower=True, trans="T"), beta


def mean_and_gradient(xi, alpha, xt, p, theta, noise, Pt=None, beta=None, J=None):
    """(zpm, gzpm) from the weights; no diagonal term, the gradient term of a coincident pair is 0."""
    Kit, Sit, ir2 = pgn.cov_parts(xi, xt, p, theta, noise)          # n x m
    diff = xt[None, :, :] - xi[:, None, :]                          # (n, m, d)
    zpm = Kit.T @ alpha
    gm = ir2 * np.einsum("it,itj->tj", alpha[:, None] * Sit, diff)
    if beta is not None and len(beta):
        zpm = zpm + Pt @ beta
        if J is not None:
            gm = gm + np.einsum("a,taj->tj", beta, J)
    return zpm, gm


def tolerance(xi, p, theta, noise, base=1e-9):
    """The rule of tests/test_predict_grad_gpu.py: max(1e-9, 100 * 1e-16 * cond(K)), relative to max(1, max|ref|); K without its
    diagonal term, as there."""
    K, _, _ = pgn.cov_parts(xi, xi, p, theta, noise)
    return max(base, 1e-16 * 100 * np.linalg.cond(K))


def close(a, ref, tol, what):
    a, ref = np.asarray(a), np.asarray(ref)
    err = np.max(np.abs(a - ref)) if a.size else 0.0
    assert a.shape == ref.shape, (what, a.shape, ref.shape)
    assert err <= tol * max(1.0, np.max(np.abs(ref)) if ref.size else 1.0), (what, err, tol)


def fixture_case(g, c):
    """Inputs, designs and reference outputs of case c of ref_predict_grad.npz.  A parameterized mean comes back as q = 0 with the
    prior mean / gradient to centre z with and to add back (what a C host does)."""
    cs = pgn.case(g, c)
    kind, xi, xt = cs["kind"], cs["xi"], cs["xt"]
    out = dict(cs, Pi=None, Pt=None, J=None, zc=cs["zi"], prior=0.0, prior_grad=0.0, zpm=g[f"c{c}_zpm"], gzpm=g[f"c{c}_gzpm"])
    if kind == "param":
        mi, _ = pgn.designs(kind, xi, cs["meanparam"])
        mt, gt = pgn.designs(kind, xt, cs["meanparam"])
        out.update(zc=cs["zi"] - mi, prior=mt, prior_grad=gt)
    elif kind in ("const", "lin"):
        Pi, _ = pgn.designs(kind, xi)
        Pt, J = pgn.designs(kind, xt)
        out.update(Pi=Pi, Pt=Pt, J=J)
    return out
