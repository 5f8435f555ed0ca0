"""NumPy restatement of the prediction gradients (include/gpmp_hip.h, gpmp_predict_grad), independent of the library: the Matern
correlation K_p, S(h) = K_p'(h) / h, the kriging predictor by dense solves and

    d mean_t / d x_t = D[gamma]_t + beta^T J_t,   d var_t / d x_t = -2 D[lambda_t]_t - 2 mu_t^T J_t,
    D[w]_{t,j} = sigma^2 rho_j^-2 sum_i w_it S(h_it) (x_tj - x_ij).

Inputs of tests/golden/ref_predict_grad.npz (make_fixtures_predict_grad.py) are decoded by ``case``."""
import math

import numpy as np

from .wide_dim_inputs import decode


def matern_coeffs(p):
    q = np.zeros(p + 1)
    q[0] = 1.0
    for i in range(p):
        q[p - i] = math.exp(math.lgamma(p + 1) - math.lgamma(2 * p + 1) + math.lgamma(p + i + 1) - math.lgamma(i + 1) - math.lgamma(p - i + 1))
    return q


def matern_k_and_s(p, h):
    """K_p(h) and S(h) = K_p'(h) / h (0 at h = 0)."""
    c = 2.0 * math.sqrt(p + 0.5)
    t = 2.0 * c * h
    q = matern_coeffs(p)
    e = np.exp(-0.5 * t)
    K = e * np.polyval(q[::-1], t)
    if p == 0:
        with np.errstate(divide="ignore", invalid="ignore"):
            S = np.where(h > 0, -c * e / np.where(h > 0, h, 1.0), 0.0)
        return K, S
    s = np.array([(k + 1) * q[k + 1] - 0.5 * q[k] if k < p else -0.5 * q[k] for k in range(p + 1)])
    # K'(h) = 2c e sum_k s_k t^k with s_0 = 0, so K'(h) / h = (2c)^2 e sum_{k>=1} s_k t^(k-1)
    S = (2.0 * c) ** 2 * e * np.polyval(s[1:][::-1], t)
    return K, S


def cov_parts(x, y, p, theta, noise):
    d = x.shape[1]
    sigma2 = math.exp(theta[0])
    invrho = np.exp(theta[1 + noise:1 + noise + d])
    diff = (x[:, None, :] - y[None, :, :]) * invrho
    h = np.sqrt(np.sum(diff ** 2, axis=2))
    K, S = matern_k_and_s(p, h)
    return sigma2 * K, sigma2 * S, invrho ** 2


def predict_grad(xi, zi, xt, p, theta, noise, Pi=None, Pt=None, J=None, clamp=True):
    """(zpm, zpv, gzpm, gzpv) for a zero mean (Pi None) or a linear predictor with designs Pi (n x q), Pt (m x q) and the Jacobian J
    (m x q x d).  Dense solves in fp64."""
    n = xi.shape[0]
    sigma2 = math.exp(theta[0])
    Kii, _, _ = cov_parts(xi, xi, p, theta, noise)
    Kii = Kii + (math.exp(theta[1]) if noise else 10.0 * sigma2 * np.finfo(float).eps) * np.eye(n)
    Kit, Sit, ir2 = cov_parts(xi, xt, p, theta, noise)     # n x m
    Kinv_Kit = np.linalg.solve(Kii, Kit)
    alpha = np.linalg.solve(Kii, zi)
    if Pi is not None:
        U = np.linalg.solve(Kii, Pi)
        S = Pi.T @ U
        beta = np.linalg.solve(S, U.T @ zi)
        gamma = np.linalg.solve(Kii, zi - Pi @ beta)
        mu = np.linalg.solve(S, U.T @ Kit - Pt.T)           # q x m
        lam = Kinv_Kit - U @ mu
        zpm = lam.T @ zi
        zpv = sigma2 - np.sum(lam * Kit, axis=0) - np.sum(mu * Pt.T, axis=0)
    else:
        gamma, lam = alpha, Kinv_Kit
        zpm = Kit.T @ alpha
        zpv = sigma2 - np.sum(lam * Kit, axis=0)
    diff = xt[None, :, :] - xi[:, None, :]                  # (n, m, d)

    def D(w):                                              # w: (n,) or (n, m)
        W = (w[:, None] if w.ndim == 1 else w) * Sit
        return ir2 * np.einsum("it,itj->tj", W, diff)

    gm = D(gamma)
    gv = -2.0 * D(lam)
    if Pi is not None:
        gm = gm + np.einsum("a,taj->tj", beta, J)
        gv = gv - 2.0 * np.einsum("at,taj->tj", mu, J)
    if clamp:
        neg = zpv < 0
        zpv = np.where(neg, 0.0, zpv)
        gv = np.where(neg[:, None], 0.0, gv)
    return zpm, zpv, gm, gv


def case(g, c):
    """Case c of the fixture: dict with xi, xt, zi, theta, d, p, noise, mean kind, meanparam and the reference outputs."""
    pre = f"c{c}_"
    sub = decode(_Sub(g, pre))
    d, p, noise, n, m = (int(v) for v in g[pre + "spec"])
    sub.update(d=d, p=p, noise=noise, n=n, m=m, kind=str(g[pre + "mean"]))
    return sub


class _Sub:
    """The keys of one case, without their prefix (the interface of an NpzFile that decode() needs)."""

    def __init__(self, g, pre):
        self.g, self.pre = g, pre
        self.files = [k[len(pre):] for k in g.files if k.startswith(pre)]

    def __getitem__(self, k):
        return self.g[self.pre + k]


def designs(kind, x, meanparam=None):
    """Mean design, its Jacobian, and the prior mean / its gradient for the fixture's mean kinds (NumPy)."""
    m, d = x.shape
    if kind == "const":
        return np.ones((m, 1)), np.zeros((m, 1, d))
    if kind == "lin":
        k = min(d, 3)
        J = np.zeros((m, 1 + k, d))
        for a in range(k):
            J[:, 1 + a, a] = 1.0
        return np.hstack((np.ones((m, 1)), x[:, :k])), J
    if kind == "param":
        g = np.zeros((m, d))
        g[:, 0] = meanparam[1]
        return meanparam[0] + meanparam[1] * x[:, 0], g
    return None, None
