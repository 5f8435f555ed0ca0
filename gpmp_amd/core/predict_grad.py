"""Gradients of the posterior mean and variance with respect to the prediction points.

The reference obtains them by torch autograd through ``Model.predict`` (``xt.requires_grad_()``); the HIP kernels record no
autograd graph, so this module states them analytically (include/gpmp_hip.h, gpmp_predict_grad):

    d mean_t / d x_t = D[gamma]_t + beta^T J_t,          gamma = K^-1 (z - P beta)
    d var_t  / d x_t = -2 D[lambda_t]_t - 2 mu_t^T J_t,  lambda_t, mu_t: kriging weights and Lagrange multipliers

with D[w]_t = sum_i w_i d k(x_i, x_t) / d x_t (one fused pass, gpmp_predict_grad_reduce) and J_t the Jacobian of the mean design
at x_t.  A prediction that fits one chunk is one library call; a larger one reuses the chunked predictor of ``kriging``.
"""
import numpy
import torch

from .. import num as gnp
from .kriging import _Predictor, _chunk_cols, _prior_variance
from .utils import mean_values as _mean_values


def _check_model(model):
    from ..kernel.matern import MaternCovariance

    if not isinstance(model.covariance, MaternCovariance):
        raise NotImplementedError(
            "predict_gradient needs a gpmp_amd.kernel.MaternCovariance covariance; for another covariance differentiate "
            "Model.predict by finite differences with gnp.grad")
    if model.meantype not in ("zero", "parameterized", "linear_predictor"):
        raise ValueError(f"Invalid meantype {model.meantype}.")
    if model.meantype == "parameterized" and model.meanparam is None:
        raise ValueError("For meantype 'parameterized', meanparam should not be None.")
    if model.covparam is None:
        raise ValueError("covparam is None")


def _mean_jacobian(model, xt, mean_gradient):
    """J (m, q, d) of the mean design at xt (parameterized: q = 1), from ``mean_gradient`` or by autograd, column by column (row t of
    the design is assumed to depend on x_t only)."""
    m, d = xt.shape
    if mean_gradient is not None:
        J = gnp.asarray(mean_gradient(xt, model.meanparam)).to(torch.float64)
        if model.meantype == "parameterized" and J.dim() == 2:
            J = J.reshape(m, 1, d)
        if J.dim() != 3 or J.shape[0] != m or J.shape[2] != d:
            raise ValueError(f"mean_gradient returned shape {tuple(J.shape)}, expected (m, q, d) = ({m}, q, {d})")
        return J.contiguous()
    x = xt.detach().clone().requires_grad_(True)
    try:
        with torch.enable_grad():
            P = gnp.asarray(model.mean(x, model.meanparam))
            P = P.reshape(m, -1)
            q = P.shape[1]
            J = torch.zeros((m, q, d), dtype=torch.float64, device=xt.device)
            for a in range(q):
                g = None
                if P.requires_grad:
                    (g,) = torch.autograd.grad(P[:, a].sum(), x, retain_graph=True, allow_unused=True)
                if g is not None:
                    J[:, a, :] = g
                elif bool(torch.any(P[:, a] != P[0, a])):
                    # no autograd path to x, yet the column varies with the point: the mean left torch
                    raise RuntimeError(f"column {a} of the mean design is not differentiable by autograd")
    except Exception as e:   # the mean left torch (a NumPy or library call): autograd cannot see through it
        raise ValueError("cannot differentiate the mean function by autograd; pass mean_gradient(x, meanparam) returning its "
                         "Jacobian, shape (m, q, d)") from e
    return J.detach()


def _theta(model, d):
    cov = model.covariance
    theta = gnp._host_params(model.covparam)
    if len(theta) != 1 + (1 if cov.noise else 0) + d:
        raise ValueError(f"covparam has {len(theta)} entries, expected {1 + (1 if cov.noise else 0) + d}")
    return theta


def _reduce(model, xi, xt, u, lam, theta):
    """D[u] and D[lambda] (either may be None) through gpmp_predict_grad_reduce."""
    lib = gnp._lib.load()
    n, d = xi.shape
    m = xt.shape[0]
    ws = torch.empty(max(int(lib.gpmp_predict_grad_reduce_ws_elems(n, m, d)), 1), dtype=torch.float64, device=xi.device)
    gu = torch.empty((m, d), dtype=torch.float64, device=xi.device) if u is not None else None
    gl = torch.empty((m, d), dtype=torch.float64, device=xi.device) if lam is not None else None
    cov = model.covariance
    gnp._lib.check(
        lib.gpmp_predict_grad_reduce(gnp._ptr(xi), gnp._ptr(xt), n, m, d, cov.p, gnp._lib.host_vec(theta), 1 if cov.noise else 0,
                                     gnp._ptr(u), gnp._ptr(lam), gnp._ld(lam) if lam is not None else m, gnp._ptr(gu), gnp._ptr(gl),
                                     gnp._ptr(ws), gnp._stream()),
        "gpmp_predict_grad_reduce")
    return gu, gl


def _one_call(model, xi, zc, xt, Pi, Pt, J, theta, variance, clamp):
    lib = gnp._lib.load()
    n, d = xi.shape
    m = xt.shape[0]
    q = 0 if Pi is None else int(Pi.shape[1])
    dev = xi.device
    f64 = dict(dtype=torch.float64, device=dev)
    zpm, zpv = torch.empty(m, **f64), torch.empty(m, **f64)
    gm = torch.empty((m, d), **f64)
    gv = torch.empty((m, d), **f64) if variance else None
    info = torch.zeros(1, dtype=torch.int32, device=dev)
    ws = torch.empty(int(lib.gpmp_predict_grad_ws_elems(n, m, d, q)), **f64)
    cov = model.covariance
    gnp._lib.check(
        lib.gpmp_predict_grad(gnp._ptr(xi), gnp._ptr(zc), gnp._ptr(Pi), gnp._ld(Pi) if q else 0, gnp._ptr(xt), gnp._ptr(Pt),
                              gnp._ld(Pt) if q else 0, gnp._ptr(J), n, m, d, q, cov.p, gnp._lib.host_vec(theta), 1 if cov.noise else 0,
                              1 if clamp else 0, 1 if variance else 0, gnp._ptr(ws), gnp._ptr(zpm), gnp._ptr(zpv), gnp._ptr(gm), gnp._ptr(gv), gnp._ptr(info),
                              gnp._stream()),
        "gpmp_predict_grad")
    k = int(info.item())
    if k != 0:
        what = "K is not positive definite" if k <= n else "P^T K^-1 P is singular (rank-deficient mean design)"
        raise numpy.linalg.LinAlgError(f"predict_gradient: {what} (info = {k})")
    return zpm, zpv, gm, gv


def _chunked(model, xi, zc, xt, use_mean, J, theta, variance, mc):
    """Factor once (kriging._Predictor), then per chunk of xt: the chunk's mean, variance and kriging weights, and the reduction."""
    pred = _Predictor(model, xi, zc, use_mean)
    W = pred.W
    y = W[:, 0].clone()
    beta = None
    if pred.q:
        beta = gnp.matmul(gnp.asarray(pred.Sinv), gnp.asarray(pred.b))     # S^-1 Wp^T w
        y = y - gnp.matmul(W[:, 1:], beta)
    gamma = pred.F.solve_lower(gnp.as_matrix(y.reshape(-1, 1), copy=True), trans=True, overwrite=True).reshape(-1).contiguous()
    means, reds, gms, gvs = [], [], [], []
    for j0 in range(0, xt.shape[0], mc):
        xtc = xt[j0 : j0 + mc].contiguous()
        mean, red, lam, mu = pred.chunk(xtc, variance)
        gm, gl = _reduce(model, xi, xtc, gamma, gnp.as_matrix(lam) if variance else None, theta)
        if beta is not None:
            gm = gm + torch.einsum("a,tad->td", beta, J[j0 : j0 + mc])
        if variance:
            gv = -2.0 * gl
            if mu is not None:
                gv = gv - 2.0 * torch.einsum("at,tad->td", mu, J[j0 : j0 + mc])
            gvs.append(gv)
        means.append(mean)
        reds.append(red)
        gms.append(gm)
    zpm, red = torch.cat(means), torch.cat(reds)
    zpv = _prior_variance(model, xt) - red
    return zpm, zpv, torch.cat(gms), (torch.cat(gvs) if variance else None)


def predict_gradient(model, xi, zi, xt, variance=True, mean_gradient=None, zero_neg_variances=True):
    """(zpm, zpv, dzpm, dzpv) on the device; dzpm / dzpv of shape (m, d), dzpv None unless ``variance``."""
    _check_model(model)
    xi, xt = gnp._points(xi), gnp._points(xt)
    n, d = xi.shape
    m = xt.shape[0]
    theta = _theta(model, d)
    zc = gnp.asarray(zi).reshape(-1).to(torch.float64)
    prior_mean, prior_grad = 0.0, None
    Pi = Pt = J = None
    if model.meantype == "parameterized":
        zc = zc - _mean_values(model, xi, model.meanparam).reshape(-1)
        prior_mean = _mean_values(model, xt, model.meanparam).reshape(-1)
        prior_grad = _mean_jacobian(model, xt, mean_gradient).reshape(m, d)
    elif model.meantype == "linear_predictor":
        Pi = gnp.as_matrix(_mean_values(model, xi, model.meanparam))
        Pt = gnp.as_matrix(_mean_values(model, xt, model.meanparam))
        J = _mean_jacobian(model, xt, mean_gradient)
        if J.shape[1] != Pi.shape[1]:
            raise ValueError(f"the mean Jacobian has {J.shape[1]} columns, the mean design {Pi.shape[1]}")
    zc = zc.contiguous()
    if m == 0:
        e = torch.zeros((0, d), dtype=torch.float64, device=xi.device)
        return torch.zeros(0, dtype=torch.float64, device=xi.device), torch.zeros(0, dtype=torch.float64, device=xi.device), e, \
            (e if variance else None)
    mc = _chunk_cols(n, m)
    if mc >= m:
        zpm, zpv, gm, gv = _one_call(model, xi, zc, xt, Pi, Pt, J, theta, variance, zero_neg_variances)
    else:
        zpm, zpv, gm, gv = _chunked(model, xi, zc, xt, Pi is not None, J, theta, variance, mc)
        if zero_neg_variances:
            neg = zpv < 0.0
            zpv = torch.where(neg, torch.zeros_like(zpv), zpv)
            if gv is not None:
                gv = torch.where(neg.reshape(-1, 1), torch.zeros_like(gv), gv)
    if prior_grad is not None:
        zpm = zpm + prior_mean
        gm = gm + prior_grad
    return zpm, zpv, gm, gv
