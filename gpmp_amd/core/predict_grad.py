"""Gradients of the posterior mean and variance with respect to the prediction points.

The reference obtains them by torch autograd through ``Model.predict`` (``xt.requires_grad_()``); the HIP kernels record no
autograd graph, so this module states them analytically (include/gpmp_hip.h, gpmp_predict_grad):

    d mean_t / d x_t = D[gamma]_t + beta^T J_t,          gamma = K^-1 (z - P beta)
    d var_t  / d x_t = -2 D[lambda_t]_t - 2 mu_t^T J_t,  lambda_t, mu_t: kriging weights and Lagrange multipliers

with D[w]_t = sum_i w_i d k(x_i, x_t) / d x_t (one fused pass, gpmp_predict_grad_reduce) and J_t the Jacobian of the mean design
at x_t.  A prediction that fits one chunk is one library call; a larger one reuses the chunked predictor of ``kriging``.
"""
import torch

from .. import num as gnp
from . import fused
from .kriging import _Predictor


def _one_call(st, xt, Pt, J, variance, clamp):
    n, d, q, m = st.n, st.d, st.q, xt.shape[0]
    f64 = dict(dtype=torch.float64, device=xt.device)
    zpm, zpv = torch.empty(m, **f64), torch.empty(m, **f64)
    gm = torch.empty((m, d), **f64)
    gv = torch.empty((m, d), **f64) if variance else None
    fused.call_driver("gpmp_predict_grad", gnp._lib.load().gpmp_predict_grad_ws_elems(n, m, d, q), st.X, st.zc, st.Pi, fused.ld(st.Pi), xt,
                      Pt, fused.ld(Pt), J, n, m, d, q, st.p, st.hv, st.noise, 1 if clamp else 0, 1 if variance else 0, fused.WS, zpm, zpv,
                      gm, gv, fused.INFO, n=n, who="predict_gradient")
    return zpm, zpv, gm, gv


def _chunked(st, xt, J, variance, mc):
    """Factor once (kriging._Predictor), then per chunk of xt: the chunk's mean, variance and kriging weights, and the reduction."""
    pred = _Predictor(st, st.X, st.zc, st.Pi is not None)
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
        gm, gl = fused.grad_reduce(st, xtc, gamma, gnp.as_matrix(lam) if variance else None)
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
    zpv = gnp.asarray(st.covariance(xt, None, st.covparam, pairwise=True)).reshape(-1) - red
    return zpm, zpv, torch.cat(gms), (torch.cat(gvs) if variance else None)


def predict_gradient(model, xi, zi, xt, variance=True, mean_gradient=None, zero_neg_variances=True):
    """(zpm, zpv, dzpm, dzpv) on the device; dzpm / dzpv of shape (m, d), dzpv None unless ``variance``."""
    fused.check_matern_model(model, "predict_gradient")
    st = fused.Staged(model, xi, zi)
    xt = gnp._points(xt)
    m, d = xt.shape[0], st.d
    Pt, J, prior_mean, prior_grad = st.at(xt, gradient=True, mean_gradient=mean_gradient)
    if m == 0:
        e = torch.zeros((0, d), dtype=torch.float64, device=xt.device)
        return torch.zeros(0, dtype=torch.float64, device=xt.device), torch.zeros(0, dtype=torch.float64, device=xt.device), e, \
            (e if variance else None)
    mc = fused.chunk_cols(st.n, m)
    if mc >= m:
        zpm, zpv, gm, gv = _one_call(st, xt, Pt, J, variance, zero_neg_variances)
    else:
        zpm, zpv, gm, gv = _chunked(st, xt, J, variance, mc)
        if zero_neg_variances:
            neg = zpv < 0.0
            zpv = torch.where(neg, torch.zeros_like(zpv), zpv)
            if gv is not None:
                gv = torch.where(neg.reshape(-1, 1), torch.zeros_like(gv), gv)
    if prior_grad is not None:
        zpm = zpm + prior_mean
        gm = gm + prior_grad
    return zpm, zpv, gm, gv
