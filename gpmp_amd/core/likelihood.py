"""Negative (restricted) log-likelihoods -- counterpart of gpmp/core/likelihood.py."""
import math

import numpy
import torch

from .. import num as gnp
from ..kernel.matern import MaternCovariance
from . import fused
from .utils import mean_values as _mean_values
from .linalg import MeanSpace, covariance_factor


def _scalar(v):
    return numpy.asarray(float(v), dtype=numpy.float64).reshape(())


def negative_log_likelihood_zero_mean(model, covparam, xi, zi):
    """gpmp/core/likelihood.py:18-52: 1/2 (n ln 2pi + 2 sum ln L_ii + z^T K^-1 z)."""
    xi, zi = gnp.asarray(xi), gnp.asarray(zi).reshape(-1)
    n = xi.shape[0]
    # a non-PD covariance raises HipLinAlgError (a numpy LinAlgError), as numpy.linalg.cholesky does under the reference's
    # NumPy backend; the criterion wrappers (gnp.DifferentiableSelectionCriterion) turn it into +inf.  Library / HIP
    # failures (GpmpHipError, out of memory) propagate: they are not numerical events.
    if isinstance(model.covariance, MaternCovariance):
        w, logdet = _whiten(model.covariance, covparam, xi, zi)
    else:
        F = covariance_factor(model, xi, covparam)
        w, logdet = F.solve_lower(zi), F.logdet()
    norm2 = float(gnp.sum(w * w).item())
    return _scalar(0.5 * (n * math.log(2.0 * math.pi) + logdet + norm2))


def _whiten(cov, covparam, xi, zi):
    """(L^-1 zi, ln|K|) through ONE library call, gpmp_whiten (include/gpmp_hip.h): the Gram build, the factorisation, the solve and
    the log-determinant that ``covariance_factor`` + ``solve_lower`` + ``logdet`` enqueue one by one, with the same bits -- and with
    the factor store consulted, so a call on the points and parameters of the stored factor (the ``predict`` before it, the
    criterion evaluation before it) neither builds nor factors K."""
    X = gnp._points(xi)
    n, d = X.shape
    hv, noise = fused.stage_theta(cov, gnp._host_params(covparam), d)
    Y = gnp.as_matrix(zi.reshape(-1, 1), copy=True)
    logdet = torch.empty(1, dtype=torch.float64, device=X.device)
    k = fused.call_driver("gpmp_whiten", gnp._lib.load().gpmp_whiten_ws_elems(n), X, n, d, cov.p, hv, noise, Y, 1, gnp._ld(Y), fused.WS,
                          logdet, fused.INFO)
    if k != 0:
        raise gnp.HipLinAlgError(
            f"Matrix is not positive definite: Cholesky factorization failed at leading minor {k} (potrf info={k})")
    return Y.reshape(-1), float(logdet.item())


def negative_log_likelihood(model, meanparam, covparam, xi, zi):
    """gpmp/core/likelihood.py:55-89."""
    xi, zi = gnp.asarray(xi), gnp.asarray(zi).reshape(-1)
    centered = zi - _mean_values(model, xi, meanparam).reshape(-1)
    return negative_log_likelihood_zero_mean(model, covparam, xi, centered)


def negative_log_restricted_likelihood(model, covparam, xi, zi):
    """gpmp/core/likelihood.py:92-129 without the n x n Q / W^T K W (identities in core/linalg.py)."""
    xi, zi = gnp.asarray(xi), gnp.asarray(zi).reshape(-1)
    # a non-PD covariance raises HipLinAlgError (a numpy LinAlgError), as numpy.linalg.cholesky does under the reference's
    # NumPy backend; the criterion wrappers (gnp.DifferentiableSelectionCriterion) turn it into +inf.  Library / HIP
    # failures (GpmpHipError, out of memory) propagate: they are not numerical events.
    F = covariance_factor(model, xi, covparam)
    P = _mean_values(model, xi, model.meanparam)
    n, q = P.shape
    ms = MeanSpace(F, zi, P)
    return _scalar(0.5 * ((n - q) * math.log(2.0 * math.pi) + ms.logdet_contrast() + ms.quad()))
