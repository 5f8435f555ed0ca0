"""From a ``Model`` with a declared Matern covariance to a checked call of a fused C driver (include/gpmp_hip.h).

Every Python caller of a fused driver -- ``kriging.fused_prediction``, ``predict_grad``, ``posterior_mean`` and the criterion gradients
of ``gradients`` -- prepares the same things: the header's limits, a model check, the observations centred by the mean type with the
mean design beside them, the covariance parameters as a host vector of the right length, a workspace, an info word and one sentence
for a failed factorisation.  They are stated once here; a new caller of a fused driver starts from this module.
"""
from typing import NamedTuple

import numpy
import torch

from .. import num as gnp
from ..config import get_config
from ..kernel.matern import MaternCovariance
from .utils import mean_values as _mean_values


class _Limits(NamedTuple):
    """The constants of include/gpmp_hip.h that Python needs (GPMP_<name>; tests/test_fused_staging_cpu.py compares with the header)."""
    MAX_DIM: int = 64
    MAX_DIM_WIDE: int = 16384
    MAX_P: int = 16
    MAX_RANK: int = 72
    MAX_EXTENT: int = 1 << 30
    BATCH_MAX_N: int = 4096
    BATCH_MAX_Q: int = 16


limits = _Limits()
MEAN_TYPES = ("zero", "parameterized", "linear_predictor")


def check_matern_model(model, who):
    """The models the fused drivers serve: a declared Matern covariance with parameters, a zero, parameterized or linear-predictor mean."""
    if not isinstance(model.covariance, MaternCovariance):
        raise NotImplementedError(
            f"{who} needs a gpmp_amd.kernel.MaternCovariance covariance; for another covariance differentiate "
            "Model.predict by finite differences with gnp.grad")
    if model.meantype not in MEAN_TYPES:
        raise ValueError(f"Invalid meantype {model.meantype}.")
    if model.meantype == "parameterized" and model.meanparam is None:
        raise ValueError("For meantype 'parameterized', meanparam should not be None.")
    if model.covparam is None:
        raise ValueError("covparam is None")


def chunk_cols(n, m, floor=256):
    """Columns of xt per chunk: what the configured budget allows for an n x chunk fp64 matrix, at least ``floor``, at most m."""
    mc = max(floor, get_config().predict_chunk_bytes // (8 * max(n, 1)))
    return int(min(m, mc)) if m > 0 else 0


def stage_theta(cov, theta, d):
    """(hv, noise) for a driver call: the covariance parameters ``theta`` (a host array: one vector, or one row per problem) as the
    ctypes vector a driver reads them from -- a copy, kept alive by the caller -- and the driver's noise flag.  ValueError unless a row
    has 1 + noise + d entries."""
    noise = 1 if cov.noise else 0
    if theta.shape[-1] != 1 + noise + d:
        raise ValueError(f"covparam has {theta.shape[-1]} entries, expected {1 + noise + d}")
    return gnp._lib.host_vec(theta.reshape(-1)), noise


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


class Staged:
    """What the fused drivers take from a model and its data (xi, zi), prepared once: the points ``X`` (n x d, contiguous), the
    observations centred by a parameterized mean ``zc`` (a vector; with ``columns`` the n x s matrix of s observation vectors on the
    same points, each column centred), the mean design ``Pi`` (n x q, or None with q = 0), the covariance
    parameters (``hv`` for the drivers, ``theta`` the same numbers as a host array, ``p``, ``noise``) and the mean (``mean``,
    ``meantype``, ``meanparam``).

    The parameters are copies: changing the model afterwards changes nothing here.  ``covariance`` / ``covparam`` / ``mean`` /
    ``meanparam`` are the attributes the array-level routes (``kriging._Predictor``, the wide Gram route) read from a model, so the
    object is passed to them as it is."""

    def __init__(self, model, xi, zi, columns=False):
        cov = self.covariance = model.covariance
        self.X = gnp._points(xi)
        self.n, self.d = self.X.shape
        self.p = cov.p
        self.hv, self.noise = stage_theta(cov, gnp._host_params(model.covparam), self.d)
        self.mean, self.meantype = model.mean, model.meantype
        mp = model.meanparam
        self.meanparam = mp.detach().clone() if isinstance(mp, torch.Tensor) else (None if mp is None else numpy.array(mp, copy=True))
        zc = gnp.asarray(zi)
        if columns and (zc.dim() != 2 or zc.shape[0] != self.n):
            raise ValueError(f"the observation columns have shape {tuple(zc.shape)}, expected ({self.n}, s)")
        zc = zc if columns else zc.reshape(-1)
        if zc.dtype != torch.float64:
            zc = zc.to(torch.float64)
        self.Pi, self.q = None, 0
        if self.meantype == "parameterized":
            zc = zc - _mean_values(self, self.X, self.meanparam).reshape((-1, 1) if columns else (-1,))
        elif self.meantype == "linear_predictor":
            self.Pi = gnp.as_matrix(_mean_values(self, self.X, self.meanparam))
            self.q = self.Pi.shape[1]
        self.zc = zc.contiguous()

    @property
    def theta(self):
        """The staged covariance parameters as a host array (a view of ``hv``, not of the model's array)."""
        return numpy.ctypeslib.as_array(self.hv)

    covparam = theta

    def at(self, xt, gradient=False, mean_gradient=None):
        """(Pt, J, prior_mean, prior_grad) at the points xt (m x d): the mean design and, with ``gradient``, its Jacobian (m, q, d) for
        a linear-predictor mean; the prior mean (m,) and its gradient (m, d), to be added back, for a parameterized one; else None."""
        m, d = xt.shape
        Pt = J = prior_mean = prior_grad = None
        if self.meantype == "parameterized":
            prior_mean = _mean_values(self, xt, self.meanparam).reshape(-1)
            if gradient:
                prior_grad = _mean_jacobian(self, xt, mean_gradient).reshape(m, d)
        elif self.meantype == "linear_predictor":
            Pt = gnp.as_matrix(_mean_values(self, xt, self.meanparam))
            if Pt.shape[1] != self.q:
                raise ValueError(f"the mean design has {Pt.shape[1]} columns at xt, {self.q} at xi")
            if gradient:
                J = _mean_jacobian(self, xt, mean_gradient)
                if J.shape[1] != self.q:
                    raise ValueError(f"the mean Jacobian has {J.shape[1]} columns, the mean design {self.q}")
        return Pt, J, prior_mean, prior_grad


def ld(P):
    """Leading dimension of a mean design as the drivers take it: 0 when there is none."""
    return 0 if P is None else gnp._ld(P)


WS, INFO = object(), object()       # in a driver's argument list: the workspace / the info word that ``call_driver`` allocates


def call_driver(name, ws_elems, *args, n=None, who=None):
    """One checked call of the library symbol ``name`` on the current stream (the trailing stream argument is added here).  ``args``
    are the driver's arguments in order, the first a device tensor: tensors become pointers (None is NULL), ``WS`` a fresh workspace
    of max(ws_elems, 1) doubles, ``INFO`` a zeroed int32 word.  Returns info (0 without an ``INFO`` argument).  With ``who``, a
    non-zero info raises numpy.linalg.LinAlgError: a failed factorisation of K for info <= n, a rank-deficient mean design above;
    without it the caller decides."""
    dev = args[0].device
    ws = torch.empty(max(int(ws_elems), 1), dtype=torch.float64, device=dev)
    info = None
    cargs = []
    for a in args:
        if isinstance(a, torch.Tensor):
            a = a.data_ptr()
        elif a is WS:
            a = ws.data_ptr()
        elif a is INFO:
            info = torch.zeros(1, dtype=torch.int32, device=dev)
            a = info.data_ptr()
        cargs.append(a)
    gnp._lib.check(getattr(gnp._lib.load(), name)(*cargs, gnp._stream()), name)
    k = 0 if info is None else int(info.item())
    if k != 0 and who is not None:
        what = "K is not positive definite" if k <= n else "P^T K^-1 P is singular (rank-deficient mean design)"
        raise numpy.linalg.LinAlgError(f"{who}: {what} (info = {k})")
    return k


def grad_reduce(st, xt, u, lam):
    """D[u] and D[lambda] (either may be None) through gpmp_predict_grad_reduce, D[w]_t = sum_i w_i d k(x_i, x_t) / d x_t: every input
    dimension, shared by the chunked route of ``predict_grad`` and the wide route of ``posterior_mean``."""
    n, d, m = st.n, st.d, xt.shape[0]
    gu = torch.empty((m, d), dtype=torch.float64, device=xt.device) if u is not None else None
    gl = torch.empty((m, d), dtype=torch.float64, device=xt.device) if lam is not None else None
    call_driver("gpmp_predict_grad_reduce", gnp._lib.load().gpmp_predict_grad_reduce_ws_elems(n, m, d), st.X, xt, n, m, d, st.p, st.hv,
                st.noise, u, lam, gnp._ld(lam) if lam is not None else m, gu, gl, WS)
    return gu, gl
