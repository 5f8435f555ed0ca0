"""A fitted posterior mean: the weights once, then one matrix-free pass per evaluation.

Every prediction entry point starts from (xi, zi, theta) and pays for the Gram matrices, the factorisation and the n^2 m solve
again.  The posterior MEAN needs none of that per call: in its dual form (include/gpmp_hip.h, gpmp_posterior_weights /
gpmp_posterior_mean)

    beta = (P^T K^-1 P)^-1 P^T K^-1 z,    alpha = K^-1 (z - P beta)
    mean(x) = sum_i alpha_i k(x, x_i) + p(x)^T beta,      d mean / d x_j = D[alpha]_{.,j} + beta^T J_{.,.,j}

everything that depends on the data is two vectors.  ``PosteriorMean`` owns device copies of xi, alpha and beta and a snapshot of
the model's parameters; it holds no factor and no library state.  Input dimensions above GPMP_MAX_DIM (64) have no matrix-free
kernel: the value is then K(xt, xi) alpha by chunks of xt on the wide Gram route, the gradient gpmp_predict_grad_reduce.
"""
import numpy
import torch

from .. import num as gnp
from ..config import get_config
from . import predict_grad
from .utils import ensure_shapes_and_type
from .utils import mean_values as _mean_values

MAX_DIM = 64          # GPMP_MAX_DIM


class _Snapshot:
    """What predict_grad's helpers read from a model, frozen at fit time."""

    def __init__(self, model, theta):
        self.covariance = model.covariance
        self.covparam = numpy.array(theta, dtype=numpy.float64)       # a host copy: what the covariance hands to the library
        self.mean = model.mean
        self.meantype = model.meantype
        mp = model.meanparam
        self.meanparam = mp.detach().clone() if isinstance(mp, torch.Tensor) else (None if mp is None else numpy.array(mp, copy=True))


class PosteriorMean:
    """The posterior mean of ``model`` given (xi, zi), as a callable.

    ``post(xt)`` returns zpm; ``post.mean_and_gradient(xt)`` returns (zpm, dzpm) with dzpm of shape (m, d).  Built by
    ``Model.posterior_mean``.  Changing ``model.covparam`` or ``model.meanparam`` afterwards does not change an existing object.
    """

    def __init__(self, model, xi, zi):
        predict_grad._check_model(model)
        xi = gnp._points(xi)
        n, d = xi.shape
        if n < 1:
            raise ValueError("posterior_mean needs at least one observation")
        theta = predict_grad._theta(model, d)
        self._model = _Snapshot(model, theta)
        self._theta = theta
        self._p = int(model.covariance.p)
        self._noise = 1 if model.covariance.noise else 0
        self.xi = xi.clone()
        zc = gnp.asarray(zi).reshape(-1).to(torch.float64)
        Pi = None
        if model.meantype == "parameterized":
            zc = zc - _mean_values(self._model, self.xi, self._model.meanparam).reshape(-1)
        elif model.meantype == "linear_predictor":
            Pi = gnp.as_matrix(_mean_values(self._model, self.xi, self._model.meanparam))
        self.alpha, self.beta = self._weights(zc.contiguous(), Pi)

    @property
    def n(self):
        return int(self.xi.shape[0])

    @property
    def d(self):
        return int(self.xi.shape[1])

    @property
    def q(self):
        return 0 if self.beta is None else int(self.beta.shape[0])

    def _weights(self, zc, Pi):
        lib = gnp._lib.load()
        n, d = self.xi.shape
        q = 0 if Pi is None else int(Pi.shape[1])
        f64 = dict(dtype=torch.float64, device=self.xi.device)
        alpha = torch.empty(n, **f64)
        beta = torch.empty(q, **f64) if q else None
        info = torch.zeros(1, dtype=torch.int32, device=self.xi.device)
        ws = torch.empty(max(int(lib.gpmp_posterior_weights_ws_elems(n, q)), 1), **f64)
        gnp._lib.check(
            lib.gpmp_posterior_weights(gnp._ptr(self.xi), gnp._ptr(zc), gnp._ptr(Pi), gnp._ld(Pi) if q else 0, n, d, q, self._p,
                                       gnp._lib.host_vec(self._theta), self._noise, gnp._ptr(ws), gnp._ptr(alpha), gnp._ptr(beta),
                                       gnp._ptr(info), gnp._stream()),
            "gpmp_posterior_weights")
        k = int(info.item())
        if k != 0:
            what = "K is not positive definite" if k <= n else "P^T K^-1 P is singular (rank-deficient mean design)"
            raise numpy.linalg.LinAlgError(f"posterior_mean: {what} (info = {k})")
        return alpha, beta

    # ------------------------------------------------------------------ evaluation
    def _kernel(self, xt, Pt, J, gradient):
        """gpmp_posterior_mean: the matrix-free pass (d <= GPMP_MAX_DIM)."""
        lib = gnp._lib.load()
        n, d = self.xi.shape
        m = xt.shape[0]
        q = self.q
        f64 = dict(dtype=torch.float64, device=xt.device)
        zpm = torch.empty(m, **f64)
        gm = torch.empty((m, d), **f64) if gradient else None
        ws = torch.empty(max(int(lib.gpmp_posterior_mean_ws_elems(n, m, d, 1 if gradient else 0)), 1), **f64)
        gnp._lib.check(
            lib.gpmp_posterior_mean(gnp._ptr(self.xi), gnp._ptr(self.alpha), gnp._ptr(xt), gnp._ptr(Pt), gnp._ld(Pt) if q else 0,
                                    gnp._ptr(self.beta), gnp._ptr(J), n, m, d, q, self._p, gnp._lib.host_vec(self._theta), self._noise,
                                    gnp._ptr(ws), gnp._ptr(zpm), gnp._ptr(gm), gnp._stream()),
            "gpmp_posterior_mean")
        return zpm, gm

    def _wide(self, xt, Pt, J, gradient):
        """d > GPMP_MAX_DIM: K(xt_chunk, xi) alpha on the wide Gram route, the gradient through gpmp_predict_grad_reduce."""
        n = self.n
        m = xt.shape[0]
        mc = int(max(1, min(m, get_config().predict_chunk_bytes // (8 * max(n, 1)))))
        parts = []
        for j0 in range(0, m, mc):
            Kc = gnp.as_matrix(gnp.asarray(self._model.covariance(xt[j0 : j0 + mc].contiguous(), self.xi, self._model.covparam)))
            parts.append(gnp.matmul(Kc, self.alpha).reshape(-1))
        zpm = parts[0] if len(parts) == 1 else torch.cat(parts)
        if Pt is not None:
            zpm = zpm + gnp.matmul(Pt, self.beta).reshape(-1)
        gm = None
        if gradient:
            gm, _ = predict_grad._reduce(self._model, self.xi, xt, self.alpha, None, self._theta)
            if J is not None:
                gm = gm + torch.einsum("a,tad->td", self.beta, J)
        return zpm, gm

    def _evaluate(self, xt, mean_gradient, gradient, convert_in):
        _, _, xt = ensure_shapes_and_type(xi=self.xi, xt=xt, convert=convert_in)
        xt = gnp._points(xt)
        m, d = xt.shape
        dev = self.xi.device
        if m == 0:
            return torch.zeros(0, dtype=torch.float64, device=dev), (torch.zeros((0, d), dtype=torch.float64, device=dev) if gradient else None)
        model = self._model
        prior_mean = prior_grad = Pt = J = None
        if model.meantype == "parameterized":
            prior_mean = _mean_values(model, xt, model.meanparam).reshape(-1)
            if gradient:
                prior_grad = predict_grad._mean_jacobian(model, xt, mean_gradient).reshape(m, d)
        elif model.meantype == "linear_predictor":
            Pt = gnp.as_matrix(_mean_values(model, xt, model.meanparam))
            if Pt.shape[1] != self.q:
                raise ValueError(f"the mean design has {Pt.shape[1]} columns at xt, {self.q} at xi")
            if gradient:
                J = predict_grad._mean_jacobian(model, xt, mean_gradient)
                if J.shape[1] != self.q:
                    raise ValueError(f"the mean Jacobian has {J.shape[1]} columns, the mean design {self.q}")
        zpm, gm = (self._kernel if d <= MAX_DIM else self._wide)(xt, Pt, J, gradient)
        if prior_mean is not None:
            zpm = zpm + prior_mean
            if gradient:
                gm = gm + prior_grad
        return zpm, gm

    def __call__(self, xt, convert_in=True, convert_out=True):
        zpm, _ = self._evaluate(xt, None, False, convert_in)
        return gnp.to_np(zpm) if convert_out else zpm

    def mean_and_gradient(self, xt, mean_gradient=None, convert_in=True, convert_out=True):
        """(zpm, dzpm) at xt; ``mean_gradient(x, meanparam)`` as in ``Model.predict_gradient`` (autograd through the mean without it)."""
        zpm, gm = self._evaluate(xt, mean_gradient, True, convert_in)
        if convert_out:
            return gnp.to_np(zpm), gnp.to_np(gm)
        return zpm, gm
