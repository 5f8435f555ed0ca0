"""Sample paths as functions: a random-Fourier-feature prior plus the exact matrix-free update (pathwise conditioning).

``Model.sample_paths`` draws paths at points chosen in advance, through the dense covariance of all of them.  Here a prior path is
a finite trigonometric sum over R frequencies drawn from the spectral measure of the Matern covariance,

    f_c(x) = sum_k W[k, c] cos(2 pi (omega_k . x + b_k)),        W[k, c] = sqrt(2 sigma^2 / R) w_kc,  w ~ N(0, 1),  b ~ U[0, 1)

and a posterior path adds the update of ``conditional_sample_paths_from_data`` to it,

    post_c(x) = f_c(x) + PosteriorMeans(xi, zi - f_c(xi) - eps_c)(x),        eps_c ~ N(0, noise variance) if the covariance has one,

which is exact given the prior function: only the prior is approximate in law, its covariance within O(R^-1/2) of the Matern
one.  Both are evaluated anywhere after construction: gpmp_fourier_paths (csrc/fourier_paths.hip) computes f at m points for all
paths in one launch, without the m x R block of features, and the update is one gpmp_posterior_mean_multi pass.

The spectral measure.  This project's Matern covariance is exp(-2 sqrt(nu) h) poly(h), nu = p + 1/2, h the distance scaled by
rho: a standard Matern with length scale rho / sqrt(2), whose spectral measure is a multivariate Student t with 2 nu degrees of
freedom.  In angular units omega_k = (sqrt(2) / rho) * g_k sqrt((2p + 1) / u_k), g_k ~ N(0, I_d), u_k ~ chi^2 with 2p + 1 degrees
of freedom (the sum of 2p + 1 squared standard normals); the kernel takes TURNS, so the draw divides by 2 pi once.  Everything
random is drawn on the HOST from one ``torch.Generator(device="cpu")``: a seed gives the same paths on any machine.
"""
import math

import torch

from .. import num as gnp
from . import fused
from .posterior_mean import MAX_COLUMNS, PosteriorMeans
from .utils import ensure_shapes_and_type


def draw_features(p, theta, noise, nb_paths, nb_features, generator):
    """(omega, phase, w) as host tensors, fp64: omega (R x d) and phase (R) in turns, w (R x s) standard normal -- the weights of
    the paths are sqrt(2 sigma^2 / R) w.  ``theta`` = [log sigma^2, (log noise variance,) log(1 / rho_1) .. log(1 / rho_d)]."""
    invrho = torch.exp(torch.as_tensor(theta[1 + noise:], dtype=torch.float64))
    R, d, dof = int(nb_features), invrho.shape[0], 2 * int(p) + 1
    g = torch.randn((R, d), dtype=torch.float64, generator=generator)
    u = torch.randn((R, dof), dtype=torch.float64, generator=generator).square().sum(dim=1)
    omega = g * (math.sqrt(2.0) * invrho) * torch.sqrt(dof / u).reshape(-1, 1) / (2.0 * math.pi)
    phase = torch.rand(R, dtype=torch.float64, generator=generator)
    w = torch.randn((R, int(nb_paths)), dtype=torch.float64, generator=generator)
    return omega, phase, w


def _generator(seed):
    gen = torch.Generator(device="cpu")
    if seed is None:
        gen.seed()
    else:
        gen.manual_seed(int(seed))
    return gen


class PriorPaths:
    """``nb_paths`` prior sample paths of ``model`` as a callable: ``prior(xt)`` is (m, nb_paths).  Built by ``Model.prior_paths``.
    Keeps omega, phase and W on the device and a snapshot of the covariance parameters; no library state."""

    def __init__(self, model, nb_paths, nb_features=4096, seed=None, generator=None):
        fused.check_matern_model(model, "prior_paths")
        if not 1 <= nb_paths <= MAX_COLUMNS:
            raise ValueError(f"prior_paths takes 1 to {MAX_COLUMNS} paths, got {nb_paths}")
        if not 1 <= nb_features <= fused.limits.MAX_EXTENT:
            raise ValueError(f"nb_features must be in [1, {fused.limits.MAX_EXTENT}], got {nb_features}")
        cov = model.covariance
        self.theta = gnp._host_params(model.covparam).copy()
        self.p, self.noise = cov.p, 1 if cov.noise else 0
        self.d = self.theta.shape[0] - 1 - self.noise
        if not 1 <= self.d <= fused.limits.MAX_DIM_WIDE:
            raise ValueError(f"covparam has {self.theta.shape[0]} entries: no input dimension in [1, {fused.limits.MAX_DIM_WIDE}]")
        self.s, self.r = int(nb_paths), int(nb_features)
        self.generator = generator if generator is not None else _generator(seed)
        omega, phase, w = draw_features(self.p, self.theta, self.noise, self.s, self.r, self.generator)
        self.omega, self.phase = gnp.asarray(omega).contiguous(), gnp.asarray(phase).contiguous()
        self.W = (gnp.asarray(w) * math.sqrt(2.0 * math.exp(self.theta[0]) / self.r)).contiguous()

    def _evaluate(self, xt):
        """(m, s) on the device from device points (m x d, contiguous)."""
        m, s = xt.shape[0], self.s
        out = torch.empty((m, s), dtype=torch.float64, device=xt.device)
        if m > 0:
            fused.call_driver("gpmp_fourier_paths", gnp._lib.load().gpmp_fourier_paths_ws_elems(m, self.r, s, self.d), xt, self.omega,
                              self.d, self.phase, self.W, s, m, self.r, s, self.d, fused.WS, out, s)
        return out

    def __call__(self, xt, convert_in=True, convert_out=True):
        _, _, xt = ensure_shapes_and_type(xt=xt, convert=convert_in)
        xt = gnp._points(xt)
        if xt.shape[1] != self.d:
            raise ValueError(f"xt is {xt.shape[1]}-dimensional but the covariance parameters are for {self.d} dimensions")
        out = self._evaluate(xt)
        return gnp.to_np(out) if convert_out else out

    paths = __call__


class PosteriorPaths:
    """``nb_paths`` posterior sample paths of ``model`` given (xi, zi) as a callable: ``post(xt)`` is (m, nb_paths).  Built by
    ``Model.posterior_paths``.  ``prior`` is the ``PriorPaths`` object, ``eps`` the (n, nb_paths) noise draws (None without a noise
    parameter) and ``means`` the ``PosteriorMeans`` of the residual columns zi - prior(xi) - eps; a zero, parameterized or
    linear-predictor mean is handled there, as in ``conditional_sample_paths_from_data``."""

    def __init__(self, model, xi, zi, nb_paths, nb_features=4096, seed=None):
        self.prior = PriorPaths(model, nb_paths, nb_features, seed)
        xi = gnp._points(xi)
        if xi.shape[1] != self.prior.d:
            raise ValueError(f"xi is {xi.shape[1]}-dimensional but the covariance parameters are for {self.prior.d} dimensions")
        delta = gnp.asarray(zi).reshape(-1, 1) - self.prior._evaluate(xi)
        self.eps = None
        if self.prior.noise:
            std = math.exp(0.5 * self.prior.theta[1])
            self.eps = gnp.asarray(std * torch.randn((xi.shape[0], self.prior.s), dtype=torch.float64, generator=self.prior.generator))
            delta = delta - self.eps
        self.means = PosteriorMeans(model, xi, delta)

    def __call__(self, xt, convert_in=True, convert_out=True):
        _, _, xt = ensure_shapes_and_type(xi=self.means.xi, xt=xt, convert=convert_in)
        xt = gnp._points(xt)
        out = self.prior._evaluate(xt) + self.means(xt, convert_in=False, convert_out=False)
        return gnp.to_np(out) if convert_out else out

    paths = __call__
