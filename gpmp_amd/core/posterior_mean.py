"""A fitted posterior mean: the weights once, then one matrix-free pass per evaluation.

Every prediction entry point starts from (xi, zi, theta) and pays for the Gram matrices, the factorisation and the n^2 m solve
again.  The posterior MEAN needs none of that per call: in its dual form (include/gpmp_hip.h, gpmp_posterior_weights /
gpmp_posterior_mean)

    beta = (P^T K^-1 P)^-1 P^T K^-1 z,    alpha = K^-1 (z - P beta)
    mean(x) = sum_i alpha_i k(x, x_i) + p(x)^T beta,      d mean / d x_j = D[alpha]_{.,j} + beta^T J_{.,.,j}

everything that depends on the data is two vectors.  ``PosteriorMean`` owns device copies of xi, alpha and beta and a snapshot of
the model's parameters; it holds no factor and no library state.  Input dimensions above GPMP_MAX_DIM (64) take the value from
gpmp_posterior_mean_wide, the matrix-free kernel that streams d (s = 1 for ``PosteriorMean``), wherever it was measured to be no
slower than K(xt, xi) W by chunks of xt on the wide Gram route (``wide_kernel_serves``), and from that route elsewhere.  The
gradient at d > 64 stays gpmp_predict_grad_reduce: a matrix-free Jacobian at wide d would repeat an entry's 2 d distance
instructions once per block of components, a cost that grows as d^2 per entry, so it is not built.

``PosteriorMeans`` is the same for s observation vectors on one design (gpmp_posterior_weights_multi / gpmp_posterior_mean_multi):
one factorisation, the weights A = K^-1 (Z - P B) (n x s) and B (q x s), and per evaluation one pass in which every covariance
entry is computed once and contracted against all columns by fp64 matrix instructions.  ``PosteriorMeans.mean_and_gradient`` adds
the Jacobian of the s outputs from the same kind of pass (gpmp_posterior_mean_multi_grad): value and gradient are d + 1 components
per (point, column), all contracted from the same entries.
"""
import torch

from .. import num as gnp
from . import fused
from .utils import ensure_shapes_and_type

MAX_DIM = fused.limits.MAX_DIM
MAX_COLUMNS = 4096          # GPMP_MAX_COLUMNS of include/gpmp_hip.h
# PosteriorMeans.mean_and_gradient below this many columns: one gpmp_posterior_mean call per column.  Measured on one MI355X at
# n = 32768, m = 50000, d = 8, p = 2 (tools/posterior_mean_multi_grad_bench.py): gpmp_posterior_mean with the gradient 5.04 ms per
# column; gpmp_posterior_mean_multi_grad 18.7 ms at s = 1 and 21.3 ms at s = 16, so three columns are cheaper one by one, four are not.
GRAD_SINGLE_BELOW = 4


# gpmp_posterior_mean_wide against the chunked Gram route at d > GPMP_MAX_DIM.  Measured on one MI355X at n = 32768, m = 50000, p = 2
# (tools/posterior_mean_wide_bench.py, HIP events, ms, kernel / chunked route):
#   s = 1:   d = 65  16.4 / 23.1    96  22.7 / 28.0    128  29.2 / 32.7    160  36.2 / 37.8    192  43.1 / 42.4    256  57.1 / 52.1
#            1024  225 / 173
#   s = 4:   d = 65  16.5 / 20.8    128  29.4 / 29.9          s = 16:  d = 65  16.8 / 20.9    128  29.4 / 29.7
#   s = 64:  d = 65  24.7 / 20.7    128  39.5 / 29.6    1024  270 / 170
# so the kernel serves one column up to d = 160 and 2 to 16 columns up to d = 128 (17 to 63 columns were not measured); everything
# else keeps the chunked route.  The kernel's peak memory is the scaled points (n d doubles, 50 to 340 MB here) against the
# 12.5 GB Gram block of the chunked route.
WIDE_KERNEL_MAX_DIM_SINGLE = 160
WIDE_KERNEL_MAX_DIM = 128
WIDE_KERNEL_MAX_COLUMNS = 16


def wide_kernel_serves(d, s):
    """Whether gpmp_posterior_mean_wide (not the chunked Gram route) evaluates s columns at input dimension d > GPMP_MAX_DIM."""
    return d <= WIDE_KERNEL_MAX_DIM_SINGLE if s == 1 else (s <= WIDE_KERNEL_MAX_COLUMNS and d <= WIDE_KERNEL_MAX_DIM)


def _wide_value(st, xt, W, s, Pt, B):
    """The value at d > GPMP_MAX_DIM, (m, s): W the weights (n x s, or a vector with s = 1), B (q x s, or a vector) or None.
    gpmp_posterior_mean_wide, the matrix-free pass, or K(xt_chunk, xi) @ W by chunks of xt on the wide Gram route plus Pt B."""
    m = xt.shape[0]
    if wide_kernel_serves(st.d, s):
        out = torch.empty((m, s), dtype=torch.float64, device=xt.device)
        fused.call_driver("gpmp_posterior_mean_wide", gnp._lib.load().gpmp_posterior_mean_wide_ws_elems(st.n, m, s, st.d), st.X, W, s, xt,
                          Pt, fused.ld(Pt), B, s, st.n, m, s, st.d, st.q, st.p, st.hv, st.noise, fused.WS, out, s)
        return out
    mc = fused.chunk_cols(st.n, m, floor=1)
    out = torch.cat([gnp.matmul(gnp.as_matrix(gnp.asarray(st.covariance(xt[j0 : j0 + mc].contiguous(), st.X, st.covparam))), W.reshape(-1, s))
                     for j0 in range(0, m, mc)])
    return out if Pt is None else out + gnp.matmul(Pt, B.reshape(-1, s))


class PosteriorMean:
    """The posterior mean of ``model`` given (xi, zi), as a callable.

    ``post(xt)`` returns zpm; ``post.mean_and_gradient(xt)`` returns (zpm, dzpm) with dzpm of shape (m, d).  Built by
    ``Model.posterior_mean``.  Changing ``model.covparam`` or ``model.meanparam`` afterwards does not change an existing object.
    """

    def __init__(self, model, xi, zi):
        fused.check_matern_model(model, "posterior_mean")
        xi = gnp._points(xi)
        if xi.shape[0] < 1:
            raise ValueError("posterior_mean needs at least one observation")
        st = self._st = fused.Staged(model, xi.clone(), zi)         # (its own copy of the points, as of the parameters)
        n, q = st.n, st.q
        self.alpha = torch.empty(n, dtype=torch.float64, device=st.X.device)
        self.beta = torch.empty(q, dtype=torch.float64, device=st.X.device) if q else None
        fused.call_driver("gpmp_posterior_weights", gnp._lib.load().gpmp_posterior_weights_ws_elems(n, q), st.X, st.zc, st.Pi,
                          fused.ld(st.Pi), n, st.d, q, st.p, st.hv, st.noise, fused.WS, self.alpha, self.beta, fused.INFO, n=n,
                          who="posterior_mean")

    xi = property(lambda self: self._st.X)
    n = property(lambda self: self._st.n)
    d = property(lambda self: self._st.d)
    q = property(lambda self: self._st.q)

    # ------------------------------------------------------------------ evaluation
    def _kernel(self, xt, Pt, J, gradient):
        """gpmp_posterior_mean: the matrix-free pass (d <= GPMP_MAX_DIM)."""
        st, m = self._st, xt.shape[0]
        zpm = torch.empty(m, dtype=torch.float64, device=xt.device)
        gm = torch.empty((m, st.d), dtype=torch.float64, device=xt.device) if gradient else None
        fused.call_driver("gpmp_posterior_mean", gnp._lib.load().gpmp_posterior_mean_ws_elems(st.n, m, st.d, 1 if gradient else 0), st.X,
                          self.alpha, xt, Pt, fused.ld(Pt), self.beta, J, st.n, m, st.d, st.q, st.p, st.hv, st.noise, fused.WS, zpm, gm)
        return zpm, gm

    def _wide(self, xt, Pt, J, gradient):
        """d > GPMP_MAX_DIM: the value from ``_wide_value`` (s = 1), the gradient through gpmp_predict_grad_reduce."""
        st = self._st
        zpm = _wide_value(st, xt, self.alpha, 1, Pt, self.beta).reshape(-1)
        gm = None
        if gradient:
            gm, _ = fused.grad_reduce(st, xt, self.alpha, None)
            if J is not None:
                gm = gm + torch.einsum("a,tad->td", self.beta, J)
        return zpm, gm

    def _evaluate(self, xt, mean_gradient, gradient, convert_in):
        _, _, xt = ensure_shapes_and_type(xi=self.xi, xt=xt, convert=convert_in)
        xt = gnp._points(xt)
        m, d = xt.shape
        if m == 0:
            dev = self.xi.device
            return torch.zeros(0, dtype=torch.float64, device=dev), (torch.zeros((0, d), dtype=torch.float64, device=dev) if gradient else None)
        Pt, J, prior_mean, prior_grad = self._st.at(xt, gradient, mean_gradient)
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


class PosteriorMeans:
    """The posterior means of ``model`` given xi and the s columns of ``zi_columns`` (n x s), as a callable: ``post(xt)`` is (m, s),
    column c the posterior mean for the observations ``zi_columns[:, c]``; ``post.mean_and_gradient(xt)`` returns (O, G) with G of
    shape (m, s, d), the Jacobian of the s outputs at each point.  Built by ``Model.posterior_means``; the parameter snapshot is
    that of ``PosteriorMean``."""

    def __init__(self, model, xi, zi_columns):
        fused.check_matern_model(model, "posterior_means")
        xi = gnp._points(xi)
        if xi.shape[0] < 1:
            raise ValueError("posterior_means needs at least one observation")
        st = self._st = fused.Staged(model, xi.clone(), zi_columns, columns=True)
        n, q, s = st.n, st.q, st.zc.shape[1]
        if not 1 <= s <= MAX_COLUMNS:
            raise ValueError(f"posterior_means takes 1 to {MAX_COLUMNS} observation columns, got {s}")
        self.s = s
        self.A = torch.empty((n, s), dtype=torch.float64, device=st.X.device)
        self.B = torch.empty((q, s), dtype=torch.float64, device=st.X.device) if q else None
        fused.call_driver("gpmp_posterior_weights_multi", gnp._lib.load().gpmp_posterior_weights_multi_ws_elems(n, s, q), st.X, st.zc, s,
                          st.Pi, fused.ld(st.Pi), n, s, st.d, q, st.p, st.hv, st.noise, fused.WS, self.A, s, self.B, s, fused.INFO, n=n,
                          who="posterior_means")

    xi = property(lambda self: self._st.X)
    n = property(lambda self: self._st.n)
    d = property(lambda self: self._st.d)
    q = property(lambda self: self._st.q)

    def _kernel(self, xt, Pt):
        """gpmp_posterior_mean_multi: the matrix-free pass (d <= GPMP_MAX_DIM)."""
        st, m, s = self._st, xt.shape[0], self.s
        out = torch.empty((m, s), dtype=torch.float64, device=xt.device)
        fused.call_driver("gpmp_posterior_mean_multi", gnp._lib.load().gpmp_posterior_mean_multi_ws_elems(st.n, m, s, st.d), st.X, self.A, s,
                          xt, Pt, fused.ld(Pt), self.B, s, st.n, m, s, st.d, st.q, st.p, st.hv, st.noise, fused.WS, out, s)
        return out

    def _wide(self, xt, Pt):
        """d > GPMP_MAX_DIM: ``_wide_value``."""
        return _wide_value(self._st, xt, self.A, self.s, Pt, self.B)

    def _kernel_grad(self, xt, Pt, J):
        """gpmp_posterior_mean_multi_grad: value and Jacobian from one matrix-free pass (d <= GPMP_MAX_DIM); G is (m, d, s)."""
        st, m, s = self._st, xt.shape[0], self.s
        out = torch.empty((m, s), dtype=torch.float64, device=xt.device)
        G = torch.empty((m, st.d, s), dtype=torch.float64, device=xt.device)
        if s < GRAD_SINGLE_BELOW:                # the single-column kernel, column by column
            zpm, gm = torch.empty(m, dtype=torch.float64, device=xt.device), torch.empty((m, st.d), dtype=torch.float64, device=xt.device)
            for c in range(s):
                fused.call_driver("gpmp_posterior_mean", gnp._lib.load().gpmp_posterior_mean_ws_elems(st.n, m, st.d, 1), st.X,
                                  self.A[:, c].contiguous(), xt, Pt, fused.ld(Pt), None if self.B is None else self.B[:, c].contiguous(), J,
                                  st.n, m, st.d, st.q, st.p, st.hv, st.noise, fused.WS, zpm, gm)
                out[:, c], G[:, :, c] = zpm, gm
            return out, G
        fused.call_driver("gpmp_posterior_mean_multi_grad", gnp._lib.load().gpmp_posterior_mean_multi_grad_ws_elems(st.n, m, s, st.d), st.X,
                          self.A, s, xt, Pt, fused.ld(Pt), self.B, s, J, st.n, m, s, st.d, st.q, st.p, st.hv, st.noise, fused.WS, out, s, G, s)
        return out, G

    def _wide_grad(self, xt, Pt, J):
        """d > GPMP_MAX_DIM: the value as ``_wide``, the gradient column by column through gpmp_predict_grad_reduce."""
        G = torch.stack([fused.grad_reduce(self._st, xt, self.A[:, c].contiguous(), None)[0] for c in range(self.s)], dim=2)
        if J is not None:
            G = G + torch.einsum("ac,tad->tdc", self.B, J)
        return self._wide(xt, Pt), G.contiguous()

    def _evaluate(self, xt, mean_gradient, gradient, convert_in):
        """(O, G) as device tensors, G in the kernel's layout (m, d, s), or None without ``gradient``."""
        _, _, xt = ensure_shapes_and_type(xi=self.xi, xt=xt, convert=convert_in)
        xt = gnp._points(xt)
        m, d = xt.shape
        if m == 0:
            dev = self.xi.device
            return (torch.zeros((0, self.s), dtype=torch.float64, device=dev),
                    torch.zeros((0, d, self.s), dtype=torch.float64, device=dev) if gradient else None)
        Pt, J, prior_mean, prior_grad = self._st.at(xt, gradient, mean_gradient)
        if gradient:
            out, G = (self._kernel_grad if d <= MAX_DIM else self._wide_grad)(xt, Pt, J)
        else:
            out, G = (self._kernel if d <= MAX_DIM else self._wide)(xt, Pt), None
        if prior_mean is not None:
            out = out + prior_mean.reshape(-1, 1)
            if gradient:
                G = G + prior_grad.reshape(m, d, 1)
        return out, G

    def __call__(self, xt, convert_in=True, convert_out=True):
        out, _ = self._evaluate(xt, None, False, convert_in)
        return gnp.to_np(out) if convert_out else out

    def mean_and_gradient(self, xt, mean_gradient=None, convert_in=True, convert_out=True):
        """(O, G) at xt: O (m, s) as ``post(xt)``, G (m, s, d) with G[t, c] the gradient of output c at x_t (with
        ``convert_out=False`` a permuted view of the (m, d, s) device buffer the kernel writes).  ``mean_gradient(x, meanparam)`` as
        in ``PosteriorMean.mean_and_gradient``; a parameterized mean adds its prior gradient to every column."""
        out, G = self._evaluate(xt, mean_gradient, True, convert_in)
        G = G.permute(0, 2, 1)
        return (gnp.to_np(out), gnp.to_np(G)) if convert_out else (out, G)
