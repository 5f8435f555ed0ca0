"""Inputs of dimension d > GPMP_MAX_DIM (= 64) through every path that builds a covariance: the wide-dimension kernels
(the wide route of gpmp_amd/csrc/gram.hip) behind gpmp_matern_gram, gpmp_scaled_distance, gpmp_matern_pairwise, gpmp_matern_gram_deriv,
gpmp_matern_grad_trace(_cross) and the fused drivers, checked against the reference's own outputs (tests/golden/ref_wide_dim.npz,
written by make_fixtures_wide_dim.py) and the CPU oracle.

Tolerance of K against the reference's cdist: both sides sum the d squared scaled differences of one entry one after the other, in
different roundings (fma here, separate multiply and add there) and with the scale 2 c / rho applied before (here) or after (there)
the square root.  The relative difference of h^2 is then at most about d u (u = 2^-53), that of h half of it, and that of K(h) is
|h K'(h) / K(h)| times that of h.  The bound used is  rtol = 1e-14 + amp d u  with amp = max |h K'(h) / K(h)| over the entries of
the case (computed from the oracle), which stays below 1e-13 up to d = 200 and is about 5e-13 at d = 1000."""
import ctypes
import math

import numpy as np
import pytest

from tests.helpers import rel_err

pytestmark = pytest.mark.gpu

U = 2.0 ** -53


@pytest.fixture(scope="module")
def env():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import gpmp_amd as gp
    import gpmp_amd.num as gnp
    from gpmp_amd import _lib

    return torch, gp, gnp, _lib, _lib.load()


@pytest.fixture(scope="module")
def wide(golden):
    from tests.wide_dim_inputs import decode

    return decode(golden("wide_dim"))


def _orc():
    from oracle import gp_oracle as orc

    return orc


def _theta_wide(d, sigma2=1.0):
    rho = 0.5 * np.sqrt(d) * 0.5 * (1.0 + np.arange(d) / d)
    return np.concatenate(([np.log(sigma2)], -np.log(rho)))


def _xz(n, d, seed):
    rng = np.random.default_rng(seed)
    x = rng.random((n, d))
    return x, np.sin(2 * np.pi * x[:, 0]) + x[:, 1:].sum(axis=1) / np.sqrt(d)


def _k_rtol(p, h, d):
    """1e-14 + amp d u, amp = max |h K'(h) / K(h)| over h > 0 (see the module docstring)."""
    orc = _orc()
    h = np.asarray(h, dtype=np.float64).ravel()
    h = h[h > 0]
    k = orc.maternp_kernel(p, h)
    dk = orc.maternp_dkernel_over_h(p, h) * h * h
    amp = float(np.max(np.abs(dk / k))) if h.size else 1.0
    return 1e-14 + max(amp, 1.0) * d * U


# ------------------------------------------------------------------------------------------------ Gram, distance, pairwise
@pytest.mark.parametrize("d", [65, 200, 1000])
def test_gram_distance_pairwise_vs_reference(env, wide, d):
    torch, gp, gnp, _lib, lib = env
    g = wide
    x, y, th, thn = g[f"gram_d{d}_x"], g[f"gram_d{d}_y"], g[f"gram_d{d}_theta"], g[f"gram_d{d}_theta_noise"]
    xt, yt = gnp.asarray(x), gnp.asarray(y)
    D = gnp.to_np(gnp.scaled_distance(th[1:], xt, yt))
    np.testing.assert_allclose(D, g[f"dist_d{d}"], rtol=1e-14 + d * U, atol=0)
    hii = _orc().scaled_distance(th[1:], x, x)
    for p in (0, 2, 5):
        rt = _k_rtol(p, np.concatenate((D.ravel(), hii.ravel())), d)
        assert rt < (1e-13 if d <= 200 else 1e-12)
        mc = gp.kernel.maternp_covariance
        np.testing.assert_allclose(gnp.to_np(mc(xt, None, p, th)), g[f"gram_d{d}_p{p}_ii"], rtol=rt)
        np.testing.assert_allclose(gnp.to_np(mc(xt, xt, p, th)), g[f"gram_d{d}_p{p}_ii"], rtol=rt)
        np.testing.assert_allclose(gnp.to_np(mc(xt, yt, p, th)), g[f"gram_d{d}_p{p}_it"], rtol=rt)
        np.testing.assert_allclose(gnp.to_np(mc(xt[:yt.shape[0]], yt, p, th, True)), g[f"gram_d{d}_p{p}_pw"], rtol=rt)
        cov = gp.kernel.MaternCovariance(p, noise=True)
        np.testing.assert_allclose(gnp.to_np(cov(xt, None, thn)), g[f"gram_d{d}_p{p}_noise_ii"], rtol=rt)
        np.testing.assert_allclose(gnp.to_np(cov(xt, yt, thn)), g[f"gram_d{d}_p{p}_noise_it"], rtol=rt)


def test_seam_d64_vs_d65_with_a_zero_coordinate(env):
    """d = 64 takes gram_kernel_v3, d = 65 the wide kernel: a 65th coordinate that is zero everywhere must give the same K."""
    torch, gp, gnp, _lib, lib = env
    rng = np.random.default_rng(7)
    x64, y64 = rng.random((333, 64)), rng.random((201, 64))
    x65, y65 = np.hstack((x64, np.zeros((333, 1)))), np.hstack((y64, np.zeros((201, 1))))
    th64 = _theta_wide(64, 0.7)
    th65 = np.concatenate((th64, [0.3]))
    for p in (0, 1, 2, 3, 7):
        for a, b in ((None, None), (y64, y65)):
            K64 = gnp.to_np(gp.kernel.maternp_covariance(gnp.asarray(x64), None if a is None else gnp.asarray(a), p, th64))
            K65 = gnp.to_np(gp.kernel.maternp_covariance(gnp.asarray(x65), None if b is None else gnp.asarray(b), p, th65))
            assert rel_err(K65, K64) <= 1e-15, (p, rel_err(K65, K64))
    D64 = gnp.to_np(gnp.scaled_distance(th64[1:], gnp.asarray(x64), gnp.asarray(y64)))
    D65 = gnp.to_np(gnp.scaled_distance(th65[1:], gnp.asarray(x65), gnp.asarray(y65)))
    assert rel_err(D65, D64) <= 1e-15


def test_lower_only_leaves_the_upper_tiles_and_padding_untouched(env):
    torch, gp, gnp, _lib, lib = env
    n, d, p = 333, 97, 2
    x, _ = _xz(n, d, 11)
    th = _theta_wide(d)
    ref = _orc().maternp_covariance(x, x, p, th)
    guard = -7.25
    for ld in (n, n + 1, n + 16):                      # even and odd leading dimensions
        buf = torch.full((n * ld + 8,), guard, dtype=torch.float64, device=gnp._dev())
        X = torch.as_tensor(x, device=gnp._dev())
        diag = 10.0 * math.exp(th[0]) * np.finfo(float).eps
        _lib.check(lib.gpmp_matern_gram(gnp._ptr(X), None, n, n, d, p, _lib.host_vec(th), 0, diag, 1, gnp._ptr(buf), ld,
                                        gnp._stream()), "gpmp_matern_gram")
        K = buf[:n * ld].view(n, ld).cpu().numpy()
        assert np.all(buf[n * ld:].cpu().numpy() == guard)
        rows, cols = np.arange(n)[:, None] // 128, np.arange(n)[None, :] // 64
        written = cols * 64 <= rows * 128 + 127
        rt = _k_rtol(p, _orc().scaled_distance(th[1:], x, x), d)
        np.testing.assert_allclose(K[:, :n][written], ref[written], rtol=rt)
        assert np.all(K[:, :n][~written] == guard)
        assert np.all(K[:, n:] == guard)


def test_ragged_tiles_and_odd_leading_dimension(env):
    torch, gp, gnp, _lib, lib = env
    orc = _orc()
    for n, m, d in ((1, 1, 65), (129, 65, 130), (257, 63, 777)):
        x, _ = _xz(n, d, n)
        y, _ = _xz(m, d, m + 1)
        th = _theta_wide(d, 1.7)
        ld = m + 3
        buf = torch.full((n * ld + 4,), 3.5, dtype=torch.float64, device=gnp._dev())
        X, Y = torch.as_tensor(x, device=gnp._dev()), torch.as_tensor(y, device=gnp._dev())
        _lib.check(lib.gpmp_matern_gram(gnp._ptr(X), gnp._ptr(Y), n, m, d, 3, _lib.host_vec(th), 0, 0.0, 0, gnp._ptr(buf[1:]), ld,
                                        gnp._stream()), "gpmp_matern_gram")
        out = buf.cpu().numpy()
        K = out[1:1 + n * ld].reshape(n, ld)
        ref = orc.maternp_covariance(x, y, 3, th)
        np.testing.assert_allclose(K[:, :m], ref, rtol=_k_rtol(3, orc.scaled_distance(th[1:], x, y), d))
        assert np.all(K[:, m:] == 3.5) and out[0] == 3.5 and np.all(out[1 + n * ld:] == 3.5)


def test_two_streams_do_not_share_length_scales(env):
    """Each call stages its own copy of the length scales: two different parameter vectors enqueued back to back on two streams
    give each its own matrix."""
    torch, gp, gnp, _lib, lib = env
    n, d = 700, 300
    x, _ = _xz(n, d, 3)
    X = torch.as_tensor(x, device=gnp._dev())
    ths = [_theta_wide(d, 1.0), _theta_wide(d, 1.0) + np.concatenate(([0.0], np.full(d, 0.4)))]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    outs = [gnp.alloc_matrix(n, n) for _ in ths]
    for _ in range(3):
        for th, s, K in zip(ths, streams, outs):
            with torch.cuda.stream(s):
                _lib.check(lib.gpmp_matern_gram(gnp._ptr(X), None, n, n, d, 2, _lib.host_vec(th), 0, 0.0, 0, gnp._ptr(K), gnp._ld(K),
                                                gnp._stream()), "gpmp_matern_gram")
    torch.cuda.synchronize()
    for th, K in zip(ths, outs):
        ref = _orc().maternp_covariance(x, x, 2, th) - 10.0 * np.finfo(float).eps * np.eye(n)   # (diag_add 0 here)
        np.testing.assert_allclose(K.cpu().numpy(), ref, rtol=1e-13, atol=1e-15)


def test_near_duplicate_points(env, wide):
    torch, gp, gnp, _lib, lib = env
    g = wide
    xd, zd, thd = g["dup_xi"], g["dup_zi"], g["dup_theta"]
    K = gnp.to_np(gp.kernel.maternp_covariance(gnp.asarray(xd), None, 2, thd))
    np.testing.assert_allclose(K, g["dup_K"], rtol=_k_rtol(2, _orc().scaled_distance(thd[1:], xd, xd), 200))
    model = gp.Model(None, gp.kernel.MaternCovariance(2), None, thd, "zero")
    nll = float(model.negative_log_likelihood_zero_mean(thd, xd, zd))
    # K is nearly singular (pairs 1e-6 apart; the 10 sigma^2 eps nugget keeps it positive definite): the value carries cond(K) u
    assert math.isfinite(nll) and abs(nll - float(g["dup_nll"])) < 1e-6 * abs(float(g["dup_nll"]))


# ------------------------------------------------------------------------------------------------ criteria, gradients, predictions
def _const(gnp):
    return lambda x, prm: gnp.ones((x.shape[0], 1))


def _lin(gnp):
    return lambda x, prm: gnp.hstack((gnp.ones((x.shape[0], 1)), gnp.asarray(x)[:, :3]))     # (as make_fixtures_wide_dim.py)


def test_criteria_and_gradients_vs_reference_autograd(env, wide):
    torch, gp, gnp, _lib, lib = env
    g = wide
    xi, zi, th = g["crit_xi"], g["crit_zi"], g["crit_theta"]
    cov = gp.kernel.MaternCovariance(2)
    for name, model, crit in (("nll", gp.Model(None, cov, None, None, "zero"), gp.kernel.negative_log_likelihood_zero_mean),
                              ("reml_const", gp.Model(_const(gnp), cov, None, None), gp.kernel.negative_log_restricted_likelihood)):
        _, pre, _, grad = gp.kernel.make_selection_criterion_with_gradient(model, crit, xi, zi)
        v, gr = float(pre(th)), np.asarray(grad(th), dtype=float)
        assert abs(v - float(g[f"crit_{name}"])) < 1e-11 * abs(float(g[f"crit_{name}"])), name
        assert rel_err(gr, g[f"crit_{name}_grad"]) < 1e-7, (name, rel_err(gr, g[f"crit_{name}_grad"]))
    # noisy kernel, p = 0 (subgradient 0 at coincident points)
    covn = gp.kernel.MaternCovariance(0, noise=True)
    _, pre, _, grad = gp.kernel.make_selection_criterion_with_gradient(gp.Model(None, covn, None, None, "zero"),
                                                                       gp.kernel.negative_log_likelihood_zero_mean, g["critn_xi"], g["critn_zi"])
    v, gr = float(pre(g["critn_theta"])), np.asarray(grad(g["critn_theta"]), dtype=float)
    assert abs(v - float(g["critn_nll"])) < 1e-11 * abs(float(g["critn_nll"]))
    assert rel_err(gr, g["critn_nll_grad"]) < 1e-7


def test_predictions_and_loo_vs_reference(env, wide):
    torch, gp, gnp, _lib, lib = env
    g = wide
    xi, zi, th, xt = g["crit_xi"], g["crit_zi"], g["crit_theta"], g["pred_xt"]
    cov = gp.kernel.MaternCovariance(2)
    for tag, model in (("zero", gp.Model(None, cov, None, th, "zero")), ("const", gp.Model(_const(gnp), cov, None, th)),
                       ("lin", gp.Model(_lin(gnp), cov, None, th))):
        zpm, zpv = model.predict(xi, zi, xt)
        assert rel_err(gnp.to_np(zpm), g[f"pred_{tag}_zpm"]) < 1e-11, tag
        assert rel_err(gnp.to_np(zpv), g[f"pred_{tag}_zpv"]) < 1e-9, tag     # (1 - |V|^2: cancellation at the data scale)
    xl, zl, thl = g["loo_xi"], g["loo_zi"], g["loo_theta"]
    for tag, model in (("zero", gp.Model(None, cov, None, thl, "zero")), ("const", gp.Model(_const(gnp), cov, None, thl))):
        zloo, s2, eloo = (gnp.to_np(a) for a in model.loo(xl, zl))
        assert rel_err(zloo, g[f"loo_{tag}_zloo"]) < 1e-11 and rel_err(eloo, g[f"loo_{tag}_eloo"]) < 1e-10, tag
        assert rel_err(s2, g[f"loo_{tag}_s2"]) < 1e-10, tag


class _Drivers:
    """The fused C-ABI drivers through ctypes (as a non-Python host calls them)."""

    def __init__(self, env, x, z, P, p):
        torch, gp, gnp, _lib, lib = self.env = env
        dev = gnp._dev()
        self.n, self.d = x.shape
        self.q, self.p = (0 if P is None else P.shape[1]), p
        self.X, self.Z = torch.as_tensor(x, device=dev), torch.as_tensor(z, device=dev)
        self.P = None if P is None else torch.as_tensor(np.ascontiguousarray(P), device=dev)
        self.info = torch.zeros(1, dtype=torch.int32, device=dev)

    def _args(self, th):
        torch, gp, gnp, _lib, lib = self.env
        return (gnp._ptr(self.X), gnp._ptr(self.Z), gnp._ptr(self.P), max(self.q, 1), self.n, self.d, self.q, self.p, _lib.host_vec(th), 0)

    def value_grad(self, th):
        torch, gp, gnp, _lib, lib = self.env
        ws = torch.empty(int(lib.gpmp_nll_grad_ws_elems(self.n, self.d, self.q)), dtype=torch.float64, device=gnp._dev())
        val = torch.empty(1, dtype=torch.float64, device=gnp._dev())
        gr = torch.empty(len(th), dtype=torch.float64, device=gnp._dev())
        _lib.check(lib.gpmp_nll_grad(*self._args(th), gnp._ptr(ws), gnp._ptr(val), gnp._ptr(gr), gnp._ptr(self.info), gnp._stream()),
                   "gpmp_nll_grad")
        return float(val.item()), gr.cpu().numpy(), int(self.info.item())

    def reml(self, th):
        torch, gp, gnp, _lib, lib = self.env
        ws = torch.empty(int(lib.gpmp_reml_ws_elems(self.n, self.q)), dtype=torch.float64, device=gnp._dev())
        val = torch.empty(1, dtype=torch.float64, device=gnp._dev())
        _lib.check(lib.gpmp_reml(*self._args(th), gnp._ptr(ws), gnp._ptr(val), gnp._ptr(self.info), gnp._stream()), "gpmp_reml")
        return float(val.item()), int(self.info.item())

    def loo(self, th):
        torch, gp, gnp, _lib, lib = self.env
        ws = torch.empty(int(lib.gpmp_loo_ws_elems(self.n, self.q)), dtype=torch.float64, device=gnp._dev())
        out = [torch.empty(self.n, dtype=torch.float64, device=gnp._dev()) for _ in range(3)]
        _lib.check(lib.gpmp_loo(*self._args(th), gnp._ptr(ws), *(gnp._ptr(o) for o in out), gnp._ptr(self.info), gnp._stream()), "gpmp_loo")
        return [o.cpu().numpy() for o in out], int(self.info.item())

    def predict_zero(self, th, xt):
        torch, gp, gnp, _lib, lib = self.env
        m = xt.shape[0]
        XT = torch.as_tensor(xt, device=gnp._dev())
        ws = torch.empty(int(lib.gpmp_predict_ws_elems(self.n, m)), dtype=torch.float64, device=gnp._dev())
        zpm, zpv = (torch.empty(m, dtype=torch.float64, device=gnp._dev()) for _ in range(2))
        _lib.check(lib.gpmp_predict_zero_mean(gnp._ptr(self.X), gnp._ptr(self.Z), gnp._ptr(XT), self.n, m, self.d, self.p, _lib.host_vec(th),
                                              0, 1, gnp._ptr(ws), gnp._ptr(zpm), gnp._ptr(zpv), gnp._ptr(self.info), gnp._stream()),
                   "gpmp_predict_zero_mean")
        return zpm.cpu().numpy(), zpv.cpu().numpy(), int(self.info.item())

    def predict_mean(self, th, xt, Pt):
        torch, gp, gnp, _lib, lib = self.env
        m = xt.shape[0]
        XT, PT = torch.as_tensor(xt, device=gnp._dev()), torch.as_tensor(np.ascontiguousarray(Pt), device=gnp._dev())
        ws = torch.empty(int(lib.gpmp_predict_mean_ws_elems(self.n, m, self.q)), dtype=torch.float64, device=gnp._dev())
        zpm, zpv = (torch.empty(m, dtype=torch.float64, device=gnp._dev()) for _ in range(2))
        _lib.check(lib.gpmp_predict_mean(gnp._ptr(self.X), gnp._ptr(self.Z), gnp._ptr(self.P), self.q, gnp._ptr(XT), gnp._ptr(PT), self.q,
                                         self.n, m, self.d, self.q, self.p, _lib.host_vec(th), 0, 1, gnp._ptr(ws), gnp._ptr(zpm),
                                         gnp._ptr(zpv), gnp._ptr(self.info), gnp._stream()), "gpmp_predict_mean")
        return zpm.cpu().numpy(), zpv.cpu().numpy(), int(self.info.item())


@pytest.mark.parametrize("d", [65, 128, 777])
def test_fused_drivers_vs_python_criteria_and_oracle(env, d):
    torch, gp, gnp, _lib, lib = env
    from gpmp_amd.core.gradients import MLZeroMeanAnalytic, REMLAnalytic

    orc = _orc()
    n, m = 397, 45
    x, z = _xz(n, d, d)
    xt, _ = _xz(m, d, d + 1)
    th = _theta_wide(d, 0.8) + 0.05 * np.random.default_rng(d).standard_normal(d + 1)
    cov = gp.kernel.MaternCovariance(2)
    ones = np.ones((n, 1))
    for P, model, crit in ((None, gp.Model(None, cov, None, th, "zero"), MLZeroMeanAnalytic),
                           (ones, gp.Model(_const(gnp), cov, None, th), REMLAnalytic)):
        c = _Drivers(env, x, z, P, 2)
        v, gr, info = c.value_grad(th)
        pv, state = crit(model).value_and_state(th, gnp.asarray(x), gnp.asarray(z))
        pg = crit(model).gradient_from_state(state)
        assert info == 0 and abs(v - pv) < 1e-11 * abs(pv) and rel_err(gr, pg) < 1e-9, (d, P is None, rel_err(gr, pg))
        ov, og = (orc.nll_zero_mean_value_and_grad(x, z, 2, th) if P is None else orc.reml_value_and_grad(x, z, ones, 2, th))
        assert abs(v - ov) < 1e-9 * abs(ov) and rel_err(gr, og) < 1e-7, (d, rel_err(gr, og))
        rv, info = c.reml(th)
        assert info == 0 and abs(rv - ov) < 1e-9 * abs(ov)
        (zl, s2, el), info = c.loo(th)
        pz, ps, pe = (gnp.to_np(a) for a in model.loo(x, z))
        assert info == 0 and rel_err(zl, pz) < 1e-9 and rel_err(s2, ps) < 1e-9 and rel_err(el, pe) < 1e-9
    ozm, ozv = orc.predict(orc.OracleModel(None, lambda a, b, t, pairwise=False: orc.maternp_covariance(a, b, 2, t, pairwise), None, th, "zero"), x, z, xt)
    zpm, zpv, info = _Drivers(env, x, z, None, 2).predict_zero(th, xt)
    assert info == 0 and rel_err(zpm, ozm) < 1e-10 and rel_err(zpv, ozv) < 1e-8
    lin = np.hstack((np.ones((n, 1)), x[:, :3]))
    lint = np.hstack((np.ones((m, 1)), xt[:, :3]))
    om = orc.OracleModel(lambda a, prm: np.hstack((np.ones((a.shape[0], 1)), a[:, :3])),
                         lambda a, b, t, pairwise=False: orc.maternp_covariance(a, b, 2, t, pairwise), None, th, "linear_predictor")
    ozm, ozv = orc.predict(om, x, z, xt)
    zpm, zpv, info = _Drivers(env, x, z, lin, 2).predict_mean(th, xt, lint)
    assert info == 0 and rel_err(zpm, ozm) < 1e-10 and rel_err(zpv, ozv) < 1e-8


def test_grad_trace_cross_and_gram_deriv(env):
    """gpmp_matern_grad_trace_cross (the block-cyclic path's per-tile call) and gpmp_matern_gram_deriv (Fisher information) at
    d > 64 against NumPy restatements of the oracle's formulas."""
    torch, gp, gnp, _lib, lib = env
    orc = _orc()
    dev = gnp._dev()
    n, m, d, p, r = 203, 131, 150, 2, 3
    rng = np.random.default_rng(5)
    x, y = rng.random((n, d)), rng.random((m, d))
    M = rng.standard_normal((n, m))
    F, G = rng.standard_normal((n, r)), rng.standard_normal((m, r))
    th = _theta_wide(d, 1.3)
    sigma2, invrho = math.exp(th[0]), np.exp(th[1:])
    xs, ys = x * invrho, y * invrho
    H = orc._sp_cdist(xs, ys)
    Me = M - F @ G.T
    ref = np.empty(1 + d)
    ref[0] = sigma2 * np.sum(Me * orc.maternp_kernel(p, H))
    R = sigma2 * orc.maternp_dkernel_over_h(p, H) * Me
    for j in range(d):
        ref[1 + j] = np.sum(R * (xs[:, j][:, None] - ys[:, j][None, :]) ** 2)
    Md = torch.as_tensor(M, device=dev)
    Xd, Yd = torch.as_tensor(x, device=dev), torch.as_tensor(y, device=dev)
    Fd, Gd = torch.as_tensor(F, device=dev), torch.as_tensor(G, device=dev)
    out = torch.zeros(1 + d, dtype=torch.float64, device=dev)
    ws = torch.empty(int(lib.gpmp_grad_ws_elems(n, d)), dtype=torch.float64, device=dev)
    _lib.check(lib.gpmp_matern_grad_trace_cross(gnp._ptr(Md), m, gnp._ptr(Xd), n, gnp._ptr(Yd), m, d, p, _lib.host_vec(th), 0,
                                                gnp._ptr(Fd), gnp._ptr(Gd), r, r, gnp._ptr(out), gnp._ptr(ws), gnp._stream()),
               "gpmp_matern_grad_trace_cross")
    assert rel_err(out.cpu().numpy(), ref) < 1e-11
    # derivative matrices
    xk = x[:97]
    Hk = orc.scaled_distance(th[1:], xk, xk)
    K = sigma2 * orc.maternp_kernel(p, Hk)
    dkh = sigma2 * orc.maternp_dkernel_over_h(p, Hk)
    Xk = torch.as_tensor(xk, device=dev)
    for j in (0, 1, 77, d):
        D = gnp.alloc_matrix(97, 97)
        _lib.check(lib.gpmp_matern_gram_deriv(gnp._ptr(Xk), 97, d, p, _lib.host_vec(th), 0, j, gnp._ptr(D), gnp._ld(D), gnp._stream()),
                   "gpmp_matern_gram_deriv")
        if j == 0:
            want = K + 10.0 * sigma2 * np.finfo(float).eps * np.eye(97)
        else:
            c = xk[:, j - 1] * invrho[j - 1]
            want = dkh * (c[:, None] - c[None, :]) ** 2
        assert rel_err(gnp.to_np(D), want) < 1e-12, j
    fi = gnp.to_np(gp.Model(None, gp.kernel.MaternCovariance(p), None, th, "zero").fisher_information(xk))
    assert fi.shape == (d + 1, d + 1) and np.all(np.isfinite(fi)) and np.allclose(fi, fi.T, rtol=1e-10)


def test_batched_criterion_falls_back_above_64(env):
    """The batched small-problem driver keeps d <= 64; evaluate_many at d > 64 takes the one-problem-at-a-time route."""
    torch, gp, gnp, _lib, lib = env
    x, z = _xz(150, 90, 2)
    th = _theta_wide(90)
    model = gp.Model(None, gp.kernel.MaternCovariance(2), None, None, "zero")
    _, pre, _, grad = gp.kernel.make_selection_criterion_with_gradient(model, gp.kernel.negative_log_likelihood_zero_mean, x, z)
    P = th + 0.1 * np.random.default_rng(1).standard_normal((3, th.size))
    vals, grads = pre.__self__.evaluate_many(P, want_grad=True)
    for c in range(3):
        assert abs(vals[c] - pre(P[c])) < 1e-11 * abs(vals[c]) and rel_err(grads[c], grad(P[c])) < 1e-10


def test_predict_and_reml_selection_end_to_end_n2000_d300(env):
    torch, gp, gnp, _lib, lib = env
    n, d = 2000, 300
    x, z = _xz(n, d, 2000)
    xt, _ = _xz(300, d, 2001)
    model = gp.Model(_const(gnp), gp.kernel.MaternCovariance(2), None, None)
    th0 = _theta_wide(d)
    model, info = gp.kernel.select_parameters_with_reml(model, x, z, covparam0=th0, info=True, method_options={"maxiter": 15})
    th = gnp.to_np(model.covparam)
    crit0 = float(model.negative_log_restricted_likelihood(th0, x, z))
    crit1 = float(model.negative_log_restricted_likelihood(th, x, z))
    assert np.all(np.isfinite(th)) and crit1 <= crit0
    zpm, zpv = (gnp.to_np(a) for a in model.predict(x, z, xt))
    assert zpm.shape == (300,) and np.all(np.isfinite(zpm)) and np.all(zpv >= 0)
    # accuracy at the starting point: the selected parameters give a K with rcond ~ 1e-17 (long length scales on 2000 points),
    # where any two Cholesky-based predictors differ at the 1e-7 level whatever builds K
    orc = _orc()
    om = orc.OracleModel(lambda a, prm: np.ones((a.shape[0], 1)), lambda a, b, t, pairwise=False: orc.maternp_covariance(a, b, 2, t, pairwise),
                         None, th0, "linear_predictor")
    ozm, ozv = orc.predict(om, x, z, xt)
    m0 = gp.Model(_const(gnp), gp.kernel.MaternCovariance(2), None, th0)
    zpm0, zpv0 = (gnp.to_np(a) for a in m0.predict(x, z, xt))
    assert rel_err(zpm0, ozm) < 1e-10 and rel_err(zpv0, ozv) < 1e-8, (rel_err(zpm0, ozm), rel_err(zpv0, ozv))
    paths = gnp.to_np(model.sample_paths(gnp.asarray(xt[:50]), 4))
    assert np.all(np.isfinite(paths))
