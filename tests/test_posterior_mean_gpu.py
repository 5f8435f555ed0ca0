"""Model.posterior_mean / PosteriorMean and the C entry points gpmp_posterior_weights / gpmp_posterior_mean on the GPU: the reference's
outputs (tests/golden/ref_predict_grad.npz), Model.predict / Model.predict_gradient, the library's own Gram matrix, the NumPy
restatement (tests/posterior_mean_numpy.py), tiling and slicing seams, strides and guard values, coincident and far points, a
failed factorisation, the object's semantics and the example.

Slice constants of csrc/posterior_mean.hip this file relies on: a wave owns 64 prediction points (PM_TM) and at least 64
observation points (PM_MIN_ROWS), it visits them 4 at a time (PM_IB), and a call is split into min(ceil(4096 / ceil(m / 64)),
ceil(n / 64)) slices: n = 1000 at m = 1 gives 16 slices of 63 rows (15 full blocks of 4 and a short one) and a last slice of 55."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from . import posterior_mean_numpy as pmn
from . import predict_grad_numpy as pgn

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "ref_predict_grad.npz")


@pytest.fixture(scope="module")
def env():
    import torch

    assert torch.cuda.is_available()
    import gpmp_amd as gp
    import gpmp_amd.num as gnp
    from gpmp_amd import _lib

    return gp, gnp, _lib, torch


def _means(gnp, kind, d):
    k = min(d, 3)
    if kind == "const":
        return lambda x, param: gnp.ones((x.shape[0], 1))
    if kind == "lin":
        return lambda x, param: gnp.hstack((gnp.ones((x.shape[0], 1)), x[:, :k]))
    if kind == "param":
        return lambda x, param: (param[0] + param[1] * x[:, 0]).reshape(-1, 1)
    return None


def _model(env, p, noise, theta, kind="zero", d=1, meanparam=None):
    gp, gnp, _, _ = env
    from gpmp_amd.kernel import MaternCovariance

    mt = {"zero": "zero", "param": "parameterized", "const": "linear_predictor", "lin": "linear_predictor"}[kind]
    return gp.Model(_means(gnp, kind, d), MaternCovariance(p, noise=bool(noise)), meanparam, theta, mt)


def _dev(env, a):
    torch = env[3]
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda")


def _c_weights(env, xi, zi, p, theta, noise, Pi=None):
    """gpmp_posterior_weights through ctypes, as a non-Python host calls it: (alpha, beta) on the device, info."""
    _, gnp, _lib, torch = env
    lib = _lib.load()
    n, d = xi.shape
    q = 0 if Pi is None else Pi.shape[1]
    X, Z, PI = _dev(env, xi), _dev(env, zi), _dev(env, Pi)
    alpha = torch.empty(n, dtype=torch.float64, device="cuda")
    beta = torch.empty(q, dtype=torch.float64, device="cuda") if q else None
    info = torch.zeros(1, dtype=torch.int32, device="cuda")
    ws = torch.empty(int(lib.gpmp_posterior_weights_ws_elems(n, q)), dtype=torch.float64, device="cuda")
    rc = lib.gpmp_posterior_weights(gnp._ptr(X), gnp._ptr(Z), gnp._ptr(PI), q, n, d, q, p, _lib.host_vec(theta), noise, gnp._ptr(ws),
                                    gnp._ptr(alpha), gnp._ptr(beta), gnp._ptr(info), gnp._stream())
    _lib.check(rc, "gpmp_posterior_weights")
    return alpha, beta, int(info.item())


def _c_mean(env, X, alpha, XT, p, theta, noise, Pt=None, ldpt=0, beta=None, J=None, gradient=True, zpm=None, gzpm=None):
    """gpmp_posterior_mean through ctypes on device tensors; returns (zpm, gzpm) tensors (gzpm None without the gradient)."""
    _, gnp, _lib, torch = env
    lib = _lib.load()
    n, d = X.shape
    m = XT.shape[0]
    q = 0 if beta is None else int(beta.shape[0])
    if zpm is None:
        zpm = torch.empty(m, dtype=torch.float64, device="cuda")
    if gradient and gzpm is None:
        gzpm = torch.empty((m, d), dtype=torch.float64, device="cuda")
    ws = torch.empty(int(lib.gpmp_posterior_mean_ws_elems(n, m, d, 1 if gradient else 0)), dtype=torch.float64, device="cuda")
    rc = lib.gpmp_posterior_mean(gnp._ptr(X), gnp._ptr(alpha), gnp._ptr(XT), gnp._ptr(Pt), ldpt, gnp._ptr(beta), gnp._ptr(J), n, m, d, q, p,
                                 _lib.host_vec(theta), noise, gnp._ptr(ws), gnp._ptr(zpm), gnp._ptr(gzpm if gradient else None), gnp._stream())
    _lib.check(rc, "gpmp_posterior_mean")
    return zpm, (gzpm if gradient else None)


# ---- 1. the reference's cases --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", range(20))
def test_fixture_case_through_the_object_and_the_c_entries(env, c):
    torch = env[3]
    g = np.load(FIXTURE)
    cs = pmn.fixture_case(g, c)
    xi, xt, zi, th, kind, p, noise, d = cs["xi"], cs["xt"], cs["zi"], cs["theta"], cs["kind"], cs["p"], cs["noise"], cs["d"]
    tol = pmn.tolerance(xi, p, th, noise)
    mp = cs.get("meanparam")
    model = _model(env, p, noise, th, kind, d, None if mp is None else torch.as_tensor(mp, dtype=torch.float64, device="cuda"))
    post = model.posterior_mean(xi, zi)
    zpm, gm = post.mean_and_gradient(xt)
    pmn.close(zpm, cs["zpm"], tol, ("object", "zpm"))
    pmn.close(gm, cs["gzpm"], tol, ("object", "gzpm"))
    pmn.close(post(xt), cs["zpm"], tol, ("object, value only", "zpm"))
    pz, _ = model.predict(xi, zi, xt)
    gz, _, gg, _ = model.predict_gradient(xi, zi, xt, variance=False)
    pmn.close(zpm, pz, tol, "zpm vs predict")
    pmn.close(zpm, gz, tol, "zpm vs predict_gradient")
    pmn.close(gm, gg, tol, "gzpm vs predict_gradient")
    if d > 64:
        return
    # as a non-Python host: weights, then the matrix-free pass (a parameterized mean is centred by the host: q = 0)
    alpha, beta, info = _c_weights(env, xi, cs["zc"], p, th, noise, cs["Pi"])
    assert info == 0
    q = 0 if cs["Pi"] is None else cs["Pi"].shape[1]
    a, b = _c_mean(env, _dev(env, xi), alpha, _dev(env, xt), p, th, noise, _dev(env, cs["Pt"]), q, beta, _dev(env, cs["J"]))
    pmn.close(a.cpu().numpy() + cs["prior"], cs["zpm"], tol, ("gpmp_posterior_mean", "zpm"))
    pmn.close(b.cpu().numpy() + cs["prior_grad"], cs["gzpm"], tol, ("gpmp_posterior_mean", "gzpm"))


# ---- 2. the kernel against the library's own Gram matrix -----------------------------------------------------------------

NS = (1, 63, 64, 65, 129, 1000)
MS = (1, 63, 64, 65, 130)


@pytest.mark.parametrize("d", [1, 3, 64])
def test_value_equals_the_gram_matrix_times_alpha(env, d):
    """gpmp_posterior_mean (q = 0) against G^T alpha with G = gpmp_matern_gram(xi, xt), in fp64 by torch.  Every entry of the pass is
    the entry the Gram kernel writes, so both sides are sums of the same n terms in different orders: each is within
    n 2^-53 sum_i |G_it alpha_i| of the exact sum, the bound is their sum with a factor 2 of margin."""
    _, gnp, _lib, torch = env
    lib = _lib.load()
    rng = np.random.default_rng(50 + d)
    XI, XT = _dev(env, rng.random((max(NS), d))), _dev(env, rng.random((max(MS), d)))
    AL = _dev(env, rng.standard_normal(max(NS)))
    rho = 0.4 * np.sqrt(d) * (1.0 + np.arange(d) / d)
    worst = 0.0
    for noise in (0, 1):
        th = np.concatenate(([0.3], [-1.0] if noise else [], -np.log(rho)))
        for p in (0, 1, 4, 5, 16):
            for n in NS:
                for m in MS:
                    X, Y, al = XI[:n], XT[:m], AL[:n]
                    G = torch.empty((n, m), dtype=torch.float64, device="cuda")
                    _lib.check(lib.gpmp_matern_gram(gnp._ptr(X), gnp._ptr(Y), n, m, d, p, _lib.host_vec(th), noise, 0.0, 0, gnp._ptr(G), m,
                                                    gnp._stream()), "gpmp_matern_gram")
                    ref = G.t() @ al
                    bound = 4.0 * n * 2.0 ** -53 * (G.abs().t() @ al.abs())
                    v0, _ = _c_mean(env, X, al, Y, p, th, noise, gradient=False)
                    v1, g1 = _c_mean(env, X, al, Y, p, th, noise, gradient=True)
                    for v in (v0, v1):
                        ratio = float(((v - ref).abs() / bound).max())
                        worst = max(worst, ratio)
                        assert ratio <= 1.0, (noise, p, n, m, ratio)
                    assert bool(torch.isfinite(g1).all())
    print(f"d={d}: worst |zpm - G^T alpha| / bound = {worst:.3f}")


# ---- 3. mean part and strides ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("q, d", [(1, 3), (4, 3), (4, 17)])
def test_mean_part_strides_and_guards(env, q, d):
    torch = env[3]
    n, m, p, ldpt, pad = 130, 67, 2, q + 3, 16
    rng = np.random.default_rng(7 * q + d)
    xi, xt = rng.random((n, d)), rng.random((m, d))
    th = np.concatenate(([0.2], -np.log(0.4 * np.sqrt(d) * (1.0 + np.arange(d) / d))))
    alpha, beta = rng.standard_normal(n), rng.standard_normal(q)
    Pt, J = rng.standard_normal((m, q)), rng.standard_normal((m, q, d))
    ref_v, ref_g = pmn.mean_and_gradient(xi, alpha, xt, p, th, 0, Pt, beta, J)
    tol = pmn.tolerance(xi, p, th, 0)
    PT = torch.full((m, ldpt), float("nan"), dtype=torch.float64, device="cuda")      # what lies behind the q columns is never read
    PT[:, :q] = _dev(env, Pt)
    vbuf = torch.full((m + 2 * pad,), -7.25, dtype=torch.float64, device="cuda")
    gbuf = torch.full((m * d + 2 * pad,), -7.25, dtype=torch.float64, device="cuda")
    for gradient in (True, False):
        vbuf.fill_(-7.25)
        gbuf.fill_(-7.25)
        _c_mean(env, _dev(env, xi), _dev(env, alpha), _dev(env, xt), p, th, 0, PT, ldpt, _dev(env, beta), _dev(env, J), gradient=gradient,
                zpm=vbuf[pad : pad + m], gzpm=gbuf[pad : pad + m * d])
        v, gr = vbuf.cpu().numpy(), gbuf.cpu().numpy()
        assert np.all(v[:pad] == -7.25) and np.all(v[pad + m :] == -7.25)
        pmn.close(v[pad : pad + m], ref_v, tol, ("zpm", gradient))
        if gradient:
            assert np.all(gr[:pad] == -7.25) and np.all(gr[pad + m * d :] == -7.25)
            pmn.close(gr[pad : pad + m * d].reshape(m, d), ref_g, tol, "gzpm")
        else:
            assert np.all(gr == -7.25)               # a value-only call never touches a gradient buffer


# ---- 4. special points -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("p", [0, 1, 3])
def test_coincident_points(env, p):
    n, d = 70, 3
    rng = np.random.default_rng(p)
    xi = rng.random((n, d))
    xt = np.vstack((xi[:40], rng.random((30, d))))
    th = np.concatenate(([0.1], -np.log([0.5, 0.7, 0.9])))
    alpha = rng.standard_normal(n)
    ref_v, ref_g = pmn.mean_and_gradient(xi, alpha, xt, p, th, 0)
    v, g = _c_mean(env, _dev(env, xi), _dev(env, alpha), _dev(env, xt), p, th, 0)
    v, g = v.cpu().numpy(), g.cpu().numpy()
    assert np.all(np.isfinite(v)) and np.all(np.isfinite(g))
    tol = pmn.tolerance(xi, p, th, 0)
    pmn.close(v, ref_v, tol, "zpm")
    pmn.close(g, ref_g, tol, "gzpm")
    # one observation, evaluated at itself: the value is alpha sigma^2 K_p(0) = alpha sigma^2, the pair contributes no gradient
    s2 = float(np.exp(th[0]))
    v, g = _c_mean(env, _dev(env, xi[:1]), _dev(env, np.array([1.5])), _dev(env, xi[:1]), p, th, 0)
    assert float(v[0]) == 1.5 * s2 and np.all(g.cpu().numpy() == 0.0)


@pytest.mark.parametrize("q", [0, 4])
def test_far_points(env, q):
    """xt at 10^4 length scales from every observation: the covariance underflows to an exact 0, what is left is the mean part alone
    (dyadic designs and coefficients: every product and sum below is exact in fp64, whatever its order)."""
    n, m, d = 200, 70, 3
    rng = np.random.default_rng(q)
    xi = rng.random((n, d))
    rho = np.array([0.5, 0.25, 1.0])
    xt = 1.0 + 1e4 * rho * (1.0 + rng.random((m, d)))
    th = np.concatenate(([0.0], -np.log(rho)))
    alpha = rng.standard_normal(n)
    beta = Pt = J = None
    ref_v, ref_g = np.zeros(m), np.zeros((m, d))
    if q:
        beta = rng.integers(-8, 9, q) / 4.0
        Pt = rng.integers(-16, 17, (m, q)) / 8.0
        J = rng.integers(-16, 17, (m, q, d)) / 8.0
        ref_v, ref_g = Pt @ beta, np.einsum("a,taj->tj", beta, J)
    for p in (0, 2, 16):
        v, g = _c_mean(env, _dev(env, xi), _dev(env, alpha), _dev(env, xt), p, th, 0, _dev(env, Pt), q, _dev(env, beta), _dev(env, J))
        v, g = v.cpu().numpy(), g.cpu().numpy()
        assert np.all(np.isfinite(v)) and np.all(np.isfinite(g))
        assert np.array_equal(v, ref_v) and np.array_equal(g, ref_g), p


# ---- 5. the weights driver -------------------------------------------------------------------------------------------------

def _problem(n, m, d, seed):
    rng = np.random.default_rng(seed)
    xi, xt = rng.random((n, d)), rng.random((m, d))
    zi = np.sin(2 * np.pi * xi[:, 0]) + xi[:, 1:].sum(axis=1) / np.sqrt(d)
    theta = np.concatenate(([0.2], -np.log(0.4 * np.sqrt(d) * (1.0 + np.arange(d) / d))))
    return xi, zi, xt, theta


def _design(q, x):
    return None if q == 0 else pgn.designs("const" if q == 1 else "lin", x)[0]


@pytest.mark.parametrize("n, q, d", [(2, 0, 3), (2, 1, 3), (129, 0, 3), (129, 1, 3), (129, 4, 3), (300, 0, 3), (300, 1, 3), (300, 4, 3),
                                     (300, 4, 70)])
def test_weights_against_the_numpy_cholesky_route(env, n, q, d):
    xi, zi, _, th = _problem(n, 1, d, 31 * n + q)
    Pi = _design(q, xi)
    ra, rb = pmn.weights(xi, zi, 2, th, 0, Pi)
    alpha, beta, info = _c_weights(env, xi, zi, 2, th, 0, Pi)
    assert info == 0
    tol = pmn.tolerance(xi, 2, th, 0)
    pmn.close(alpha.cpu().numpy(), ra, tol, "alpha")
    if q:
        pmn.close(beta.cpu().numpy(), rb, tol, "beta")


def test_more_mean_columns_than_observations_is_an_argument_error(env):
    _, gnp, _lib, torch = env
    xi, zi, _, th = _problem(2, 1, 3, 1)
    with pytest.raises(_lib.GpmpHipError, match="argument 5"):
        _c_weights(env, xi, zi, 2, th, 0, pgn.designs("lin", xi)[0])


def test_failed_factorisation(env):
    """The failing matrix of tests/test_predict_grad_gpu.py: p = 10, 400 points on a line, a long length scale."""
    xi = np.linspace(0.0, 1.0, 400).reshape(-1, 1)
    zi = np.sin(xi[:, 0])
    th = np.array([0.0, -np.log(20.0)])
    alpha, _, info = _c_weights(env, xi, zi, 10, th, 0)
    assert info != 0
    assert np.all(np.isnan(alpha.cpu().numpy()))
    alpha, beta, info = _c_weights(env, xi, zi, 10, th, 0, np.ones((400, 1)))
    assert info != 0
    assert np.all(np.isnan(alpha.cpu().numpy())) and np.all(np.isnan(beta.cpu().numpy()))
    with pytest.raises(np.linalg.LinAlgError, match="info ="):
        _model(env, 10, 0, th, "zero", 1).posterior_mean(xi, zi)


# ---- 6. the object ---------------------------------------------------------------------------------------------------------

def test_object_semantics(env):
    gp, gnp, _, torch = env
    xi, zi, xt, th = _problem(500, 700, 4, 5)
    tol = pmn.tolerance(xi, 2, th, 0)
    for kind in ("zero", "lin", "param"):
        mp = torch.tensor([0.3, 1.1], dtype=torch.float64, device="cuda") if kind == "param" else None
        model = _model(env, 2, 0, th.copy(), kind, 4, mp)
        post = model.posterior_mean(xi, zi)
        assert isinstance(post, gp.core.PosteriorMean) and (post.n, post.d) == (500, 4)
        before = []
        for m in (1, 65, 700):                                       # three batches of different sizes from one object
            v, g = post.mean_and_gradient(xt[:m])
            rv, _, rg, _ = model.predict_gradient(xi, zi, xt[:m], variance=False)
            pmn.close(v, rv, tol, (kind, m, "zpm"))
            pmn.close(g, rg, tol, (kind, m, "gzpm"))
            assert v.shape == (m,) and g.shape == (m, 4)
            before.append((v, g))
        # the snapshot: new parameters on the model do not reach the object; two evaluations give the same bits
        model.covparam = th + 0.5
        if kind == "param":
            model.meanparam = torch.tensor([5.0, -2.0], dtype=torch.float64, device="cuda")
        for m, (v, g) in zip((1, 65, 700), before):
            v2, g2 = post.mean_and_gradient(xt[:m])
            np.testing.assert_array_equal(v2, v)
            np.testing.assert_array_equal(g2, g)
            np.testing.assert_array_equal(post(xt[:m]), v)
        # device in, device out
        vt = post(torch.as_tensor(xt, device="cuda"), convert_in=False, convert_out=False)
        assert isinstance(vt, torch.Tensor) and vt.is_cuda
        np.testing.assert_array_equal(vt.cpu().numpy(), before[2][0])
        # no points
        v, g = post.mean_and_gradient(np.zeros((0, 4)))
        assert v.shape == (0,) and g.shape == (0, 4) and post(np.zeros((0, 4))).shape == (0,)


def test_explicit_mean_jacobian(env):
    torch = env[3]
    xi, zi, xt, th = _problem(300, 40, 6, 12)
    model = _model(env, 1, 0, th, "lin", 6)
    post = model.posterior_mean(xi, zi)

    def jac(x, param):
        J = torch.zeros((x.shape[0], 4, 6), dtype=torch.float64, device="cuda")
        for k in range(3):
            J[:, 1 + k, k] = 1.0
        return J

    a = post.mean_and_gradient(xt)
    b = post.mean_and_gradient(xt, mean_gradient=jac)
    np.testing.assert_array_equal(a[1], b[1])


def test_other_covariances_are_not_implemented(env):
    gp = env[0]
    model = gp.Model(None, lambda x, y, c, pairwise=False: None, None, np.zeros(2), "zero")
    with pytest.raises(NotImplementedError, match="gnp.grad"):
        model.posterior_mean(np.zeros((3, 1)), np.zeros(3))


# ---- 7. the example --------------------------------------------------------------------------------------------------------

def test_posterior_mean_example_runs():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "example_posterior_mean.py")], capture_output=True, text=True,
                       timeout=300, cwd=ROOT, env=dict(os.environ, MPLBACKEND="Agg"))
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert "posterior mean check" in r.stdout
