"""Model.posterior_means / PosteriorMeans, conditional_sample_paths_from_data and the C entry points gpmp_posterior_weights_multi /
gpmp_posterior_mean_multi on the GPU, against the library's own Gram matrix and the NumPy restatement (posterior_mean_numpy.py).

Tile extents of csrc/posterior_mean_multi.hip this file relies on: a matrix instruction takes 4 observation points, 16 run in lock
step, 32 make an LDS chunk, a slice has at least 128 (n = 1000 at m <= 64, s <= 64: 8 slices of 128 rows, the last of 104 = three
chunks and a short one); a wave owns 16 prediction points, a workgroup 64; a column tile is 16 wide, a lane keeps 1 to 4 of them
(s <= 16, <= 32, <= 48, more) and a workgroup 64 columns."""
import numpy as np
import pytest

from . import posterior_mean_numpy as pmn
from . import predict_grad_numpy as pgn
from .test_posterior_mean_gpu import _c_weights, _dev, _model, _problem, env  # noqa: F401

pytestmark = pytest.mark.gpu
NS = (1, 3, 4, 5, 15, 16, 17, 31, 32, 33, 127, 129, 1000)
MS = (1, 15, 16, 17, 63, 64, 65, 130)
SS = (1, 15, 16, 17, 32, 33, 48, 49, 64, 65, 130)


def _c_weights_multi(env, xi, Z, p, theta, noise, Pi=None):
    """gpmp_posterior_weights_multi through ctypes: (A, B) on the device, info."""
    _, gnp, _lib, torch = env
    lib = _lib.load()
    (n, d), s, q = xi.shape, Z.shape[1], 0 if Pi is None else Pi.shape[1]
    X, ZD, PI = _dev(env, xi), _dev(env, Z), _dev(env, Pi)
    A = torch.empty((n, s), dtype=torch.float64, device="cuda")
    B = torch.empty((q, s), dtype=torch.float64, device="cuda") if q else None
    info = torch.zeros(1, dtype=torch.int32, device="cuda")
    ws = torch.empty(int(lib.gpmp_posterior_weights_multi_ws_elems(n, s, q)), dtype=torch.float64, device="cuda")
    _lib.check(lib.gpmp_posterior_weights_multi(gnp._ptr(X), gnp._ptr(ZD), s, gnp._ptr(PI), q, n, s, d, q, p, _lib.host_vec(theta), noise,
                                                gnp._ptr(ws), gnp._ptr(A), s, gnp._ptr(B), s, gnp._ptr(info), gnp._stream()),
               "gpmp_posterior_weights_multi")
    return A, B, int(info.item())


def _c_mean_multi(env, X, A, XT, s, p, theta, noise, Pt=None, B=None, O=None):
    """gpmp_posterior_mean_multi through ctypes on device tensors (leading dimensions = row strides); returns O (m x s view)."""
    _, gnp, _lib, torch = env
    lib = _lib.load()
    (n, d), m, q = X.shape, XT.shape[0], 0 if B is None else B.shape[0]
    if O is None:
        O = torch.empty((m, s), dtype=torch.float64, device="cuda")
    ws = torch.empty(int(lib.gpmp_posterior_mean_multi_ws_elems(n, m, s, d)), dtype=torch.float64, device="cuda")
    _lib.check(lib.gpmp_posterior_mean_multi(gnp._ptr(X), gnp._ptr(A), A.stride(0), gnp._ptr(XT), gnp._ptr(Pt), Pt.stride(0) if q else 0,
                                             gnp._ptr(B), B.stride(0) if q else 0, n, m, s, d, q, p, _lib.host_vec(theta), noise,
                                             gnp._ptr(ws), gnp._ptr(O), O.stride(0), gnp._stream()), "gpmp_posterior_mean_multi")
    return O[:, :s]


@pytest.mark.parametrize("d", [1, 3, 64])
def test_values_equal_the_gram_matrix_times_the_weights(env, d):
    """gpmp_posterior_mean_multi (q = 0) against G^T A with G = gpmp_matern_gram(xi, xt), in fp64 by torch.  Every entry of the pass is
    the entry the Gram kernel writes, so both sides sum the same n products: each is within n 2^-53 sum_i |G_it A_ic| of the exact sum,
    the bound is their sum with a factor 2 of margin.  d = 3, p = 2 runs NS x MS x SS (every tile extent - 1, + 0, + 1), every other
    (d, p, noise) a subset with a short last group, chunk, slice, point tile and column tile."""
    from gpmp_amd.kernel import MaternCovariance

    rng = np.random.default_rng(60 + d)
    XI, XT, AL = _dev(env, rng.random((1000, d))), _dev(env, rng.random((130, d))), _dev(env, rng.standard_normal((1000, 130)))
    for noise in (0, 1):
        th = np.insert(_problem(1, 1, d, 0)[3], 1, [-1.0] * noise)
        for p in (0, 2, 16):
            full = d == 3 and p == 2 and noise == 0
            for n in NS if full else (5, 33, 1000):
                for m in MS if full else (17, 130):
                    G = MaternCovariance(p, noise=bool(noise))(XI[:n], XT[:m], th)      # gpmp_matern_gram(xi, xt)
                    for s in SS if full else (17, 65):
                        A = AL[:n, :s].contiguous()
                        O = _c_mean_multi(env, XI[:n], A, XT[:m], s, p, th, noise)
                        bound = 4.0 * n * 2.0 ** -53 * (G.abs().t() @ A.abs())
                        assert bool(((O - G.t() @ A).abs() <= bound).all()), (noise, p, n, m, s)


@pytest.mark.parametrize("n, m, s", [(1000, 65, 17), (33, 130, 65)])
def test_leading_dimensions_and_guards(env, n, m, s):
    """lda > s with NaN behind column s of A, O (ldo > s) inside a guard-valued buffer: the bound above, the guards intact."""
    from gpmp_amd.kernel import MaternCovariance

    torch, rng = env[3], np.random.default_rng(n)
    X, XT, th = _dev(env, rng.random((n, 3))), _dev(env, rng.random((m, 3))), _problem(1, 1, 3, 0)[3]
    A = torch.full((n, s + 5), float("nan"), dtype=torch.float64, device="cuda")
    A[:, :s] = _dev(env, rng.standard_normal((n, s)))
    buf = torch.full((16 + m * (s + 3) + 16,), -7.25, dtype=torch.float64, device="cuda")
    O = _c_mean_multi(env, X, A, XT, s, 2, th, 0, O=buf[16 : 16 + m * (s + 3)].view(m, s + 3))
    G = MaternCovariance(2)(X, XT, th)
    assert bool(((O - G.t() @ A[:, :s]).abs() <= 4.0 * n * 2.0 ** -53 * (G.abs().t() @ A[:, :s].abs())).all())
    assert bool((buf[:16] == -7.25).all()) and bool((buf[-16:] == -7.25).all()) and bool((buf[16:-16].view(m, s + 3)[:, s:] == -7.25).all())


def test_far_and_coincident_points(env):
    """xt at 10^4 length scales from every observation: the covariance underflows to an exact 0 and what is left is Pt B, exact for
    dyadic designs and coefficients (padded leading dimensions, NaN behind the q and s columns).  Then xt = some xi."""
    torch, rng = env[3], np.random.default_rng(4)
    n, m, s, q, d = 200, 70, 17, 4, 3
    xi, rho = rng.random((n, d)), np.array([0.5, 0.25, 1.0])
    th = np.concatenate(([0.0], -np.log(rho)))
    A = rng.standard_normal((n, s))
    Pt = torch.full((m, q + 3), float("nan"), dtype=torch.float64, device="cuda")
    B = torch.full((q, s + 2), float("nan"), dtype=torch.float64, device="cuda")
    Pt[:, :q], B[:, :s] = _dev(env, rng.integers(-16, 17, (m, q)) / 8.0), _dev(env, rng.integers(-8, 9, (q, s)) / 4.0)
    far = _dev(env, 1.0 + 1e4 * rho * (1.0 + rng.random((m, d))))
    for p in (0, 2, 16):
        O = _c_mean_multi(env, _dev(env, xi), _dev(env, A), far, s, p, th, 0, Pt, B)
        assert np.array_equal(O.cpu().numpy(), (Pt[:, :q] @ B[:, :s]).cpu().numpy()), p
        xt = np.vstack((xi[:40], rng.random((30, d))))
        O = _c_mean_multi(env, _dev(env, xi), _dev(env, A), _dev(env, xt), s, p, th, 0).cpu().numpy()
        assert np.all(np.isfinite(O))
        pmn.close(O, pgn.cov_parts(xi, xt, p, th, 0)[0].T @ A, pmn.tolerance(xi, p, th, 0), ("coincident", p))


@pytest.mark.parametrize("n, s, q, d", [(2, 1, 0, 3), (2, 3, 1, 3), (129, 17, 0, 3), (129, 17, 4, 3), (300, 65, 4, 3), (300, 16, 4, 70)])
def test_weights_against_the_numpy_cholesky_route(env, n, s, q, d):
    xi, zi, _, th = _problem(n, 1, d, 31 * n + q)
    Z = np.cos(np.outer(zi, 1.0 + np.arange(s) / s))
    Pi = None if q == 0 else pgn.designs("const" if q == 1 else "lin", xi)[0]
    ra, rb = pmn.weights(xi, Z, 2, th, 0, Pi)
    A, B, info = _c_weights_multi(env, xi, Z, 2, th, 0, Pi)
    tol = pmn.tolerance(xi, 2, th, 0)
    assert info == 0
    pmn.close(A.cpu().numpy(), ra, tol, "A")
    if q:
        pmn.close(B.cpu().numpy(), rb, tol, "B")
    if s == 1:
        pmn.close(A.cpu().numpy()[:, 0], _c_weights(env, xi, Z[:, 0], 2, th, 0, Pi)[0].cpu().numpy(), tol, "A vs gpmp_posterior_weights")


def test_failed_factorisation(env):
    """The failing matrix of tests/test_posterior_mean_gpu.py: p = 10, 400 points on a line, a long length scale."""
    xi = np.linspace(0.0, 1.0, 400).reshape(-1, 1)
    Z, th = np.hstack((np.sin(xi), np.cos(xi))), np.array([0.0, -np.log(20.0)])
    for Pi in (None, np.ones((400, 1))):
        A, B, info = _c_weights_multi(env, xi, Z, 10, th, 0, Pi)
        assert info != 0 and np.all(np.isnan(A.cpu().numpy())) and (Pi is None or np.all(np.isnan(B.cpu().numpy())))
    with pytest.raises(np.linalg.LinAlgError, match="info ="):
        _model(env, 10, 0, th, "zero", 1).posterior_means(xi, Z)


@pytest.mark.parametrize("kind", ["zero", "lin", "param"])
def test_object_and_conditional_paths(env, kind):
    gp, gnp, _, torch = env
    n, m, s, d = 300, 130, 17, 4
    xi, zi, xt, th = _problem(n, m, d, 9)
    Z = np.cos(np.outer(zi, 1.0 + np.arange(s) / s))
    tol = pmn.tolerance(xi, 2, th, 0)
    mp = np.array([0.3, 1.1])
    model = _model(env, 2, 0, th.copy(), kind, d, torch.as_tensor(mp, device="cuda") if kind == "param" else None)
    prior_i, prior_t = (pgn.designs("param", x, mp)[0] if kind == "param" else 0.0 for x in (xi, xt))
    Pi, Pt = (pgn.designs("lin", x)[0] if kind == "lin" else None for x in (xi, xt))

    def ref(cols):                                                   # the NumPy restatement, column by column
        ra, rb = pmn.weights(xi, cols - np.reshape(prior_i, (-1, 1)), 2, th, 0, Pi)
        return np.stack([pmn.mean_and_gradient(xi, ra[:, c], xt, 2, th, 0, Pt, rb[:, c] if kind == "lin" else None)[0] + prior_t
                         for c in range(cols.shape[1])], axis=1)

    post = model.posterior_means(xi, Z)
    O = post(xt)
    assert isinstance(post, gp.core.PosteriorMeans) and O.shape == (m, s) and post(np.zeros((0, d))).shape == (0, s)
    pmn.close(O, ref(Z), tol, (kind, "NumPy"))
    pmn.close(O, np.stack([model.posterior_mean(xi, Z[:, c])(xt) for c in range(s)], axis=1), tol, (kind, "posterior_mean"))
    model.covparam = th + 0.5                                        # the snapshot; two evaluations give the same bits
    np.testing.assert_array_equal(post(xt), O)
    Ot = post(torch.as_tensor(xt, device="cuda"), convert_in=False, convert_out=False)
    assert isinstance(Ot, torch.Tensor) and Ot.is_cuda and np.array_equal(Ot.cpu().numpy(), O)
    model.covparam = th
    # conditional paths: ztsim_t + mean(zi - ztsim_i), and the lambda-based route
    ztsim = np.random.default_rng(3).standard_normal((n + m, 5))
    xi_ind, xt_ind = np.arange(n), n + np.arange(m)
    paths = model.conditional_sample_paths_from_data(ztsim, xi, xi_ind, zi, xt, xt_ind)
    pmn.close(paths, ztsim[n:] + ref(zi[:, None] - ztsim[:n]), tol, (kind, "paths"))
    lam = model.predict(xi, zi, xt, return_lambdas=True)[2]
    old = (model.conditional_sample_paths_parameterized_mean(ztsim, xi, xi_ind, zi, xt, xt_ind, lam) if kind == "param"
           else model.conditional_sample_paths(ztsim, xi_ind, zi, xt_ind, lam))
    pmn.close(paths, old, tol, (kind, "lambda route"))
