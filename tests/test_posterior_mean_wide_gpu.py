"""gpmp_posterior_mean_wide and the objects that reach it at d > 64, on the GPU.  Extents of csrc/posterior_mean_wide.hip relied on:
x_t passes through registers 8 dimensions at a time, the observation points through LDS 32 at a time; a chunk has 64 observation
points, a slice at least 256 (n = 257 at small m: slices of 192 and 65 rows); a wave owns 32 prediction points, a workgroup 128;
a column tile is 16 wide, a lane keeps 1 to 4 of them and a workgroup 64 columns."""
import numpy as np
import pytest

from . import posterior_mean_numpy as pmn
from . import predict_grad_numpy as pgn
from .test_posterior_mean_gpu import _dev, _model, _problem, env  # noqa: F401
from .test_posterior_mean_multi_gpu import _c_mean_multi

pytestmark = pytest.mark.gpu
U = 2.0 ** -53
BASE = dict(d=70, n=130, m=65, s=17, p=2, q=0)
SWEEPS = dict(d=(1, 7, 8, 9, 64, 65, 96, 97), n=(1, 63, 64, 65, 255, 256, 257, 1000), m=(1, 63, 64, 65, 128, 130), s=(1, 16, 17, 65),
              p=(0, 2, 16), q=(0, 3))


def _c_mean_wide(env, X, A, XT, s, p, theta, noise=0, Pt=None, B=None, O=None):
    """gpmp_posterior_mean_wide through ctypes on device tensors (leading dimensions = row strides); returns O (m x s view)."""
    _, gnp, _lib, torch = env
    lib = _lib.load()
    (n, d), m, q = X.shape, XT.shape[0], 0 if B is None else B.shape[0]
    if O is None:
        O = torch.empty((m, s), dtype=torch.float64, device="cuda")
    ws = torch.empty(int(lib.gpmp_posterior_mean_wide_ws_elems(n, m, s, d)), dtype=torch.float64, device="cuda")
    _lib.check(lib.gpmp_posterior_mean_wide(gnp._ptr(X), gnp._ptr(A), A.stride(0), gnp._ptr(XT), gnp._ptr(Pt), Pt.stride(0) if q else 0,
                                            gnp._ptr(B), B.stride(0) if q else 0, n, m, s, d, q, p, _lib.host_vec(theta), noise,
                                            gnp._ptr(ws), gnp._ptr(O), O.stride(0), gnp._stream()), "gpmp_posterior_mean_wide")
    return O[:, :s]


@pytest.fixture(scope="module")
def data(env):
    rng = np.random.default_rng(77)
    return {k: _dev(env, v) for k, v in dict(xi=rng.random((1000, 97)), xt=rng.random((130, 97)), A=rng.standard_normal((1000, 65)),
                                             Pt=rng.standard_normal((130, 3)), B=rng.standard_normal((3, 65))).items()}


@pytest.mark.parametrize("axis", list(SWEEPS))
def test_values_equal_the_gram_matrix_times_the_weights(env, data, axis):
    """O against G^T A (+ Pt B), G = gpmp_matern_gram(xi, xt), the product in fp64 by torch: both sides sum the same n terms in different
    orders, each within n 2^-53 sum_i |G_it A_ic| of the exact sum (likewise the q mean terms).  One axis at a time; same bits twice."""
    from gpmp_amd.kernel import MaternCovariance

    worst = 0.0
    for v in SWEEPS[axis]:
        c = dict(BASE, **{axis: v})
        d, n, m, s, p, q = (c[k] for k in ("d", "n", "m", "s", "p", "q"))
        th = _problem(1, 1, d, 0)[3]
        X, XT, A = data["xi"][:n, :d].contiguous(), data["xt"][:m, :d].contiguous(), data["A"][:n, :s].contiguous()
        Pt, B = (data["Pt"][:m, :q].contiguous(), data["B"][:q, :s].contiguous()) if q else (None, None)
        G = MaternCovariance(p)(X, XT, th)                             # gpmp_matern_gram(xi, xt)
        ref, bound = G.t() @ A, 2.0 * n * U * (G.abs().t() @ A.abs())
        if q:
            ref, bound = ref + Pt @ B, bound + 2.0 * q * U * (Pt.abs() @ B.abs())
        O = _c_mean_wide(env, X, A, XT, s, p, th, 0, Pt, B).clone()
        ratio = float(((O - ref).abs() / bound).max())
        worst = max(worst, ratio)
        assert ratio <= 1.0, (axis, v, ratio)
        assert bool((_c_mean_wide(env, X, A, XT, s, p, th, 0, Pt, B) == O).all()), (axis, v)
    print(f"{axis}: worst |O - G^T A| / bound = {worst:.3f}")


def test_leading_dimensions_and_guards(env, data):
    """lda, ldb, ldpt > s, q with NaN behind the columns, O (ldo > s) inside a guard-valued buffer with a guard row after row m - 1."""
    from gpmp_amd.kernel import MaternCovariance

    torch = env[3]
    n, m, s, d, q = 257, 130, 17, 70, 3
    X, XT, th = data["xi"][:n, :d].contiguous(), data["xt"][:m, :d].contiguous(), _problem(1, 1, d, 0)[3]
    A, B, Pt = (torch.full(sh, float("nan"), dtype=torch.float64, device="cuda") for sh in ((n, s + 5), (q, s + 2), (m, q + 3)))
    A[:, :s], B[:, :s], Pt[:, :q] = data["A"][:n, :s], data["B"][:q, :s], data["Pt"][:m, :q]
    buf = torch.full(((m + 1) * (s + 3),), -7.25, dtype=torch.float64, device="cuda").view(m + 1, s + 3)
    O = _c_mean_wide(env, X, A, XT, s, 2, th, 0, Pt, B, O=buf[:m])
    G = MaternCovariance(2)(X, XT, th)
    bound = 2.0 * n * U * (G.abs().t() @ A[:, :s].abs()) + 2.0 * q * U * (Pt[:, :q].abs() @ B[:, :s].abs())
    assert bool(((O - (G.t() @ A[:, :s] + Pt[:, :q] @ B[:, :s])).abs() <= bound).all())
    assert bool((buf[:m, s:] == -7.25).all()) and bool((buf[m] == -7.25).all())


def test_zero_padded_points_give_the_result_of_the_register_tier_kernel(env, data):
    """d = 64 through gpmp_posterior_mean_multi; the same points padded with zero coordinates to d = 80 (arbitrary length scales on
    the padded dimensions) through gpmp_posterior_mean_wide: the same entries, summed in another order."""
    from gpmp_amd.kernel import MaternCovariance

    torch = env[3]
    n, m, s, d = 1000, 130, 17, 64
    X, XT, A, th = data["xi"][:n, :d].contiguous(), data["xt"][:m, :d].contiguous(), data["A"][:n, :s].contiguous(), _problem(1, 1, d, 0)[3]
    pad = lambda x: torch.cat((x, torch.zeros((x.shape[0], 16), dtype=torch.float64, device="cuda")), dim=1).contiguous()  # noqa: E731
    th80 = np.concatenate((th, np.linspace(-3.0, 2.0, 16)))
    G = MaternCovariance(2)(X, XT, th)
    diff = (_c_mean_wide(env, pad(X), A, pad(XT), s, 2, th80) - _c_mean_multi(env, X, A, XT, s, 2, th, 0)).abs()
    assert bool((diff <= 2.0 * n * U * (G.abs().t() @ A.abs())).all()), float(diff.max())


@pytest.mark.parametrize("kind", ["zero", "lin", "param"])
def test_objects_and_conditional_paths_at_d_70(env, kind, monkeypatch):
    gp, _, _, torch = env
    from gpmp_amd.core import fused

    n, m, s, d = 300, 130, 5, 70
    xi, zi, xt, th = _problem(n, m, d, 11)
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

    called, real = [], fused.call_driver
    monkeypatch.setattr(fused, "call_driver", lambda name, *a, **k: (called.append(name), real(name, *a, **k))[1])
    post, posts = model.posterior_mean(xi, zi), model.posterior_means(xi, Z)
    del called[:]
    pmn.close(post(xt), ref(zi[:, None])[:, 0], tol, (kind, "posterior_mean"))
    pmn.close(posts(xt), ref(Z), tol, (kind, "posterior_means"))
    assert called == ["gpmp_posterior_mean_wide"] * 2, called
    pmn.close(posts.mean_and_gradient(xt)[0], ref(Z), tol, (kind, "value of mean_and_gradient"))
    Z17 = np.cos(np.outer(zi, 1.0 + np.arange(17) / 17))               # more columns than the kernel serves: the chunked Gram route
    pmn.close(model.posterior_means(xi, Z17)(xt), ref(Z17), tol, (kind, "17 columns"))
    ztsim = np.random.default_rng(3).standard_normal((n + m, 4))
    paths = model.conditional_sample_paths_from_data(ztsim, xi, np.arange(n), zi, xt, n + np.arange(m))
    pmn.close(paths, ztsim[n:] + ref(zi[:, None] - ztsim[:n]), tol, (kind, "paths"))
