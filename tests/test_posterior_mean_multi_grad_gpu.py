"""PosteriorMeans.mean_and_gradient and the C entry gpmp_posterior_mean_multi_grad on the GPU, against the library's own Gram matrix
(value), the NumPy restatement (posterior_mean_numpy.py, Jacobian) and the single-column kernel gpmp_posterior_mean.

Tile extents of csrc/posterior_mean_multi.hip (its gradient instances) this file relies on: a matrix instruction takes 4 observation points, 16 run in
lock step, 32 make an LDS chunk, a slice has at least 128 (n = 1000 at m <= 64: 8 slices of 128 rows, the last of 104 = three
chunks and a short one; n = 300: 3 slices, the last of 44); a wave owns 16 prediction points, a workgroup 64; a column tile is 16
wide and a workgroup has 1 to 4 of them (s <= 16, <= 32, <= 48, more), with at most 12 / 8 / 5 / 4 of the d + 1 components per
workgroup: s in (15, 17, 33, 65) meets every one of those, d + 1 in 3 .. 9 and 11 .. 13 each of them - 1, + 0, + 1; x_t is in
registers for d <= 8 and d <= 16 and in LDS above (d = 8 | 9, 16 | 17)."""
import numpy as np
import pytest

from . import posterior_mean_numpy as pmn
from . import predict_grad_numpy as pgn
from .test_posterior_mean_gpu import _c_mean, _dev, _model, _problem, env  # noqa: F401
from .test_posterior_mean_multi_gpu import _c_mean_multi

pytestmark = pytest.mark.gpu
NS = (1, 3, 4, 5, 15, 16, 17, 31, 32, 33, 127, 128, 129, 1000)
MS = (1, 15, 16, 17, 63, 64, 65, 130)
SS = (1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 130)
SUB = ((5, 33, 300), (17, 65), (15, 17, 33, 65))                  # short last group, chunk, slice, point tile and column tile


def _c_multi_grad(env, X, A, XT, s, p, theta, noise, Pt=None, B=None, J=None, O=None, G=None):
    """gpmp_posterior_mean_multi_grad through ctypes on device tensors (leading dimensions = strides); O (m x s), G (m x d x s) views."""
    _, gnp, _lib, torch = env
    lib = _lib.load()
    (n, d), m, q = X.shape, XT.shape[0], 0 if B is None else B.shape[0]
    O = torch.empty((m, s), dtype=torch.float64, device="cuda") if O is None else O
    G = torch.empty((m, d, s), dtype=torch.float64, device="cuda") if G is None else G
    ws = torch.empty(int(lib.gpmp_posterior_mean_multi_grad_ws_elems(n, m, s, d)), dtype=torch.float64, device="cuda")
    _lib.check(lib.gpmp_posterior_mean_multi_grad(
        gnp._ptr(X), gnp._ptr(A), A.stride(0), gnp._ptr(XT), gnp._ptr(Pt), Pt.stride(0) if q else 0, gnp._ptr(B), B.stride(0) if q else 0,
        gnp._ptr(J), n, m, s, d, q, p, _lib.host_vec(theta), noise, gnp._ptr(ws), gnp._ptr(O), O.stride(0), gnp._ptr(G), G.stride(1),
        gnp._stream()), "gpmp_posterior_mean_multi_grad")
    return O[:, :s], G[:, :, :s]


def _jacobian(xi, A, xt, p, th, noise, Pt=None, B=None, J=None):
    """pmn.mean_and_gradient column by column: (m, d, s)."""
    return np.stack([pmn.mean_and_gradient(xi, A[:, c], xt, p, th, noise, Pt, None if B is None else B[:, c], J)[1]
                     for c in range(A.shape[1])], axis=2)


@pytest.mark.parametrize("d", [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 16, 17, 64])
def test_value_bound_and_jacobian_at_every_tile_extent(env, d):
    """q = 0, random A.  Component 0 is the Gram entry, so O is within the value kernel's bound 4 n 2^-53 |G|^T |A| of G^T A; the
    Jacobian within 1e-9 of max(1, max|ref|) (pmn.close) of NumPy's.  d = 3, p = 2 runs NS x MS x SS, everything else SUB."""
    from gpmp_amd.kernel import MaternCovariance

    rng = np.random.default_rng(80 + d)
    xi, xt, al = rng.random((1000, d)), rng.random((130, d)), rng.standard_normal((1000, 130))
    XI, XT, AL = _dev(env, xi), _dev(env, xt), _dev(env, al)
    for p, noise in ((2, 0), (0, 0), (16, 0), (2, 1)) if d == 3 else ((2, 0),):
        th = np.insert(_problem(1, 1, d, 0)[3], 1, [-1.0] * noise)
        ns, ms, ss = (NS, MS, SS) if (d, p, noise) == (3, 2, 0) else SUB
        for n in ns:
            ref = _jacobian(xi[:n], al[:n, : max(ss)], xt[: max(ms)], p, th, noise)      # once per n: rows and columns are prefixes
            for m in ms:
                K = MaternCovariance(p, noise=bool(noise))(XI[:n], XT[:m], th)          # gpmp_matern_gram(xi, xt)
                for s in ss:
                    A = AL[:n, :s].contiguous()
                    O, G = _c_multi_grad(env, XI[:n], A, XT[:m], s, p, th, noise)
                    assert bool(((O - K.t() @ A).abs() <= 4.0 * n * 2.0 ** -53 * (K.abs().t() @ A.abs())).all()), (p, noise, n, m, s)
                    pmn.close(G.cpu().numpy(), ref[:m, :, :s], 1e-9, (p, noise, n, m, s))


@pytest.mark.parametrize("n, m, s, q, d", [(1000, 65, 17, 1, 3), (33, 130, 65, 4, 3), (300, 17, 33, 4, 17)])
def test_mean_part_strides_and_guards(env, n, m, s, q, d):
    """Padded lda, ldb, ldpt, ldo, ldg with NaN behind column s of A and B and column q of Pt; O and G inside guard-valued buffers."""
    from gpmp_amd.kernel import MaternCovariance

    torch, rng = env[3], np.random.default_rng(n + q)
    xi, xt, th = rng.random((n, d)), rng.random((m, d)), _problem(1, 1, d, 0)[3]
    a, b, pt, jac = rng.standard_normal((n, s)), rng.standard_normal((q, s)), rng.standard_normal((m, q)), rng.standard_normal((m, q, d))
    A, B, Pt = (torch.full((r, c + 5), float("nan"), dtype=torch.float64, device="cuda") for r, c in ((n, s), (q, s), (m, q)))
    A[:, :s], B[:, :s], Pt[:, :q] = _dev(env, a), _dev(env, b), _dev(env, pt)
    obuf, gbuf = (torch.full((32 + k * (s + 3),), -7.25, dtype=torch.float64, device="cuda") for k in (m, m * d))
    O, G = _c_multi_grad(env, _dev(env, xi), A, _dev(env, xt), s, 2, th, 0, Pt, B, _dev(env, jac),
                         obuf[16:-16].view(m, s + 3), gbuf[16:-16].view(m, d, s + 3))
    K = MaternCovariance(2)(_dev(env, xi), _dev(env, xt), th)
    bound = 4.0 * n * 2.0 ** -53 * (K.abs().t() @ A[:, :s].abs() + Pt[:, :q].abs() @ B[:, :s].abs())
    assert bool(((O - K.t() @ A[:, :s] - Pt[:, :q] @ B[:, :s]).abs() <= bound).all())
    pmn.close(G.cpu().numpy(), _jacobian(xi, a, xt, 2, th, 0, pt, b, jac), 1e-9, "G")
    for buf, rows in ((obuf, m), (gbuf, m * d)):
        assert bool((buf[:16] == -7.25).all() and (buf[-16:] == -7.25).all() and (buf[16:-16].view(rows, s + 3)[:, s:] == -7.25).all())


def test_far_and_coincident_points(env):
    """xt at 10^4 length scales: the covariance underflows to an exact 0, what is left is Pt B and sum_a B[a][c] J, exact for dyadic
    designs and coefficients.  Then xt = some xi: finite, and NumPy's result (the term of a coincident pair is 0)."""
    rng = np.random.default_rng(4)
    n, m, s, q, d = 200, 70, 17, 4, 3
    xi, rho, A = rng.random((n, d)), np.array([0.5, 0.25, 1.0]), rng.standard_normal((n, s))
    th = np.concatenate(([0.0], -np.log(rho)))
    Pt, B, J = rng.integers(-16, 17, (m, q)) / 8.0, rng.integers(-8, 9, (q, s)) / 4.0, rng.integers(-16, 17, (m, q, d)) / 8.0
    far, xt = 1.0 + 1e4 * rho * (1.0 + rng.random((m, d))), np.vstack((xi[:40], rng.random((30, d))))
    for p in (0, 2, 16):
        O, G = _c_multi_grad(env, _dev(env, xi), _dev(env, A), _dev(env, far), s, p, th, 0, _dev(env, Pt), _dev(env, B), _dev(env, J))
        assert np.array_equal(O.cpu().numpy(), Pt @ B) and np.array_equal(G.cpu().numpy(), np.einsum("ac,taj->tjc", B, J)), p
        O, G = (v.cpu().numpy() for v in _c_multi_grad(env, _dev(env, xi), _dev(env, A), _dev(env, xt), s, p, th, 0))
        assert np.all(np.isfinite(O)) and np.all(np.isfinite(G))
        pmn.close(O, pgn.cov_parts(xi, xt, p, th, 0)[0].T @ A, 1e-9, ("coincident O", p))
        pmn.close(G, _jacobian(xi, A, xt, p, th, 0), 1e-9, ("coincident G", p))


@pytest.mark.parametrize("s", [1, 17])
def test_against_the_single_column_kernel(env, s):
    """Every column against gpmp_posterior_mean with the gradient on the same weights; two calls give the same bits (m = 40: 8 slices)."""
    rng = np.random.default_rng(s)
    n, m, q, d = 1000, 40, 4, 5
    th = _problem(1, 1, d, 0)[3]
    X, XT, A = _dev(env, rng.random((n, d))), _dev(env, rng.random((m, d))), _dev(env, rng.standard_normal((n, s)))
    Pt, B, J = _dev(env, rng.standard_normal((m, q))), _dev(env, rng.standard_normal((q, s))), _dev(env, rng.standard_normal((m, q, d)))
    O, G = _c_multi_grad(env, X, A, XT, s, 2, th, 0, Pt, B, J)
    O2, G2 = _c_multi_grad(env, X, A, XT, s, 2, th, 0, Pt, B, J)
    assert bool((O == O2).all() and (G == G2).all())
    for c in range(s):
        v, g = _c_mean(env, X, A[:, c].contiguous(), XT, 2, th, 0, Pt, q, B[:, c].contiguous(), J)
        pmn.close(O[:, c].cpu().numpy(), v.cpu().numpy(), 1e-9, ("value", c))
        pmn.close(G[:, :, c].cpu().numpy(), g.cpu().numpy(), 1e-9, ("gradient", c))


def test_value_bits_are_those_of_the_value_entry(env):
    """n <= 128 is one slice in both entries whatever m and s, and component 0 of the gradient pass runs the value entry's code
    (one kernel template, one finalize kernel): the two O are the same bits, with and without the mean part."""
    torch, rng = env[3], np.random.default_rng(7)
    for d in (3, 17):
        th = _problem(1, 1, d, 0)[3]
        X, XT, AL = _dev(env, rng.random((128, d))), _dev(env, rng.random((65, d))), _dev(env, rng.standard_normal((128, 65)))
        Pt, BL, J = _dev(env, rng.standard_normal((65, 2))), _dev(env, rng.standard_normal((2, 65))), _dev(env, rng.standard_normal((65, 2, d)))
        for n in (5, 128):
            for s in (17, 65):
                A, B = AL[:n, :s].contiguous(), BL[:, :s].contiguous()
                for mean in ((), (Pt, B)):
                    O = _c_mean_multi(env, X[:n], A, XT, s, 2, th, 0, *mean)
                    Og, _ = _c_multi_grad(env, X[:n], A, XT, s, 2, th, 0, *mean, *((J,) if mean else ()))
                    assert torch.equal(O, Og), (d, n, s, len(mean))


@pytest.mark.parametrize("kind, d, s", [("zero", 4, 17), ("lin", 4, 17), ("param", 4, 17), ("lin", 70, 17), ("lin", 4, 3)])
def test_object(env, kind, d, s):
    """PosteriorMeans.mean_and_gradient column by column against PosteriorMean.mean_and_gradient (d = 70: the fallback route; s = 3:
    below posterior_mean.GRAD_SINGLE_BELOW, the single-column kernel per column)."""
    torch = env[3]
    n, m = 300, 130
    xi, zi, xt, th = _problem(n, m, d, 9)
    Z = np.cos(np.outer(zi, 1.0 + np.arange(s) / s))
    tol = pmn.tolerance(xi, 2, th, 0)
    model = _model(env, 2, 0, th.copy(), kind, d, torch.as_tensor([0.3, 1.1], device="cuda") if kind == "param" else None)
    post = model.posterior_means(xi, Z)
    O, G = post.mean_and_gradient(xt)
    assert O.shape == (m, s) and G.shape == (m, s, d)
    for c in range(s):
        v, g = model.posterior_mean(xi, Z[:, c]).mean_and_gradient(xt)
        pmn.close(O[:, c], v, tol, (kind, "value", c))
        pmn.close(G[:, c, :], g, tol, (kind, "gradient", c))
    pmn.close(O, post(xt), tol, (kind, "__call__"))
    model.covparam = th + 0.5                                        # the snapshot; two evaluations give the same bits
    Ot, Gt = post.mean_and_gradient(torch.as_tensor(xt, device="cuda"), convert_in=False, convert_out=False)
    assert Ot.is_cuda and Gt.is_cuda and Gt.shape == (m, s, d) and Gt.stride(1) == 1
    assert np.array_equal(Ot.cpu().numpy(), O) and np.array_equal(Gt.cpu().numpy(), G)
    O0, G0 = post.mean_and_gradient(np.zeros((0, d)))
    assert O0.shape == (0, s) and G0.shape == (0, s, d)
