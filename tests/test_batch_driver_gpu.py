"""gpmp_nll_grad_batch (include/gpmp_hip.h): B small problems per call, every kernel batched over the problems --
SURVEY 8(f).4, the throughput caller behind gnp.BatchDifferentiableSelectionCriterion (gpmp/num/torch_backend.py:607-718)
and multi-parameter log_prob evaluations (gpmp/mcmc/param_posterior.py:229-278).  Checked problem by problem against the
single-problem driver gpmp_nll_grad (itself pinned on the reference's fixtures in tests/test_c_abi_mean_drivers_gpu.py),
on ragged sizes across the diagonal-block / panel boundaries, shared and per-problem parameters, q = 0 ... 16 mean columns,
slots up to 4096 points (round 5: the limits were q <= 7, n <= 2048)."""
import ctypes
import math

import numpy as np
import pytest

from tests.helpers import rel_err

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import gpmp_amd.num as gnp
    from gpmp_amd import _lib

    return torch, gnp, _lib, _lib.load()


def _single(env, x, z, P, theta, p=2, noise=0):
    torch, gnp, _lib, lib = env
    dev = gnp._dev()
    n, d = x.shape
    q = 0 if P is None else P.shape[1]
    X, Z = torch.as_tensor(np.ascontiguousarray(x), device=dev), torch.as_tensor(np.ascontiguousarray(z), device=dev)
    Pt = None if P is None else torch.as_tensor(np.ascontiguousarray(P), device=dev)
    ws = torch.empty(int(lib.gpmp_nll_grad_ws_elems(n, d, q)), dtype=torch.float64, device=dev)
    val = torch.empty(1, dtype=torch.float64, device=dev)
    g = torch.empty(len(theta), dtype=torch.float64, device=dev)
    info = torch.zeros(1, dtype=torch.int32, device=dev)
    _lib.check(lib.gpmp_nll_grad(gnp._ptr(X), gnp._ptr(Z), gnp._ptr(Pt), max(q, 1), n, d, q, p, _lib.host_vec(theta), noise, gnp._ptr(ws),
                                 gnp._ptr(val), gnp._ptr(g), gnp._ptr(info), gnp._stream()), "gpmp_nll_grad")
    return float(val.item()), g.cpu().numpy(), int(info.item())


def _batch(env, xs, zs, Ps, thetas, shared, p=2, noise=0, want_grad=True):
    """stack into padded (B, nmax, .) arrays and call the driver"""
    torch, gnp, _lib, lib = env
    dev = gnp._dev()
    B, ns = len(xs), [len(z) for z in zs]
    nmax, d = max(ns), xs[0].shape[1]
    q = 0 if Ps is None else Ps[0].shape[1]
    X, Z, P = np.zeros((B, nmax, d)), np.zeros((B, nmax)), np.zeros((B, nmax, max(q, 1)))
    for b in range(B):
        X[b, : ns[b]], Z[b, : ns[b]] = xs[b], zs[b]
        if q:
            P[b, : ns[b]] = Ps[b]
    Xt, Zt, Pt = (torch.as_tensor(a, device=dev) for a in (X, Z, P))
    th = np.ascontiguousarray(thetas, dtype=np.float64)
    ntheta = th.shape[-1]
    ws = torch.empty(int(lib.gpmp_batch_ws_elems(nmax, d, q, B, int(want_grad))), dtype=torch.float64, device=dev)
    vals = torch.empty(B, dtype=torch.float64, device=dev)
    grads = torch.empty((B, ntheta), dtype=torch.float64, device=dev) if want_grad else None
    info = torch.zeros(B, dtype=torch.int32, device=dev)
    n_host = (ctypes.c_int * B)(*ns)
    _lib.check(lib.gpmp_nll_grad_batch(gnp._ptr(Xt), nmax * d, gnp._ptr(Zt), nmax, gnp._ptr(Pt) if q else None, max(q, 1), nmax * max(q, 1), q,
                                       n_host, nmax, d, B, p, _lib.host_vec(th.reshape(-1)), 0 if shared else ntheta, noise, gnp._ptr(ws),
                                       gnp._ptr(vals), gnp._ptr(grads), gnp._ptr(info), gnp._stream()), "gpmp_nll_grad_batch")
    return vals.cpu().numpy(), (grads.cpu().numpy() if want_grad else None), info.cpu().numpy()


def _design(x, q):
    """mean design with up to 1 + 6 d columns: [1, x, x^2] (the first 1 + 2 d, as before round 5), then cos(k pi x), k = 1 .. 4"""
    cols = [np.ones((len(x), 1)), x, x * x] + [np.cos(k * np.pi * x) for k in range(1, 5)]
    return np.hstack(cols)[:, :q]


def _data(n, d, seed):
    rng = np.random.default_rng(seed)
    x = rng.random((n, d))
    return x, np.sin(3 * x[:, 0]) + x.sum(axis=1) + 0.02 * rng.standard_normal(n)


@pytest.mark.parametrize("q", [0, 1, 3])
@pytest.mark.parametrize("sizes", [(300, 128, 77, 257, 300), (1024, 1000, 513), (90, 64, 31), (640, 640, 640, 640, 640, 640, 640), (2048, 1300, 1537)])
def test_batch_driver_ragged_sizes_shared_parameters(env, sizes, q):
    d = 3
    th = np.concatenate(([0.2], -np.log(0.3 + 0.2 * np.arange(d))))
    data = [_data(n, d, 100 + n + k) for k, n in enumerate(sizes)]
    xs, zs = [a for a, _ in data], [b for _, b in data]
    Ps = None if q == 0 else [np.hstack((np.ones((len(x), 1)), x))[:, :q] for x in xs]
    vals, grads, info = _batch(env, xs, zs, Ps, th, shared=True)
    vals_only, none, _ = _batch(env, xs, zs, Ps, th, shared=True, want_grad=False)
    assert none is None and np.array_equal(vals_only, vals)
    assert np.all(info == 0)
    for b in range(len(sizes)):
        v, g, i = _single(env, xs[b], zs[b], None if q == 0 else Ps[b], th)
        # (d = 3: above ~1000 points K is ill-conditioned at these length scales, and the one-stream / look-ahead routes of the two
        #  drivers round differently: 2e-9 relative on the value at n = 2048)
        tol_v, tol_g = (1e-11, 1e-9) if max(sizes) <= 1024 else (1e-8, 1e-6)
        assert i == 0 and abs(vals[b] - v) < tol_v * abs(v), (b, vals[b], v)
        assert rel_err(grads[b], g) < tol_g, (b, grads[b], g)


def _cond_scale(K):
    """max(1, cond(K) / 1e6): the factor by which the SURVEY 8(c) tolerances grow with the conditioning (measured, host eigenvalues)"""
    ev = np.linalg.eigvalsh(K)
    return max(1.0, float(ev[-1] / max(ev[0], 1e-300)) / 1e6)


def _value_extended(x, z, P, theta, noise):
    """The criterion value (Matern 5/2; NLL for P = None, else REML) evaluated in np.longdouble: Gram matrix, Cholesky,
    W = L^-1 [z, P] and the q x q algebra, by the identities of DESIGN.md section 2.  With the 64-bit mantissa of x86 this is
    2048 times finer than fp64, so at cond(K) ~ 5e8 it is still good to ~1e-9 where the fp64 oracle (an explicit inverse) is not.
    None where long double is no wider than double."""
    LD = np.longdouble
    if np.finfo(LD).eps >= np.finfo(np.float64).eps:
        return None

    def chol(A):
        n = A.shape[0]
        L = np.zeros((n, n), dtype=LD)
        for j in range(n):
            col = A[j:, j] - L[j:, :j] @ L[j, :j] if j else A[j:, j]
            L[j:, j] = col / np.sqrt(col[0])
        return L

    def logdet(L):
        return 2 * np.log(np.diag(L)).sum()

    n, d = x.shape
    th = np.asarray(theta, dtype=np.float64).astype(LD)
    s2, invrho = np.exp(th[0]), np.exp(th[(2 if noise else 1):])
    xs = x.astype(LD) * invrho
    h2 = np.zeros((n, n), dtype=LD)
    for k in range(d):
        df = xs[:, k][:, None] - xs[:, k][None, :]
        h2 += df * df
    c = 2 * np.sqrt(LD(2.5))
    t = 2 * c * np.sqrt(h2)
    K = s2 * np.exp(-t / 2) * (1 + t / 2 + t * t / 12)                       # gpmp/kernel/matern.py:54-64 at p = 2
    K[np.diag_indices(n)] += np.exp(th[1]) if noise else 10 * s2 * LD(np.finfo(np.float64).eps)      # matern.py:90
    L = chol(K)
    Y = z.astype(LD)[:, None] if P is None else np.hstack((z[:, None], P)).astype(LD)
    W = np.zeros_like(Y)
    for i in range(n):
        W[i] = (Y[i] - L[i, :i] @ W[:i] if i else Y[i]) / L[i, i]
    q = Y.shape[1] - 1
    val = (n - q) * np.log(2 * LD(np.pi)) + logdet(L) + W[:, 0] @ W[:, 0]
    if q:
        Wp, Pl = W[:, 1:], Y[:, 1:]
        R = chol(Wp.T @ Wp)                                                   # S = P^T K^-1 P = R R^T
        u = np.zeros(q, dtype=LD)
        b = Wp.T @ W[:, 0]
        for i in range(q):
            u[i] = (b[i] - R[i, :i] @ u[:i] if i else b[i]) / R[i, i]
        val += logdet(R) - logdet(chol(Pl.T @ Pl)) - u @ u                    # b^T S^-1 b = |R^-1 b|^2
    return float(val / 2)


_SMALL, _MID, _BIG = (300, 128, 77, 257), (2048, 1300, 1537), (4096, 3000)
# every q on the small ragged set; q = 0, 7, 16 on the 2048-point set (host eigenvalues + inverse per problem: 3 s a case, so one
# noise setting each -- the soak draws the rest); q = 16 with the noise term on the 4096-point set (11 s of host work)
_ORACLE_CASES = ([(_SMALL, q, nz) for q in (0, 1, 3, 4, 7, 8, 16) for nz in (0, 1)] + [(_MID, 0, 0), (_MID, 0, 1), (_MID, 7, 1), (_MID, 16, 0)]
                 + [(_BIG, 16, 1)])


@pytest.mark.parametrize("sizes,q,noise", _ORACLE_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_batch_driver_against_the_oracle_at_its_edges(env, sizes, q, noise):
    """the batched kernel against the CPU ORACLE (not against another HIP driver): ragged slots up to the 4096-point limit,
    q = 0 (ML: likelihood.py:18-52) and q = 1 ... 16 (REML: likelihood.py:92-129; q = 8, 16: the wide mean-space kernel of round 5),
    values and analytic gradients, with the SURVEY 8(c) tolerances (value rel 1e-12, gradient rel 1e-8) scaled by the MEASURED
    cond(K) / 1e6 of each problem; noise = 1 adds a 1e-4 noise variance (cond ~ 5e6), noise = 0 is the bare kernel (cond up to
    5e8 at n = 2048)"""
    from oracle import gp_oracle as orc

    d = 3
    th = np.concatenate(([0.2], -np.log(0.3 + 0.2 * np.arange(d))))
    if noise:
        th = np.concatenate(([th[0], math.log(1e-4)], th[1:]))
    data = [_data(n, d, 100 + n + k) for k, n in enumerate(sizes)]
    xs, zs = [a for a, _ in data], [b for _, b in data]
    # mean design: columns of [1, x, x^2, cos(k pi x)] (q = 4: the linear mean of d = 3; q = 16: the widest the batched path carries)
    Ps = None if q == 0 else [_design(x, q) for x in xs]
    vals, grads, info = _batch(env, xs, zs, Ps, th, shared=True, noise=noise)
    assert np.all(info == 0)
    cov = orc.noisy_maternp_covariance if noise else orc.maternp_covariance
    for b, n in enumerate(sizes):
        cs = _cond_scale(cov(xs[b], None, 2, th))
        if q == 0:
            v, g = orc.nll_zero_mean_value_and_grad(xs[b], zs[b], 2, th, noise_index=1 if noise else None)
        else:
            v, g = orc.reml_value_and_grad(xs[b], zs[b], Ps[b], 2, th, noise_index=1 if noise else None)
        if cs > 100.0:
            # cond(K) > 1e8: the fp64 oracle's own rounding error (it forms K^-1) is as large as the bound -- n = 2048, cond 5.3e8,
            # q = 0: oracle 9.8e-7 below and driver 6.3e-7 above the long-double value, bound 1.09e-6 -- so the same bound is
            # asked against the long-double value
            ve = _value_extended(xs[b], zs[b], None if q == 0 else Ps[b], th, noise)
            v = v if ve is None else ve
        assert abs(vals[b] - v) <= 1e-12 * cs * max(abs(v), n), (b, n, cs, vals[b], v)
        assert rel_err(grads[b], g) <= 1e-8 * cs, (b, n, cs, grads[b], g)


def test_batch_driver_many_parameter_vectors_one_data_set(env):
    """the sampler pattern: stride 0 on the data, one parameter row per problem; noisy kernel"""
    torch, gnp, _lib, lib = env
    n, d, B = 400, 4, 24
    x, z = _data(n, d, 7)
    rng = np.random.default_rng(3)
    th0 = np.concatenate(([0.1, -3.0], -np.log(0.4 + 0.2 * np.arange(d))))
    thetas = th0 + 0.3 * rng.standard_normal((B, len(th0)))
    dev = gnp._dev()
    X, Z = torch.as_tensor(x, device=dev), torch.as_tensor(z, device=dev)
    ws = torch.empty(int(lib.gpmp_batch_ws_elems(n, d, 0, B, 1)), dtype=torch.float64, device=dev)
    vals = torch.empty(B, dtype=torch.float64, device=dev)
    grads = torch.empty((B, len(th0)), dtype=torch.float64, device=dev)
    info = torch.zeros(B, dtype=torch.int32, device=dev)
    _lib.check(lib.gpmp_nll_grad_batch(gnp._ptr(X), 0, gnp._ptr(Z), 0, None, 1, 0, 0, None, n, d, B, 2, _lib.host_vec(thetas.reshape(-1)),
                                       len(th0), 1, gnp._ptr(ws), gnp._ptr(vals), gnp._ptr(grads), gnp._ptr(info), gnp._stream()),
               "gpmp_nll_grad_batch")
    assert np.all(info.cpu().numpy() == 0)
    for b in range(B):
        v, g, _ = _single(env, x, z, None, thetas[b], noise=1)
        assert abs(float(vals[b]) - v) < 1e-11 * abs(v) and rel_err(grads[b].cpu().numpy(), g) < 1e-9, b


def test_batch_driver_failure_is_per_problem(env, golden):
    g = golden("likelihood")
    xb, zb, thb = g["lik_bad_xi"], g["lik_bad_zi"], g["lik_bad_theta"]
    d = xb.shape[1]
    good = [_data(len(zb), d, 50 + k) for k in range(3)]
    xs, zs = [good[0][0], xb, good[1][0], good[2][0]], [good[0][1], zb, good[1][1], good[2][1]]
    thg = np.concatenate(([0.0], -np.log(0.3 + 0.2 * np.arange(d))))
    thetas = np.stack([thg, thb, thg, thg])                       # only problem 1 gets the degenerate parameters
    vals, grads, info = _batch(env, xs, zs, None, thetas, shared=False)
    assert info[1] > 0 and math.isinf(vals[1]) and np.all(grads[1] == 0.0)
    assert np.all(info[[0, 2, 3]] == 0) and np.all(np.isfinite(vals[[0, 2, 3]]))
    for b in (0, 2, 3):
        v, gr, _ = _single(env, xs[b], zs[b], None, thetas[b])
        assert abs(vals[b] - v) < 1e-8 * abs(v) and rel_err(grads[b], gr) < 1e-6      # (ill-conditioned at these length scales)
    torch, gnp, _lib, lib = env
    assert lib.gpmp_batch_ws_elems(4097, 3, 0, 4, 1) == 0 and lib.gpmp_batch_ws_elems(512, 3, 17, 4, 1) == 0
    assert lib.gpmp_batch_ws_elems(512, 3, 16, 4, 1) > 0 and lib.gpmp_batch_ws_elems(4096, 3, 16, 2, 1) > 0


def test_batch_criterion_fast_path_equals_one_at_a_time(env, golden):
    """gnp.BatchDifferentiableSelectionCriterion through the batched kernel and through the per-batch route"""
    import gpmp_amd as gp
    import gpmp_amd.num as gnp

    g = golden("batch")
    p, b = int(g["batch_p"]), g["batch_bounds"]
    loader = [(g["batch_xi"][a:c], g["batch_zi"][a:c]) for a, c in zip(b[:-1], b[1:])]
    ones = lambda x, prm: gnp.ones((x.shape[0], 1))  # noqa: E731
    k = gp.kernel.MaternCovariance(p)
    for model, crit in ((gp.Model(None, k, None, None, "zero"), gp.kernel.negative_log_likelihood_zero_mean),
                        (gp.Model(ones, k, None, None), gp.kernel.negative_log_restricted_likelihood)):
        ev, pre, nograd, grad = gp.kernel.make_selection_criterion_with_gradient(model, crit, dataloader=loader)
        obj = pre.__self__
        for t in g["batch_thetas"]:
            obj.use_batched_kernel = True
            v1, g1, e1 = pre(t), grad(t).copy(), ev(t)
            obj.use_batched_kernel = False
            v2, g2, e2 = pre(t), grad(t).copy(), ev(t)
            assert abs(v1 - v2) < 1e-12 * abs(v2) and abs(e1 - e2) < 1e-12 * abs(e2) and rel_err(g1, g2) < 1e-10
        obj.use_batched_kernel = True


def test_criterion_at_many_parameter_vectors_sampler_pattern(env, golden):
    """criterion.evaluate_many(P): the chains of a sampler ask for the criterion at many parameter vectors on the SAME data
    (gpmp/mcmc/param_posterior.py:229-278 evaluates them one after the other); one batched call must agree with the
    one-at-a-time route, value and gradient, for ML, REML and REMAP, and a row that cannot be factored gets +inf"""
    import gpmp_amd as gp
    import gpmp_amd.num as gnp

    g = golden("batch")
    p = int(g["batch_p"])
    xi, zi = g["batch_xi"][:300], g["batch_zi"][:300]
    ones = lambda x, prm: gnp.ones((x.shape[0], 1))  # noqa: E731
    k = gp.kernel.MaternCovariance(p)
    base = np.asarray(g["batch_thetas"][0], dtype=float)
    rng = np.random.default_rng(5)
    P = base + 0.3 * rng.standard_normal((9, base.size))
    for model, crit in ((gp.Model(None, k, None, None, "zero"), gp.kernel.negative_log_likelihood_zero_mean),
                        (gp.Model(ones, k, None, None), gp.kernel.negative_log_restricted_likelihood)):
        ev, pre, nograd, grad = gp.kernel.make_selection_criterion_with_gradient(model, crit, xi, zi)
        obj = pre.__self__
        vals, grads = obj.evaluate_many(P, want_grad=True)
        only_vals = obj.evaluate_many(P)
        for c in range(P.shape[0]):
            v = pre(P[c])
            gr = grad(P[c])
            assert abs(vals[c] - v) < 1e-11 * abs(v) and abs(only_vals[c] - v) < 1e-11 * abs(v), (c, vals[c], v)
            assert rel_err(grads[c], gr) < 1e-9, c
        # a row far outside anything factorable (length scales of 1e-30 .. 1e+30 alternate): +inf for that row only
        bad = P.copy()
        bad[4, 1:] = np.where(np.arange(base.size - 1) % 2 == 0, 70.0, -70.0)
        bad[4, 0] = 700.0
        v_bad = obj.evaluate_many(bad)
        ok = np.ones(P.shape[0], bool); ok[4] = False
        assert np.allclose(v_bad[ok], vals[ok], rtol=1e-11) and (not np.isfinite(v_bad[4]) or abs(v_bad[4]) > 1e10)


@pytest.mark.parametrize("B,n,d,q", [(1, 5, 1, 0), (1, 129, 2, 1), (3, 4, 1, 3), (2, 1024, 6, 2), (17, 130, 3, 0), (2, 2048, 6, 1),
                                     (2, 4096, 6, 1), (3, 700, 4, 16), (2, 3000, 3, 9), (5, 40, 3, 12)])
def test_batch_driver_edge_shapes(env, B, n, d, q):
    """one problem, tiny problems (n just above q), one-dimensional inputs, the largest slot size, a block boundary + 2"""
    th = np.concatenate(([0.1], -np.log(0.3 + 0.25 * np.arange(d))))
    data = [_data(n, d, 900 + 7 * b + n) for b in range(B)]
    xs, zs = [a for a, _ in data], [b_ for _, b_ in data]
    Ps = None if q == 0 else [_design(x, q) for x in xs]
    vals, grads, info = _batch(env, xs, zs, Ps, th, shared=True)
    assert np.all(info == 0)
    tol_v, tol_g = (1e-10, 1e-8) if n <= 2048 else (1e-8, 1e-6)      # (above 2048 the two drivers block differently: see the ragged-size test)
    for b in range(B):
        v, g, i = _single(env, xs[b], zs[b], None if q == 0 else Ps[b], th)
        assert i == 0 and abs(vals[b] - v) < tol_v * max(1.0, abs(v)), (b, vals[b], v)
        assert rel_err(grads[b], g) < tol_g, (b, grads[b], g)


def test_batched_call_cut_into_pieces_by_workspace_budget(env, monkeypatch):
    """batch_values_and_gradients cuts a call whose workspace would exceed its memory budget into pieces (GPMP_BATCH_WS_BUDGET_MB forces
    it): same values and gradients as the single call, shared and per-problem parameters, REML with a mean"""
    import gpmp_amd as gp
    import gpmp_amd.num as gnp
    from gpmp_amd.core.gradients import batch_values_and_gradients

    d, B, n = 3, 7, 300
    th = np.concatenate(([0.2], -np.log(0.3 + 0.2 * np.arange(d))))
    data = [_data(n - 11 * b, d, 40 + b) for b in range(B)]
    batches = [(gnp.asarray(x), gnp.asarray(z)) for x, z in data]
    ones = lambda x, prm: gnp.ones((x.shape[0], 1))  # noqa: E731
    k = gp.kernel.MaternCovariance(2)
    TH = th + 0.05 * np.random.default_rng(3).standard_normal((B, th.size))
    for model, use_mean in ((gp.Model(None, k, None, th, "zero"), False), (gp.Model(ones, k, None, th), True)):
        for params in (th, TH):
            monkeypatch.delenv("GPMP_BATCH_WS_BUDGET_MB", raising=False)
            v0, g0 = batch_values_and_gradients(model, params, batches, True, use_mean=use_mean)
            monkeypatch.setenv("GPMP_BATCH_WS_BUDGET_MB", "5")          # two or three problems of 300 points per piece
            v1, g1 = batch_values_and_gradients(model, params, batches, True, use_mean=use_mean)
            v2, none = batch_values_and_gradients(model, params, batches, False, use_mean=use_mean)
            assert none is None
            # (a piece is padded to ITS largest problem, so the blocking -- and the rounding -- differs from the single call's)
            assert np.allclose(v1, v0, rtol=1e-12, atol=0) and rel_err(g1, g0) < 1e-10 and np.allclose(v2, v0, rtol=1e-12, atol=0)


def test_few_large_problems_take_the_per_problem_sweeps(env):
    """(round 5) slots above 2048 points, few problems: inside the batched call the triangular solves run as the single-problem
    one-launch sweep per problem (B < nmax / 100) instead of the workgroup-per-problem kernel -- n = 4096, B = 4: 26.6 -> 10.5 ms
    (profiles/r5/batch_small_problems_throughput_r5_final.log).  Same values as one problem at a time, with and without a mean."""
    import gpmp_amd as gp
    import gpmp_amd.num as gnp
    from gpmp_amd.core.gradients import MLZeroMeanAnalytic, REMLAnalytic, batch_values_and_gradients

    d, n = 3, 2100
    th = np.concatenate(([0.2, math.log(1e-4)], -np.log(0.3 + 0.2 * np.arange(d))))
    cov = gp.kernel.MaternCovariance(2, noise=True)
    batches = [tuple(gnp.asarray(a) for a in _data(n - 7 * b, d, 300 + b)) for b in range(3)]
    lin = lambda x, prm: gnp.hstack((gnp.ones((x.shape[0], 1)), x))       # noqa: E731
    for model, ana, use_mean in ((gp.Model(None, cov, None, th, "zero"), MLZeroMeanAnalytic, False), (gp.Model(lin, cov, None, th), REMLAnalytic, True)):
        vals, grads = batch_values_and_gradients(model, th, batches, True, use_mean=use_mean)
        one = ana(model)
        for b in range(3):
            v, st = one.value_and_state(th, *batches[b])
            g = one.gradient_from_state(st)
            assert abs(vals[b] - v) < 1e-8 * abs(v) and rel_err(grads[b], g) < 1e-6


def test_batch_driver_random_soak(env):
    """Opt-in soak (GPMP_BATCH_SOAK_CASES=<count>, GPMP_BATCH_SOAK_SEED): random draws of the number of problems, ragged sizes (up to
    the 4096-point slot now and then), input dimension, regularity p, noise term, q = 0 ... 16 mean columns, shared or per-problem
    parameters -- each problem of each call against the single-problem driver: value 1e-9, gradient 1e-7, or (the two drivers block
    differently) the measured conditioning (of K and of the mean-space matrix) times 1e-14 / 1e-12 for the problems that deviate more;
    nothing is compared above 1e13.
    The soak hunts indexing errors; the fixed cases above hold the SURVEY 8(c) tolerances against the oracle."""
    import os

    from oracle import gp_oracle as orc

    ncases = int(os.environ.get("GPMP_BATCH_SOAK_CASES", "0"))
    if ncases <= 0:
        pytest.skip("opt-in: GPMP_BATCH_SOAK_CASES=<count>")
    rng = np.random.default_rng(int(os.environ.get("GPMP_BATCH_SOAK_SEED", "5")))
    bad = []
    for i in range(ncases):
        d = int(rng.integers(1, 9))
        q = int(rng.choice([0, 0, 1, 2, 3, 5, 7, 8, 12, 16]))
        q = min(q, 1 + 6 * d)
        p = int(rng.integers(0, 5))
        noise = int(rng.integers(0, 2))
        big = rng.random() < 0.08
        nmax = int(rng.integers(2100, 4097)) if big else int(rng.integers(max(q + 3, 6), 1500))
        B = int(rng.integers(1, 4)) if big else int(rng.integers(1, 25))
        sizes = [nmax] + [int(rng.integers(max(q + 2, 4, nmax // 3), nmax + 1)) for _ in range(B - 1)]
        rng.shuffle(sizes)
        shared = bool(rng.integers(0, 2))
        th0 = np.concatenate(([0.2 * rng.standard_normal()], [math.log(1e-3)] if noise else [], -np.log(0.5 + rng.random(d))))
        thetas = th0 if shared else th0 + 0.1 * rng.standard_normal((B, th0.size))
        data = [_data(n, d, 5000 + 31 * i + k) for k, n in enumerate(sizes)]
        xs, zs = [a for a, _ in data], [b_ for _, b_ in data]
        Ps = None if q == 0 else [_design(x, q) for x in xs]
        vals, grads, info = _batch(env, xs, zs, Ps, thetas, shared=shared, p=p, noise=noise)
        worst_v = worst_g = 0.0
        for b in range(B):
            v, g, i1 = _single(env, xs[b], zs[b], None if q == 0 else Ps[b], thetas if shared else thetas[b], p=p, noise=noise)
            def conditioning():
                # cond(K), and with a mean design cond(P^T K^-1 P) (a 9-point problem with 7 design columns has a well-conditioned
                # K and a mean-space matrix at 1e10): host eigenvalues, only for the problems that deviate
                cov = orc.noisy_maternp_covariance if noise else orc.maternp_covariance
                K = cov(xs[b], None, p, thetas if shared else thetas[b])
                evs = np.linalg.eigvalsh(K)
                c = float(evs[-1] / max(evs[0], 1e-300))
                if q and c < 1e13:
                    c = max(c, float(np.linalg.cond(Ps[b].T @ np.linalg.solve(K, Ps[b]))))
                return c

            if i1 != 0 or info[b] != 0:
                # a factorisation that fails in one driver only: legitimate on a numerically singular K (rounding decides), a finding otherwise
                if (i1 != 0) != (info[b] != 0) and conditioning() < 1e13:
                    bad.append((i, b, "info differs", int(info[b]), i1))
                continue
            ev, eg = abs(vals[b] - v) / max(1.0, abs(v)), rel_err(grads[b], g)
            worst_v, worst_g = max(worst_v, ev), max(worst_g, eg)
            if not (ev < 1e-9 and eg < 1e-7):
                # the two drivers block differently, so their roundings differ by O(cond(K) eps): measure it (host eigenvalues, only
                # for the problems that deviate) -- d = 1 or 2 without a noise term reaches cond(K) ~ 1e15: nothing to compare there
                cond = conditioning()
                if cond < 1e13 and not (ev < 1e-14 * cond and eg < 1e-12 * cond):
                    bad.append((i, b, sizes[b], ev, eg, cond))
        print(f"[batch soak {i:3d}] B={B} nmax={nmax} d={d} q={q} p={p} noise={noise} shared={shared}: value {worst_v:.1e} gradient {worst_g:.1e}", flush=True)
    assert not bad, bad


def test_batch_workspace_beyond_2_to_the_31_elements(env):
    """40 000 problems of 256 points in ONE call: 2.6e9 matrix elements per workspace section (every per-problem offset beyond problem
    32 768 exceeds 32 bits) -- a C host may do this (B <= 65535; the Python layer cuts its calls by a memory budget).  Values and
    gradients of the first, the last and sampled problems against the single-problem driver; all factorisations succeed."""
    torch, gnp, _lib, lib = env
    if torch.cuda.get_device_properties(0).total_memory < 150e9:
        pytest.skip("needs 150 GB of HBM")
    B, n, d, q = 40000, 256, 3, 2
    rng = np.random.default_rng(17)
    dev = gnp._dev()
    X = torch.as_tensor(rng.random((B, n, d)), device=dev)
    Z = torch.sin(3 * X[:, :, 0]) + X.sum(dim=2)
    P = torch.cat((torch.ones((B, n, 1), dtype=torch.float64, device=dev), X[:, :, :1]), dim=2).contiguous()
    th = np.concatenate(([0.2, math.log(1e-3)], -np.log(0.3 + 0.2 * np.arange(d))))
    nws = int(lib.gpmp_batch_ws_elems(n, d, q, B, 1))
    assert nws > 2 ** 31
    ws = torch.empty(nws, dtype=torch.float64, device=dev)
    vals = torch.empty(B, dtype=torch.float64, device=dev)
    grads = torch.empty((B, len(th)), dtype=torch.float64, device=dev)
    info = torch.full((B,), -1, dtype=torch.int32, device=dev)
    _lib.check(lib.gpmp_nll_grad_batch(gnp._ptr(X), n * d, gnp._ptr(Z), n, gnp._ptr(P), q, n * q, q, None, n, d, B, 2, _lib.host_vec(th), 0, 1,
                                       gnp._ptr(ws), gnp._ptr(vals), gnp._ptr(grads), gnp._ptr(info), gnp._stream()), "gpmp_nll_grad_batch")
    assert bool((info == 0).all()) and bool(torch.isfinite(vals).all()) and bool(torch.isfinite(grads).all())
    v_all, g_all = vals.cpu().numpy(), grads.cpu().numpy()
    for b in (0, 1, 32767, 32768, 32769, 39998, B - 1, int(rng.integers(B)), int(rng.integers(B))):
        v, g, i1 = _single(env, X[b].cpu().numpy(), Z[b].cpu().numpy(), P[b].cpu().numpy(), th, noise=1)
        assert i1 == 0 and abs(v_all[b] - v) < 1e-10 * max(1.0, abs(v)) and rel_err(g_all[b], g) < 1e-8, (b, v_all[b], v)
