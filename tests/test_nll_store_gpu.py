"""Model.negative_log_likelihood_zero_mean through gpmp_whiten (include/gpmp_hip.h): the zero-mean NLL reads the Cholesky factor of
K(xi, xi; theta) from the factor store (GPMP_FACTOR_STORE_MB) when a call before it -- Model.predict, another
NLL -- left the factor of the same points and parameters there.

Every comparison is torch.equal or float equality with the same calls under GPMP_FACTOR_STORE_MB=0, and the NLL also with the
composition it replaces (covariance_factor + solve_lower + torch sum + logdet).  Sizes as tests/test_factor_store_gpu.py: n = 129
(one ragged leaf), 640 (blocked, one stream), 1100 (ragged; the prediction's solve runs along the look-ahead factorisation, the
plain factorisation stays on one stream), 2304 (look-ahead above POTRF_ONE_STREAM_MAX); m = 300, d = 3, p = 2, and one case d = 70."""
import ctypes
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

M, D, P = 300, 3, 2
SIZES = (129, 640, 1100, 2304)
ON_MB = "512"                          # 8 n^2 bytes are 42 MB at n = 2304
POTF2, GRAM = 4, 5                     # kinds of the gpmp_profile_end table: diagonal-block kernel, Gram kernel


@pytest.fixture(scope="module")
def env():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import gpmp_amd as gp
    import gpmp_amd.num as gnp
    from gpmp_amd import _lib

    lib = _lib.load()
    yield torch, gnp, gp, lib
    torch.cuda.synchronize()
    lib.gpmp_device_release()


def _theta(noise=False, scale=0.4):
    return np.concatenate(([0.3], [-4.0] if noise else [], -np.log(scale + 0.3 * np.arange(D))))


def _theta_wide(d):
    """length scales that grow with sqrt(d), as the distances in the unit cube do (tests/test_wide_dim_gpu.py)"""
    return np.concatenate(([0.0], -np.log(0.25 * np.sqrt(d) * (1.0 + np.arange(d) / d))))


def _data(env, n, d=D, seed=0):
    torch, gnp = env[0], env[1]
    rng = np.random.default_rng(1000 * n + seed)
    xi, xt = rng.random((n, d)), rng.random((M, d))
    zi = np.sin(3 * xi[:, 0]) + xi.sum(axis=1)
    return tuple(torch.as_tensor(a, device=gnp._dev()).contiguous() for a in (xi, zi, xt))


def _model(env, th, p=P, noise=False):
    from gpmp_amd.kernel import MaternCovariance

    return env[2].Model(None, MaternCovariance(p, noise=noise), None, th, "zero")


def _predict(model, X, Z, T):
    return tuple(model.predict(X, Z, T, convert_in=False, convert_out=False))


def _nll(model, X, Z):
    return float(model.negative_log_likelihood_zero_mean(model.covparam, X, Z))


def _composed_nll(env, model, X, Z):
    """what core/likelihood.py enqueued call by call before gpmp_whiten"""
    from gpmp_amd.core.linalg import covariance_factor

    gnp = env[1]
    F = covariance_factor(model, X, model.covparam)
    w = F.solve_lower(Z)
    norm2 = float(gnp.sum(w * w).item())
    return float(np.asarray(0.5 * (X.shape[0] * math.log(2.0 * math.pi) + F.logdet() + norm2), dtype=np.float64))


def _cold(env):
    torch, lib = env[0], env[3]
    torch.cuda.synchronize()
    assert lib.gpmp_device_release() == 0


def _same(env, a, b):
    torch = env[0]
    assert len(a) == len(b)
    for k, (u, v) in enumerate(zip(a, b)):
        if isinstance(u, float):
            assert u == v and math.isfinite(u), (k, u, v)
        else:
            assert len(u) == len(v) and all(torch.equal(s, t) for s, t in zip(u, v)), f"output {k} differs"


def _off_on(env, monkeypatch, seq, on_mb=ON_MB):
    """seq(): a list of outputs (floats, or tuples of tensors).  Store off, then on, from a cold library each; equal bit for bit."""
    monkeypatch.setenv("GPMP_FACTOR_STORE_MB", "0")
    _cold(env)
    off = seq()
    monkeypatch.setenv("GPMP_FACTOR_STORE_MB", on_mb)
    _cold(env)
    on = seq()
    _same(env, off, on)
    return on


def _launches(env, fn):
    """(result of fn(), launches of the diagonal-block kernel, launches of the Gram kernel) while fn runs"""
    torch, lib = env[0], env[3]
    torch.cuda.synchronize()
    lib.gpmp_profile_begin_kinds((1 << POTF2) | (1 << GRAM))
    try:
        r = fn()
        torch.cuda.synchronize()
    finally:
        table = (ctypes.c_double * 36)()
        lib.gpmp_profile_end(table)
    return r, int(table[3 * POTF2]), int(table[3 * GRAM])


@pytest.mark.parametrize("n,d", [(n, D) for n in SIZES] + [(640, 70)])
def test_predict_and_nll_in_either_order_bit_equal_with_and_without_the_store(env, monkeypatch, n, d):
    X, Z, T = _data(env, n, d)
    model = _model(env, _theta() if d == D else _theta_wide(d))

    def seq():
        r = [_predict(model, X, Z, T), _nll(model, X, Z)]
        _cold(env)
        r += [_nll(model, X, Z), _predict(model, X, Z, T)]
        _cold(env)
        r += [_nll(model, X, Z), _nll(model, X, Z)]
        return r

    on = _off_on(env, monkeypatch, seq)
    want = _composed_nll(env, model, X, Z)
    assert [on[1], on[2], on[4], on[5]] == [want] * 4
    _same(env, [on[0]], [on[3]])


@pytest.mark.parametrize("n", (640, 2304))
def test_nll_after_predict_neither_builds_nor_factors(env, monkeypatch, n):
    X, Z, T = _data(env, n)
    model = _model(env, _theta())
    got = {}
    for mb in ("0", ON_MB):
        monkeypatch.setenv("GPMP_FACTOR_STORE_MB", mb)
        _cold(env)
        _predict(model, X, Z, T)
        got[mb] = _launches(env, lambda: _nll(model, X, Z))
    assert got["0"][0] == got[ON_MB][0]
    assert got["0"][1] > 0 and got["0"][2] > 0, got
    assert got[ON_MB][1] == 0 and got[ON_MB][2] == 0, got


@pytest.mark.parametrize("n", SIZES)
def test_changed_points_or_parameters_are_not_served_from_the_store(env, monkeypatch, n):
    torch = env[0]
    X, Z, T = _data(env, n)
    th, th_b, th_n = _theta(), _theta(), _theta(noise=True)
    th_b[2] = np.nextafter(th_b[2], 1.0)
    base, other, p3, noisy = _model(env, th), _model(env, th_b), _model(env, th, p=3), _model(env, th_n, noise=True)
    x = X.clone()

    def seq():
        x.copy_(X)
        r = [_predict(base, x, Z, T), _nll(base, x, Z)]
        flat = x.view(-1)                           # one entry of xi moves by one ulp IN PLACE: same pointer, other contents
        flat[n + 1] = torch.nextafter(flat[n + 1], torch.full((), 2.0, dtype=torch.float64, device=flat.device))
        r += [_nll(base, x, Z)]
        x.copy_(X)
        r += [_nll(base, x, Z), _nll(other, x, Z), _nll(base, x, Z), _nll(p3, x, Z), _nll(base, x, Z), _nll(noisy, x, Z), _nll(base, x, Z)]
        return r

    on = _off_on(env, monkeypatch, seq)
    assert on[1] == on[3] == on[5] == on[7] == on[9] == _composed_nll(env, base, X, Z)
    for k, m in ((4, other), (6, p3), (8, noisy)):
        assert on[k] == _composed_nll(env, m, X, Z)
    assert len({on[1], on[6], on[8]}) == 3          # (p and the noise term move the value visibly; one ulp may round away)


def test_predict_by_another_schedule_is_a_miss_for_the_nll(env, monkeypatch):
    """n = 1100: inside the prediction's solve-goes-along window (2 * OUTER_BLOCKS * NB = 1024 < n <= 8192, linalg.hip), so its
    factorisation is the look-ahead one, while the plain potrf of n <= POTRF_ONE_STREAM_MAX = 2048 runs on one stream.  The two
    round differently: the NLL must factor for itself, and then finds its own factor again."""
    n = 1100
    X, Z, T = _data(env, n)
    model = _model(env, _theta())
    monkeypatch.setenv("GPMP_FACTOR_STORE_MB", "0")
    _cold(env)
    off = [_predict(model, X, Z, T), _nll(model, X, Z), _nll(model, X, Z), _predict(model, X, Z, T)]
    monkeypatch.setenv("GPMP_FACTOR_STORE_MB", ON_MB)
    _cold(env)
    on = [_predict(model, X, Z, T)]
    first, potf2_a, gram_a = _launches(env, lambda: _nll(model, X, Z))
    second, potf2_b, gram_b = _launches(env, lambda: _nll(model, X, Z))
    on += [first, second, _predict(model, X, Z, T)]
    _same(env, off, on)
    assert potf2_a > 0 and gram_a > 0                # a miss
    assert potf2_b == 0 and gram_b == 0              # a hit on the factor that miss published
    assert first == _composed_nll(env, model, X, Z)


@pytest.mark.parametrize("n", (640, 2304))
def test_not_positive_definite_raises_the_same_with_and_without_the_store(env, monkeypatch, n):
    torch, gnp = env[0], env[1]
    X, Z, T = _data(env, n)
    Xd = torch.cat((X[: n // 2], X[: n // 2]), dim=0).contiguous()          # duplicated points, huge length scales, no noise
    bad, good = _model(env, np.array([0.0, -30.0, -30.0, -30.0])), _model(env, _theta())

    def failure():
        with pytest.raises(gnp.HipLinAlgError) as e:
            _nll(bad, Xd, Z)
        return str(e.value)

    def seq():
        return [failure(), failure(), _nll(good, X, Z), failure(), _nll(good, X, Z)]

    monkeypatch.setenv("GPMP_FACTOR_STORE_MB", "0")
    _cold(env)
    off = seq()
    monkeypatch.setenv("GPMP_FACTOR_STORE_MB", ON_MB)
    _cold(env)
    on = seq()
    assert off == on
    assert on[0] == on[1] == on[3] and "not positive definite" in on[0] and "leading minor" in on[0] and "(potrf info=" in on[0]
    k = int(on[0].split("potrf info=")[1].rstrip(")"))
    assert 1 <= k <= n and f"leading minor {k} " in on[0]
    with pytest.raises(gnp.HipLinAlgError) as e:                              # the composition it replaces: same text, same minor
        _composed_nll(env, bad, Xd, Z)
    assert str(e.value) == on[0]
    assert on[2] == on[4] == _composed_nll(env, good, X, Z)


@pytest.mark.parametrize("n", SIZES)
def test_budget_below_the_factor_runs_in_the_workspace(env, monkeypatch, n):
    X, Z, T = _data(env, n)
    model = _model(env, _theta())
    low_mb = repr(8.0 * n * n / 2 ** 20 * 0.999)                           # just below 8 n^2 bytes
    low = _off_on(env, monkeypatch, lambda: [_predict(model, X, Z, T), _nll(model, X, Z), _nll(model, X, Z)], on_mb=low_mb)
    _, potf2, gram = _launches(env, lambda: _nll(model, X, Z))             # (still under low_mb)
    assert potf2 > 0 and gram > 0, low_mb                                  # nothing was kept: every call factors
    assert low[1] == low[2] == _composed_nll(env, model, X, Z)


@pytest.mark.parametrize("ncols", (1, 8, 16))
@pytest.mark.parametrize("n", (129, 1100, 2304))
def test_raw_entry_equals_potrf_trsm_logdet(env, monkeypatch, n, ncols):
    torch, gnp, _, lib = env
    from gpmp_amd import _lib
    from gpmp_amd.kernel import MaternCovariance

    X, Z, T = _data(env, n)
    th = _theta(noise=True)
    cov = MaternCovariance(P, noise=True)
    ldy = ncols + 3                                                        # ragged: not a multiple of anything
    rng = np.random.default_rng(n + ncols)
    Y0 = torch.as_tensor(rng.standard_normal((n, ldy)), device=X.device)
    dev = X.device

    def composed():
        K = cov.gram_lower(X, th)
        dinv = torch.empty(int(lib.gpmp_dinv_elems(n)), dtype=torch.float64, device=dev)
        info = torch.zeros(1, dtype=torch.int32, device=dev)
        Y, out = Y0.clone(), torch.empty(1, dtype=torch.float64, device=dev)
        _lib.check(lib.gpmp_potrf_lower_async(gnp._ptr(K), n, gnp._ld(K), gnp._ptr(dinv), gnp._ptr(info), gnp._stream()), "potrf")
        _lib.check(lib.gpmp_trsm_lower(gnp._ptr(K), n, gnp._ld(K), gnp._ptr(dinv), gnp._ptr(Y), ncols, ldy, 0, None, gnp._stream()), "trsm")
        _lib.check(lib.gpmp_logdet_chol(gnp._ptr(K), n, gnp._ld(K), gnp._ptr(out), gnp._stream()), "logdet")
        return Y, out, info

    def whiten():
        ws = torch.empty(int(lib.gpmp_whiten_ws_elems(n)), dtype=torch.float64, device=dev)
        info = torch.full((1,), 7, dtype=torch.int32, device=dev)         # the call clears it, on a hit too
        Y, out = Y0.clone(), torch.empty(1, dtype=torch.float64, device=dev)
        _lib.check(lib.gpmp_whiten(gnp._ptr(X), n, D, P, _lib.host_vec(th), 1, gnp._ptr(Y), ncols, ldy, gnp._ptr(ws), gnp._ptr(out),
                                   gnp._ptr(info), gnp._stream()), "gpmp_whiten")
        return Y, out, info

    want = composed()
    assert int(want[2].item()) == 0 and torch.equal(want[0][:, ncols:], Y0[:, ncols:]) and not torch.equal(want[0][:, :ncols], Y0[:, :ncols])
    for mb in ("0", ON_MB):
        monkeypatch.setenv("GPMP_FACTOR_STORE_MB", mb)
        _cold(env)
        for _ in range(2):                                                 # store on: a miss, then a hit
            _same(env, [want], [whiten()])
