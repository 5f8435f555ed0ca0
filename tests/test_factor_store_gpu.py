"""The factor store (GPMP_FACTOR_STORE_MB): gpmp_predict_zero_mean and gpmp_nll_zero_mean keep the Cholesky
factor of K(xi, xi; theta) in the library and reuse it when the points and parameters are bit for bit those of the stored factor.

Every check is a bit-for-bit comparison (torch.equal, NaN equal to NaN) with the same calls under GPMP_FACTOR_STORE_MB=0, where the
drivers factor in the caller's workspace on every call.  n = 129 (one ragged leaf), 640 (blocked, one stream), 1100 (ragged; the
prediction's solve runs along the look-ahead factorisation) and 2304 (look-ahead above POTRF_ONE_STREAM_MAX); m = 300, d = 3, p = 2."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

M, D, P = 300, 3, 2
SIZES = (129, 640, 1100, 2304)
ON_MB = "512"                          # 8 n^2 bytes are 42 MB at n = 2304


@pytest.fixture(scope="module")
def env():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import gpmp_amd.num as gnp
    from gpmp_amd import _lib

    lib = _lib.load()
    yield torch, gnp, _lib, lib
    lib.gpmp_device_release()


def _theta(noise=False, scale=0.4):
    return np.concatenate(([0.3], [-4.0] if noise else [], -np.log(scale + 0.3 * np.arange(D))))


def _data(env, n, seed=0):
    torch, gnp, _, _ = env
    rng = np.random.default_rng(1000 * n + seed)
    xi, xt = rng.random((n, D)), rng.random((M, D))
    zi = np.sin(3 * xi[:, 0]) + xi.sum(axis=1)
    return tuple(torch.as_tensor(a, device=gnp._dev()).contiguous() for a in (xi, zi, xt))


def _predict(env, X, Z, T, th, noise=0, p=P, stream=None):
    torch, gnp, _lib, lib = env
    n, m = X.shape[0], T.shape[0]
    ws = torch.empty(int(lib.gpmp_predict_ws_elems(n, m)), dtype=torch.float64, device=X.device)
    zpm, zpv = (torch.empty(m, dtype=torch.float64, device=X.device) for _ in range(2))
    info = torch.zeros(1, dtype=torch.int32, device=X.device)
    _lib.check(lib.gpmp_predict_zero_mean(gnp._ptr(X), gnp._ptr(Z), gnp._ptr(T), n, m, D, p, _lib.host_vec(th), noise, 1, gnp._ptr(ws),
                                          gnp._ptr(zpm), gnp._ptr(zpv), gnp._ptr(info), gnp._stream() if stream is None else stream),
               "gpmp_predict_zero_mean")
    return zpm, zpv, info


def _nll(env, X, Z, th, noise=0, p=P):
    torch, gnp, _lib, lib = env
    n = X.shape[0]
    ws = torch.empty(int(lib.gpmp_nll_ws_elems(n)), dtype=torch.float64, device=X.device)
    out = torch.empty(1, dtype=torch.float64, device=X.device)
    info = torch.zeros(1, dtype=torch.int32, device=X.device)
    _lib.check(lib.gpmp_nll_zero_mean(gnp._ptr(X), gnp._ptr(Z), n, D, p, _lib.host_vec(th), noise, gnp._ptr(ws), gnp._ptr(out),
                                      gnp._ptr(info), gnp._stream()), "gpmp_nll_zero_mean")
    return out, info


def _same(env, a, b):
    torch = env[0]
    assert len(a) == len(b)
    for k, (u, v) in enumerate(zip(a, b)):
        assert torch.equal(torch.nan_to_num(u.double(), nan=1.25e300), torch.nan_to_num(v.double(), nan=1.25e300)) and \
            torch.equal(torch.isnan(u.double()), torch.isnan(v.double())), f"output {k} differs"


def _both(env, monkeypatch, calls):
    """`calls`: functions without arguments, each one driver call returning its outputs.  They run in order with the store off, then
    in the same order with the store on; every output must agree bit for bit.  Returns the outputs of the second pass."""
    monkeypatch.setenv("GPMP_FACTOR_STORE_MB", "0")
    off = [c() for c in calls]
    monkeypatch.setenv("GPMP_FACTOR_STORE_MB", ON_MB)
    on = [c() for c in calls]
    for k, (a, b) in enumerate(zip(off, on)):
        _same(env, a, b)
    return on


@pytest.mark.parametrize("n", SIZES)
def test_predict_nll_predict_bit_equal_with_and_without_the_store(env, monkeypatch, n):
    X, Z, T = _data(env, n)
    th = _theta()
    out = _both(env, monkeypatch, [lambda: _predict(env, X, Z, T, th), lambda: _nll(env, X, Z, th), lambda: _predict(env, X, Z, T, th)])
    assert all(int(o[-1].item()) == 0 for o in out)
    _same(env, out[0], out[2])                      # the miss and the hit


@pytest.mark.parametrize("n", SIZES)
def test_every_change_of_the_key_is_a_miss(env, monkeypatch, n):
    torch = env[0]
    X, Z, T = _data(env, n)
    X2, Z2, T2 = _data(env, 257, seed=1)
    th, th_b, th_n = _theta(), _theta(), _theta(noise=True)
    th_b[2] = np.nextafter(th_b[2], 1.0)
    state = {"x": X.clone()}

    def bump():                                     # one entry of xi moves by one ulp IN PLACE: same pointer, other contents
        flat = state["x"].view(-1)
        flat[n + 1] = torch.nextafter(flat[n + 1], torch.ones((), dtype=torch.float64, device=flat.device) * 2)

    def restore():
        state["x"].copy_(X)

    def seq():
        x = state["x"]
        r = [_predict(env, x, Z, T, th), _nll(env, x, Z, th)]
        bump()
        r += [_predict(env, x, Z, T, th), _nll(env, x, Z, th)]
        restore()
        r += [_nll(env, x, Z, th), _nll(env, x, Z, th_b), _predict(env, x, Z, T, th_b)]             # one theta component, one ulp
        r += [_predict(env, x, Z, T, th_n, noise=1), _nll(env, x, Z, th_n, noise=1), _nll(env, x, Z, th)]   # the noise term on, off
        r += [_nll(env, x, Z, th, p=3), _predict(env, x, Z, T, th, p=3), _predict(env, x, Z, T, th)]         # p
        r += [_predict(env, X2, Z2, T2, th), _nll(env, x, Z, th), _nll(env, X2, Z2, th), _predict(env, x, Z, T, th)]   # n, and back
        return r

    monkeypatch.setenv("GPMP_FACTOR_STORE_MB", "0")
    off = seq()
    monkeypatch.setenv("GPMP_FACTOR_STORE_MB", ON_MB)
    on = seq()
    for a, b in zip(off, on):
        _same(env, a, b)
    assert all(int(o[-1].item()) == 0 for o in on)


@pytest.mark.parametrize("n", SIZES)
def test_new_observations_and_new_prediction_points_hit_without_going_stale(env, monkeypatch, n):
    torch = env[0]
    X, Z, T = _data(env, n)
    th = _theta()
    Z2 = torch.cos(Z)
    T2 = torch.flip(T, dims=(0,)).contiguous() * 0.5
    out = _both(env, monkeypatch, [lambda: _predict(env, X, Z, T, th), lambda: _predict(env, X, Z2, T, th), lambda: _nll(env, X, Z2, th),
                                   lambda: _predict(env, X, Z, T2, th), lambda: _nll(env, X, Z, th), lambda: _predict(env, X.clone(), Z, T, th)])
    assert not torch.equal(out[0][0], out[1][0]) and not torch.equal(out[2][0], out[4][0])
    _same(env, out[0], out[5])                      # the same points in another buffer


@pytest.mark.parametrize("n", (640, 2304))
def test_failed_factorisation_is_reported_the_same_and_leaves_no_entry(env, monkeypatch, n):
    torch, gnp = env[0], env[1]
    X, Z, T = _data(env, n)
    Xd = torch.cat((X[: n // 2], X[: n // 2]), dim=0).contiguous()          # duplicated points, huge length scales, no noise
    th_bad = np.array([0.0, -30.0, -30.0, -30.0])
    th = _theta()
    calls = [lambda: _predict(env, Xd, Z, T, th_bad), lambda: _predict(env, Xd, Z, T, th_bad), lambda: _nll(env, Xd, Z, th_bad),
             lambda: _nll(env, Xd, Z, th_bad), lambda: _predict(env, X, Z, T, th), lambda: _nll(env, X, Z, th)]
    out = _both(env, monkeypatch, calls)
    for o in out[:4]:
        assert int(o[-1].item()) > 0
    assert bool(torch.isnan(out[1][0]).all()) and bool(torch.isinf(out[3][0]).all())
    assert int(out[4][-1].item()) == 0 and int(out[5][-1].item()) == 0


@pytest.mark.parametrize("n", SIZES)
def test_budget_below_the_factor_runs_in_the_workspace(env, monkeypatch, n):
    lib = env[3]
    X, Z, T = _data(env, n)
    th = _theta()
    monkeypatch.setenv("GPMP_FACTOR_STORE_MB", "0")
    off = [_predict(env, X, Z, T, th), _nll(env, X, Z, th), _predict(env, X, Z, T, th)]
    monkeypatch.setenv("GPMP_FACTOR_STORE_MB", repr(8.0 * n * n / 2 ** 20 * 0.999))       # just below 8 n^2 bytes
    low = [_predict(env, X, Z, T, th), _nll(env, X, Z, th), _predict(env, X, Z, T, th)]
    for a, b in zip(off, low):
        _same(env, a, b)


def test_release_returns_the_store_and_the_next_call_works(env, monkeypatch):
    torch, _, _, lib = env
    monkeypatch.setenv("GPMP_FACTOR_STORE_MB", ON_MB)
    torch.cuda.synchronize()
    assert lib.gpmp_device_release() == 0
    before = lib.gpmp_device_state_count()
    X, Z, T = _data(env, 2304)
    th = _theta()
    free = []
    for _ in range(3):                               # miss, hit, release: the first round also warms the runtime's own pools
        a = _predict(env, X, Z, T, th)
        b = _predict(env, X, Z, T, th)
        assert lib.gpmp_device_state_count() == before + 1
        _same(env, a, b)
        torch.cuda.synchronize()
        assert lib.gpmp_device_release() == 0
        assert lib.gpmp_device_state_count() == before
        free.append(torch.cuda.mem_get_info()[0])
    assert free[2] >= free[1] - (8 << 20), free      # the 51 MB of the entry do not add up from round to round
    c = _predict(env, X.clone(), Z, T, th)           # the next call works: a miss into a fresh store
    _same(env, a, c)


@pytest.mark.parametrize("n", (1100, 2304))
def test_miss_on_one_stream_then_hit_on_another(env, monkeypatch, n):
    """A miss enqueued on stream A and, at once, a hit on stream B (no host synchronise in between besides the hit's own read of
    the flag word): B orders itself behind the factorisation through the entry's event."""
    torch = env[0]
    X, Z, T = _data(env, n)
    th = _theta()
    monkeypatch.setenv("GPMP_FACTOR_STORE_MB", "0")
    ref = _predict(env, X, Z, T, th)
    torch.cuda.synchronize()
    monkeypatch.setenv("GPMP_FACTOR_STORE_MB", ON_MB)
    env[3].gpmp_device_release()
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    with torch.cuda.stream(sa):
        a = _predict(env, X, Z, T, th, stream=sa.cuda_stream)
    with torch.cuda.stream(sb):
        b = _predict(env, X, Z, T, th, stream=sb.cuda_stream)
    with torch.cuda.stream(sa):                       # and a miss that has to wait for the reader on B before it overwrites
        X3 = X * 0.5
        c = _predict(env, X3, Z, T, th, stream=sa.cuda_stream)
    torch.cuda.synchronize()
    _same(env, ref, a)
    _same(env, ref, b)
    monkeypatch.setenv("GPMP_FACTOR_STORE_MB", "0")
    _same(env, _predict(env, X3, Z, T, th), c)
