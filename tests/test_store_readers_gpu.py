"""The factor store (GPMP_FACTOR_STORE_MB) through the four readers that carry a mean: gpmp_predict_mean,
gpmp_predict_grad, gpmp_reml and gpmp_posterior_weights (include/gpmp_hip.h), called through ctypes on device tensors.

Every comparison between two calls is bit for bit (torch.equal, NaN equal to NaN), info word included: a call sequence from a cold
library under GPMP_FACTOR_STORE_MB=0, where every call factors in its workspace, against the same sequence from a cold library with
the store on.  Whether a call was a hit is read from the launch counts of the diagonal-block and the Gram kernel (gpmp_profile_end).
Inputs as tests/test_factor_store_gpu.py: n = 129 (one ragged leaf), 640 (blocked, one stream), 1100 (ragged; with more than
TRSV_FEW_MAX = 16 columns the solve runs along the look-ahead factorisation) and 2304 (above POTRF_ONE_STREAM_MAX = 2048); m = 300,
d = 3, p = 2; mean designs q = 1 (constant), q = 4 (linear in d = 3) and q = 10 (linear in d = 9: [z, P] is 11 columns, two passes of
the few-column sweep); one case d = 70 (the wide Gram route) and one noisy case.

The route in the key (factor_route, linalg.hip): 1 when n > POTRF_ONE_STREAM_MAX, or when 1024 < n <= 8192 and the solve has more
than 16 columns (mb = m + 1 + q rounded up to even); 0 otherwise.  gpmp_reml, gpmp_posterior_weights and gpmp_whiten carry the plain
factorisation's route (mb = 0).  At n = 640 and 2304 every reader shares one factor; at n = 1100 a prediction shares with them only
when mb <= 16."""
import copy
import math

import numpy as np
import pytest
import scipy.linalg as sla

from . import posterior_mean_numpy as pmn
from . import predict_grad_numpy as pgn
from .test_c_abi_mean_drivers_gpu import _Call
from .test_factor_store_gpu import _predict as _predict_zero_mean
from .test_nll_store_gpu import _cold, _data, _launches, _theta, _theta_wide    # (_data as test_factor_store_gpu's, with d)
from .test_posterior_mean_multi_gpu import _c_weights_multi

pytestmark = pytest.mark.gpu

M, D, P = 300, 3, 2
SIZES = (129, 640, 1100, 2304)
ON_MB = "512"                          # 8 n^2 bytes are 42 MB at n = 2304
# (n, q, d, noise): every size with both designs, then the single cases
MEAN_CASES = [(n, q, D, 0) for n in SIZES for q in (1, 4)] + [(640, 10, 9, 0), (640, 4, 70, 0), (640, 4, D, 1)]
ANY_CASES = [(n, q, D, 0) for n in SIZES for q in (0, 1, 4)] + [(640, 10, 9, 0), (640, 4, 70, 0), (640, 4, D, 1)]


@pytest.fixture(scope="module")
def env():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import gpmp_amd.num as gnp
    from gpmp_amd import _lib

    lib = _lib.load()
    yield torch, gnp, _lib, lib
    torch.cuda.synchronize()
    lib.gpmp_device_release()


def _design(torch, x, q, kind="lin"):
    """(design, its Jacobian) on the device.  lin: [1, x_1 .. x_{q-1}];  alt: the same with 1 + x_1 as its first column;  dup: the
    last column repeats x_1 (a rank-deficient design)."""
    if q == 0:
        return None, None
    m, d = x.shape
    ncoord = q - 2 if kind == "dup" else q - 1
    cols = [torch.ones((m, 1), dtype=torch.float64, device=x.device), x[:, :ncoord]]
    J = torch.zeros((m, q, d), dtype=torch.float64, device=x.device)
    for a in range(ncoord):
        J[:, 1 + a, a] = 1.0
    if kind == "dup":
        cols.append(x[:, :1])
        J[:, q - 1, 0] = 1.0
    Pm = torch.cat(cols, dim=1).contiguous()
    if kind == "alt":
        Pm[:, 0] += x[:, 0]
        J[:, 0, 0] = 1.0
    assert Pm.shape == (m, q)
    return Pm, J


class _Case:
    """Device inputs of one problem and the drivers as methods; but() gives a copy with some inputs replaced."""

    def __init__(self, env, n, q=0, d=D, noise=0, p=P, m=M, seed=0, kind="lin"):
        self.env = env
        self.X, self.Z, T = _data(env, n, d, seed)
        self.T = T[:m].contiguous()
        self.q, self.noise, self.p, self.kind = q, noise, p, kind
        self.th = _theta(noise=bool(noise)) if d == D else _theta_wide(d)
        self._designs()

    def _designs(self):
        torch = self.env[0]
        self.Pi, _ = _design(torch, self.X, self.q, self.kind)
        self.Pt, self.J = _design(torch, self.T, self.q, self.kind)

    def but(self, **over):
        c = copy.copy(self)
        for k, v in over.items():
            assert hasattr(c, k), k
            setattr(c, k, v)
        c._designs()
        return c

    @property
    def n(self):
        return self.X.shape[0]

    def _common(self, stream):
        torch, gnp, _lib, _ = self.env
        new = lambda *shape: torch.empty(shape, dtype=torch.float64, device=self.X.device)  # noqa: E731
        info = torch.full((1,), 7, dtype=torch.int32, device=self.X.device)       # every call clears it, on a hit too
        return gnp._ptr, new, info, (gnp._stream() if stream is None else stream.cuda_stream), _lib.host_vec(self.th)

    def predict_mean(self, stream=None):
        _, _, _lib, lib = self.env
        ptr, new, info, st, th = self._common(stream)
        (n, d), m, q = self.X.shape, self.T.shape[0], self.q
        ws, zpm, zpv = new(int(lib.gpmp_predict_mean_ws_elems(n, m, q))), new(m), new(m)
        _lib.check(lib.gpmp_predict_mean(ptr(self.X), ptr(self.Z), ptr(self.Pi), q, ptr(self.T), ptr(self.Pt), q, n, m, d, q, self.p, th,
                                         self.noise, 1, ptr(ws), ptr(zpm), ptr(zpv), ptr(info), st), "gpmp_predict_mean")
        return zpm, zpv, info

    def predict_grad(self, variance=1, stream=None):
        _, _, _lib, lib = self.env
        ptr, new, info, st, th = self._common(stream)
        (n, d), m, q = self.X.shape, self.T.shape[0], self.q
        ws = new(int(lib.gpmp_predict_grad_ws_elems(n, m, d, q)))
        zpm, zpv, gzpm, gzpv = new(m), new(m), new(m, d), (new(m, d) if variance else None)
        _lib.check(lib.gpmp_predict_grad(ptr(self.X), ptr(self.Z), ptr(self.Pi), q, ptr(self.T), ptr(self.Pt), q, ptr(self.J), n, m, d, q,
                                         self.p, th, self.noise, 1, variance, ptr(ws), ptr(zpm), ptr(zpv), ptr(gzpm), ptr(gzpv), ptr(info),
                                         st), "gpmp_predict_grad")
        return (zpm, zpv, gzpm, gzpv, info) if variance else (zpm, zpv, gzpm, info)

    def predict_grad_mean_only(self, stream=None):
        return self.predict_grad(0, stream)

    def reml(self, stream=None):
        _, _, _lib, lib = self.env
        ptr, new, info, st, th = self._common(stream)
        (n, d), q = self.X.shape, self.q
        ws, val = new(int(lib.gpmp_reml_ws_elems(n, q))), new(1)
        _lib.check(lib.gpmp_reml(ptr(self.X), ptr(self.Z), ptr(self.Pi), max(q, 1), n, d, q, self.p, th, self.noise, ptr(ws), ptr(val),
                                 ptr(info), st), "gpmp_reml")
        return val, info

    def weights(self, stream=None):
        _, _, _lib, lib = self.env
        ptr, new, info, st, th = self._common(stream)
        (n, d), q = self.X.shape, self.q
        ws, alpha, beta = new(int(lib.gpmp_posterior_weights_ws_elems(n, q))), new(n), (new(q) if q else None)
        _lib.check(lib.gpmp_posterior_weights(ptr(self.X), ptr(self.Z), ptr(self.Pi), q, n, d, q, self.p, th, self.noise, ptr(ws),
                                              ptr(alpha), ptr(beta), ptr(info), st), "gpmp_posterior_weights")
        return (alpha, beta, info) if q else (alpha, info)

    def predict_zero_mean(self):
        assert self.X.shape[1] == D
        return _predict_zero_mean(self.env, self.X, self.Z, self.T, self.th, noise=self.noise, p=self.p)

    def whiten(self, Y0, ncols, stream=None):
        _, _, _lib, lib = self.env
        ptr, new, info, st, th = self._common(stream)
        n, d = self.X.shape
        ws, out, Y = new(int(lib.gpmp_whiten_ws_elems(n))), new(1), Y0.clone()
        _lib.check(lib.gpmp_whiten(ptr(self.X), n, d, self.p, th, self.noise, ptr(Y), ncols, Y.shape[1], ptr(ws), ptr(out), ptr(info), st),
                   "gpmp_whiten")
        return Y, out, info

    # the drivers that do not go through the store, by the helpers of their own tests (fresh device copies of the same numbers)
    def _host(self, t):
        return None if t is None else t.cpu().numpy()

    def _bypassing_call(self):
        return _Call(self.env, self._host(self.X), self._host(self.Z), self._host(self.Pi), self.p, noise=self.noise)

    def bypassing(self):
        """gpmp_nll_grad, gpmp_loo and gpmp_posterior_weights_multi (two observation columns), one after the other"""
        torch, gnp, _lib, _ = self.env
        call = self._bypassing_call()
        infos = [call.value_grad(self.th)[-1], call.loo(self.th)[-1]]
        Zs = np.stack((self._host(self.Z), np.cos(self._host(self.Z))), axis=1)
        infos.append(_c_weights_multi((None, gnp, _lib, torch), self._host(self.X), Zs, self.p, self.th, self.noise, self._host(self.Pi))[-1])
        assert infos == [0, 0, 0]

    def nll_grad_value(self):
        v, _, info = self._bypassing_call().value_grad(self.th)
        return v, info


READERS = ("predict_mean", "predict_grad", "predict_grad_mean_only", "reml", "weights")


def _same(env, a, b, what=""):
    torch = env[0]
    assert len(a) == len(b), what
    for k, (u, v) in enumerate(zip(a, b)):
        u, v = u.double(), v.double()
        assert u.shape == v.shape and torch.equal(torch.isnan(u), torch.isnan(v)) and \
            torch.equal(torch.nan_to_num(u, nan=1.25e300), torch.nan_to_num(v, nan=1.25e300)), f"{what}: output {k} differs"


def _all_same(env, off, on):
    assert len(off) == len(on)
    for k, (a, b) in enumerate(zip(off, on)):
        _same(env, a, b, f"call {k}, store off against store on")


def _off_on(env, monkeypatch, seq):
    """seq(): a list of driver outputs (tuples of tensors).  From a cold library with the store off, then from a cold library with the
    store on; every output agrees bit for bit.  Returns the outputs of the second pass."""
    monkeypatch.setenv("GPMP_FACTOR_STORE_MB", "0")
    _cold(env)
    off = seq()
    monkeypatch.setenv("GPMP_FACTOR_STORE_MB", ON_MB)
    _cold(env)
    on = seq()
    _all_same(env, off, on)
    return on


def _info(out):
    return int(out[-1].item())


def _counted(env, counts, fn):
    """fn() with its launches of the diagonal-block kernel appended to counts"""
    r, potf2, _ = _launches(env, fn)
    counts.append(potf2)
    return r


def _factored(counts, want):
    """counts against a pattern: True -- the call factored, False -- it did not, None -- either"""
    assert len(counts) == len(want)
    for k, (c, w) in enumerate(zip(counts, want)):
        assert w is None or (c > 0) == w, (k, counts, want)


# ---- 1. each reader: store on equals store off, a hit equals its miss, a hit reads the new observations ------------------------

# (gpmp_predict_mean takes q >= 1; its q = 0 is gpmp_predict_zero_mean: tests/test_factor_store_gpu.py)
@pytest.mark.parametrize("reader,n,q,d,noise", [(r,) + c for r in READERS for c in (MEAN_CASES if r == "predict_mean" else ANY_CASES)])
def test_miss_hit_and_hit_with_new_observations(env, monkeypatch, reader, n, q, d, noise):
    torch = env[0]
    c = _Case(env, n, q, d, noise)
    c3 = c.but(Z=torch.cos(c.Z), T=(torch.flip(c.T, dims=(0,)) * 0.5).contiguous())
    on = _off_on(env, monkeypatch, lambda: [getattr(c, reader)(), getattr(c, reader)(), getattr(c3, reader)()])
    assert all(_info(o) == 0 for o in on)
    _same(env, on[0], on[1], "the miss and the hit")
    for k, (a, b) in enumerate(zip(on[0][:-1], on[2][:-1])):      # nothing stale: every output follows the new zi (and xt)
        assert not torch.equal(a, b), (reader, k)


# ---- 2. hits really are hits -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("reader", ("predict_mean", "predict_grad", "reml", "weights"))
@pytest.mark.parametrize("n", (640, 2304))
def test_second_identical_call_neither_factors_nor_builds_k(env, monkeypatch, reader, n):
    c = _Case(env, n, 1)
    got = {}
    for mb in ("0", ON_MB):
        monkeypatch.setenv("GPMP_FACTOR_STORE_MB", mb)
        _cold(env)
        first = getattr(c, reader)()
        second, potf2, gram = _launches(env, getattr(c, reader))
        _same(env, first, second)
        got[mb] = (second, potf2, gram)
    _same(env, got["0"][0], got[ON_MB][0])
    assert got["0"][1] > 0 and got["0"][2] > 0, got
    assert got[ON_MB][1] == 0, got
    if reader in ("reml", "weights"):
        assert got[ON_MB][2] == 0, got
    else:                                              # K(xi, xt) is still built, K(xi, xi) is not
        assert got[ON_MB][2] < got["0"][2], got


# ---- 3. cross-driver sharing follows the route -------------------------------------------------------------------------------

@pytest.mark.parametrize("n", (640, 2304))
def test_one_factor_serves_every_reader(env, monkeypatch, n):
    torch = env[0]
    c1, c4 = _Case(env, n, 1), _Case(env, n, 4)
    Y0 = torch.as_tensor(np.random.default_rng(n).standard_normal((n, 5)), device=c1.X.device)
    counts = []

    def seq():
        del counts[:]
        calls = (c1.predict_zero_mean, c1.predict_mean, c4.predict_grad, c4.reml, c1.weights, lambda: c1.whiten(Y0, 3))
        return [_counted(env, counts, f) for f in calls]

    on = _off_on(env, monkeypatch, seq)
    assert all(_info(o) == 0 for o in on)
    _factored(counts, [True, False, False, False, False, False])


def test_solve_along_route_keeps_its_factor_to_itself(env, monkeypatch):
    """n = 1100, m = 300: the prediction factors along the look-ahead schedule (route 1), gpmp_reml by the plain one-stream potrf
    (route 0).  Neither may read the other's factor: each factors once, the second replaces the first."""
    c = _Case(env, 1100, 1)
    counts = []

    def seq():
        del counts[:]
        calls = (c.predict_mean, c.reml, c.reml, c.predict_mean, c.predict_grad, c.weights, c.predict_grad)
        return [_counted(env, counts, f) for f in calls]

    on = _off_on(env, monkeypatch, seq)
    assert all(_info(o) == 0 for o in on)
    _factored(counts, [True, True, False, True, False, True, True])
    _same(env, on[0], on[3])
    _same(env, on[4], on[6])


@pytest.mark.parametrize("m,shares", [(14, True), (15, False)])
def test_few_column_prediction_shares_with_reml_at_the_threshold(env, monkeypatch, m, shares):
    """n = 1100, q = 1: m = 14 gives mb = 16 = TRSV_FEW_MAX columns, the few-column sweep behind the plain factorisation (route 0, as
    gpmp_reml); m = 15 gives 17 columns, padded to 18, and the solve goes along (route 1)."""
    c = _Case(env, 1100, 1, m=m)
    counts = []

    def seq():
        del counts[:]
        return [_counted(env, counts, f) for f in (c.predict_mean, c.reml, c.predict_mean, c.weights)]

    on = _off_on(env, monkeypatch, seq)
    assert all(_info(o) == 0 for o in on)
    _factored(counts, [True, False, False, False] if shares else [True, True, True, True])
    _same(env, on[0], on[2])


# ---- 4. every change of the key is a miss ------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", SIZES)
def test_every_change_of_the_key_is_a_miss_through_the_mean_drivers(env, monkeypatch, n):
    """The sequence of tests/test_factor_store_gpu.py with gpmp_predict_mean and gpmp_reml, and two changes of the mean design, which
    may hit (the factor does not depend on P) and must follow the new design all the same."""
    torch = env[0]
    base = _Case(env, n, 1)
    x = base.X.clone()
    c = base.but(X=x)
    th_b = base.th.copy()
    th_b[2] = np.nextafter(th_b[2], 1.0)
    cb, cn, c3 = c.but(th=th_b), c.but(th=_theta(noise=True), noise=1), c.but(p=3)
    other = _Case(env, 257, 1, seed=1)
    counts = []
    want = []

    def run(f, factored):
        want.append(factored)
        return _counted(env, counts, f)

    def seq():
        del counts[:], want[:]
        x.copy_(base.X)
        r = [run(c.predict_mean, True), run(c.reml, n == 1100)]
        flat = x.view(-1)                                # one entry of xi moves by one ulp IN PLACE: same pointer, other contents
        flat[n + 1] = torch.nextafter(flat[n + 1], torch.full((), 2.0, dtype=torch.float64, device=flat.device))
        r += [run(c.predict_mean, True), run(c.reml, n == 1100)]
        x.copy_(base.X)
        r += [run(c.reml, True), run(cb.reml, True), run(cb.predict_mean, n == 1100)]                 # one theta component, one ulp
        r += [run(cn.predict_mean, True), run(cn.reml, n == 1100), run(c.reml, True)]                # the noise term on, off
        r += [run(c3.reml, True), run(c3.predict_mean, n == 1100), run(c.predict_mean, True)]        # p
        r += [run(other.predict_mean, True), run(c.reml, True), run(other.reml, True), run(c.predict_mean, True)]   # n, and back
        r += [run(c.but(q=4).predict_mean, None), run(c.predict_mean, None), run(c.but(q=4).reml, None), run(c.reml, None)]      # q
        r += [run(c.but(kind="alt").predict_mean, None), run(c.but(kind="alt").reml, None), run(c.predict_mean, None)]   # Pi, same q
        return r

    on = _off_on(env, monkeypatch, seq)
    assert all(_info(o) == 0 for o in on)
    _factored(counts, want)
    _same(env, on[0], on[12])
    _same(env, on[0], on[18])
    _same(env, on[0], on[23])
    assert not torch.equal(on[17][0], on[0][0]) and not torch.equal(on[19][0], on[1][0])              # the new q shows
    assert not torch.equal(on[21][0], on[0][0]) and not torch.equal(on[22][0], on[1][0])              # the new Pi shows


# ---- 5. the drivers that do not go through the store ---------------------------------------------------------------------------

@pytest.mark.parametrize("n", (640, 2304))
def test_bypassing_drivers_leave_the_entry_valid(env, monkeypatch, n):
    c = _Case(env, n, 4)
    monkeypatch.setenv("GPMP_FACTOR_STORE_MB", "0")
    _cold(env)
    off = c.predict_mean()
    monkeypatch.setenv("GPMP_FACTOR_STORE_MB", ON_MB)
    _cold(env)
    first = c.predict_mean()
    c.bypassing()                                      # gpmp_nll_grad, gpmp_loo, gpmp_posterior_weights_multi on the same (xi, theta)
    last, potf2, _ = _launches(env, c.predict_mean)
    assert potf2 == 0
    _same(env, first, last)
    _same(env, off, last)


@pytest.mark.parametrize("n,q", [(640, 0), (640, 1), (640, 4), (2304, 4)])
def test_nll_grad_publishes_nothing_and_reml_returns_its_value(env, monkeypatch, n, q):
    c = _Case(env, n, q)
    values = {}
    for mb in ("0", ON_MB):
        monkeypatch.setenv("GPMP_FACTOR_STORE_MB", mb)
        _cold(env)
        counts = []
        v, info = _counted(env, counts, c.nll_grad_value)
        miss = _counted(env, counts, c.reml)
        hit = _counted(env, counts, c.reml)
        v2, info2 = _counted(env, counts, c.nll_grad_value)
        _factored(counts, [True, True, mb == "0", True])
        assert info == 0 and info2 == 0 and _info(miss) == 0 and _info(hit) == 0
        values[mb] = [v, float(miss[0].item()), float(hit[0].item()), v2]
    assert math.isfinite(values["0"][0])
    assert values["0"] == [values["0"][0]] * 4 and values[ON_MB] == values["0"], values


# ---- 6. failure conventions on a hit -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", (640, 2304))
def test_rank_deficient_design_on_a_hit(env, monkeypatch, n):
    """A valid factor is in the store; a duplicated mean column is reported as info = n + k, with the outputs of the store-off call,
    and the factor stays: the next sound call hits."""
    torch = env[0]
    good = _Case(env, n, 4)
    bad = good.but(q=5, kind="dup")
    counts = []

    def seq():
        del counts[:]
        calls = (good.predict_zero_mean, bad.reml, bad.weights, bad.predict_mean, bad.predict_grad, good.reml, good.weights,
                 good.predict_mean, good.predict_grad)
        return [_counted(env, counts, f) for f in calls]

    on = _off_on(env, monkeypatch, seq)
    _factored(counts, [True] + [False] * 8)
    for o in on[1:5]:
        assert n < _info(o) <= n + 5, _info(o)
    assert bool(torch.isinf(on[1][0]).all()) and bool((on[1][0] > 0).all())
    for o in on[2:5]:
        assert all(bool(torch.isnan(t).all()) for t in o[:-1])
    assert all(_info(o) == 0 for o in on[5:])


@pytest.mark.parametrize("reader", ("predict_mean", "predict_grad", "reml", "weights"))
@pytest.mark.parametrize("n", (640, 2304))
def test_failed_factorisation_is_reported_the_same_and_leaves_no_entry(env, monkeypatch, reader, n):
    torch = env[0]
    good = _Case(env, n, 1)
    Xd = torch.cat((good.X[: n // 2], good.X[: n // 2]), dim=0).contiguous()          # duplicated points, huge length scales, no noise
    bad = good.but(X=Xd, th=np.array([0.0, -30.0, -30.0, -30.0]))
    counts = []

    def seq():
        del counts[:]
        return [_counted(env, counts, f) for f in (getattr(bad, reader), getattr(bad, reader), getattr(good, reader), getattr(good, reader))]

    on = _off_on(env, monkeypatch, seq)
    _factored(counts, [True, True, True, False])         # the failed factor is never read: the second call factors again
    assert 0 < _info(on[0]) <= n and _info(on[1]) == _info(on[0])
    _same(env, on[0], on[1])
    for t in on[0][:-1]:
        assert bool(torch.isinf(t).all()) if reader == "reml" else bool(torch.isnan(t).all())
    assert _info(on[2]) == 0 and _info(on[3]) == 0
    _same(env, on[2], on[3])


# ---- 7. two hits side by side --------------------------------------------------------------------------------------------------

def test_two_hits_side_by_side_behind_a_miss_on_another_stream(env, monkeypatch):
    """A miss by gpmp_predict_grad enqueued on stream A; at once the same call on stream B with its own workspace and a
    gpmp_posterior_weights on A, both reading the factor the miss is still producing; one synchronise at the end."""
    torch = env[0]
    c = _Case(env, 2304, 1)
    monkeypatch.setenv("GPMP_FACTOR_STORE_MB", "0")
    _cold(env)
    ref_g, ref_w = c.predict_grad(), c.weights()
    monkeypatch.setenv("GPMP_FACTOR_STORE_MB", ON_MB)
    _cold(env)
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    with torch.cuda.stream(sa):
        a = c.predict_grad(stream=sa)
    with torch.cuda.stream(sb):
        b = c.predict_grad(stream=sb)
    with torch.cuda.stream(sa):
        w = c.weights(stream=sa)
    torch.cuda.synchronize()
    _same(env, ref_g, a)
    _same(env, ref_g, b)
    _same(env, ref_w, w)


# ---- 8. right, not only consistent -----------------------------------------------------------------------------------------------

def _reml_numpy(xi, zi, p, theta, noise, Pi):
    """The restricted likelihood of gpmp/core/likelihood.py in float64: contrasts W (an orthonormal basis of the null space of P^T,
    from a complete QR), G = W^T K W = C C^T, 0.5 ((n - q) ln 2 pi + ln|G| + (W^T z)^T G^-1 (W^T z)); q = 0: W = I."""
    K = pmn.gram(xi, p, theta, noise)
    n = len(zi)
    q = 0 if Pi is None else Pi.shape[1]
    G, wz = K, zi
    if q:
        W = np.linalg.qr(Pi, mode="complete")[0][:, q:]
        G, wz = W.T @ K @ W, W.T @ zi
    C = np.linalg.cholesky(G)
    u = sla.solve_triangular(C, wz, lower=True)
    return 0.5 * ((n - q) * math.log(2.0 * math.pi) + 2.0 * np.sum(np.log(np.diag(C))) + u @ u)


@pytest.fixture(scope="module")
def numpy_reference():
    """per (n, q): the restatements' outputs, computed once"""
    cache = {}

    def get(c):
        key = (c.n, c.q)
        if key not in cache:
            h = c._host
            xi, zi, xt, Pi, Pt, J = h(c.X), h(c.Z), h(c.T), h(c.Pi), h(c.Pt), h(c.J)
            cache[key] = dict(xi=xi, zi=zi, grad=pgn.predict_grad(xi, zi, xt, c.p, c.th, c.noise, Pi, Pt, J),
                              weights=pmn.weights(xi, zi, c.p, c.th, c.noise, Pi), reml=_reml_numpy(xi, zi, c.p, c.th, c.noise, Pi),
                              tol=pmn.tolerance(xi, c.p, c.th, c.noise))
        return cache[key]

    return get


def _from_a_hit(env, monkeypatch, fn):
    monkeypatch.setenv("GPMP_FACTOR_STORE_MB", ON_MB)
    _cold(env)
    fn()
    out, potf2, _ = _launches(env, fn)
    assert potf2 == 0 and _info(out) == 0
    return [t.cpu().numpy() for t in out[:-1]]


@pytest.mark.parametrize("n", (129, 640))
def test_predict_mean_from_a_hit_against_numpy(env, monkeypatch, numpy_reference, n):
    c = _Case(env, n, 4)
    ref = numpy_reference(c)
    zpm, zpv = _from_a_hit(env, monkeypatch, c.predict_mean)
    em, ev = np.max(np.abs(zpm - ref["grad"][0])), np.max(np.abs(zpv - ref["grad"][1]))
    print(f"n={n}: |zpm - ref| {em:.3e} (bound {1e-9 * np.max(np.abs(ref['zi'])):.3e}), |zpv - ref| {ev:.3e} (bound {1e-9 * math.exp(c.th[0]):.3e})")
    assert em < 1e-9 * np.max(np.abs(ref["zi"])) and ev < 1e-9 * math.exp(c.th[0])


@pytest.mark.parametrize("n", (129, 640))
def test_predict_grad_from_a_hit_against_numpy(env, monkeypatch, numpy_reference, n):
    c = _Case(env, n, 4)
    ref = numpy_reference(c)
    out = _from_a_hit(env, monkeypatch, c.predict_grad)
    for a, r, k in zip(out, ref["grad"], ("zpm", "zpv", "gzpm", "gzpv")):
        print(f"n={n} {k}: |got - ref| {np.max(np.abs(a - r)):.3e}, tolerance {ref['tol']:.3e} x {max(1.0, np.max(np.abs(r))):.3e}")
    for a, r, k in zip(out, ref["grad"], ("zpm", "zpv", "gzpm", "gzpv")):
        pmn.close(a, r, ref["tol"], k)


@pytest.mark.parametrize("n", (129, 640))
def test_posterior_weights_from_a_hit_against_numpy(env, monkeypatch, numpy_reference, n):
    c = _Case(env, n, 4)
    ref = numpy_reference(c)
    alpha, beta = _from_a_hit(env, monkeypatch, c.weights)
    for a, r, k in zip((alpha, beta), ref["weights"], ("alpha", "beta")):
        print(f"n={n} {k}: |got - ref| {np.max(np.abs(a - r)):.3e}, tolerance {ref['tol']:.3e} x {max(1.0, np.max(np.abs(r))):.3e}")
    pmn.close(alpha, ref["weights"][0], ref["tol"], "alpha")
    pmn.close(beta, ref["weights"][1], ref["tol"], "beta")


@pytest.mark.parametrize("n", (129, 640))
def test_reml_from_a_hit_against_numpy(env, monkeypatch, numpy_reference, n):
    c = _Case(env, n, 4)
    ref = numpy_reference(c)["reml"]
    (v,) = _from_a_hit(env, monkeypatch, c.reml)
    print(f"n={n}: reml {float(v[0])!r}, ref {ref!r}, |diff| {abs(float(v[0]) - ref):.3e}, bound {1e-12 * max(1.0, abs(ref)):.3e}")
    assert abs(float(v[0]) - ref) < 1e-12 * max(1.0, abs(ref))
