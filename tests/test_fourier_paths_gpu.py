"""gpmp_fourier_paths and the objects that reach it (Model.prior_paths / Model.posterior_paths) on the GPU, against the same sum in
np.longdouble from the same stored inputs.

Extents of csrc/fourier_paths.hip this file relies on: a matrix instruction takes 4 dimensions / 4 features, a tile is 16 features
x 16 points, 32 features make a chunk and 32 dimensions an LDS chunk, a wave owns 32 points and a workgroup 128; a column tile is
16 wide, a lane keeps 1 to 4 of them and a workgroup 64 columns; a slice has at least 128 features and a call is sliced towards
512 workgroups (m = 17, r = 1000: 8 slices of 128 features, the last of 104; r = 200 with m <= 300: two slices)."""
import numpy as np
import pytest

from . import posterior_mean_numpy as pmn
from .test_posterior_mean_gpu import _dev, _model, _problem, env  # noqa: F401

pytestmark = pytest.mark.gpu
LD = np.longdouble
EPS = np.finfo(np.float64).eps


def _reference(x, omega, phase, W):
    """(the sum in np.longdouble, the forward bound per column): eps sum_k |W[k, c]| (r + 4 + 2 pi (d + 2) U), U the largest
    sum_j |x_tj omega_kj| + |b_k| -- the phase rounding is <= (d + 2) eps U turns, cos is 1-Lipschitz, the cosine's own error is 4 eps
    and the sum over r is bounded by gamma_r."""
    u = x.astype(LD) @ omega.astype(LD).T + phase.astype(LD)
    ref = np.cos(2 * np.arccos(LD(-1)) * (u - np.rint(u))) @ W.astype(LD)
    U = np.max(np.abs(x) @ np.abs(omega).T + np.abs(phase))
    r, d = omega.shape
    return ref, EPS * np.abs(W).sum(axis=0) * (r + 4 + 2 * np.pi * (d + 2) * U)


def _c_paths(env, X, OM, PH, WW, s, out=None):
    """gpmp_fourier_paths through ctypes on device tensors (leading dimensions = row strides); returns out (m x s view)."""
    _, gnp, _lib, torch = env
    lib = _lib.load()
    (m, d), r = X.shape, OM.shape[0]
    if out is None:
        out = torch.empty((m, s), dtype=torch.float64, device="cuda")
    ws = torch.empty(int(lib.gpmp_fourier_paths_ws_elems(m, r, s, d)), dtype=torch.float64, device="cuda")
    _lib.check(lib.gpmp_fourier_paths(gnp._ptr(X), gnp._ptr(OM), OM.stride(0), gnp._ptr(PH), gnp._ptr(WW), WW.stride(0), m, r, s, d,
                                      gnp._ptr(ws), gnp._ptr(out), out.stride(0), gnp._stream()), "gpmp_fourier_paths")
    return out[:, :s]


@pytest.mark.parametrize("m, r, s, d, kind", [
    (1, 1, 1, 1, ""), (17, 3, 17, 3, ""), (129, 65, 65, 5, ""), (300, 200, 1, 64, ""), (300, 200, 17, 70, ""), (1, 200, 17, 70, ""),
    (300, 65, 65, 1, ""), (129, 3, 1, 64, ""), (300, 1, 65, 5, ""),
    (129, 200, 65, 3, "ld"),          # ld > extent on omega, W and out: NaN behind the columns, guard values around out
    (17, 65, 17, 5, "far"),           # points scaled so that |u| reaches about 10^3 turns
    (17, 1000, 17, 3, "split"),       # 8 slices over the features and the finalize kernel
])
def test_kernel_against_the_longdouble_sum(env, m, r, s, d, kind):
    torch, rng = env[3], np.random.default_rng(1000 * m + r + s + d)
    x, omega = rng.random((m, d)) * (300.0 if kind == "far" else 1.0), rng.standard_normal((r, d)) * 2.0
    phase, W = rng.random(r), rng.standard_normal((r, s))
    ref, bound = _reference(x, omega, phase, W)
    assert kind != "far" or np.max(np.abs(x @ omega.T)) > 900.0
    pad = 3 if kind == "ld" else 0
    OM = torch.full((r, d + pad), float("nan"), dtype=torch.float64, device="cuda")
    WW = torch.full((r, s + pad), float("nan"), dtype=torch.float64, device="cuda")
    OM[:, :d], WW[:, :s] = _dev(env, omega), _dev(env, W)
    buf = torch.full((16 + m * (s + pad) + 16,), -7.25, dtype=torch.float64, device="cuda")
    outs = [_c_paths(env, _dev(env, x), OM, _dev(env, phase), WW, s, out=buf[16:-16].view(m, s + pad)).cpu().numpy().copy() for _ in range(2)]
    err = np.abs(outs[0].astype(LD) - ref)
    print(f"max error / bound = {float(np.max(err / bound)):.3f}")
    assert np.all(err <= bound), float(np.max(err / bound))
    assert np.array_equal(outs[0], outs[1])                    # no atomics: the same bits from run to run
    assert bool((buf[:16] == -7.25).all()) and bool((buf[-16:] == -7.25).all()) and bool((buf[16:-16].view(m, s + pad)[:, s:] == -7.25).all())


def test_prior_paths_object(env):
    gp, _, _, torch = env
    xt, th = _problem(1, 130, 3, 5)[2:]
    prior = _model(env, 2, 0, th).prior_paths(5, nb_features=200, seed=3)
    assert isinstance(prior, gp.core.PriorPaths) and prior.omega.shape == (200, 3) and prior.W.shape == (200, 5)
    ref, bound = _reference(xt, *(t.cpu().numpy() for t in (prior.omega, prior.phase, prior.W)))
    O = prior.paths(xt)
    assert O.shape == (130, 5) and np.all(np.abs(O.astype(LD) - ref) <= bound) and prior.paths(np.zeros((0, 3))).shape == (0, 5)
    again = _model(env, 2, 0, th).prior_paths(5, nb_features=200, seed=3)        # the seed fixes the paths
    assert np.array_equal(again.paths(xt), O) and not np.array_equal(_model(env, 2, 0, th).prior_paths(5, 200, seed=4).paths(xt), O)


@pytest.mark.parametrize("noise, kind", [(0, "zero"), (1, "zero"), (0, "lin"), (1, "param")])
def test_posterior_paths_equal_prior_plus_posterior_means(env, noise, kind):
    """post(xt) = prior(xt) + posterior_means(xi, zi - prior(xi) - eps)(xt), the right-hand side assembled from public pieces; the
    tolerance of tests/test_posterior_mean_multi_gpu.py for that pass."""
    gp, _, _, torch = env
    n, m, s, d = 200, 300, 5, 3
    xi, zi, xt, th = _problem(n, m, d, 21)
    th = np.insert(th, 1, [-3.0] * noise)
    model = _model(env, 2, noise, th, kind, d, torch.as_tensor([0.3, 1.1], device="cuda") if kind == "param" else None)
    post = model.posterior_paths(xi, zi, s, nb_features=300, seed=11)
    assert isinstance(post, gp.core.PosteriorPaths) and (post.eps is None) == (noise == 0)
    eps = 0.0 if noise == 0 else post.eps.cpu().numpy()
    assert noise == 0 or (eps.shape == (n, s) and 0.5 < eps.std() / np.exp(0.5 * th[1]) < 1.5)
    rhs = post.prior.paths(xt) + model.posterior_means(xi, zi[:, None] - post.prior.paths(xi) - eps)(xt)
    O = post.paths(xt)
    assert O.shape == (m, s)
    pmn.close(O, rhs, pmn.tolerance(xi, 2, th, noise), (noise, kind))
