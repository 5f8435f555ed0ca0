"""The fused prediction drivers with and without the Strassen step in the solve's updates (gpmp_set_strassen_thresholds).

n = 2048, m = 1500, d = 3; gpmp_predict_zero_mean and gpmp_predict_mean (q = 2) run three times:
  raised    thresholds above every update: the plain recursion
  lowered   512 rows / 256 columns: the updates of 1024 and 512 rows take the step (quadrants of 512 and 256 rows, peeled columns)
  default   a problem of this size is below the default thresholds: bit-identical to `raised`
`raised` and `lowered` agree to 1e-12 (mean relative to max|z|, variance relative to sigma^2); each meets the CPU oracle within the
tolerance of tests/test_config_sizes_gpu.py (1e-10 x max(1, cond(K) / 1e6)); the last 64 prediction points are observations
(mean within 1e-6 max|z|, variance below 1e-6 sigma^2)."""
import math

import numpy as np
import pytest

from tests.helpers import theta_aniso

pytestmark = pytest.mark.gpu

N, M, D, Q = 2048, 1500, 3, 2
HUGE = 1 << 30


@pytest.fixture(scope="module")
def env():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import gpmp_amd.num as gnp
    from gpmp_amd import _lib

    return torch, gnp, _lib, _lib.load()


def _design(x):
    return np.column_stack((np.ones(x.shape[0]), x[:, 0]))


@pytest.fixture(scope="module")
def problem():
    """inputs and the oracle's answers, computed once and left unchanged"""
    from oracle import gp_oracle as orc

    rng = np.random.default_rng(1234)
    xi = rng.random((N, D))
    zi = np.sin(2 * np.pi * xi[:, 0]) + xi[:, 1:].sum(axis=1)
    xt = np.random.default_rng(4321).random((M, D))
    idx = np.random.default_rng(3).choice(N, 64, replace=False)
    xt[-64:] = xi[idx]
    th = theta_aniso(D)
    kern = lambda x, y, t, pairwise=False: orc.maternp_covariance(x, y, 2, t, pairwise)  # noqa: E731
    ev = np.linalg.eigvalsh(orc.maternp_covariance(xi, None, 2, th))
    ref = {
        "zero": orc.predict(orc.OracleModel(None, kern, None, th, "zero"), xi, zi, xt),
        "mean": orc.predict(orc.OracleModel(lambda x, p: _design(x), kern, None, th, "linear_predictor"), xi, zi, xt),
    }
    return {"xi": xi, "zi": zi, "xt": xt, "idx": idx, "th": th, "scale": max(1.0, ev[-1] / ev[0] / 1e6), "ref": ref}


def _run(env, pb, kind):
    torch, gnp, _lib, lib = env
    dev = gnp._dev()
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=dev)  # noqa: E731
    X, Z, Xt = t(pb["xi"]), t(pb["zi"]), t(pb["xt"])
    zpm = torch.empty(M, dtype=torch.float64, device=dev)
    zpv = torch.empty(M, dtype=torch.float64, device=dev)
    info = torch.zeros(1, dtype=torch.int32, device=dev)
    hv = _lib.host_vec(pb["th"])
    if kind == "zero":
        ws = torch.empty(int(lib.gpmp_predict_ws_elems(N, M)), dtype=torch.float64, device=dev)
        _lib.check(lib.gpmp_predict_zero_mean(gnp._ptr(X), gnp._ptr(Z), gnp._ptr(Xt), N, M, D, 2, hv, 0, 0, gnp._ptr(ws), gnp._ptr(zpm),
                                              gnp._ptr(zpv), gnp._ptr(info), gnp._stream()), "gpmp_predict_zero_mean")
    else:
        Pi, Pt = t(_design(pb["xi"])), t(_design(pb["xt"]))
        ws = torch.empty(int(lib.gpmp_predict_mean_ws_elems(N, M, Q)), dtype=torch.float64, device=dev)
        _lib.check(lib.gpmp_predict_mean(gnp._ptr(X), gnp._ptr(Z), gnp._ptr(Pi), Q, gnp._ptr(Xt), gnp._ptr(Pt), Q, N, M, D, Q, 2, hv, 0, 0,
                                         gnp._ptr(ws), gnp._ptr(zpm), gnp._ptr(zpv), gnp._ptr(info), gnp._stream()), "gpmp_predict_mean")
    torch.cuda.synchronize()
    assert int(info.item()) == 0
    return zpm.cpu().numpy(), zpv.cpu().numpy()


@pytest.mark.parametrize("kind", ["zero", "mean"])
def test_predict_with_and_without_the_strassen_step(env, problem, kind):
    lib = env[3]
    zmax, s2 = float(np.max(np.abs(problem["zi"]))), math.exp(problem["th"][0])
    q = 0 if kind == "zero" else Q
    cols = M + 1 + q + ((M + 1 + q) & 1)
    try:
        lib.gpmp_set_strassen_thresholds(HUGE, HUGE)
        assert lib.gpmp_strassen_ws_elems(N, cols) == 0
        raised = _run(env, problem, kind)
        lib.gpmp_set_strassen_thresholds(512, 256)
        assert lib.gpmp_strassen_ws_elems(N, cols) == 512 * 512 + 512 * ((cols // 2) // 128 * 128)
        lowered = _run(env, problem, kind)
    finally:
        lib.gpmp_set_strassen_thresholds(0, 0)
    assert lib.gpmp_strassen_ws_elems(N, cols) == 0
    default = _run(env, problem, kind)
    assert np.array_equal(default[0], raised[0]) and np.array_equal(default[1], raised[1])
    dm = float(np.max(np.abs(lowered[0] - raised[0]))) / zmax
    dv = float(np.max(np.abs(lowered[1] - raised[1]))) / s2
    print(f"{kind}: strassen vs plain: mean {dm:.3e} max|z|, variance {dv:.3e} sigma^2")
    assert dm < 1e-12 and dv < 1e-12, (dm, dv)
    ozpm, ozpv = problem["ref"][kind]
    tol = 1e-10 * problem["scale"]
    for name, (zpm, zpv) in (("raised", raised), ("lowered", lowered)):
        em, evar = float(np.max(np.abs(zpm - ozpm))) / zmax, float(np.max(np.abs(zpv - ozpv))) / s2
        print(f"{kind} {name}: vs oracle: mean {em:.3e} max|z|, variance {evar:.3e} sigma^2 (tolerance {tol:.1e})")
        assert em < tol and evar < tol, (name, em, evar, tol)
        assert np.max(np.abs(zpm[-64:] - problem["zi"][problem["idx"]])) < 1e-6 * zmax
        assert np.max(zpv[-64:]) < 1e-6 * s2
