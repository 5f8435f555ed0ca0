"""Host-side checks of the wide-dimension route (d > GPMP_MAX_DIM): the argument contract at GPMP_MAX_DIM_WIDE, the gradient
workspace query, the compile-time resources of the new kernels, and the CPU oracle against the reference fixture
(tests/golden/ref_wide_dim.npz, written by make_fixtures_wide_dim.py).  No GPU needed."""
import ctypes
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gpmp_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


def _header_int(name):
    text = open(os.path.join(ROOT, "include", "gpmp_hip.h")).read()
    return int(re.search(rf"#define {name} (\d+)", text).group(1))


@pytest.fixture(scope="module")
def lib():
    from gpmp_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g

        g.build()
    return _lib.load()


def test_header_limits():
    assert _header_int("GPMP_MAX_DIM") == 64
    assert _header_int("GPMP_MAX_DIM_WIDE") == 16384


def test_dimension_above_the_wide_limit_is_rejected(lib):
    """Every d-taking entry point rejects d = GPMP_MAX_DIM_WIDE + 1 (and 2^31 - 1) before touching a pointer, with a message; the
    pointers below are never dereferenced."""
    from gpmp_amd import _lib

    fake = ctypes.c_void_p(0x1000)
    theta = _lib.host_vec(np.zeros(3))
    for d in (_header_int("GPMP_MAX_DIM_WIDE") + 1, 2 ** 31 - 1):
        calls = {
            "gpmp_matern_gram": lambda: lib.gpmp_matern_gram(fake, None, 10, 10, d, 2, theta, 0, 0.0, 0, fake, 10, None),
            "gpmp_scaled_distance": lambda: lib.gpmp_scaled_distance(fake, fake, 10, 10, d, theta, fake, 10, None),
            "gpmp_matern_pairwise": lambda: lib.gpmp_matern_pairwise(fake, fake, 10, d, 2, theta, 0, fake, None),
            "gpmp_matern_gram_deriv": lambda: lib.gpmp_matern_gram_deriv(fake, 10, d, 2, theta, 0, 0, fake, 10, None),
            "gpmp_matern_grad_trace": lambda: lib.gpmp_matern_grad_trace(fake, 10, fake, 10, d, 2, theta, 0, None, None, 0, 1, fake,
                                                                         fake, None),
            "gpmp_matern_grad_trace_cross": lambda: lib.gpmp_matern_grad_trace_cross(fake, 10, fake, 10, fake, 10, d, 2, theta, 0, None,
                                                                                     None, 0, 1, fake, fake, None),
            "gpmp_reml": lambda: lib.gpmp_reml(fake, fake, None, 0, 10, d, 0, 2, theta, 0, fake, fake, fake, None),
            "gpmp_predict_mean": lambda: lib.gpmp_predict_mean(fake, fake, fake, 1, fake, fake, 1, 10, 10, d, 1, 2, theta, 0, 1, fake,
                                                               fake, fake, fake, None),
        }
        for name, call in calls.items():
            rc = call()
            assert rc < 0, (name, d, rc)
            msg = lib.gpmp_last_error().decode()
            assert "GPMP_MAX_DIM_WIDE" in msg, (name, d, msg)


def test_grad_workspace_grows_with_d_above_64(lib):
    n = 1000
    w64, w65, w200, w1000 = (lib.gpmp_grad_ws_elems(n, d) for d in (64, 65, 200, 1000))
    assert w64 > 0 and w65 > 0
    assert w65 < w200 < w1000
    # one row of d + 2 partials per workgroup plus the d staged scale factors
    assert w1000 - w200 >= 800 * 2
    assert lib.gpmp_grad_ws_elems(n, _header_int("GPMP_MAX_DIM_WIDE") + 1) == 0
    # the fused gradient driver's workspace follows
    assert lib.gpmp_nll_grad_ws_elems(n, 1000, 1) - lib.gpmp_nll_grad_ws_elems(n, 200, 1) >= w1000 - w200


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_wide_instances_in_gram_hip_use_no_scratch_and_no_spills():
    cmd = [HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-mllvm", "-amdgpu-mfma-vgpr-form=1",
           "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(CSRC, "gram.hip"), "-o", os.devnull]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    res, name = {}, None
    for line in out.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            res[name] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", line)
        if m and name:
            res[name][m.group(1).strip()] = int(m.group(2))
    for frag in ("gram_kernel_v3", "GramWideParams", "grad_trace_wide_kernel", "PairWideParams", "DerivWideParams",
                 "grad_wide_finalize_kernel"):
        hit = {k: v for k, v in res.items() if frag in k}
        assert hit, (frag, sorted(res))
        for k, v in hit.items():
            assert v.get("ScratchSize", 0) == 0, (k, v)
            assert v.get("VGPRs Spill", 0) == 0, (k, v)
    # every instance of the Gram tile, wide or not, keeps the register budget of two workgroups per CU
    for k, v in res.items():
        if "gram_kernel_v3" in k:
            assert v["VGPRs"] <= 128, (k, v)


# ---------------------------------------------------------------- oracle vs reference fixture
@pytest.fixture(scope="module")
def wide(golden):
    from tests.wide_dim_inputs import decode

    return decode(golden("wide_dim"))


def _k(p, noise=False):
    from oracle import gp_oracle as orc

    f = orc.noisy_maternp_covariance if noise else orc.maternp_covariance
    return lambda x, y, t, pairwise=False: f(x, y, p, t, pairwise)


def _const(x, param):
    return np.ones((x.shape[0], 1))


def _lin(x, param):
    return np.hstack((np.ones((x.shape[0], 1)), x[:, :3]))     # (as make_fixtures_wide_dim.py)


@pytest.mark.parametrize("d", [65, 200, 1000])
def test_oracle_gram_matches_reference(wide, d):
    from oracle import gp_oracle as orc

    g = wide
    x, y, th, thn = g[f"gram_d{d}_x"], g[f"gram_d{d}_y"], g[f"gram_d{d}_theta"], g[f"gram_d{d}_theta_noise"]
    np.testing.assert_allclose(orc.scaled_distance(th[1:], x, y), g[f"dist_d{d}"], rtol=1e-15)
    for p in (0, 2, 5):
        np.testing.assert_allclose(orc.maternp_covariance(x, x, p, th), g[f"gram_d{d}_p{p}_ii"], rtol=1e-15)
        np.testing.assert_allclose(orc.maternp_covariance(x, y, p, th), g[f"gram_d{d}_p{p}_it"], rtol=1e-15)
        np.testing.assert_allclose(orc.maternp_covariance(x[:y.shape[0]], y, p, th, True), g[f"gram_d{d}_p{p}_pw"], rtol=1e-15)
        np.testing.assert_allclose(orc.noisy_maternp_covariance(x, x, p, thn), g[f"gram_d{d}_p{p}_noise_ii"], rtol=1e-15)
        np.testing.assert_allclose(orc.noisy_maternp_covariance(x, y, p, thn), g[f"gram_d{d}_p{p}_noise_it"], rtol=1e-15)


def test_oracle_criteria_predictions_and_loo_match_reference(wide):
    from oracle import gp_oracle as orc

    g = wide
    xi, zi, th = g["crit_xi"], g["crit_zi"], g["crit_theta"]
    mz = orc.OracleModel(None, _k(2), None, th, "zero")
    mc = orc.OracleModel(_const, _k(2), None, th, "linear_predictor")
    ml = orc.OracleModel(_lin, _k(2), None, th, "linear_predictor")
    assert math.isclose(orc.negative_log_likelihood_zero_mean(mz, th, xi, zi), float(g["crit_nll"]), rel_tol=1e-12)
    assert math.isclose(orc.negative_log_restricted_likelihood(mc, th, xi, zi), float(g["crit_reml_const"]), rel_tol=1e-12)
    for tag, model in (("zero", mz), ("const", mc), ("lin", ml)):
        zpm, zpv = orc.predict(model, xi, zi, g["pred_xt"])
        np.testing.assert_allclose(zpm, g[f"pred_{tag}_zpm"], rtol=1e-10, atol=1e-12)
        np.testing.assert_allclose(zpv, g[f"pred_{tag}_zpv"], rtol=1e-9, atol=1e-12)
    xl, zl, thl = g["loo_xi"], g["loo_zi"], g["loo_theta"]
    for tag, model in (("zero", orc.OracleModel(None, _k(2), None, thl, "zero")),
                       ("const", orc.OracleModel(_const, _k(2), None, thl, "linear_predictor"))):
        zloo, s2, eloo = orc.loo(model, xl, zl)
        np.testing.assert_allclose(zloo, g[f"loo_{tag}_zloo"], rtol=1e-10, atol=1e-12)
        np.testing.assert_allclose(s2, g[f"loo_{tag}_s2"], rtol=1e-10)
        np.testing.assert_allclose(eloo, g[f"loo_{tag}_eloo"], rtol=1e-10, atol=1e-12)


def test_oracle_gradients_match_reference_autograd(wide):
    from oracle import gp_oracle as orc

    g = wide
    xi, zi, th = g["crit_xi"], g["crit_zi"], g["crit_theta"]
    v, gr = orc.nll_zero_mean_value_and_grad(xi, zi, 2, th)
    assert math.isclose(v, float(g["crit_nll_torch"]), rel_tol=1e-12)
    np.testing.assert_allclose(gr, g["crit_nll_grad"], rtol=1e-7, atol=1e-9 * np.abs(g["crit_nll_grad"]).max())
    v, gr = orc.reml_value_and_grad(xi, zi, np.ones((len(zi), 1)), 2, th)
    assert math.isclose(v, float(g["crit_reml_const_torch"]), rel_tol=1e-12)
    np.testing.assert_allclose(gr, g["crit_reml_const_grad"], rtol=1e-7, atol=1e-9 * np.abs(g["crit_reml_const_grad"]).max())
    v, gr = orc.nll_zero_mean_value_and_grad(g["critn_xi"], g["critn_zi"], 0, g["critn_theta"], noise_index=1)
    assert math.isclose(v, float(g["critn_nll"]), rel_tol=1e-12)
    np.testing.assert_allclose(gr, g["critn_nll_grad"], rtol=1e-7, atol=1e-9 * np.abs(g["critn_nll_grad"]).max())


def test_oracle_near_duplicates_match_reference(wide):
    from oracle import gp_oracle as orc

    g = wide
    xd, zd, thd = g["dup_xi"], g["dup_zi"], g["dup_theta"]
    np.testing.assert_allclose(orc.maternp_covariance(xd, xd, 2, thd), g["dup_K"], rtol=1e-15)
    m = orc.OracleModel(None, _k(2), None, thd, "zero")
    assert math.isclose(orc.negative_log_likelihood_zero_mean(m, thd, xd, zd), float(g["dup_nll"]), rel_tol=1e-9)
