"""gpmp_amd/core/fused.py without a GPU: the table of limits against include/gpmp_hip.h, the model check, the chunk width, and the
staging object on host tensors (no library call, no device)."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_defines():
    """GPMP_<NAME> -> int for every integer #define of the header (a decimal number or (a << b)); comments removed first."""
    text = open(os.path.join(ROOT, "include", "gpmp_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    out = {}
    for name, a, b in re.findall(r"^#define\s+GPMP_(\w+)\s+\(?\s*(\d+)\s*(?:<<\s*(\d+)\s*)?\)?\s*$", text, flags=re.M):
        out[name] = int(a) << int(b or 0)
    return out


def test_limits_equal_the_header():
    from gpmp_amd.core import fused

    header = _header_defines()
    table = fused.limits._asdict()
    assert set(table) == {"MAX_DIM", "MAX_DIM_WIDE", "MAX_P", "MAX_RANK", "MAX_EXTENT", "BATCH_MAX_N", "BATCH_MAX_Q"}
    for name, value in table.items():
        assert header[name] == value, name
    with pytest.raises(AttributeError):
        fused.limits.MAX_DIM = 65


def test_old_names_are_aliases_of_the_table():
    from gpmp_amd.core import fused, gradients, posterior_mean

    assert gradients.BATCH_MAX_N == fused.limits.BATCH_MAX_N
    assert gradients.BATCH_MAX_Q == fused.limits.BATCH_MAX_Q
    assert gradients.MLZeroMeanAnalytic.batch_max_points == fused.limits.BATCH_MAX_N
    assert posterior_mean.MAX_DIM == fused.limits.MAX_DIM


def test_check_matern_model():
    import gpmp_amd as gp
    from gpmp_amd.core import fused
    from gpmp_amd.kernel import MaternCovariance

    mean = lambda x, param: x[:, :1]  # noqa: E731
    good = gp.Model(mean, MaternCovariance(2), np.ones(1), np.zeros(3), "parameterized")
    fused.check_matern_model(good, "predict_gradient")
    other = gp.Model(None, lambda x, y, c, pairwise=False: None, None, np.zeros(2), "zero")
    with pytest.raises(NotImplementedError, match="predict_gradient needs a gpmp_amd.kernel.MaternCovariance.*gnp.grad"):
        fused.check_matern_model(other, "predict_gradient")
    bad = gp.Model(None, MaternCovariance(2), None, np.zeros(3), "zero")
    bad.meantype = "constant"
    with pytest.raises(ValueError, match="Invalid meantype constant"):
        fused.check_matern_model(bad, "predict_gradient")
    good.meanparam = None
    with pytest.raises(ValueError, match="meanparam should not be None"):
        fused.check_matern_model(good, "predict_gradient")
    good.meanparam, good.covparam = np.ones(1), None
    with pytest.raises(ValueError, match="covparam is None"):
        fused.check_matern_model(good, "predict_gradient")


def test_one_chunk_width_with_the_floor_of_each_caller(monkeypatch):
    """The prediction routes never go below 256 columns, the wide posterior mean goes down to 1; both stop at m."""
    from gpmp_amd.config import get_config
    from gpmp_amd.core import fused

    monkeypatch.setattr(get_config(), "predict_chunk_bytes", 8 * 1500 * 300)
    assert fused.chunk_cols(1500, 2000) == 300 and fused.chunk_cols(1500, 2000, floor=1) == 300
    assert fused.chunk_cols(1500, 200) == 200 and fused.chunk_cols(1500, 0) == 0
    assert fused.chunk_cols(3000, 2000) == 256 and fused.chunk_cols(3000, 2000, floor=1) == 150
    assert fused.chunk_cols(3000, 100) == 100
    monkeypatch.setattr(get_config(), "predict_chunk_bytes", 0)
    assert fused.chunk_cols(10, 5, floor=1) == 1 and fused.chunk_cols(0, 5, floor=1) == 1


@pytest.fixture
def host(monkeypatch):
    """The package's arrays on the host for one test: the staging object calls no library entry point."""
    import torch
    from gpmp_amd.config import get_config

    monkeypatch.setattr(get_config(), "device", "cpu")
    return torch


def _lin(x, param):
    import gpmp_amd.num as gnp

    return gnp.hstack((gnp.ones((x.shape[0], 1)), x))


def test_staged_on_host_tensors(host):
    import gpmp_amd as gp
    from gpmp_amd.core import fused
    from gpmp_amd.kernel import MaternCovariance

    rng = np.random.default_rng(0)
    xi, zi, xt = rng.random((9, 2)), rng.random(9), rng.random((4, 2))
    th = np.array([0.1, -2.0, 0.3, 0.4])
    model = gp.Model(_lin, MaternCovariance(3, noise=True), None, th, "linear_predictor")
    st = fused.Staged(model, xi, zi)
    assert (st.n, st.d, st.q, st.p, st.noise, st.meantype) == (9, 2, 3, 3, 1, "linear_predictor")
    assert st.X.is_contiguous() and st.zc.is_contiguous() and st.zc.dtype == host.float64
    np.testing.assert_array_equal(st.X.numpy(), xi)
    np.testing.assert_array_equal(st.zc.numpy(), zi)
    np.testing.assert_array_equal(st.Pi.numpy(), np.hstack((np.ones((9, 1)), xi)))
    assert list(st.hv) == list(th) and fused.ld(st.Pi) >= 3 and fused.ld(None) == 0
    th[0] = 7.0                                                    # the model's array written in place: the staged copy stays
    assert st.theta[0] == 0.1 and st.hv[0] == 0.1 and list(st.covparam) == [0.1, -2.0, 0.3, 0.4]
    Pt, J, prior_mean, prior_grad = st.at(host.as_tensor(xt), gradient=True)
    assert prior_mean is None and prior_grad is None
    np.testing.assert_array_equal(Pt.numpy(), np.hstack((np.ones((4, 1)), xt)))
    ref = np.zeros((4, 3, 2))
    ref[:, 1, 0] = ref[:, 2, 1] = 1.0
    np.testing.assert_array_equal(J.numpy(), ref)
    assert st.at(host.as_tensor(xt))[1] is None                    # no Jacobian unless asked for
    # a parameterized mean centres zi and returns what to add back
    pm = gp.Model(lambda x, param: (param[0] + param[1] * x[:, 0]).reshape(-1, 1), MaternCovariance(1), host.tensor([0.5, 2.0], dtype=host.float64),
                  th[[0, 2, 3]], "parameterized")
    sp = fused.Staged(pm, xi, zi)
    pm.meanparam = np.array([9.0, 9.0])
    np.testing.assert_array_equal(sp.zc.numpy(), zi - (0.5 + 2.0 * xi[:, 0]))
    assert sp.Pi is None and sp.q == 0 and sp.noise == 0
    Pt, J, prior_mean, prior_grad = sp.at(host.as_tensor(xt), gradient=True)
    assert Pt is None and J is None
    np.testing.assert_array_equal(prior_mean.numpy(), 0.5 + 2.0 * xt[:, 0])
    np.testing.assert_array_equal(prior_grad.numpy(), np.tile([2.0, 0.0], (4, 1)))


def test_staged_refuses_a_wrong_parameter_count_and_changing_design_widths(host):
    import gpmp_amd as gp
    from gpmp_amd.core import fused
    from gpmp_amd.kernel import MaternCovariance

    xi, zi, xt = np.random.default_rng(1).random((6, 2)), np.zeros(6), host.zeros((4, 2), dtype=host.float64)
    for noise, nth in ((False, 4), (False, 2), (True, 3)):
        model = gp.Model(None, MaternCovariance(1, noise=noise), None, np.zeros(nth), "zero")
        with pytest.raises(ValueError, match=f"covparam has {nth} entries, expected {4 if noise else 3}"):
            fused.Staged(model, xi, zi)
    with pytest.raises(ValueError, match="covparam has 2 entries, expected 3"):
        fused.stage_theta(MaternCovariance(1), np.zeros((5, 2)), 2)               # one row per problem: the row length counts
    hv, noise = fused.stage_theta(MaternCovariance(1, noise=True), np.arange(8.0).reshape(2, 4), 2)
    assert list(hv) == list(range(8)) and noise == 1
    # a design with as many columns as points: 1 + 6 at xi, 1 + 4 at xt
    ragged = lambda x, param: host.ones((x.shape[0], 1 + x.shape[0]), dtype=host.float64)  # noqa: E731
    st = fused.Staged(gp.Model(ragged, MaternCovariance(1), None, np.zeros(3), "linear_predictor"), xi, zi)
    with pytest.raises(ValueError, match="the mean design has 5 columns at xt, 7 at xi"):
        st.at(xt)
    st = fused.Staged(gp.Model(_lin, MaternCovariance(1), None, np.zeros(3), "linear_predictor"), xi, zi)
    with pytest.raises(ValueError, match="the mean Jacobian has 2 columns, the mean design 3"):
        st.at(xt, gradient=True, mean_gradient=lambda x, param: host.zeros((x.shape[0], 2, 2), dtype=host.float64))
    with pytest.raises(ValueError, match=r"mean_gradient returned shape \(4, 2\)"):
        st.at(xt, gradient=True, mean_gradient=lambda x, param: host.zeros((x.shape[0], 2), dtype=host.float64))
