"""gpmp_whiten (include/gpmp_hip.h) and the zero-mean NLL's use of it, without a GPU: the workspace query as host arithmetic, and
the covariance-as-a-plain-callable path of core/likelihood.py, which must not reach the new entry."""
import math

import numpy as np
import pytest


@pytest.fixture(scope="module")
def lib():
    from gpmp_amd import _lib

    return _lib.load()


def _pad16(v):
    return (v + 15) // 16 * 16


def test_ws_query_is_zero_out_of_range(lib):
    for n in (0, -1, -2 ** 31, 2 ** 30 + 1, 2 ** 31 - 1):
        assert lib.gpmp_whiten_ws_elems(n) == 0, n


@pytest.mark.parametrize("n,want", ((2, 32 + 16384), (129, 129 * 144 + 2 * 16384), (1500, 1500 * 1504 + 12 * 16384 + 64 * 16384)))
def test_ws_query_is_the_K_and_dinv_slots(lib, n, want):
    """n pad16(n) doubles for L and gpmp_dinv_elems(n) for its block inverses (128 x 128 each, and above n = 1024 the 1024 x 1024
    leaf scratch), each slot padded to 16: the literals are that sum written out"""
    assert lib.gpmp_whiten_ws_elems(n) == want == _pad16(n * _pad16(n)) + _pad16(lib.gpmp_dinv_elems(n))
    assert lib.gpmp_whiten_ws_elems(n) < lib.gpmp_nll_ws_elems(n)        # no column block, no scalars, no column-dot scratch


def test_callable_covariance_keeps_the_composed_path(monkeypatch):
    """a covariance that is not a MaternCovariance: covariance_factor + solve_lower + logdet as before, the driver is never called"""
    import torch

    from gpmp_amd.core import fused, likelihood

    class Factor:
        def solve_lower(self, z):
            return 0.5 * z

        def logdet(self):
            return 3.0

    seen = []

    def factor(model, xi, covparam):
        seen.append((model, tuple(xi.shape), covparam))
        return Factor()

    def no_driver(*a, **k):
        raise AssertionError("a plain callable covariance reached a fused driver")

    monkeypatch.setattr(likelihood.gnp, "asarray", lambda x: torch.as_tensor(np.asarray(x), dtype=torch.float64))
    monkeypatch.setattr(likelihood, "covariance_factor", factor)
    monkeypatch.setattr(fused, "call_driver", no_driver)

    class Model:
        covariance = staticmethod(lambda x, y, t, pairwise=False: None)

    xi, zi, th = np.zeros((4, 2)), np.array([1.0, 2.0, 3.0, 4.0]), np.array([0.1, 0.2, 0.3])
    v = likelihood.negative_log_likelihood_zero_mean(Model, th, xi, zi)
    assert len(seen) == 1 and seen[0][0] is Model and seen[0][1] == (4, 2) and seen[0][2] is th
    assert float(v) == 0.5 * (4 * math.log(2.0 * math.pi) + 3.0 + 0.25 * 30.0)
