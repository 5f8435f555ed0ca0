"""The seven fused C-ABI drivers (csrc/drivers.hip) depend on nothing in their workspace and stay inside it.  Each driver runs
twice per shape on a workspace that is a slice of a buffer of ws_elems + 64 doubles, filled with -7.25 the first time and with
3500.0 the second: outputs and info must be bit-identical, finite and info == 0, and the 64 doubles behind the workspace must
still hold the fill.  That is what a change of the shared workspace layout can break: a slot that is too small, two live slots
that overlap, a read of something never written.  (Two finite fills, not NaN: a discarded lane that multiplies garbage by zero
must not fail the test.)"""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# (n, m, d, q); the drivers without prediction points ignore m, the zero-mean drivers ignore q, gpmp_predict_mean skips q = 0
SHAPES = [
    (5, 1, 2, 0),         # m + 1 + q even, smallest
    (5, 1, 2, 1),         # odd; m < 1 + q: the reduction scratch is sized by 1 + q
    (5, 2, 2, 3),         # m + 1 + q even
    (129, 130, 3, 0),     # second diagonal block; the leading dimension of [K(xi, xt) | z | P] pads
    (129, 131, 3, 2),     # m + 1 + q even
    (129, 130, 3, 10),    # 11 right-hand sides: two passes of the few-column sweep
    (130, 7, 65, 1),      # the d > 64 route: gradient-trace workspace tail and the reduce slot
]
FILLS = (-7.25, 3500.0)
TAIL = 64
DRIVERS = ("gpmp_nll_zero_mean", "gpmp_predict_zero_mean", "gpmp_reml", "gpmp_nll_grad", "gpmp_loo", "gpmp_predict_mean",
           "gpmp_predict_grad")


@pytest.fixture(scope="module")
def env():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import gpmp_amd.num as gnp
    from gpmp_amd import _lib

    return torch, gnp, _lib, _lib.load()


def make_inputs(n, m, d, q):
    rng = np.random.default_rng(100 * n + m + q)
    design = lambda a: np.hstack((np.ones((len(a), 1)), a, a ** 2, a ** 3))[:, :q]  # noqa: E731
    x = rng.random((n, d))
    xt = rng.random((m, d))
    z = np.sin(3 * x[:, 0]) + x.sum(axis=1)
    theta = np.concatenate(([0.2, math.log(1e-3)], -np.log(0.4 + 0.3 * np.arange(d) / d)))
    return x, z, xt, (design(x) if q else None), (design(xt) if q else None), theta


def run_driver(env, name, shape, fill):
    """One call of driver `name` at `shape` (noise on, p = 2, clamped variances, variance gradient on, J = 0) on a workspace
    pre-filled with `fill`.  Returns ({output name: array}, info, the TAIL doubles behind the workspace)."""
    torch, gnp, _lib, lib = env
    dev = gnp._dev()
    n, m, d, q = shape
    if name in ("gpmp_nll_zero_mean", "gpmp_predict_zero_mean"):
        q = 0
    x, z, xt, P, Pt, theta = make_inputs(*shape)
    t = lambda a: None if a is None or q == 0 else torch.as_tensor(np.ascontiguousarray(a), device=dev)  # noqa: E731
    X, Z, XT = (torch.as_tensor(np.ascontiguousarray(a), device=dev) for a in (x, z, xt))
    PI, PT = t(P), t(Pt)
    J = torch.zeros(m * q * d, dtype=torch.float64, device=dev) if q else None
    size = {"gpmp_nll_zero_mean": lambda: lib.gpmp_nll_ws_elems(n), "gpmp_predict_zero_mean": lambda: lib.gpmp_predict_ws_elems(n, m),
            "gpmp_reml": lambda: lib.gpmp_reml_ws_elems(n, q), "gpmp_nll_grad": lambda: lib.gpmp_nll_grad_ws_elems(n, d, q),
            "gpmp_loo": lambda: lib.gpmp_loo_ws_elems(n, q), "gpmp_predict_mean": lambda: lib.gpmp_predict_mean_ws_elems(n, m, q),
            "gpmp_predict_grad": lambda: lib.gpmp_predict_grad_ws_elems(n, m, d, q)}[name]()
    size = int(size)
    assert size > 0
    buf = torch.full((size + TAIL,), fill, dtype=torch.float64, device=dev)
    ws = buf[:size]
    out = lambda *shp: torch.full(shp, float("nan"), dtype=torch.float64, device=dev)  # noqa: E731
    info = torch.full((1,), -1, dtype=torch.int32, device=dev)
    hv, ptr, st = _lib.host_vec(theta), gnp._ptr, gnp._stream()
    mean_args = (ptr(X), ptr(Z), ptr(PI), max(q, 1), n, d, q, 2, hv, 1, ptr(ws))
    if name == "gpmp_nll_zero_mean":
        outs = {"nll": out(1)}
        rc = lib.gpmp_nll_zero_mean(ptr(X), ptr(Z), n, d, 2, hv, 1, ptr(ws), ptr(outs["nll"]), ptr(info), st)
    elif name == "gpmp_predict_zero_mean":
        outs = {"zpm": out(m), "zpv": out(m)}
        rc = lib.gpmp_predict_zero_mean(ptr(X), ptr(Z), ptr(XT), n, m, d, 2, hv, 1, 1, ptr(ws), ptr(outs["zpm"]), ptr(outs["zpv"]), ptr(info), st)
    elif name == "gpmp_reml":
        outs = {"value": out(1)}
        rc = lib.gpmp_reml(*mean_args, ptr(outs["value"]), ptr(info), st)
    elif name == "gpmp_nll_grad":
        outs = {"value": out(1), "grad": out(len(theta))}
        rc = lib.gpmp_nll_grad(*mean_args, ptr(outs["value"]), ptr(outs["grad"]), ptr(info), st)
    elif name == "gpmp_loo":
        outs = {"zloo": out(n), "sigma2loo": out(n), "eloo": out(n)}
        rc = lib.gpmp_loo(*mean_args, ptr(outs["zloo"]), ptr(outs["sigma2loo"]), ptr(outs["eloo"]), ptr(info), st)
    elif name == "gpmp_predict_mean":
        outs = {"zpm": out(m), "zpv": out(m)}
        rc = lib.gpmp_predict_mean(ptr(X), ptr(Z), ptr(PI), q, ptr(XT), ptr(PT), q, n, m, d, q, 2, hv, 1, 1, ptr(ws), ptr(outs["zpm"]),
                                   ptr(outs["zpv"]), ptr(info), st)
    else:
        outs = {"zpm": out(m), "zpv": out(m), "gzpm": out(m, d), "gzpv": out(m, d)}
        rc = lib.gpmp_predict_grad(ptr(X), ptr(Z), ptr(PI), q, ptr(XT), ptr(PT), q, ptr(J), n, m, d, q, 2, hv, 1, 1, 1, ptr(ws),
                                   ptr(outs["zpm"]), ptr(outs["zpv"]), ptr(outs["gzpm"]), ptr(outs["gzpv"]), ptr(info), st)
    _lib.check(rc, name)
    return {k: v.cpu().numpy() for k, v in outs.items()}, int(info.item()), buf[size:].cpu().numpy()


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "n%d_m%d_d%d_q%d" % s)
def test_drivers_do_not_depend_on_workspace_content_and_stay_inside(env, shape):
    for name in DRIVERS:
        if name == "gpmp_predict_mean" and shape[3] == 0:
            continue
        runs = [run_driver(env, name, shape, fill) for fill in FILLS]
        for (outs, info, tail), fill in zip(runs, FILLS):
            assert info == 0, (name, fill, info)
            for k, v in outs.items():
                assert np.isfinite(v).all(), (name, k, fill)
            assert np.array_equal(tail, np.full(TAIL, fill)), (name, fill)
        (a, ia, _), (b, ib, _) = runs
        assert ia == ib
        for k in a:
            assert np.array_equal(a[k], b[k]), (name, k, float(np.max(np.abs(a[k] - b[k]))))
