"""The fitted posterior mean without a GPU: the dual form against the reference's outputs (NumPy only), the four new symbols, their
argument checks (host code, no device), and the compile-time resources of the new kernels."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from . import posterior_mean_numpy as pmn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "ref_predict_grad.npz")
CSRC = os.path.join(ROOT, "gpmp_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
NEW = ("gpmp_posterior_weights_ws_elems", "gpmp_posterior_weights", "gpmp_posterior_mean_ws_elems", "gpmp_posterior_mean")


@pytest.mark.parametrize("c", range(20))
def test_dual_form_reproduces_the_reference(c):
    """alpha, beta by the Cholesky route, then value and gradient from the weights alone: zpm and gzpm of the reference's autograd
    run, under the tolerance rule.  Pins the formula the kernel implements, independent of the library."""
    g = np.load(FIXTURE)
    cs = pmn.fixture_case(g, c)
    xi, xt, th, p, noise = cs["xi"], cs["xt"], cs["theta"], cs["p"], cs["noise"]
    alpha, beta = pmn.weights(xi, cs["zc"], p, th, noise, cs["Pi"])
    zpm, gm = pmn.mean_and_gradient(xi, alpha, xt, p, th, noise, cs["Pt"], beta, cs["J"])
    tol = pmn.tolerance(xi, p, th, noise)
    pmn.close(zpm + cs["prior"], cs["zpm"], tol, "zpm")
    pmn.close(gm + cs["prior_grad"], cs["gzpm"], tol, "gzpm")


@pytest.fixture(scope="module")
def lib():
    from gpmp_amd import _lib

    return _lib.load()


def _pad16(v):
    return (v + 15) // 16 * 16


def test_new_symbols_are_declared_exported_and_bound(lib):
    from gpmp_amd import _lib

    text = open(os.path.join(ROOT, "include", "gpmp_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(gpmp_[a-z0-9_]+)\s*\(", text))
    for name in NEW:
        assert name in declared, name
        assert name in _lib.SIGNATURES, name
        assert hasattr(lib, name), name
    assert lib.gpmp_hip_abi_version() == 1
    from gpmp_amd.core import PosteriorMean  # noqa: F401
    from gpmp_amd import Model

    assert callable(Model.posterior_mean)


def test_workspace_queries(lib):
    w, pm = lib.gpmp_posterior_weights_ws_elems, lib.gpmp_posterior_mean_ws_elems
    for bad in ((0, 0), (-1, 0), (5, -1), (5, 72), (2 ** 31 - 1, 0)):
        assert w(*bad) == 0, bad
    for n, q in ((1, 0), (2, 1), (129, 10), (1500, 71)):
        assert w(n, q) >= n * _pad16(n) + lib.gpmp_dinv_elems(n) > 0, (n, q)
    for bad in ((0, 1, 3, 0), (2, 0, 3, 0), (2, 1, 0, 0), (2, 1, 65, 0), (2, 1, 65, 1), (-1, 1, 3, 0), (2, -1, 3, 1), (2 ** 31 - 1, 1, 3, 0),
                (2, 2 ** 31 - 1, 3, 0)):
        assert pm(*bad) == 0, bad
    for n, m, d in ((1, 1, 1), (129, 1, 64), (1000, 65, 3), (32768, 50000, 8)):
        assert pm(n, m, d, 0) >= n * d, (n, m, d)
        assert pm(n, m, d, 1) >= pm(n, m, d, 0), (n, m, d)         # the query with the gradient covers the call without
    # the partial slices are bounded however large the problem is (32 MB), the scaled points are not
    assert pm(2 ** 20, 2 ** 20, 64, 1) <= _pad16(2 ** 20 * 64) + (1 << 22) + 16


def _scratch():
    buf = (ctypes.c_double * 8192)()
    return buf, ctypes.cast(buf, ctypes.c_void_p)


def _mean_args(**kw):
    """Valid arguments of gpmp_posterior_mean over host scratch (never launched: every case below fails a host check)."""
    keep = []
    a = {}
    for k in ("xi", "alpha", "xt", "Pt", "beta", "J", "theta", "ws", "zpm", "gzpm"):
        buf, a[k] = _scratch()
        keep.append(buf)
    a.update(ldpt=4, n=5, m=3, d=2, q=2, p=2, noise=0)
    a.update(kw)
    order = ("xi", "alpha", "xt", "Pt", "ldpt", "beta", "J", "n", "m", "d", "q", "p", "theta", "noise", "ws", "zpm", "gzpm")
    return keep, [a[k] for k in order] + [None]


def _weights_args(**kw):
    keep = []
    a = {}
    for k in ("xi", "zi", "Pi", "theta", "ws", "alpha", "beta", "info"):
        buf, a[k] = _scratch()
        keep.append(buf)
    a.update(ldpi=4, n=5, d=2, q=2, p=2, noise=0)
    a.update(kw)
    order = ("xi", "zi", "Pi", "ldpi", "n", "d", "q", "p", "theta", "noise", "ws", "alpha", "beta", "info")
    return keep, [a[k] for k in order] + [None]


@pytest.mark.parametrize("kw, arg, word", [
    (dict(d=65), 10, b"d outside"),
    (dict(beta=None), 6, b"beta"),
    (dict(Pt=None), 4, b"Pt"),
    (dict(ldpt=1), 4, b"ldpt"),
    (dict(J=None), 7, b"J is NULL"),
    (dict(p=17), 12, b"p outside"),
    (dict(q=72), 11, b"q outside"),
    (dict(m=0), 9, b"m outside"),
    (dict(ws=None), 15, b"ws"),
])
def test_posterior_mean_argument_checks(lib, kw, arg, word):
    keep, args = _mean_args(**kw)
    rc = lib.gpmp_posterior_mean(*args)
    msg = lib.gpmp_last_error()
    assert rc == -arg and b"argument" in msg and word in msg, (rc, msg)


@pytest.mark.parametrize("kw, arg, word", [
    (dict(beta=None), 13, b"beta_dev"),
    (dict(n=2), 5, b"n <= q"),
    (dict(p=17), 8, b"p outside"),
    (dict(Pi=None), 3, b"Pi"),
    (dict(ldpi=1), 3, b"ldpi"),
    (dict(d=16385), 6, b"d outside"),
])
def test_posterior_weights_argument_checks(lib, kw, arg, word):
    keep, args = _weights_args(**kw)
    rc = lib.gpmp_posterior_weights(*args)
    msg = lib.gpmp_last_error()
    assert rc == -arg and b"argument" in msg and word in msg, (rc, msg)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_new_kernels_use_no_scratch_and_spill_no_vector_registers():
    """As tests/test_kernel_resources_cpu.py: one store into the by-value parameter block, or one register too many in the widest
    dimension tier, and the compiler moves the block or the accumulators to scratch memory without a line of arithmetic changing."""
    cmd = [HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-mllvm", "-amdgpu-mfma-vgpr-form=1",
           "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(CSRC, "posterior_mean.hip"), "-o", os.devnull]
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
    main = [k for k in res if "posterior_mean_kernel" in k]
    assert len(main) == 10, sorted(res)                    # five dimension tiers, with and without the gradient
    for frag in ("posterior_mean_kernel", "posterior_mean_finalize_kernel", "pm_scale_points_kernel"):
        hit = {k: v for k, v in res.items() if frag in k}
        assert hit, (frag, sorted(res))
        for k, v in hit.items():
            assert "ScratchSize" in v and "VGPRs Spill" in v, (k, v)
            assert v["ScratchSize"] == 0, (k, v)
            assert v["VGPRs Spill"] == 0, (k, v)
