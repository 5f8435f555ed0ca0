"""Host-side checks of the prediction gradients (Model.predict_gradient, gpmp_predict_grad / gpmp_predict_grad_reduce): the NumPy
restatement against the reference fixture, the workspace queries, the compile-time resources of the new kernels and the
exported surface.  No GPU needed."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from . import predict_grad_numpy as pgn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gpmp_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
FIXTURE = os.path.join(ROOT, "tests", "golden", "ref_predict_grad.npz")
NEW = ("gpmp_predict_grad_reduce_ws_elems", "gpmp_predict_grad_reduce", "gpmp_predict_grad_ws_elems", "gpmp_predict_grad")


@pytest.fixture(scope="module")
def lib():
    from gpmp_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g

        g.build()
    return _lib.load()


def numpy_case(g, c):
    cs = pgn.case(g, c)
    xi, xt, zi, th, kind = cs["xi"], cs["xt"], cs["zi"], cs["theta"], cs["kind"]
    if kind in ("const", "lin"):
        Pi, _ = pgn.designs(kind, xi)
        Pt, J = pgn.designs(kind, xt)
        return cs, pgn.predict_grad(xi, zi, xt, cs["p"], th, cs["noise"], Pi, Pt, J)
    if kind == "param":
        mi, _ = pgn.designs(kind, xi, cs["meanparam"])
        mt, gt = pgn.designs(kind, xt, cs["meanparam"])
        a, b, gm, gv = pgn.predict_grad(xi, zi - mi, xt, cs["p"], th, cs["noise"])
        return cs, (a + mt, b, gm + gt, gv)
    return cs, pgn.predict_grad(xi, zi, xt, cs["p"], th, cs["noise"])


def test_fixture_covers_the_issue_grid():
    g = np.load(FIXTURE)
    specs = [pgn.case(g, c) for c in range(int(g["ncases"]))]
    assert {s["p"] for s in specs} == {0, 1, 2, 3, 6, 10}
    assert {s["noise"] for s in specs} == {0, 1}
    assert {s["kind"] for s in specs} == {"zero", "param", "const", "lin"}
    assert {1, 3, 8} <= {s["d"] for s in specs} and max(s["d"] for s in specs) > 64
    for s in specs:      # two rows of xt coincide with rows of xi
        assert sum(bool(np.any(np.all(s["xi"] == r, axis=1))) for r in s["xt"]) == 2


@pytest.mark.parametrize("c", range(20))
def test_numpy_restatement_matches_the_reference_autograd(c):
    g = np.load(FIXTURE)
    cs, out = numpy_case(g, c)
    K, _, _ = pgn.cov_parts(cs["xi"], cs["xi"], cs["p"], cs["theta"], cs["noise"])
    tol = max(1e-12, 1e-16 * np.linalg.cond(K) * 100)
    for val, key in zip(out, ("zpm", "zpv", "gzpm", "gzpv")):
        ref = g[f"c{c}_{key}"]
        assert np.max(np.abs(val - ref)) <= tol * max(1.0, np.max(np.abs(ref))), (key, np.max(np.abs(val - ref)))


def test_workspace_queries_are_host_only_and_monotone(lib):
    assert lib.gpmp_predict_grad_ws_elems(0, 10, 3, 0) == 0 and lib.gpmp_predict_grad_ws_elems(10, 0, 3, 0) == 0
    assert lib.gpmp_predict_grad_ws_elems(10, 10, 0, 0) == 0 and lib.gpmp_predict_grad_ws_elems(10, 10, 3, -1) == 0
    assert lib.gpmp_predict_grad_ws_elems(10, 10, 3, 72) == 0 and lib.gpmp_predict_grad_ws_elems(10, 10, 16385, 0) == 0
    assert lib.gpmp_predict_grad_reduce_ws_elems(10, 10, 0) == 0 and lib.gpmp_predict_grad_reduce_ws_elems(-1, 10, 3) == 0
    sizes = (1, 2, 63, 64, 65, 129, 1000, 5000, 32768)
    for d in (1, 8, 64, 65, 300):
        for q in (0, 1, 4, 71):
            prev_n = 0
            for n in sizes:
                prev_m = 0
                for m in sizes:
                    w = lib.gpmp_predict_grad_ws_elems(n, m, d, q)
                    assert w > 0 and w >= prev_m, (n, m, d, q)
                    if q:
                        assert w >= lib.gpmp_predict_grad_ws_elems(n, m, d, q - 1)
                    prev_m = w
                w = lib.gpmp_predict_grad_ws_elems(n, 5000, d, q)
                assert w >= prev_n
                prev_n = w
            r = [lib.gpmp_predict_grad_reduce_ws_elems(n, m, d) for n in sizes for m in sizes]
            assert min(r) >= d
    for a, b in ((1, 2), (64, 65), (1000, 5000)):
        assert lib.gpmp_predict_grad_reduce_ws_elems(a, 100, 8) <= lib.gpmp_predict_grad_reduce_ws_elems(b, 100, 8)
        assert lib.gpmp_predict_grad_reduce_ws_elems(5000, a, 8) <= lib.gpmp_predict_grad_reduce_ws_elems(5000, b, 8)


def test_bad_arguments_are_rejected_before_any_device_call(lib):
    import ctypes

    from gpmp_amd import _lib

    fake = ctypes.c_void_p(0x1000)
    th = _lib.host_vec(np.zeros(4))
    # u without gu, neither weight, ldl < m, p above the limit, d above the wide limit
    assert lib.gpmp_predict_grad_reduce(fake, fake, 10, 10, 3, 2, th, 0, fake, None, 10, None, None, fake, None) < 0
    assert lib.gpmp_predict_grad_reduce(fake, fake, 10, 10, 3, 2, th, 0, None, None, 10, None, None, fake, None) < 0
    assert lib.gpmp_predict_grad_reduce(fake, fake, 10, 10, 3, 2, th, 0, None, fake, 9, None, fake, fake, None) < 0
    assert lib.gpmp_predict_grad_reduce(fake, fake, 10, 10, 3, 17, th, 0, fake, None, 10, fake, None, fake, None) < 0
    assert lib.gpmp_predict_grad_reduce(fake, fake, 10, 10, 16385, 2, th, 0, fake, None, 10, fake, None, fake, None) < 0
    assert b"argument" in lib.gpmp_last_error()
    # q > 0 needs J; the variance gradient needs its output
    args = [fake, fake, fake, 2, fake, fake, 2, None, 10, 10, 3, 2, 2, th, 0, 1, 1, fake, fake, fake, fake, fake, fake, None]
    assert lib.gpmp_predict_grad(*args) < 0 and b"J" in lib.gpmp_last_error()
    args[7], args[21] = fake, None
    assert lib.gpmp_predict_grad(*args) < 0 and b"gzpv" in lib.gpmp_last_error()


def test_new_symbols_are_declared_exported_and_bound(lib):
    from gpmp_amd import _lib

    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gpmp_hip.h")).read(), flags=re.S)
    for name in NEW:
        assert re.search(rf"\b{name}\s*\(", text), name
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_new_kernels_use_no_scratch_and_do_not_spill():
    cmd = [HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-mllvm", "-amdgpu-mfma-vgpr-form=1",
           "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(CSRC, "predict_grad.hip"), "-o", os.devnull]
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
    kernels = {k: v for k, v in res.items() if "predict_grad" in k}
    # 5 register tiers x 3 weight combinations, 3 wide variants, the finalize
    assert sum("predict_grad_kernel" in k for k in kernels) == 15 and sum("predict_grad_wide_kernel" in k for k in kernels) == 3
    for k, v in kernels.items():
        assert v.get("ScratchSize", 0) == 0, (k, v)
        assert v.get("VGPRs Spill", 0) == 0, (k, v)
