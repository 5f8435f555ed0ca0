"""The many-column posterior mean without a GPU: the four symbols, their workspace queries and argument checks (host code, no
device), and the compile-time resources of the kernels of csrc/posterior_mean_multi.hip (value and gradient instances), compiled
by the Makefile's own command."""
import ctypes
import os
import re

import pytest

from .test_kernel_resources_cpu import HIPCC, resources_by_makefile
from .test_posterior_mean_cpu import lib  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gpmp_posterior_weights_multi_ws_elems", "gpmp_posterior_weights_multi", "gpmp_posterior_mean_multi_ws_elems",
       "gpmp_posterior_mean_multi")
WEIGHTS = ("xi", "Z", "ldz", "Pi", "ldpi", "n", "s", "d", "q", "p", "theta", "noise", "ws", "A", "lda", "B", "ldb", "info")
MEAN = ("xi", "A", "lda", "xt", "Pt", "ldpt", "B", "ldb", "n", "m", "s", "d", "q", "p", "theta", "noise", "ws", "O", "ldo")
INTS = dict(ldz=8, ldpi=4, lda=8, ldb=8, ldpt=4, ldo=8, n=5, m=3, s=3, d=2, q=2, p=2, noise=0)


def test_symbols_are_declared_exported_and_bound(lib):
    from gpmp_amd import Model, _lib
    from gpmp_amd.core import PosteriorMeans, posterior_mean  # noqa: F401

    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gpmp_hip.h")).read(), flags=re.S)
    for name in NEW:
        assert re.search(rf"\b{name}\s*\(", text) and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert callable(Model.posterior_means) and callable(Model.conditional_sample_paths_from_data)
    assert posterior_mean.MAX_COLUMNS == int(re.search(r"#define\s+GPMP_MAX_COLUMNS\s+(\d+)", text).group(1))


def test_workspace_queries(lib):
    w, pm = lib.gpmp_posterior_weights_multi_ws_elems, lib.gpmp_posterior_mean_multi_ws_elems
    for bad in ((0, 1, 0), (-1, 1, 0), (5, 0, 0), (5, 4097, 0), (5, 1, -1), (5, 1, 72), (2, 1, 2), (2 ** 31 - 1, 1, 0)):
        assert w(*bad) == 0, bad
    for n, s, q in ((1, 1, 0), (2, 3, 1), (129, 17, 10), (1500, 4096, 71)):
        assert w(n, s, q) >= n * ((n + 15) // 16 * 16) + lib.gpmp_dinv_elems(n) + n * s, (n, s, q)
    for bad in ((0, 1, 1, 3), (2, 0, 1, 3), (2, 1, 0, 3), (2, 1, 4097, 3), (2, 1, 1, 0), (2, 1, 1, 65), (2 ** 31 - 1, 1, 1, 3)):
        assert pm(*bad) == 0, bad
    assert pm(1000, 65, 17, 3) >= 1000 * 3
    # the partial slices are bounded however large the problem is (32 MB), the scaled points are not
    assert 2 ** 26 <= pm(2 ** 20, 2 ** 20, 64, 64) <= 2 ** 26 + (1 << 22) + 16


@pytest.mark.parametrize("fn, order, kw, arg", [
    (NEW[1], WEIGHTS, dict(s=4097), 7), (NEW[1], WEIGHTS, dict(ldz=2), 3), (NEW[1], WEIGHTS, dict(lda=2), 14),
    (NEW[1], WEIGHTS, dict(ldb=2), 16), (NEW[1], WEIGHTS, dict(B=None), 16), (NEW[1], WEIGHTS, dict(n=2), 6),
    (NEW[3], MEAN, dict(d=65), 12), (NEW[3], MEAN, dict(s=0), 11), (NEW[3], MEAN, dict(lda=2), 3), (NEW[3], MEAN, dict(ldo=2), 19),
    (NEW[3], MEAN, dict(ldb=2), 7), (NEW[3], MEAN, dict(ldpt=1), 5),
])
def test_argument_checks(lib, fn, order, kw, arg):
    """Every case fails a host check, so the host scratch behind the pointers is never handed to a kernel."""
    bufs = {k: (ctypes.c_double * 64)() for k in order if k not in INTS}
    a = dict({k: ctypes.cast(b, ctypes.c_void_p) for k, b in bufs.items()}, **INTS)
    a.update(kw)
    rc = getattr(lib, fn)(*[a[k] for k in order], None)
    assert rc == -arg and b"argument" in lib.gpmp_last_error(), (rc, lib.gpmp_last_error())


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_value_and_gradient_kernels_use_no_scratch_and_spill_no_vector_registers():
    """One template serves both entries: its value instances have one component slot (the last template argument)."""
    res = resources_by_makefile("posterior_mean_multi.o")
    main = {k: tuple(map(int, re.search(r"pmm_contract_kernelILi(\d+)ELi(\d+)ELi(\d+)EE", k).groups())) for k in res if "pmm_contract_kernel" in k}
    assert len(main) == 32, sorted(res)
    value, grad = ({(dt, ct) for dt, ct, nc in main.values() if (nc == 1) == one} for one in (True, False))
    assert len(value) == 20, sorted(value)                   # five dimension tiers x 1 .. 4 column tiles
    assert len(grad) == 12, sorted(grad)                     # x_t in registers (d <= 8, d <= 16) or in LDS x 1 .. 4 column tiles
    assert any("pmm_finalize_kernel" in k for k in res) and any("scale_points_kernel" in k for k in res)
    for k, v in res.items():
        assert v["ScratchSize"] == 0 and v["VGPRs Spill"] == 0, (k, v)
    assert all(res[k]["VGPRs"] <= 256 for k in main)
