"""gpmp_posterior_mean_wide without a GPU: the two symbols, the workspace query, the argument checks (host code, no device) and the
compile-time resources of the kernels of csrc/posterior_mean_wide.hip, compiled by the Makefile's own command."""
import ctypes
import os
import re

import pytest

from .test_kernel_resources_cpu import HIPCC, resources_by_makefile
from .test_posterior_mean_cpu import lib  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gpmp_posterior_mean_wide_ws_elems", "gpmp_posterior_mean_wide")
MEAN = ("xi", "A", "lda", "xt", "Pt", "ldpt", "B", "ldb", "n", "m", "s", "d", "q", "p", "theta", "noise", "ws", "O", "ldo")
INTS = dict(lda=8, ldb=8, ldpt=4, ldo=8, n=5, m=3, s=3, d=70, q=2, p=2, noise=0)


def test_symbols_are_declared_exported_and_bound(lib):
    from gpmp_amd import _lib

    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gpmp_hip.h")).read(), flags=re.S)
    for name in NEW:
        assert re.search(rf"\b{name}\s*\(", text) and name in _lib.SIGNATURES and hasattr(lib, name), name


def test_workspace_query(lib):
    ws = lib.gpmp_posterior_mean_wide_ws_elems
    for bad in ((0, 1, 1, 3), (2, 0, 1, 3), (2, 1, 0, 3), (2, 1, 4097, 3), (2, 1, 1, 0), (2, 1, 1, 16385), (2 ** 31 - 1, 1, 1, 3)):
        assert ws(*bad) == 0, bad
    for n, m, s, d in ((1, 1, 1, 1), (1000, 65, 17, 70), (300, 7, 4096, 16384)):
        assert ws(n, m, s, d) >= n * d + d, (n, m, s, d)
    # the partial slices are bounded however large the problem is (32 MB); the scaled points and the d scales are not
    assert 2 ** 27 + 128 <= ws(2 ** 20, 2 ** 20, 64, 128) <= 2 ** 27 + 128 + (1 << 22) + 16


@pytest.mark.parametrize("kw, arg", [(dict(lda=2), 3), (dict(ldo=2), 19), (dict(ldb=2), 7), (dict(ldpt=1), 5), (dict(s=0), 11),
                                     (dict(d=16385), 12), (dict(B=None), 7)])
def test_argument_checks(lib, kw, arg):
    """Every case fails a host check, so the host scratch behind the pointers is never handed to a kernel."""
    bufs = {k: (ctypes.c_double * 128)() for k in MEAN if k not in INTS}
    a = dict({k: ctypes.cast(b, ctypes.c_void_p) for k, b in bufs.items()}, **INTS)
    a.update(kw)
    rc = lib.gpmp_posterior_mean_wide(*[a[k] for k in MEAN], None)
    assert rc == -arg and b"argument" in lib.gpmp_last_error(), (rc, lib.gpmp_last_error())


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_kernels_use_no_scratch_and_spill_no_vector_registers():
    res = resources_by_makefile("posterior_mean_wide.o")
    main = [k for k in res if "pmw_contract_kernel" in k]
    assert len(main) == 4, sorted(res)                       # 1 .. 4 column tiles
    assert any("pmw_finalize_kernel" in k for k in res) and any("scale_points_kernel" in k for k in res)
    for k, v in res.items():
        assert v["ScratchSize"] == 0 and v["VGPRs Spill"] == 0 and v["VGPRs"] <= 256, (k, v)
