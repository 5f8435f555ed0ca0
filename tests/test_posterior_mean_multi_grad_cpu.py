"""The many-column posterior mean with its Jacobian without a GPU: the two symbols, the workspace query and the argument checks (host
code, no device).  The compile-time resources of its kernels: test_posterior_mean_multi_cpu.py."""
import ctypes
import os
import re

import pytest

from .test_posterior_mean_cpu import lib  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gpmp_posterior_mean_multi_grad_ws_elems", "gpmp_posterior_mean_multi_grad")
ORDER = ("xi", "A", "lda", "xt", "Pt", "ldpt", "B", "ldb", "J", "n", "m", "s", "d", "q", "p", "theta", "noise", "ws", "O", "ldo", "G", "ldg")
INTS = dict(lda=8, ldb=8, ldpt=4, ldo=8, ldg=8, n=5, m=3, s=3, d=2, q=2, p=2, noise=0)


def test_symbols_are_declared_exported_and_bound(lib):
    from gpmp_amd import _lib
    from gpmp_amd.core import PosteriorMeans

    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gpmp_hip.h")).read(), flags=re.S)
    for name in NEW:
        assert re.search(rf"\b{name}\s*\(", text) and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert callable(PosteriorMeans.mean_and_gradient)


def test_workspace_query(lib):
    ws = lib.gpmp_posterior_mean_multi_grad_ws_elems
    for bad in ((0, 1, 1, 3), (2, 0, 1, 3), (2, 1, 0, 3), (2, 1, 4097, 3), (2, 1, 1, 0), (2, 1, 1, 65), (2 ** 31 - 1, 1, 1, 3)):
        assert ws(*bad) == 0, bad
    assert ws(1000, 65, 17, 3) >= 1000 * 3 + 7 * 65 * 17 * 4            # the scaled points and 7 partial slices of both outputs
    # the partial slices are bounded however large the problem is (32 MB), the scaled points are not
    assert 2 ** 26 <= ws(2 ** 20, 2 ** 20, 64, 64) <= 2 ** 26 + (1 << 22) + 16


@pytest.mark.parametrize("kw, arg", [(dict(d=65), 13), (dict(s=0), 12), (dict(lda=2), 3), (dict(ldo=2), 20), (dict(ldg=2), 22), (dict(ldb=2), 7),
                                     (dict(ldpt=1), 5), (dict(Pt=None), 5), (dict(B=None), 7), (dict(J=None), 9), (dict(G=None), 21)])
def test_argument_checks(lib, kw, arg):
    """Every case fails a host check, so the host scratch behind the pointers is never handed to a kernel."""
    bufs = {k: (ctypes.c_double * 64)() for k in ORDER if k not in INTS}
    a = dict({k: ctypes.cast(b, ctypes.c_void_p) for k, b in bufs.items()}, **INTS)
    a.update(kw)
    rc = lib.gpmp_posterior_mean_multi_grad(*[a[k] for k in ORDER], None)
    assert rc == -arg and b"argument" in lib.gpmp_last_error(), (rc, lib.gpmp_last_error())
