"""gpmp_fourier_paths without a GPU: the two symbols, the workspace query, the argument checks (host code, no device), the
compile-time resources of csrc/fourier_paths.hip by the Makefile's own command, and the law of the host-side feature draw."""
import ctypes
import os
import re

import numpy as np
import pytest

from .test_kernel_resources_cpu import HIPCC, resources_by_makefile
from .test_posterior_mean_cpu import lib  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = ("xt", "omega", "ldomega", "phase", "W", "ldw", "m", "r", "s", "d", "ws", "out", "ldo")
INTS = dict(ldomega=8, ldw=8, ldo=8, m=3, r=5, s=3, d=7)


def test_symbols_are_declared_exported_and_bound(lib):
    from gpmp_amd import _lib

    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gpmp_hip.h")).read(), flags=re.S)
    for name in ("gpmp_fourier_paths_ws_elems", "gpmp_fourier_paths"):
        assert re.search(rf"\b{name}\s*\(", text) and name in _lib.SIGNATURES and hasattr(lib, name), name


def test_workspace_query(lib):
    ws = lib.gpmp_fourier_paths_ws_elems
    for bad in ((0, 1, 1, 3), (2, 0, 1, 3), (2, 1, 0, 3), (2, 1, 4097, 3), (2, 1, 1, 0), (2, 1, 1, 16385), (2 ** 31 - 1, 1, 1, 3)):
        assert ws(*bad) == 0, bad
    for m, r, s, d in ((1, 1, 1, 1), (65, 1000, 17, 70), (7, 300, 4096, 16384)):
        assert ws(m, r, s, d) > 0, (m, r, s, d)
    assert ws(17, 4096, 5, 3) >= 31 * 17 * 5                  # one slice per 128 features when m is small
    assert ws(2 ** 20, 2 ** 20, 64, 8) <= (1 << 22) + 16      # bounded (32 MB) however large the problem is


@pytest.mark.parametrize("kw, arg", [(dict(ldomega=6), 3), (dict(ldw=2), 6), (dict(ldo=2), 13), (dict(m=0), 7), (dict(r=2 ** 30 + 1), 8),
                                     (dict(s=4097), 9), (dict(d=16385), 10), (dict(phase=None), 4), (dict(ws=None), 11)])
def test_argument_checks(lib, kw, arg):
    """Every case fails a host check, so the host scratch behind the pointers is never handed to a kernel."""
    bufs = {k: (ctypes.c_double * 128)() for k in ARGS if k not in INTS}
    a = dict({k: ctypes.cast(b, ctypes.c_void_p) for k, b in bufs.items()}, **INTS)
    a.update(kw)
    rc = lib.gpmp_fourier_paths(*[a[k] for k in ARGS], None)
    assert rc == -arg and b"argument" in lib.gpmp_last_error(), (rc, lib.gpmp_last_error())


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_kernels_use_no_scratch_and_spill_no_vector_registers():
    res = resources_by_makefile("fourier_paths.o")
    assert len([k for k in res if "fp_paths_kernel" in k]) == 4 and any("fp_finalize_kernel" in k for k in res), sorted(res)
    for k, v in res.items():
        assert v["ScratchSize"] == 0 and v["VGPRs Spill"] == 0 and v["VGPRs"] <= 256, (k, v)


@pytest.mark.parametrize("p, d", [(0, 1), (0, 3), (2, 1), (2, 3)])
def test_feature_draw_has_the_matern_covariance(p, d):
    """K^(x, y) = (2 sigma^2 / R) sum_k cos(2 pi (w_k.x + b_k)) cos(2 pi (w_k.y + b_k)) from the host draw against the oracle's Matern
    covariance on 100 pairs.  2 cos a cos b = cos(a - b) + cos(a + b) with a uniform phase has variance <= 1, so the standard
    error of K^ is <= sigma^2 sqrt(2 / R); the bound is 6 of those (derived, not measured)."""
    import torch

    from gpmp_amd.core.fourier_paths import draw_features
    from oracle import gp_oracle as orc

    R, rng = 16384, np.random.default_rng(7 + p + d)
    theta = np.concatenate(([np.log(1.7)], -np.log(0.3 + 0.5 * rng.random(d))))
    omega, phase, w = (t.numpy() for t in draw_features(p, theta, 0, 2, R, torch.Generator(device="cpu").manual_seed(1234)))
    assert omega.shape == (R, d) and phase.shape == (R,) and w.shape == (R, 2) and 0.0 <= phase.min() and phase.max() < 1.0
    x = rng.random((100, d))
    y = x + rng.standard_normal((100, d)) * 0.4 * rng.random((100, 1))
    cx, cy = (np.cos(2.0 * np.pi * (pts @ omega.T + phase)) for pts in (x, y))
    khat = 2.0 * np.exp(theta[0]) / R * np.sum(cx * cy, axis=1)
    err = np.abs(khat - orc.maternp_covariance(x, y, p, theta, pairwise=True))
    assert err.max() <= 6.0 * np.exp(theta[0]) * np.sqrt(2.0 / R), err.max() / (np.exp(theta[0]) * np.sqrt(2.0 / R))
