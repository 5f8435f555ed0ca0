"""The Strassen step of the forward solve's large updates (linalg.hip: strassen_update) through its test hook
gpmp_debug_strassen_update:  B2 (R x N) -= L21 (R x R) X1 (R x N)  by seven half-size products that accumulate straight into the
quadrants of B2 (two-destination epilogue of the LDS-direct GEMM) plus the block sums of the operands.

Reference: the product in numpy.longdouble on the host.  Allowed error: 8 x the error of the plain GEMM route (gpmp_dgemm) on the
same inputs against the same reference -- one Strassen level multiplies the normwise error constant by a small factor (Higham,
Accuracy and Stability of Numerical Algorithms, 23.2.2) and gives up the componentwise bound -- with a floor of
4 K u max|A| max|B| so that an unusually accurate plain run cannot fail the test.  Both errors are printed.
Sentinels around every buffer and in the padding of every row: nothing outside the R x N window of B2 may change."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GUARD = 64                      # doubles before and after every buffer (keeps the 16-byte alignment)
SENTINEL = -7.25e7

# (R, N, extra leading dimension)
CASES = [
    (256, 258, 0),              # one tile per quadrant plus a peeled pair of columns
    (512, 770, 0),              # peel of 2 columns beside a 2 x 3-tile quadrant
    (512, 1024, 0),             # no peel
    (768, 1150, 18),            # strided blocks (ld > N), quadrant rows 384, peel of 126 columns
]


@pytest.fixture(scope="module")
def env():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import gpmp_amd.num as gnp
    from gpmp_amd import _lib

    return torch, gnp, _lib, _lib.load()


def _six_decades(rng, shape):
    return rng.choice([-1.0, 1.0], size=shape) * 10.0 ** rng.uniform(-3.0, 3.0, size=shape)


def _guarded(torch, dev, host, ld):
    """host (rows x cols) inside a sentinel-filled device buffer: GUARD doubles, rows x ld, GUARD doubles"""
    rows, cols = host.shape
    full = np.full(2 * GUARD + rows * ld, SENTINEL)
    full[GUARD:GUARD + rows * ld].reshape(rows, ld)[:, :cols] = host
    return torch.as_tensor(full, device=dev), full


@pytest.mark.parametrize("R, N, pad", CASES, ids=[f"R{r}_N{n}_pad{p}" for r, n, p in CASES])
def test_strassen_update_vs_longdouble(env, R, N, pad):
    torch, gnp, _lib, lib = env
    dev = gnp._dev()
    rng = np.random.default_rng(1000 * R + N)
    A = rng.uniform(-1.0, 1.0, size=(R, R))
    X = _six_decades(rng, (R, N))
    C0 = _six_decades(rng, (R, N))
    ref = C0.astype(np.longdouble) - A.astype(np.longdouble) @ X.astype(np.longdouble)
    ldl, ldx, ldb = R + pad, N + pad, N + pad
    dA, hA = _guarded(torch, dev, A, ldl)
    dX, hX = _guarded(torch, dev, X, ldx)
    dC, hC = _guarded(torch, dev, C0, ldb)
    dP, _ = _guarded(torch, dev, C0, ldb)                       # the plain route works on its own copy
    ne = int(lib.gpmp_debug_strassen_ws_elems(R, N))
    nh = (N // 2) // 128 * 128
    assert ne == (R // 2) * (R // 2) + (R // 2) * nh            # (both terms are multiples of 16 here)
    dS = torch.full((2 * GUARD + ne,), SENTINEL, dtype=torch.float64, device=dev)
    base = lambda t: t.data_ptr() + 8 * GUARD  # noqa: E731
    _lib.check(lib.gpmp_debug_strassen_update(base(dA), ldl, base(dX), ldx, base(dC), ldb, R, N, base(dS), ne, gnp._stream()),
               "gpmp_debug_strassen_update")
    _lib.check(lib.gpmp_dgemm(0, 0, R, N, R, -1.0, base(dA), ldl, base(dX), ldx, 1.0, base(dP), ldb, 0, gnp._stream()), "gpmp_dgemm")
    torch.cuda.synchronize()

    def window(t):
        return t.cpu().numpy()[GUARD:GUARD + R * ldb].reshape(R, ldb)[:, :N]

    err_s = float(np.max(np.abs(window(dC).astype(np.longdouble) - ref)))
    err_p = float(np.max(np.abs(window(dP).astype(np.longdouble) - ref)))
    u = 2.0 ** -53
    floor = 4.0 * R * u * np.max(np.abs(A)) * np.max(np.abs(X))
    print(f"R={R} N={N} ld+{pad}: strassen err {err_s:.3e}  plain err {err_p:.3e}  ratio {err_s / err_p:.2f}  floor {floor:.3e}")
    assert err_s <= max(8.0 * err_p, floor), (err_s, err_p, floor)
    # nothing outside the R x N window of B2 changed: guards, row padding; the operands are bit-for-bit what they were
    out = dC.cpu().numpy()
    mask = np.ones(out.shape, dtype=bool)
    mask[GUARD:GUARD + R * ldb].reshape(R, ldb)[:, :N] = False
    assert np.array_equal(out[mask], hC[mask])
    assert np.array_equal(dA.cpu().numpy(), hA) and np.array_equal(dX.cpu().numpy(), hX)
    s = dS.cpu().numpy()
    assert np.all(s[:GUARD] == SENTINEL) and np.all(s[GUARD + ne:] == SENTINEL)


def test_strassen_hook_rejects_shapes_it_cannot_take(env):
    torch, gnp, _lib, lib = env
    dev = gnp._dev()
    buf = torch.zeros(4096, dtype=torch.float64, device=dev)
    p = buf.data_ptr()
    assert lib.gpmp_debug_strassen_ws_elems(384, 512) == 0 and lib.gpmp_debug_strassen_ws_elems(256, 254) == 0
    assert lib.gpmp_debug_strassen_update(p, 384, p, 512, p, 512, 384, 512, p, 4096, gnp._stream()) < 0        # R not a multiple of 256
    assert lib.gpmp_debug_strassen_update(p, 256, p, 257, p, 258, 256, 257, p, 4096, gnp._stream()) < 0        # odd N
    assert lib.gpmp_debug_strassen_update(p, 256, p, 258, p, 258, 256, 258, p, 16, gnp._stream()) < 0          # scratch too small
    assert b"argument" in lib.gpmp_last_error()
