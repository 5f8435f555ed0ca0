"""Host arithmetic of the Strassen step (no GPU): the workspace queries of the prediction drivers return what they returned before
below the thresholds and grow by exactly the documented scratch above them (include/gpmp_hip.h: gpmp_strassen_ws_elems), and the
column split is a multiple of 128 that leaves an even number of columns over."""
import pytest

HUGE = 1 << 30


@pytest.fixture(scope="module")
def lib():
    from gpmp_amd import _lib

    return _lib.load()


def _pad16(v):
    return (v + 15) // 16 * 16


def _even(c):
    return c + (c & 1)


# (n, m): gpmp_predict_ws_elems, gpmp_predict_mean_ws_elems(q = 2), gpmp_predict_grad_ws_elems(d = 8, q = 2) before the step existed
OLD = {
    (32768, 50000): (2732409024, 2732509296, 2741080720),
    (16384, 16384): (545030176, None, None),
    (16384, 16000): (538627360, None, None),
    (4096, 10000): (62275648, None, None),
}


def test_workspace_sizes_below_and_above_the_thresholds(lib):
    try:
        for (n, m), (old, old_mean, old_grad) in OLD.items():
            lib.gpmp_set_strassen_thresholds(0, 0)
            need = {q: lib.gpmp_strassen_ws_elems(n, _even(m + 1 + q)) for q in (0, 2)}
            got = lib.gpmp_predict_ws_elems(n, m)
            got_mean, got_grad = lib.gpmp_predict_mean_ws_elems(n, m, 2), lib.gpmp_predict_grad_ws_elems(n, m, 8, 2)
            # the documented size: the largest qualifying update, R = n / 2 rows of X1 at the top of a power-of-two solve
            qualifies = n // 2 >= 8192 and _even(m + 1) >= 16384
            for q in (0, 2):
                nh = (_even(m + 1 + q) // 2) // 128 * 128
                assert need[q] == (_pad16((n // 4) ** 2) + _pad16((n // 4) * nh) if qualifies else 0), (n, m, q)
            assert got == old + need[0], (n, m)
            if old_mean is not None:
                assert got_mean == old_mean + need[2] and got_grad == old_grad + need[2]
            # thresholds above every update: the sizes from before the step
            lib.gpmp_set_strassen_thresholds(HUGE, HUGE)
            assert lib.gpmp_strassen_ws_elems(n, _even(m + 1)) == 0
            assert lib.gpmp_predict_ws_elems(n, m) == old
            if old_mean is not None:
                assert lib.gpmp_predict_mean_ws_elems(n, m, 2) == old_mean and lib.gpmp_predict_grad_ws_elems(n, m, 8, 2) == old_grad
        # lowered: a solve of 2048 rows qualifies with its 1024-row top update; the drivers without prediction points never grow
        lib.gpmp_set_strassen_thresholds(512, 256)
        assert lib.gpmp_strassen_ws_elems(2048, 1502) == 512 * 512 + 512 * 640
        assert lib.gpmp_strassen_ws_elems(2048, 16) == 0                      # few right-hand sides: the single-vector sweep
        assert lib.gpmp_strassen_ws_elems(512, 1502) == 0                     # one leaf, no update
        nll_low = lib.gpmp_nll_ws_elems(32768)
        lib.gpmp_set_strassen_thresholds(0, 0)
        assert lib.gpmp_nll_ws_elems(32768) == nll_low == 1079509296
    finally:
        lib.gpmp_set_strassen_thresholds(0, 0)


def test_column_split_is_whole_tiles_with_an_even_remainder(lib):
    """gpmp_debug_strassen_ws_elems(R, N) = pad16((R / 2)^2) + pad16((R / 2) Nh): Nh read back from it for N = 2 ... 60000"""
    for R in (256, 512, 1024, 2048, 4096, 8192, 16384):
        h = R // 2
        step = 1 if R == 256 else 97
        for N in range(2, 60001, step):
            e = lib.gpmp_debug_strassen_ws_elems(R, N)
            if N % 2 or N < 256:
                assert e == 0, (R, N)
                continue
            rest = e - h * h
            assert rest > 0 and rest % h == 0, (R, N, e)
            nh = rest // h
            assert nh % 128 == 0 and 2 * nh <= N and nh == (N // 2) // 128 * 128, (R, N, nh)
            assert (N - 2 * nh) % 2 == 0 and 0 <= N - 2 * nh < 256, (R, N, nh)
    for R in (0, -256, 128, 384, 300):
        assert lib.gpmp_debug_strassen_ws_elems(R, 1024) == 0
