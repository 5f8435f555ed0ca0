"""Workspace sizes of the fused C-ABI drivers (csrc/drivers.hip) and of the batched driver, as literals: host arithmetic, no GPU.
All seven single-problem drivers share one layout description; five of the queries below keep the value they had before the
drivers were folded into one file, three lost a slot that no path of their entry point touched:
  gpmp_predict_ws_elems(n, m)         = pad16(before - 16 n)                  (the separate w column; every slot is padded now)
  gpmp_predict_mean_ws_elems(n, m, q) = before - pad16(n pad16(1 + q))        (the separate [z, P] block)
  gpmp_reml_ws_elems(n, q)            = before - pad16(n pad16(1 + q))        (the back-solve block X)
"""
import pytest


@pytest.fixture(scope="module")
def lib():
    from gpmp_amd import _lib

    return _lib.load()


def _pad16(v):
    return (v + 15) // 16 * 16


UNCHANGED = {
    "gpmp_nll_ws_elems": {(2,): 16480, (129,): 53456, (1500,): 3525312},
    "gpmp_loo_ws_elems": {(2, 1): 16768, (129, 10): 77168, (1500, 71): 6178080},
    "gpmp_nll_grad_ws_elems": {(2, 3, 0): 22912, (129, 70, 10): 115968, (1500, 3, 71): 6268496},
    "gpmp_predict_grad_ws_elems": {(2, 1, 3, 0): 16720, (129, 1, 3, 71): 92064, (129, 130, 70, 10): 112848, (1500, 701, 3, 71): 4982160},
    "gpmp_batch_ws_elems": {(512, 3, 16, 4, 1): 2647520, (4096, 3, 0, 2, 0): 34734848},
}

# (value before the fold, value now)
SHRUNK = {
    "gpmp_predict_ws_elems": {(2, 1): (16521, 16496), (129, 130): (74612, 72560), (1500, 701): (4658300, 4634304)},
    "gpmp_predict_mean_ws_elems": {(2, 1, 1): (16752, 16720), (129, 1, 71): (96496, 86176), (129, 130, 10): (76688, 74624),
                                   (1500, 701, 71): (4947504, 4827504)},
    "gpmp_reml_ws_elems": {(2, 0): (16672, 16640), (129, 10): (56320, 54256), (1500, 71): (3766352, 3646352)},
}


@pytest.mark.parametrize("name", sorted(UNCHANGED))
def test_unchanged_workspace_queries(lib, name):
    for args, want in UNCHANGED[name].items():
        assert getattr(lib, name)(*args) == want, (name, args)


@pytest.mark.parametrize("name", sorted(SHRUNK))
def test_queries_without_their_dead_slot(lib, name):
    for args, (before, now) in SHRUNK[name].items():
        assert getattr(lib, name)(*args) == now, (name, args)
        n, q = args[0], args[-1]
        if name == "gpmp_predict_ws_elems":
            assert now == _pad16(before - 16 * n)
        else:
            assert now == before - _pad16(n * _pad16(1 + q))


def test_out_of_range_arguments_give_zero(lib):
    assert lib.gpmp_nll_ws_elems(0) == 0
    assert lib.gpmp_predict_ws_elems(0, 1) == 0 and lib.gpmp_predict_ws_elems(2, 0) == 0
    assert lib.gpmp_reml_ws_elems(0, 0) == 0 and lib.gpmp_reml_ws_elems(5, 72) == 0
    assert lib.gpmp_loo_ws_elems(0, 1) == 0 and lib.gpmp_loo_ws_elems(5, 72) == 0
    assert lib.gpmp_nll_grad_ws_elems(0, 3, 0) == 0 and lib.gpmp_nll_grad_ws_elems(5, 3, 72) == 0 and lib.gpmp_nll_grad_ws_elems(5, 0, 0) == 0
    assert lib.gpmp_predict_mean_ws_elems(0, 1, 1) == 0 and lib.gpmp_predict_mean_ws_elems(2, 0, 1) == 0
    assert lib.gpmp_predict_mean_ws_elems(2, 1, 0) == 0 and lib.gpmp_predict_mean_ws_elems(2, 1, 72) == 0       # q = 0: gpmp_predict_ws_elems
    for bad in ((0, 1, 3, 0), (2, 0, 3, 0), (2, 1, 0, 0), (2, 1, 16385, 0), (2, 1, 3, 72)):
        assert lib.gpmp_predict_grad_ws_elems(*bad) == 0, bad
    for bad in ((0, 3, 0, 2, 0), (512, 0, 0, 2, 0), (512, 3, 17, 2, 0), (512, 3, 0, 0, 0)):
        assert lib.gpmp_batch_ws_elems(*bad) == 0, bad
