"""The Python callers of the fused drivers on top of gpmp_amd/core/fused.py, at n = 40, m = 7, d = 2: where ``fused_prediction`` steps
aside instead of raising, the snapshot of a fitted posterior mean, and the one sentence of a failed call."""
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
N, M, D = 40, 7, 2


@pytest.fixture(scope="module")
def env():
    import torch

    assert torch.cuda.is_available()
    import gpmp_amd as gp
    import gpmp_amd.num as gnp

    rng = np.random.default_rng(2026)
    xi, xt = rng.random((N, D)), rng.random((M, D))
    zi = np.sin(3.0 * xi[:, 0]) + xi[:, 1]
    theta = np.array([0.2, -np.log(0.4), -np.log(0.6)])
    return gp, gnp, torch, xi, zi, xt, theta


def _lin(gnp):
    return lambda x, param: gnp.hstack((gnp.ones((x.shape[0], 1)), x))


def _dup(gnp):
    return lambda x, param: gnp.hstack((gnp.ones((x.shape[0], 1)), gnp.ones((x.shape[0], 1))))


def _model(env, mean, theta=None, meantype="linear_predictor", meanparam=None):
    gp, gnp, _, _, _, _, th = env
    return gp.Model(mean, gp.kernel.MaternCovariance(2), meanparam, th.copy() if theta is None else theta, meantype)


def _outcome(f):
    """What a call gives: its arrays, or the type and text of what it raises."""
    try:
        return ("value",) + tuple(np.asarray(a) for a in f())
    except Exception as e:  # noqa: BLE001 -- the comparison below is the assertion
        return ("raised", type(e), str(e))


def test_fused_prediction_steps_aside_without_raising(env, monkeypatch):
    gp, gnp, torch, xi, zi, xt, th = env
    from gpmp_amd.core import kriging

    X, Z, XT = gnp.asarray(xi), gnp.asarray(zi), gnp.asarray(xt)
    monkeypatch.delenv("GPMP_PREDICT_FUSED", raising=False)
    for model in (_model(env, None, meantype="zero"), _model(env, _lin(gnp))):
        out = kriging.fused_prediction(model, X, Z, XT)
        assert out is not None and out[0].shape == (M,) and out[1].shape == (M,)      # the route itself is open here
        assert kriging.fused_prediction(model, X, Z, X) is None                        # xt is xi
        monkeypatch.setenv("GPMP_PREDICT_FUSED", "0")
        assert kriging.fused_prediction(model, X, Z, XT) is None
        monkeypatch.delenv("GPMP_PREDICT_FUSED")
        model.covparam = np.zeros(5)                                                    # 1 + d = 3 expected
        assert kriging.fused_prediction(model, X, Z, XT) is None
        with pytest.raises(ValueError, match="covparam has 5 entries, expected 3"):    # the general route states the error
            model.predict(xi, zi, xt)


def test_rank_deficient_design_goes_to_the_general_route(env, monkeypatch):
    gp, gnp, torch, xi, zi, xt, th = env
    from gpmp_amd.core import kriging

    monkeypatch.delenv("GPMP_PREDICT_FUSED", raising=False)
    bad = _model(env, _dup(gnp))
    assert kriging.fused_prediction(bad, gnp.asarray(xi), gnp.asarray(zi), gnp.asarray(xt)) is None
    through_fused = _outcome(lambda: bad.predict(xi, zi, xt))
    monkeypatch.setenv("GPMP_PREDICT_FUSED", "0")
    general = _outcome(lambda: bad.predict(xi, zi, xt))
    assert through_fused[0] == general[0]
    if general[0] == "raised":
        assert through_fused[1:] == general[1:]
    else:
        for a, b in zip(through_fused[1:], general[1:]):
            np.testing.assert_array_equal(a, b)


def test_one_sentence_with_the_same_info_for_both_callers(env):
    """Two equal columns: the second pivot of P^T K^-1 P fails, info = n + 2, in gpmp_predict_grad and in gpmp_posterior_weights."""
    gp, gnp, torch, xi, zi, xt, th = env
    bad = _model(env, _dup(gnp))
    with pytest.raises(np.linalg.LinAlgError) as eg:
        bad.predict_gradient(xi, zi, xt)
    with pytest.raises(np.linalg.LinAlgError) as ep:
        bad.posterior_mean(xi, zi)
    sentence = r"P\^T K\^-1 P is singular \(rank-deficient mean design\) \(info = (\d+)\)"
    mg = re.fullmatch("predict_gradient: " + sentence, str(eg.value))
    mp = re.fullmatch("posterior_mean: " + sentence, str(ep.value))
    assert mg and mp, (str(eg.value), str(ep.value))
    assert int(mg.group(1)) == int(mp.group(1)) == N + 2


def test_posterior_mean_keeps_its_parameters(env):
    gp, gnp, torch, xi, zi, xt, th = env
    mean = lambda x, param: (param[0] + param[1] * x[:, 0]).reshape(-1, 1)  # noqa: E731
    mp = torch.tensor([0.3, 1.1], dtype=torch.float64, device="cuda")
    for model in (_model(env, mean, meantype="parameterized", meanparam=mp.clone()), _model(env, _lin(gnp))):
        post = model.posterior_mean(xi, zi)
        v, g = post.mean_and_gradient(xt)
        a, b = post.alpha.clone(), None if post.beta is None else post.beta.clone()
        model.covparam[:] = th + 0.7                                 # in place, then replaced
        model.covparam = th - 0.3
        if model.meanparam is not None:
            model.meanparam.fill_(4.0)
            model.meanparam = torch.tensor([5.0, -2.0], dtype=torch.float64, device="cuda")
        v2, g2 = post.mean_and_gradient(xt)
        np.testing.assert_array_equal(v2, v)
        np.testing.assert_array_equal(g2, g)
        np.testing.assert_array_equal(post(xt), v)
        assert torch.equal(post.alpha, a) and (b is None or torch.equal(post.beta, b))
        assert (post.n, post.d, post.q, tuple(post.xi.shape)) == (N, D, 0 if b is None else 3, (N, D))
