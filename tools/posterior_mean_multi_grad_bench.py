#!/usr/bin/env python3
"""Cost of the many-column posterior mean WITH its Jacobian at the config-3 inputs of bench.py (n = 32768, m = 50000, d = 8, zero
mean, Matern p = 2) on one GPU, for s in {1, 16, 48, 64} columns:

    one gpmp_posterior_mean_multi_grad call  against  s calls of gpmp_posterior_mean with the gradient      (HIP events)
    the same call next to gpmp_posterior_mean_multi (value only): what the d gradient components add        (HIP events)
    PosteriorMeans.mean_and_gradient, device in, device out, largest s                                      (wall, synchronised)
    the Jacobian's error over n 2^-53 sum_i |term| against a long-double sum, at n = 2048, m = 256, s = 16   (information)

    python tools/posterior_mean_multi_grad_bench.py [N M D] [--ss S1,S2,...] [--reps R]

One JSON line per measurement (median of the repetitions after one warm-up).  flop = 2 n m (d + 1) x columns: `useful` counts the s
columns asked for, `executed` the column tiles of 16 that the matrix instructions run."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
from posterior_mean_bench import events, option, synth, wall  # noqa: E402

PEAK = 78.6e12          # fp64 matrix instructions, MI355X


def main():
    import torch

    import gpmp_amd as gp
    import gpmp_amd.num as gnp
    from gpmp_amd import _lib
    from gpmp_amd.kernel import MaternCovariance
    from tests import predict_grad_numpy as pgn

    reps = int(option("--reps", 3))
    ss = [int(v) for v in str(option("--ss", "1,16,48,64")).split(",")]
    n, m, d = (int(a) for a in sys.argv[1:4]) if len(sys.argv) >= 4 else (32768, 50000, 8)
    p = 2
    xi_h, zi_h, xt_h, theta = synth(n, m, d)
    dev = torch.device("cuda")
    lib, hv = _lib.load(), _lib.host_vec(theta)
    X, XT = gnp._points(torch.as_tensor(xi_h, device=dev)), gnp._points(torch.as_tensor(xt_h, device=dev))
    A_all = torch.as_tensor(np.random.default_rng(7).standard_normal((n, max(ss))), device=dev)

    def emit(**kw):
        print(json.dumps(dict(dict(n=n, m=m, d=d, p=p, reps=reps), **kw)), flush=True)

    def grad_call(X, A, XT, O, G, ws):
        (n_, d_), m_, s_ = X.shape, XT.shape[0], A.shape[1]
        _lib.check(lib.gpmp_posterior_mean_multi_grad(gnp._ptr(X), gnp._ptr(A), s_, gnp._ptr(XT), None, 0, None, 0, None, n_, m_, s_, d_, 0, p,
                                                      hv, 0, gnp._ptr(ws), gnp._ptr(O), s_, gnp._ptr(G), s_, gnp._stream()),
                   "gpmp_posterior_mean_multi_grad")

    zpm, gz = torch.empty(m, dtype=torch.float64, device=dev), torch.empty((m, d), dtype=torch.float64, device=dev)
    ws1 = torch.empty(int(lib.gpmp_posterior_mean_ws_elems(n, m, d, 1)), dtype=torch.float64, device=dev)
    for s in ss:
        A = A_all[:, :s].contiguous()
        cols = [A[:, c].contiguous() for c in range(s)]
        O, G, O1 = (torch.empty(sh, dtype=torch.float64, device=dev) for sh in ((m, s), (m, d, s), (m, s)))
        ws = torch.empty(int(lib.gpmp_posterior_mean_multi_grad_ws_elems(n, m, s, d)), dtype=torch.float64, device=dev)
        wsv = torch.empty(int(lib.gpmp_posterior_mean_multi_ws_elems(n, m, s, d)), dtype=torch.float64, device=dev)

        def value_only():
            _lib.check(lib.gpmp_posterior_mean_multi(gnp._ptr(X), gnp._ptr(A), s, gnp._ptr(XT), None, 0, None, 0, n, m, s, d, 0, p, hv, 0,
                                                     gnp._ptr(wsv), gnp._ptr(O1), s, gnp._stream()), "gpmp_posterior_mean_multi")

        def singles():
            for a in cols:
                _lib.check(lib.gpmp_posterior_mean(gnp._ptr(X), gnp._ptr(a), gnp._ptr(XT), None, 0, None, None, n, m, d, 0, p, hv, 0,
                                                   gnp._ptr(ws1), gnp._ptr(zpm), gnp._ptr(gz), gnp._stream()), "gpmp_posterior_mean")

        tg, tv, t1 = events(lambda: grad_call(X, A, XT, O, G, ws), reps), events(value_only, reps), events(singles, reps)
        # the last single-column call left column s - 1 in zpm / gz
        err = max(float((O[:, s - 1] - zpm).abs().max() / zpm.abs().max()), float((G[:, :, s - 1] - gz).abs().max() / gz.abs().max()))
        flop, se = 2.0 * n * m * (d + 1), (s + 15) // 16 * 16
        emit(what="gpmp_posterior_mean_multi_grad", s=s, ms=tg, useful_tflops=flop * s / tg * 1e-9, executed_tflops=flop * se / tg * 1e-9,
             executed_share_of_peak=flop * se / (tg * 1e-3) / PEAK)
        emit(what="gpmp_posterior_mean_multi (value only)", s=s, ms=tv, grad_over_value=tg / tv)
        emit(what="s calls of gpmp_posterior_mean with gradient", s=s, ms=t1, ratio=t1 / tg, max_rel_diff_last_column=err)
    s = max(ss)
    model = gp.Model(None, MaternCovariance(p), None, theta, "zero")
    post = model.posterior_means(X, torch.cos(torch.outer(torch.as_tensor(zi_h, device=dev), 1.0 + torch.arange(s, device=dev) / s)))
    emit(what="PosteriorMeans.mean_and_gradient (wall)", s=s, ms=wall(lambda: post.mean_and_gradient(XT, convert_in=False, convert_out=False), reps))
    # error of the Jacobian over n 2^-53 sum_i |term|, against a long-double sum of the fp64 terms
    n2, m2, s2 = min(n, 2048), min(m, 256), min(s, 16)
    O, G = (torch.empty(sh, dtype=torch.float64, device=dev) for sh in ((m2, s2), (m2, d, s2)))
    ws = torch.empty(int(lib.gpmp_posterior_mean_multi_grad_ws_elems(n2, m2, s2, d)), dtype=torch.float64, device=dev)
    grad_call(X[:n2], A_all[:n2, :s2].contiguous(), XT[:m2], O, G, ws)
    _, S, ir2 = pgn.cov_parts(xi_h[:n2], xt_h[:m2], p, theta, 0)
    a = A_all[:n2, :s2].cpu().numpy()
    worst = 0.0
    for j in range(d):
        terms = (ir2[j] * S * (xt_h[None, :m2, j] - xi_h[:n2, None, j]))[:, :, None].astype(np.longdouble) * a[:, None, :]     # (n, m, s)
        errj = np.abs(G[:, j, :].cpu().numpy() - terms.sum(axis=0)) / (n2 * 2.0 ** -53 * np.abs(terms).sum(axis=0))
        worst = max(worst, float(errj.max()))
    emit(what="Jacobian error / (n 2^-53 sum |term|), worst", n2=n2, m2=m2, s2=s2, ratio=worst)


if __name__ == "__main__":
    main()
