#!/usr/bin/env python3
"""Cost of the fitted posterior mean at the config-3 inputs of bench.py (n = 32768, d = 8, same seeds, zero mean, Matern p = 2) on
one GPU, for m in {1, 256, 50000} prediction points (the first m rows of the same xt):

    Model.predict, Model.posterior_mean (the fit), post(xt), post.mean_and_gradient(xt)                  (wall, synchronised)
    gpmp_posterior_mean, value only and value + gradient, next to the Gram pass gpmp_matern_gram(xi, xt)
    and gpmp_predict_grad_reduce with u only at the same shape                                           (HIP events)

    python tools/posterior_mean_bench.py [N D] [--ms M1,M2,...] [--reps R]

One JSON line per measurement (median of the repetitions after one warm-up); the passes also report entries (n m) per second."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def synth(n, m, d):
    # bench.py's synth(n, m, d, rank=0)
    rng = np.random.default_rng(1234)
    xi = rng.random((n, d))
    zi = np.sin(2 * np.pi * xi[:, 0]) + xi[:, 1:].sum(axis=1)
    xt = np.random.default_rng(4321).random((m, d))
    theta = np.concatenate(([0.0], -np.log(0.5 * (1.0 + np.arange(d) / d))))
    return xi, zi, xt, theta


def wall(fn, reps):
    import torch

    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(ts))


def events(fn, reps):
    import torch

    fn()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def option(name, default):
    if name not in sys.argv:
        return default
    k = sys.argv.index(name)
    value = sys.argv[k + 1]
    del sys.argv[k : k + 2]
    return value


def main():
    import torch

    import gpmp_amd as gp
    import gpmp_amd.num as gnp
    from gpmp_amd import _lib
    from gpmp_amd.kernel import MaternCovariance

    reps = int(option("--reps", 5))
    ms = [int(v) for v in str(option("--ms", "1,256,50000")).split(",")]
    args = sys.argv[1:]
    n, d = (int(a) for a in args[:2]) if len(args) >= 2 else (32768, 8)
    p = 2
    xi_h, zi_h, xt_h, theta = synth(n, max(ms), d)
    dev = torch.device("cuda")
    xi, zi, xt_all = (torch.as_tensor(a, device=dev) for a in (xi_h, zi_h, xt_h))
    model = gp.Model(None, MaternCovariance(p), None, theta, "zero")
    lib = _lib.load()
    hv = _lib.host_vec(theta)
    X = gnp._points(xi)

    def emit(**kw):
        print(json.dumps(dict(dict(n=n, d=d, p=p, reps=reps), **kw)), flush=True)

    emit(what="Model.posterior_mean (fit)", ms=wall(lambda: model.posterior_mean(xi, zi, convert_in=False), reps))
    post = model.posterior_mean(xi, zi, convert_in=False)
    u = post.alpha
    for m in ms:
        xt = xt_all[:m].contiguous()
        XT = gnp._points(xt)
        emit(what="Model.predict", m=m, ms=wall(lambda: model.predict(xi, zi, xt, convert_in=False, convert_out=False), reps))
        emit(what="post(xt)", m=m, ms=wall(lambda: post(xt, convert_in=False, convert_out=False), reps))
        emit(what="post.mean_and_gradient(xt)", m=m, ms=wall(lambda: post.mean_and_gradient(xt, convert_in=False, convert_out=False), reps))
        zpm = torch.empty(m, dtype=torch.float64, device=dev)
        gm, gu = (torch.empty((m, d), dtype=torch.float64, device=dev) for _ in range(2))
        ws = torch.empty(int(lib.gpmp_posterior_mean_ws_elems(n, m, d, 1)), dtype=torch.float64, device=dev)
        wr = torch.empty(int(lib.gpmp_predict_grad_reduce_ws_elems(n, m, d)), dtype=torch.float64, device=dev)
        K = gnp.alloc_matrix(n, m)

        def mean(grad):
            _lib.check(lib.gpmp_posterior_mean(gnp._ptr(X), gnp._ptr(u), gnp._ptr(XT), None, 0, None, None, n, m, d, 0, p, hv, 0, gnp._ptr(ws),
                                               gnp._ptr(zpm), gnp._ptr(gm if grad else None), gnp._stream()), "gpmp_posterior_mean")

        def gram():
            _lib.check(lib.gpmp_matern_gram(gnp._ptr(X), gnp._ptr(XT), n, m, d, p, hv, 0, 0.0, 0, gnp._ptr(K), gnp._ld(K), gnp._stream()),
                       "gpmp_matern_gram")

        def reduce_u():
            _lib.check(lib.gpmp_predict_grad_reduce(gnp._ptr(X), gnp._ptr(XT), n, m, d, p, hv, 0, gnp._ptr(u), None, m, gnp._ptr(gu), None,
                                                    gnp._ptr(wr), gnp._stream()), "gpmp_predict_grad_reduce")

        for what, fn in (("gram pass K(xi, xt)", gram), ("gpmp_posterior_mean (value)", lambda: mean(False)),
                         ("gpmp_posterior_mean (value + gradient)", lambda: mean(True)), ("gpmp_predict_grad_reduce (u)", reduce_u)):
            t = events(fn, reps)
            emit(what=what, m=m, ms=t, entries_per_s=n * m / (t * 1e-3))
        del K, ws, wr


if __name__ == "__main__":
    main()
