#!/usr/bin/env python3
"""Cost of the prediction gradients at the config-3 inputs of bench.py (n = 32768, m = 50000, d = 8, same seeds, zero mean,
Matern p = 2) on one GPU:

    Model.predict, Model.predict_gradient(variance=False), Model.predict_gradient(variance=True)      (wall, synchronised)
    gpmp_predict_grad_reduce alone (u; u and Lambda) next to the Gram pass gpmp_matern_gram(xi, xt)     (HIP events)

    python tools/predict_grad_bench.py [N M D] [--reps R]

One JSON line per measurement (median of the repetitions after one warm-up); the reduction and the Gram pass also report entries
(n m) per second."""
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


def main():
    import torch

    import gpmp_amd as gp
    import gpmp_amd.num as gnp
    from gpmp_amd import _lib
    from gpmp_amd.kernel import MaternCovariance

    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 3
    if "--reps" in sys.argv:
        args.remove(str(reps))
    n, m, d = (int(a) for a in args[:3]) if len(args) >= 3 else (32768, 50000, 8)
    xi_h, zi_h, xt_h, theta = synth(n, m, d)
    dev = torch.device("cuda")
    xi, zi, xt = (torch.as_tensor(a, device=dev) for a in (xi_h, zi_h, xt_h))
    model = gp.Model(None, MaternCovariance(2), None, theta, "zero")
    base = dict(n=n, m=m, d=d, reps=reps)

    def emit(**kw):
        print(json.dumps(dict(base, **kw)), flush=True)

    emit(what="Model.predict", ms=wall(lambda: model.predict(xi, zi, xt, convert_in=False, convert_out=False), reps))
    emit(what="predict_gradient(variance=False)",
         ms=wall(lambda: model.predict_gradient(xi, zi, xt, variance=False, convert_in=False, convert_out=False), reps))
    emit(what="predict_gradient(variance=True)",
         ms=wall(lambda: model.predict_gradient(xi, zi, xt, convert_in=False, convert_out=False), reps))
    lib = _lib.load()
    hv = _lib.host_vec(theta)
    X, XT = gnp._points(xi), gnp._points(xt)
    u = torch.randn(n, dtype=torch.float64, device=dev)
    gu, gl = (torch.empty((m, d), dtype=torch.float64, device=dev) for _ in range(2))
    ws = torch.empty(int(lib.gpmp_predict_grad_reduce_ws_elems(n, m, d)), dtype=torch.float64, device=dev)
    K = gnp.alloc_matrix(n, m)

    def red(lam):
        _lib.check(lib.gpmp_predict_grad_reduce(gnp._ptr(X), gnp._ptr(XT), n, m, d, 2, hv, 0, gnp._ptr(u), gnp._ptr(lam),
                                                gnp._ld(lam) if lam is not None else m, gnp._ptr(gu), gnp._ptr(None if lam is None else gl),
                                                gnp._ptr(ws), gnp._stream()), "gpmp_predict_grad_reduce")

    def gram():
        _lib.check(lib.gpmp_matern_gram(gnp._ptr(X), gnp._ptr(XT), n, m, d, 2, hv, 0, 0.0, 0, gnp._ptr(K), gnp._ld(K), gnp._stream()),
                   "gpmp_matern_gram")

    t = events(gram, reps)
    emit(what="gram pass K(xi, xt)", ms=t, entries_per_s=n * m / (t * 1e-3))
    t = events(lambda: red(None), reps)
    emit(what="reduction (u)", ms=t, entries_per_s=n * m / (t * 1e-3))
    K.normal_()
    t = events(lambda: red(K), reps)
    emit(what="reduction (u and Lambda)", ms=t, entries_per_s=n * m / (t * 1e-3))


if __name__ == "__main__":
    main()
