#!/usr/bin/env python3
"""Cost of the many-column posterior mean at the config-3 inputs of bench.py (n = 32768, m = 50000, d = 8, zero mean, Matern p = 2)
on one GPU, for s in {1, 16, 64} columns:

    one gpmp_posterior_mean_multi call  against  s calls of gpmp_posterior_mean (value only)           (HIP events)
    Model.conditional_sample_paths_from_data  against  Model.predict(return_lambdas=True) + conditional_sample_paths,
    64 paths                                                                                            (wall, synchronised)

    python tools/posterior_mean_multi_bench.py [N M D] [--ss S1,S2,...] [--reps R] [--no-paths]

One JSON line per measurement (median of the repetitions after one warm-up)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
from posterior_mean_bench import events, option, synth, wall  # noqa: E402


def main():
    import torch

    import gpmp_amd as gp
    import gpmp_amd.num as gnp
    from gpmp_amd import _lib
    from gpmp_amd.kernel import MaternCovariance

    reps = int(option("--reps", 3))
    ss = [int(v) for v in str(option("--ss", "1,16,64")).split(",")]
    paths = "--no-paths" not in sys.argv
    args = [a for a in sys.argv[1:] if a != "--no-paths"]
    n, m, d = (int(a) for a in args[:3]) if len(args) >= 3 else (32768, 50000, 8)
    p = 2
    xi_h, zi_h, xt_h, theta = synth(n, m, d)
    dev = torch.device("cuda")
    xi, zi, xt = (torch.as_tensor(a, device=dev) for a in (xi_h, zi_h, xt_h))
    lib, hv = _lib.load(), _lib.host_vec(theta)
    X, XT = gnp._points(xi), gnp._points(xt)
    A_all = torch.as_tensor(np.random.default_rng(7).standard_normal((n, max(ss))), device=dev)

    def emit(**kw):
        print(json.dumps(dict(dict(n=n, m=m, d=d, p=p, reps=reps), **kw)), flush=True)

    zpm = torch.empty(m, dtype=torch.float64, device=dev)
    ws1 = torch.empty(int(lib.gpmp_posterior_mean_ws_elems(n, m, d, 0)), dtype=torch.float64, device=dev)
    for s in ss:
        A = A_all[:, :s].contiguous()
        cols = [A[:, c].contiguous() for c in range(s)]
        out = torch.empty((m, s), dtype=torch.float64, device=dev)
        ws = torch.empty(int(lib.gpmp_posterior_mean_multi_ws_elems(n, m, s, d)), dtype=torch.float64, device=dev)

        def multi():
            _lib.check(lib.gpmp_posterior_mean_multi(gnp._ptr(X), gnp._ptr(A), s, gnp._ptr(XT), None, 0, None, 0, n, m, s, d, 0, p, hv, 0,
                                                     gnp._ptr(ws), gnp._ptr(out), s, gnp._stream()), "gpmp_posterior_mean_multi")

        def singles():
            for a in cols:
                _lib.check(lib.gpmp_posterior_mean(gnp._ptr(X), gnp._ptr(a), gnp._ptr(XT), None, 0, None, None, n, m, d, 0, p, hv, 0,
                                                   gnp._ptr(ws1), gnp._ptr(zpm), None, gnp._stream()), "gpmp_posterior_mean")

        tm, t1 = events(multi, reps), events(singles, reps)
        # the last single-column call left column s - 1 in zpm: the two kernels agree to rounding
        err = float((out[:, s - 1] - zpm).abs().max() / zpm.abs().max())
        emit(what="gpmp_posterior_mean_multi", s=s, ms=tm, entries_per_s=n * m / (tm * 1e-3))
        emit(what="s calls of gpmp_posterior_mean", s=s, ms=t1, ratio=t1 / tm, max_rel_diff_last_column=err)
    if paths:
        npaths = 64
        model = gp.Model(None, MaternCovariance(p), None, theta, "zero")
        ztsim = torch.as_tensor(np.random.default_rng(11).standard_normal((n + m, npaths)), device=dev)
        xi_ind, xt_ind = np.arange(n), n + np.arange(m)

        def new():
            return model.conditional_sample_paths_from_data(ztsim, xi, xi_ind, zi, xt, xt_ind, convert_out=False)

        def old():
            lam = model.predict(xi, zi, xt, return_lambdas=True, convert_in=False, convert_out=False)[2]
            return model.conditional_sample_paths(ztsim, xi_ind, zi, xt_ind, lam, convert_out=False)

        a, b = new(), old()
        err = float((a - b).abs().max() / b.abs().max())
        del a, b
        tn, to = wall(new, reps), wall(old, reps)
        emit(what="conditional_sample_paths_from_data", paths=npaths, ms=tn)
        emit(what="predict(return_lambdas) + conditional_sample_paths", paths=npaths, ms=to, ratio=to / tn, max_rel_diff=err)


if __name__ == "__main__":
    main()
