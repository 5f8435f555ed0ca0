#!/usr/bin/env python3
"""Cost of the posterior mean at input dimensions above 64 (n = 32768, m = 50000, zero mean, Matern p = 2) on one GPU:

    one gpmp_posterior_mean_wide call  against  the chunked Gram route it replaces in core/posterior_mean.py -- K(xt_chunk, xi) on
    the wide Gram route, chunks of ``predict_chunk_bytes``, times the weights by a torch matmul                       (HIP events)

at (d, s) = (128, 1), (128, 64), (1024, 64) by default, with the peak device memory of either route above the inputs and the
largest relative difference of the two results.

    python tools/posterior_mean_wide_bench.py [N M] [--cases D:S,D:S,...] [--reps R]

One JSON line per measurement (median of the repetitions after one warm-up, the two routes alternating per case).  ``valu_share``
is (2 d + 37) vector instructions per entry (distance, sqrt, exp, polynomial) over the fp64 vector issue rate of 256 CUs x 64
lanes at 2.4 GHz."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
from posterior_mean_bench import events, option, synth  # noqa: E402


def main():
    import torch

    import gpmp_amd.num as gnp
    from gpmp_amd import _lib
    from gpmp_amd.core import fused
    from gpmp_amd.kernel import MaternCovariance

    reps = int(option("--reps", 3))
    cases = [tuple(int(v) for v in c.split(":")) for c in str(option("--cases", "128:1,128:64,1024:64")).split(",")]
    args = sys.argv[1:]
    n, m = (int(a) for a in args[:2]) if len(args) >= 2 else (32768, 50000)
    p, dev, lib = 2, torch.device("cuda"), _lib.load()
    cov = MaternCovariance(p)
    for d, s in cases:
        xi_h, _, xt_h, theta = synth(n, m, d)
        X, XT = (gnp._points(torch.as_tensor(a, device=dev)) for a in (xi_h, xt_h))
        A = torch.as_tensor(np.random.default_rng(7).standard_normal((n, s)), device=dev)
        hv = _lib.host_vec(theta)
        res = {}

        def kernel():
            out = torch.empty((m, s), dtype=torch.float64, device=dev)
            ws = torch.empty(int(lib.gpmp_posterior_mean_wide_ws_elems(n, m, s, d)), dtype=torch.float64, device=dev)
            _lib.check(lib.gpmp_posterior_mean_wide(gnp._ptr(X), gnp._ptr(A), s, gnp._ptr(XT), None, 0, None, 0, n, m, s, d, 0, p, hv, 0,
                                                    gnp._ptr(ws), gnp._ptr(out), s, gnp._stream()), "gpmp_posterior_mean_wide")
            res["kernel"] = out

        def chunked():
            mc = fused.chunk_cols(n, m, floor=1)
            res["chunked"] = torch.cat([gnp.matmul(gnp.as_matrix(gnp.asarray(cov(XT[j0 : j0 + mc].contiguous(), X, theta))), A)
                                        for j0 in range(0, m, mc)])

        t, peak, outs = {}, {}, {}
        for _ in range(2):                                   # the two routes alternate; the second round is the one reported
            for name, fn in (("kernel", kernel), ("chunked", chunked)):
                res.clear()
                torch.cuda.synchronize()
                base = torch.cuda.memory_allocated()
                torch.cuda.reset_peak_memory_stats()
                t[name] = events(fn, reps)
                peak[name] = (torch.cuda.max_memory_allocated() - base) / 2 ** 20
                outs[name] = res.pop(name)
        err = float((outs["kernel"] - outs["chunked"]).abs().max() / outs["chunked"].abs().max())
        share = n * m * (2.0 * d + 37.0) / (256 * 64 * 2.4e9) / (t["kernel"] * 1e-3)
        print(json.dumps(dict(n=n, m=m, d=d, s=s, p=p, reps=reps, kernel_ms=t["kernel"], chunked_ms=t["chunked"],
                              ratio=t["chunked"] / t["kernel"], kernel_peak_MiB=peak["kernel"], chunked_peak_MiB=peak["chunked"],
                              max_rel_diff=err, valu_share=share)), flush=True)
        del X, XT, A, outs, res
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
