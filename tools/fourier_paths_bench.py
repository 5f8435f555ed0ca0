#!/usr/bin/env python3
"""Cost of evaluating s random-Fourier-feature sample paths (R = 4096 features) at m points on one GPU:

    (k) one gpmp_fourier_paths call (through PriorPaths), no m x R block
    (a) the route composed of existing pieces, chunked over m by ``predict_chunk_bytes``: gpmp_dgemm (xt_chunk Omega^T), + phase,
        torch.cos, gpmp_dgemm (features W)
    (b) Model.sample_paths(method="chol") on the same points, where m <= --chol-max-m (0, the default, skips it): the dense
        covariance, its factor and one product -- another law of the same paths, timed once after one warm-up

at m in {50000, 10^6}, s in {1, 16, 64}, d in {8, 64} by default (HIP events).

    python tools/fourier_paths_bench.py [--ms M,M] [--cases D:S,D:S,...] [--reps R] [--features R] [--chol-max-m M]

One JSON line per case: the median of the repetitions after one warm-up, routes (k) and (a) alternating, the second round reported.
``valu_share`` is 20 fp64 vector instructions per feature entry and column block (reduction 6, polynomial 13, sign 1) over the
fp64 vector issue rate of 256 CUs x 64 lanes at 2.4 GHz; ``mfma_share`` is ceil(d / 4) + 4 CT matrix instructions of 64 cycles per
16 x 16 tile of entries and column block over 256 CUs x 4 SIMDs at 2.4 GHz."""
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from posterior_mean_bench import events, option, synth  # noqa: E402


def main():
    import torch

    import gpmp_amd as gp
    import gpmp_amd.num as gnp
    from gpmp_amd.core import fused
    from gpmp_amd.kernel import MaternCovariance

    reps, R = int(option("--reps", 3)), int(option("--features", 4096))
    ms = [int(v) for v in str(option("--ms", "50000,1000000")).split(",")]
    cases = [tuple(int(v) for v in c.split(":")) for c in str(option("--cases", "8:1,8:16,8:64,64:1,64:16,64:64")).split(",")]
    chol_max_m = int(option("--chol-max-m", 0))
    dev = torch.device("cuda")
    for m in ms:
        for d, s in cases:
            _, _, xt_h, theta = synth(1, m, d)
            model = gp.Model(None, MaternCovariance(2), None, theta, "zero")
            prior = model.prior_paths(s, nb_features=R, seed=1)
            XT = gnp._points(torch.as_tensor(xt_h, device=dev))
            res = {}

            def kernel():
                res["kernel"] = prior.paths(XT, convert_in=False, convert_out=False)

            def composed():
                mc = fused.chunk_cols(R, m, floor=1)
                res["composed"] = torch.cat([gnp.matmul(torch.cos_((gnp.matmul(XT[j0 : j0 + mc], prior.omega, tb=True) + prior.phase)
                                                                   .mul_(2.0 * math.pi)), prior.W) for j0 in range(0, m, mc)])

            t, outs = {}, {}
            for _ in range(2):                                   # the two routes alternate; the second round is the one reported
                for name, fn in (("kernel", kernel), ("composed", composed)):
                    res.clear()
                    t[name] = events(fn, reps)
                    outs[name] = res.pop(name)
            err = float((outs["kernel"] - outs["composed"]).abs().max() / outs["composed"].abs().max())
            line = dict(m=m, r=R, d=d, s=s, reps=reps, kernel_ms=t["kernel"], composed_ms=t["composed"], ratio=t["composed"] / t["kernel"],
                        max_rel_diff=err)
            ct, cb = min(4, (s + 15) // 16), (s + 63) // 64
            line["valu_share"] = 20.0 * m * R * cb / (256 * 64 * 2.4e9) / (t["kernel"] * 1e-3)
            line["mfma_share"] = 64.0 * (m / 16) * (R / 16) * cb * ((d + 3) // 4 + 4 * ct) / (256 * 4 * 2.4e9) / (t["kernel"] * 1e-3)
            if m <= chol_max_m:
                line["chol_ms"] = events(lambda: model.sample_paths(XT, s, method="chol"), 1)
            print(json.dumps(line), flush=True)
            del XT, outs, res, prior
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
