#!/usr/bin/env python3
"""The wide-dimension route (d > 64) on one GPU: Gram pass time per dimension, and one REML value + gradient.

    python tools/wide_dim_bench.py gram D [N M] [--reps R]   K(x, y) for N x M points of dimension D (default 16384 x 16384)
    python tools/wide_dim_bench.py reml N D [--reps R]        gpmp_nll_grad with a constant mean (REML value + gradient), and its
                                                            parts: Gram build, Cholesky, gradient trace alone
    python tools/wide_dim_bench.py all                        gram at D = 64 (register tier), 65, 128, 512; reml at N = 16384, D = 256
    python tools/wide_dim_bench.py valu CSV N M               VALU wave-instructions per entry per kernel, from the counter CSV of
                                                            rocprofv3 --pmc SQ_INSTS_VALU -- python tools/wide_dim_bench.py gram D N M --reps 1

One JSON line per measurement (GPU times from HIP events on the launch stream, median of the repetitions after one warm-up)."""
import csv
import collections
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def _theta(d):
    rho = 0.5 * np.sqrt(d) * 0.5 * (1.0 + np.arange(d) / d)
    return np.concatenate(([0.0], -np.log(rho)))


def _timed(fn, reps):
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


def gram(d, n=16384, m=16384, reps=5):
    import torch

    import gpmp_amd.num as gnp
    from gpmp_amd import _lib

    lib = _lib.load()
    rng = np.random.default_rng(1)
    X = torch.as_tensor(rng.random((n, d)), device=gnp._dev())
    Y = torch.as_tensor(rng.random((m, d)), device=gnp._dev())
    K = gnp.alloc_matrix(n, m)
    hv = _lib.host_vec(_theta(d))

    def run():
        _lib.check(lib.gpmp_matern_gram(gnp._ptr(X), gnp._ptr(Y), n, m, d, 2, hv, 0, 0.0, 0, gnp._ptr(K), gnp._ld(K), gnp._stream()),
                   "gpmp_matern_gram")

    ms = _timed(run, reps)
    entries = float(n) * m
    print(json.dumps({"what": "gram", "route": "register" if d <= 64 else "wide", "n": n, "m": m, "d": d, "p": 2, "ms": round(ms, 3),
                      "ps_per_entry_dim": round(ms * 1e9 / (entries * d), 3), "TB_per_s_written": round(8 * entries / ms / 1e9, 3)}),
          flush=True)


def reml(n=16384, d=256, reps=3):
    import torch

    import gpmp_amd.num as gnp
    from gpmp_amd import _lib

    lib = _lib.load()
    dev = gnp._dev()
    rng = np.random.default_rng(2)
    x = rng.random((n, d))
    z = np.sin(2 * np.pi * x[:, 0]) + x[:, 1:].sum(axis=1) / np.sqrt(d)
    th = _theta(d)
    hv = _lib.host_vec(th)
    X, Z = torch.as_tensor(x, device=dev), torch.as_tensor(z, device=dev)
    P = torch.ones((n, 1), dtype=torch.float64, device=dev)
    ws = torch.empty(int(lib.gpmp_nll_grad_ws_elems(n, d, 1)), dtype=torch.float64, device=dev)
    val = torch.empty(1, dtype=torch.float64, device=dev)
    g = torch.empty(len(th), dtype=torch.float64, device=dev)
    info = torch.zeros(1, dtype=torch.int32, device=dev)

    def full():
        _lib.check(lib.gpmp_nll_grad(gnp._ptr(X), gnp._ptr(Z), gnp._ptr(P), 1, n, d, 1, 2, hv, 0, gnp._ptr(ws), gnp._ptr(val), gnp._ptr(g),
                                     gnp._ptr(info), gnp._stream()), "gpmp_nll_grad")

    t_full = _timed(full, reps)
    assert int(info.item()) == 0 and np.isfinite(val.item()), (info.item(), val.item())
    del ws
    K = gnp.alloc_matrix(n, n)
    dinv = torch.empty(int(lib.gpmp_dinv_elems(n)), dtype=torch.float64, device=dev)

    def gram_lower():
        _lib.check(lib.gpmp_matern_gram(gnp._ptr(X), None, n, n, d, 2, hv, 0, 1e-8, 1, gnp._ptr(K), gnp._ld(K), gnp._stream()),
                   "gpmp_matern_gram")

    def chol():
        gram_lower()
        _lib.check(lib.gpmp_potrf_lower_async(gnp._ptr(K), n, gnp._ld(K), gnp._ptr(dinv), gnp._ptr(info), gnp._stream()), "potrf")

    t_gram = _timed(gram_lower, reps)
    t_chol = _timed(chol, reps) - t_gram
    F = torch.as_tensor(rng.standard_normal((n, 2)), device=dev)
    G = torch.as_tensor(rng.standard_normal((n, 2)), device=dev)
    gws = torch.empty(int(lib.gpmp_grad_ws_elems(n, d)), dtype=torch.float64, device=dev)
    gram_lower()

    def trace():
        _lib.check(lib.gpmp_matern_grad_trace(gnp._ptr(K), gnp._ld(K), gnp._ptr(X), n, d, 2, hv, 0, gnp._ptr(F), gnp._ptr(G), 2, 2,
                                              gnp._ptr(g), gnp._ptr(gws), gnp._stream()), "gpmp_matern_grad_trace")

    t_trace = _timed(trace, reps)
    half = float(n) * (n + 1) / 2
    print(json.dumps({"what": "reml_value_and_gradient", "n": n, "d": d, "q": 1, "p": 2, "ms": round(t_full, 2),
                      "gram_lower_ms": round(t_gram, 2), "cholesky_ms": round(t_chol, 2), "grad_trace_ms": round(t_trace, 2),
                      "grad_trace_ps_per_entry_dim": round(t_trace * 1e9 / (half * d), 3)}), flush=True)


def valu(path, n, m):
    tot, disp = collections.defaultdict(float), collections.defaultdict(set)
    for r in csv.DictReader(open(path)):
        if r.get("Counter_Name") == "SQ_INSTS_VALU":
            tot[r["Kernel_Name"]] += float(r["Counter_Value"])
            disp[r["Kernel_Name"]].add(r["Dispatch_Id"])
    for k in sorted(tot, key=lambda k: -tot[k]):
        if "gram" in k:
            nd = len(disp[k])
            print(json.dumps({"kernel": k[:90], "dispatches": nd, "valu_per_entry": round(tot[k] * 64.0 / (nd * float(n) * m), 2)}))


def main(argv):
    reps = 5
    if "--reps" in argv:
        i = argv.index("--reps")
        reps = int(argv[i + 1])
        argv = argv[:i] + argv[i + 2:]
    what = argv[0] if argv else "all"
    if what == "gram":
        d = int(argv[1])
        n = int(argv[2]) if len(argv) > 2 else 16384
        m = int(argv[3]) if len(argv) > 3 else n
        gram(d, n, m, reps)
    elif what == "reml":
        reml(int(argv[1]), int(argv[2]), min(reps, 3))
    elif what == "valu":
        valu(argv[1], int(argv[2]), int(argv[3]))
    else:
        for d in (64, 65, 128, 512):
            gram(d, reps=reps)
        reml(16384, 256, 3)


if __name__ == "__main__":
    main(sys.argv[1:])
