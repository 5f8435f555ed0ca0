#!/usr/bin/env python3
"""Generate tests/golden/ref_predict_grad.npz by RUNNING THE REFERENCE (gpmp v0.9.37, torch-CPU backend): posterior mean and
variance at xt and their gradients with respect to xt, by autograd through Model.predict (what Model.predict_gradient replaces).

Run where the reference is importable:

    cd /tmp && PYTHONDONTWRITEBYTECODE=1 MPLBACKEND=Agg PYTHONPATH=<reference checkout> \\
        python3 <repo>/tests/golden/make_fixtures_predict_grad.py

Cases cover p in {0, 1, 2, 3, 6, 10}, noise on and off, the mean types zero / parameterized / linear_predictor (constant and
[1, x] designs) and d in {1, 3, 8, 70}.  The first two rows of every xt are rows of xi (the h = 0 convention); every other xt row
is a distinct point of the grid (q + 1/2) / 256, i.e. at scaled distance >= 1e-3 from xi.  Point sets are stored as the uint8 q
(decoded by tests/wide_dim_inputs.py).
"""
import os

import numpy as np

os.environ["GPMP_BACKEND"] = "torch"
os.environ.setdefault("GPMP_LOG_LEVEL", "WARNING")

import torch  # noqa: E402

import gpmp as gp  # noqa: E402  (the reference)
import gpmp.num as gnp  # noqa: E402

assert gnp._gpmp_backend_ == "torch"
HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, "ref_predict_grad.npz")

# (d, p, noise, mean, n, m): mean in zero / param (parameterized, [1, x0] . meanparam) / const / lin ([1, x], first 3 coordinates
# when d > 3)
CASES = [
    (1, 0, 0, "zero", 12, 9), (1, 2, 0, "param", 12, 9), (1, 6, 1, "lin", 14, 9), (1, 10, 1, "const", 12, 7),
    (3, 1, 1, "zero", 30, 9), (3, 3, 0, "const", 30, 9), (3, 2, 0, "lin", 30, 9), (3, 10, 0, "zero", 25, 9),
    (3, 0, 1, "lin", 30, 9), (3, 6, 0, "param", 30, 9),
    (8, 2, 0, "zero", 50, 9), (8, 2, 1, "lin", 50, 9), (8, 6, 0, "const", 50, 9), (8, 1, 1, "param", 50, 9),
    (8, 3, 0, "lin", 50, 9), (8, 10, 1, "const", 50, 9), (8, 0, 0, "zero", 50, 9),
    (70, 2, 0, "zero", 60, 7), (70, 1, 1, "lin", 60, 7), (70, 0, 0, "param", 60, 7),
]
MEANTYPE = {"zero": "zero", "param": "parameterized", "const": "linear_predictor", "lin": "linear_predictor"}


def theta_of(d, noise):
    rho = 0.25 * np.sqrt(d) * (1.0 + np.arange(d) / d)
    head = [0.3, np.log(0.05 ** 2)] if noise else [0.3]
    return np.concatenate((head, -np.log(rho)))


def kernel_of(p, noise):
    if not noise:
        return lambda x, y, covparam, pairwise=False: gp.kernel.maternp_covariance(x, y, p, covparam, pairwise)

    def kernel(x, y, param, pairwise=False):
        sigma2, noise_variance, loginvrho = gnp.exp(param[0]), gnp.exp(param[1]), param[2:]
        if y is x or y is None:
            if pairwise:
                return sigma2 * gnp.ones((x.shape[0],))
            K = gnp.scaled_distance(loginvrho, x, x)
            return sigma2 * gp.kernel.maternp_kernel(p, K) + noise_variance * gnp.eye(K.shape[0])
        K = gnp.scaled_distance_elementwise(loginvrho, x, y) if pairwise else gnp.scaled_distance(loginvrho, x, y)
        return sigma2 * gp.kernel.maternp_kernel(p, K)

    return kernel


def mean_of(kind, d):
    k = min(d, 3)
    if kind == "const":
        return lambda x, param: gnp.ones((x.shape[0], 1))
    if kind == "lin":
        return lambda x, param: gnp.hstack((gnp.ones((x.shape[0], 1)), x[:, :k]))
    if kind == "param":
        return lambda x, param: (param[0] + param[1] * x[:, 0]).reshape(-1, 1)
    return None


def main():
    out = {"ncases": np.array(len(CASES))}
    for c, (d, p, noise, kind, n, m) in enumerate(CASES):
        rng = np.random.default_rng(1000 + c)
        q = rng.choice(256 ** min(d, 3), size=n + m, replace=False) if d <= 3 else None
        if d <= 3:   # distinct grid points in low dimension
            qq = np.stack([(q // 256 ** j) % 256 for j in range(d)], axis=1).astype(np.uint8)
        else:
            qq = rng.integers(0, 256, size=(n + m, d), dtype=np.uint8)
        xiq, xtq = qq[:n], qq[n:].copy()
        xtq[:2] = xiq[[3, n - 1]]
        xi = (xiq.astype(np.float64) + 0.5) / 256.0
        xt = (xtq.astype(np.float64) + 0.5) / 256.0
        zi = np.sin(2 * np.pi * xi[:, 0]) + xi[:, 1:].sum(axis=1) / np.sqrt(d)
        if noise:
            zi = zi + 0.05 * rng.standard_normal(n)
        theta = theta_of(d, noise)
        meanparam = np.array([0.4, -0.7]) if kind == "param" else None
        model = gp.core.Model(mean_of(kind, d), kernel_of(p, noise), None if meanparam is None else torch.as_tensor(meanparam),
                              torch.as_tensor(theta), MEANTYPE[kind])
        xt_t = torch.as_tensor(xt).clone().requires_grad_(True)
        zpm, zpv = model.predict(torch.as_tensor(xi), torch.as_tensor(zi), xt_t, convert_in=False, convert_out=False)
        (gm,) = torch.autograd.grad(zpm.sum(), xt_t, retain_graph=True)
        (gv,) = torch.autograd.grad(zpv.sum(), xt_t)
        pre = f"c{c}_"
        out.update({pre + "xi_q": xiq, pre + "xt_q": xtq, pre + "zi": zi, pre + "theta": theta,
                    pre + "spec": np.array([d, p, noise, n, m]), pre + "mean": np.array(kind),
                    pre + "zpm": zpm.detach().numpy(), pre + "zpv": zpv.detach().numpy(), pre + "gzpm": gm.numpy(), pre + "gzpv": gv.numpy()})
        if meanparam is not None:
            out[pre + "meanparam"] = meanparam
    np.savez_compressed(PATH, **out)
    print("wrote", PATH, len(out), "arrays")


if __name__ == "__main__":
    main()
