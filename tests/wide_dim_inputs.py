"""Inputs of tests/golden/ref_wide_dim.npz (written by make_fixtures_wide_dim.py).

Point sets are stored as uint8 grid indices q: x = (q + 1/2) / 256 exactly in fp64, so the fixture stays small while the reference saw
exactly these points.  The near-duplicate set adds fp64 offsets to its first rows, in the generator's order of operations."""
import numpy as np


def decode(g):
    """NpzFile -> dict with every '<name>_q' index array replaced by the fp64 points '<name>'."""
    out = {}
    for k in g.files:
        v = g[k]
        if k.endswith("_q"):
            out[k[:-2]] = (v.astype(np.float64) + 0.5) / 256.0
        elif k != "dup_delta":
            out[k] = v
    if "dup_base" in out:
        base = out.pop("dup_base")
        out["dup_xi"] = np.vstack((base, base[: g["dup_delta"].shape[0]] + g["dup_delta"]))
    return out
