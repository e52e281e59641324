"""How to read the reported variance: across-key variance of the mean against var / n_est.

The variance the solve returns is the reference's per-walk sample variance.  A point's walks are
not independent draws -- antithetic pairs on stratified first directions, running control
variates -- so var / n_est is not the variance of the mean.  This measures the ratio on the CPU
oracle (bit-identical to the GPU path; no GPU needed): K independent RNG keys per point,
    ratio = Var_keys(mean) / Mean_keys(var / n_est)
pooled over the points (sum of numerators over sum of denominators) and as the per-point median,
for the solution and for each gradient component.  sqrt(ratio) scales the standard error.
    python3 tools/variance_calibration.py [--keys K] [--points N]
Needs a C compiler (tests/golden/oracle_var.c is built into a temporary directory).
"""
import argparse
import json
import os
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "tests", "golden"), os.path.join(REPO, "tests"),
                os.path.join(REPO, "neural-monte-carlo-fluid-simulation_amd")]

import numpy as np  # noqa: E402

import make_variance_golden as gen  # noqa: E402
import variance_cases as vc  # noqa: E402


def cases(n_points):
    import kat_cases
    from wos_amd import workloads
    karman = vc.case("karman_w128")
    karman["points"] = np.ascontiguousarray(workloads.karman_config(n_walks=128)["points"][:n_points])
    cube = vc.case("cube3d_w64")
    cube["points"] = kat_cases.cube3d(n_walks=64, npts=n_points)["points"]
    return [("karman2d, config B points, 128 walks", karman), ("cube3d, 64 walks", cube)]


def ratios(L, c, keys, threads):
    def one(key):
        r = gen.run_case(L, dict(c, solver=dict(c["solver"], seed=0x5EED7000 + key)))
        n = np.maximum(r["n_sol"], 1).astype(np.float64)
        ok = (2 * r["n_sol"] > c["solver"]["nWalks"]) & (r["p"] != 0)  # most walks recorded, not masked
        mean = np.concatenate([r["sol_mean"][:, None], r["g_mean"]], 1).astype(np.float64)
        var = np.concatenate([vc.expected_variance(r["sol_m2"], r["n_sol"])[:, None],
                              vc.expected_variance(r["g_m2"], r["n_sol"])], 1).astype(np.float64)
        return mean, var / n[:, None], ok

    with ThreadPoolExecutor(threads) as ex:
        res = list(ex.map(one, range(keys)))
    mean = np.stack([m for m, _, _ in res])
    rep = np.stack([v for _, v, _ in res])
    ok = np.all(np.stack([o for _, _, o in res]), 0)
    num, den = mean.var(0, ddof=1)[ok], rep.mean(0)[ok]
    return {"points": int(ok.sum()), "keys": keys,
            "pooled": [float(x) for x in num.sum(0) / den.sum(0)],
            "median": [float(x) for x in np.median(num / den, 0)]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keys", type=int, default=64)
    ap.add_argument("--points", type=int, default=2048)
    a = ap.parse_args()
    threads = max(1, min(16, len(os.sched_getaffinity(0))))
    with tempfile.TemporaryDirectory() as tmp:
        L = gen.build(tmp)
        for name, c in cases(a.points):
            out = ratios(L, c, a.keys, threads)
            out["case"] = name
            out["columns"] = ["p"] + [f"grad[{k}]" for k in range(c["dim"])]
            out["sigma_scale_pooled"] = [float(np.sqrt(x)) for x in out["pooled"]]
            print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
