"""fold_ms (wos_stats: the fold kernel's device time, HIP events) with and without the variance
outputs, on the SURVEY section 8 configurations.  GPU box only.

    python3 tools/fold_variance_timing.py [--pkg DIR] [--reps N] [--tag TAG] [configs...]   (default: B D)

The two variants alternate solve by solve on the same scene and points, after a warm-up of both;
reported per variant: median, min and max of fold_ms over the repetitions, and the same for
kernel_ms.  --pkg DIR imports wos_amd from another checkout's package directory (A/B against a
parent commit: run this script once per checkout, alternating, in one GPU visit); a package
without the variance keyword runs the default leg only.  One JSON line per config.
"""
import argparse
import inspect
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def summary(xs):
    xs = sorted(xs)
    return {"median": xs[len(xs) // 2], "min": xs[0], "max": xs[-1]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pkg", default=os.path.join(REPO, "neural-monte-carlo-fluid-simulation_amd"))
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--tag", default="")
    ap.add_argument("configs", nargs="*", default=["B", "D"])
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.pkg))
    import numpy as np
    import torch
    from wos_amd import WosScene, solver_params, workloads
    from wos_amd import _lib

    dev = torch.device("cuda", 0)
    has_var = "variance" in inspect.signature(WosScene.solve).parameters
    for name in a.configs:
        cfg = workloads.config_by_name(name)
        sc = WosScene(cfg["vertices"], cfg["prims"], cfg["source"], cfg["absorption"], watertight=True,
                      **cfg["scene_kw"])
        x = torch.from_numpy(np.ascontiguousarray(cfg["points"])).to(dev)
        prm = solver_params(cfg["solver"], cfg["output"])
        legs = {"default": {}}
        if has_var:
            legs["variance"] = {"variance": True}
        for kw in legs.values():  # warm-up: code objects, workspace
            sc.solve(x, prm, **kw)
        fold = {k: [] for k in legs}
        kern = {k: [] for k in legs}
        for _ in range(a.reps):
            for k, kw in legs.items():
                st = sc.solve(x, prm, **kw)[-1]
                fold[k].append(st["fold_ms"])
                kern[k].append(st["kernel_ms"])
        torch.cuda.synchronize()
        print(json.dumps({"tag": a.tag, "config": name, "points": int(x.shape[0]), "walks": cfg["solver"]["nWalks"],
                          "reps": a.reps, "abi": _lib.ABI_VERSION,
                          "fold_ms": {k: summary(v) for k, v in fold.items()},
                          "kernel_ms": {k: summary(v) for k, v in kern.items()}}), flush=True)
        sc.close()


if __name__ == "__main__":
    main()
