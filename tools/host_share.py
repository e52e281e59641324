"""Host share of a config-B projection through the C ABI: wall time of a blocking solve with device
pointers minus the kernel_ms its wos_stats reports (ev0 .. ev1 on the stream), per solve.

    [WOS_LIB_PATH=<another build>] python3 tools/host_share.py [--solves 200] [--warmup 3]

Prints one JSON line: median [min, max] in ms of wall, kernel_ms and wall - kernel_ms over the
solves.  What is left after kernel_ms is the launches' host time before ev0, the copy of the
counters, the stream synchronisation and the Python call (profiles/r10_capi_split.md § Host share).
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "neural-monte-carlo-fluid-simulation_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--solves", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    import torch
    from wos_amd import WosScene, _lib, solver_params, workloads
    cfg = workloads.config_by_name("B")
    dev = torch.device("cuda", 0)
    sc = WosScene(cfg["vertices"], cfg["prims"], torch.from_numpy(cfg["source"]).to(dev), cfg["absorption"],
                  watertight=True, device=0)
    pts = torch.from_numpy(cfg["points"]).to(dev)
    prm = solver_params(cfg["solver"], cfg["output"])
    wall, kern = [], []
    for i in range(a.warmup + a.solves):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _, _, st = sc.solve(pts, prm)
        t1 = time.perf_counter()
        if i >= a.warmup:
            wall.append((t1 - t0) * 1e3)
            kern.append(st["kernel_ms"])
    sc.close()
    host = [w - k for w, k in zip(wall, kern)]
    mmm = lambda v: [round(statistics.median(v), 4), round(min(v), 4), round(max(v), 4)]
    print(json.dumps({"lib": _lib.LIB_PATH, "solves": a.solves, "points": int(pts.shape[0]), "wall_ms": mmm(wall),
                      "kernel_ms": mmm(kern), "host_ms": mmm(host)}))


if __name__ == "__main__":
    main()
