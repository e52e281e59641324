#!/usr/bin/env python3
"""The measured table of the Green's-function probe (DESIGN.md "Green's-function probe"): the
largest err / tol per member, dimension and mode, of the CPU oracle (oracle_gfn) and -- with
--device -- of the device probe (wos_selftest_gfn) against tests/golden/gfn_truth.npz.

  tools/gfn_probe.py [--device] [--out profiles/gfn_probe.json] [--merge other.json]

--merge takes the "device" half from another run's file (the oracle half runs anywhere).
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "tests"), os.path.join(REPO, "neural-monte-carlo-fluid-simulation_amd")]

import gfn_cases as C  # noqa: E402
import oracle_lib  # noqa: E402


def measure(run):
    T = C.table()
    out = {}
    for d in (2, 3):
        for mode in (0, 1, 2):
            rep = C.compare(d, mode, run(d, mode, T[f"items{d}"][C.rows_of(d, mode)]))
            out[f"{d}d_mode{mode}"] = {k: {"max_err_over_tol": round(v["max"], 4), "item": v["item"], "pairs": v["n"],
                                           "out_of_float_range": v["skipped"], "unbounded": v["unbounded"]}
                                       for k, v in rep.items() if v["n"] or v["skipped"] or v["unbounded"]}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--device", action="store_true")
    ap.add_argument("--merge")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "gfn_probe.json"))
    a = ap.parse_args()
    res = {"table": "tests/golden/gfn_truth.npz", "modes": "0 harmonic, 1 Yukawa reference semantics, 2 Yukawa robust",
           "oracle": measure(oracle_lib.gfn)}
    if a.device:
        from wos_amd import selftest_gfn
        res["device"] = measure(selftest_gfn)
    elif a.merge:
        with open(a.merge) as f:
            res["device"] = json.load(f)["device"]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    worst = max(v["max_err_over_tol"] for half in ("oracle", "device") if half in res for m in res[half].values()
                for v in m.values())
    print(f"{a.out}: largest err/tol {worst}")


if __name__ == "__main__":
    main()
