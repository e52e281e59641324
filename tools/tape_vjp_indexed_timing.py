"""Walk tape adjoint, indexed: wos_tape_vjp_indexed's device time beside wos_tape_vjp's -- this
build's and the parent commit's -- on the SURVEY section 8 configurations.  GPU box only.

    python3 tools/tape_vjp_indexed_timing.py --leg LEG [--tree DIR] [--reps N] [--max-gb G] [configs...]
    python3 tools/tape_vjp_indexed_timing.py --summarize FILE.jsonl          (default configs: B C D)

A leg is one process: it records one tape per configuration and calls the transpose --reps times
after a warm-up, with a random upstream on p and grad p; times are wos_stats (HIP events):
kernel_ms, fold_ms (the adjoint fold) and walk_ms (the scatter, or the sum kernels).
    parent   wos_tape_vjp of the tree at --tree: a built checkout of the parent commit (its
             package and its library; the atomic path this change must not move)
    atomic   wos_tape_vjp of this tree
    indexed  wos_tape_vjp_indexed of this tree; the line also holds the one-time build
             (wos_tape_index_build, host clock around the blocking call), the index's bytes, its
             terms, the longest row, whether three calls agree in every bit, and the largest
             |indexed - atomic| over the grid relative to the largest |atomic|
Run the legs in alternating processes, three rounds, all lines into one file; --summarize prints
per configuration and leg the medians over the rounds with their min-max, and whether the indexed
range lies wholly below the parent's.
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("kernel_ms", "fold_ms", "walk_ms")


def summary(xs):
    xs = sorted(xs)
    return {"median": xs[len(xs) // 2], "min": xs[0], "max": xs[-1]}


def summarize(path):
    rows = [json.loads(l) for l in open(path) if l.strip().startswith("{")]
    rows = [r for r in rows if "leg" in r and "kernel_ms" in r]
    for name in sorted({r["config"] for r in rows}):
        legs = {}
        for leg in ("parent", "atomic", "indexed"):
            v = [r for r in rows if r["config"] == name and r["leg"] == leg]
            if not v:
                continue
            out = {"summary": name, "leg": leg, "rounds": len(v)}
            for k in KEYS:
                out[k] = summary([r[k]["median"] for r in v])
            if leg == "indexed":
                out["build_ms"] = summary([r["build_ms"] for r in v])
                for k in ("index_bytes", "index_terms", "max_terms_per_cell", "tape_bytes"):
                    out[k] = v[0][k]
                out["bit_equal_calls"] = all(r["bit_equal_calls"] for r in v)
                out["max_rel_diff_to_atomic"] = max(r["max_rel_diff_to_atomic"] for r in v)
            legs[leg] = out
            print(json.dumps(out), flush=True)
        if "parent" in legs and "indexed" in legs:
            p, i = legs["parent"]["kernel_ms"], legs["indexed"]["kernel_ms"]
            print(json.dumps({"summary": name, "indexed_over_parent": i["median"] / p["median"],
                              "sum_over_scatter": legs["indexed"]["walk_ms"]["median"] / legs["parent"]["walk_ms"]["median"],
                              "indexed_range_below_parent": i["max"] < p["min"],
                              "indexed_range_above_parent": i["min"] > p["max"]}), flush=True)
        if "parent" in legs and "atomic" in legs:
            p, a = legs["parent"]["kernel_ms"], legs["atomic"]["kernel_ms"]
            print(json.dumps({"summary": name, "atomic_over_parent": a["median"] / p["median"],
                              "ranges_overlap": a["min"] <= p["max"] and p["min"] <= a["max"]}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=("parent", "atomic", "indexed"), default="indexed")
    ap.add_argument("--tree", default=REPO, help="the checkout whose package and library run (parent leg)")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--max-gb", type=float, default=32.0)
    ap.add_argument("--summarize", metavar="FILE", default=None)
    ap.add_argument("configs", nargs="*", default=["B", "C", "D"])
    a = ap.parse_args()
    if a.summarize:
        return summarize(a.summarize)
    if (a.leg == "parent") == (os.path.abspath(a.tree) == REPO):
        sys.exit("--leg parent needs --tree, a built checkout of the parent commit; the other legs run this tree")
    sys.path.insert(0, os.path.join(os.path.abspath(a.tree), "neural-monte-carlo-fluid-simulation_amd"))
    import numpy as np
    import torch
    from wos_amd import WosScene, solver_params, workloads

    dev = torch.device("cuda", 0)
    for name in a.configs:
        cfg = workloads.config_by_name(name)
        sc = WosScene(cfg["vertices"], cfg["prims"], cfg["source"], cfg["absorption"], watertight=True,
                      **cfg["scene_kw"])
        x = torch.from_numpy(np.ascontiguousarray(cfg["points"])).to(dev)
        prm = solver_params(cfg["solver"], cfg["output"])
        tape = sc.record(x, prm, max_bytes=int(a.max_gb * 2 ** 30))
        n, dim = int(x.shape[0]), int(x.shape[1])
        gen = torch.Generator(device=dev).manual_seed(1)
        up_p = torch.randn(n, device=dev, generator=gen)
        up_g = torch.randn(n, dim, device=dev, generator=gen)
        row = {"leg": a.leg, "config": name, "points": n, "walks": cfg["solver"]["nWalks"], "reps": a.reps,
               "tape_entries": tape.info["n_entries"], "tape_bytes": tape.info["bytes"],
               "cells": int(np.prod(sc.source_shape))}
        kw = {}
        if a.leg == "indexed":
            kw = {"deterministic": True}
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            tape.build_index()  # blocking
            row["build_ms"] = (time.perf_counter() - t0) * 1e3
            info = tape.index_info
            row.update(index_bytes=info["bytes"], index_terms=info["n_terms"], tile_terms=info["tile_terms"],
                       max_terms_per_cell=info["max_terms_per_cell"], index_segments=info["n_segments"])
        g = tape.vjp(up_p, up_g, **kw)  # warm-up: code objects, workspace
        row["grad_source_finite"] = bool(torch.isfinite(g).all())
        if a.leg == "indexed":
            row["bit_equal_calls"] = all(torch.equal(tape.vjp(up_p, up_g, **kw).view(torch.int32), g.view(torch.int32))
                                         for _ in range(2))
            atomic = tape.vjp(up_p, up_g)
            row["max_rel_diff_to_atomic"] = float((g - atomic).abs().max() / atomic.abs().max())
        t = {key: [] for key in KEYS}
        for _ in range(a.reps):
            tape.vjp(up_p, up_g, **kw)
            st = tape.last_vjp_stats
            for key in KEYS:
                t[key].append(st[key])
        torch.cuda.synchronize()
        row.update({key: summary(v) for key, v in t.items()})
        tape.close()
        print(json.dumps(row), flush=True)
        sc.close()


if __name__ == "__main__":
    main()
