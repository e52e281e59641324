"""Walk tape adjoint: wos_tape_vjp's device time, split into the adjoint fold and the scatter,
beside wos_tape_solve's on the SURVEY section 8 configurations.  GPU box only.

    python3 tools/tape_vjp_timing.py [--reps N] [--tag TAG] [--max-gb G] [configs...]   (default: B C D)
    python3 tools/tape_vjp_timing.py --summarize FILE.jsonl

One process records one tape per configuration and then alternates, call by call, the replay
(tape.solve) and the transpose (tape.vjp with a random upstream on p and grad p), --reps times
after a warm-up; times are wos_stats (HIP events): kernel_ms, walk_ms (replay kernel / scatter
kernel) and fold_ms (fold / adjoint fold).  Each line also holds how the scatter's terms spread
over the source grid: the terms per cell at the median and the maximum, the hottest cell, and the
share of all terms that lands on the busiest 1 % of the cells.  Run the legs to compare (--tag
names a leg) in alternating processes, three rounds, all lines into one file; --summarize prints
per configuration and leg the medians over the rounds with their min-max and the ratios to the
replay.
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def summary(xs):
    xs = sorted(xs)
    return {"median": xs[len(xs) // 2], "min": xs[0], "max": xs[-1]}


KEYS = ("replay_kernel_ms", "replay_walk_ms", "replay_fold_ms", "vjp_kernel_ms", "vjp_fold_ms", "vjp_scatter_ms")


def summarize(path):
    rows = [json.loads(l) for l in open(path) if l.strip().startswith("{")]
    rows = [r for r in rows if "vjp_kernel_ms" in r]
    for name in sorted({r["config"] for r in rows}):
        for tag in sorted({r["tag"] for r in rows if r["config"] == name}):
            v = [r for r in rows if r["config"] == name and r["tag"] == tag]
            out = {"summary": name, "tag": tag, "rounds": len(v)}
            for k in KEYS:
                out[k] = summary([r[k]["median"] for r in v])
            out["vjp_over_replay"] = out["vjp_kernel_ms"]["median"] / out["replay_kernel_ms"]["median"]
            out["scatter_over_replay_kernel"] = out["vjp_scatter_ms"]["median"] / out["replay_walk_ms"]["median"]
            for k in ("tape_entries", "terms", "cells", "terms_per_cell_median", "terms_per_cell_max", "hottest_cell",
                      "top1pct_cells_share"):
                out[k] = v[0][k]
            print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--tag", default="new")
    ap.add_argument("--max-gb", type=float, default=32.0)
    ap.add_argument("--summarize", metavar="FILE", default=None)
    ap.add_argument("configs", nargs="*", default=["B", "C", "D"])
    a = ap.parse_args()
    if a.summarize:
        return summarize(a.summarize)
    sys.path.insert(0, os.path.join(REPO, "neural-monte-carlo-fluid-simulation_amd"))
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
        info = tape.info
        n, dim = int(x.shape[0]), int(x.shape[1])
        gen = torch.Generator(device=dev).manual_seed(1)
        up_p = torch.randn(n, device=dev, generator=gen)
        up_g = torch.randn(n, dim, device=dev, generator=gen)
        cells = int(np.prod(sc.source_shape))
        k = np.zeros(cells, np.int64)
        for s in range(len(tape.segments)):
            code, cnt, slot = tape.read("code", s), tape.read("cnt", s), tape.read("slot", s).astype(np.int64)
            rec = (code & 1) != 0
            k += np.bincount(tape.read("cell0", s)[rec], minlength=cells)
            used = np.where(rec, np.minimum(cnt & 0x7FFFFFFF, slot[1:] - slot[:-1]), 0)
            m = int(slot[-1]) + 1  # +1 at a walk's first entry, -1 past its last
            live = np.bincount(slot[:-1], minlength=m) - np.bincount(slot[:-1] + used, minlength=m)
            k += np.bincount(tape.read("cell", s)[np.cumsum(live)[:-1] > 0], minlength=cells)
        order = np.sort(k)[::-1]
        row = {"tag": a.tag, "config": name, "points": n, "walks": cfg["solver"]["nWalks"], "reps": a.reps,
               "tape_entries": info["n_entries"], "terms": int(k.sum()), "cells": cells,
               "terms_per_cell_median": int(np.median(k)), "terms_per_cell_max": int(order[0]),
               "hottest_cell": [int(i) for i in np.unravel_index(int(np.argmax(k)), sc.source_shape)],
               "top1pct_cells_share": float(order[:max(1, cells // 100)].sum() / max(1, k.sum()))}
        tape.solve()
        g = tape.vjp(up_p, up_g)  # warm-up: code objects, workspace
        row["grad_source_finite"] = bool(torch.isfinite(g).all())
        t = {key: [] for key in KEYS}
        for _ in range(a.reps):
            st = tape.solve()[-1]
            t["replay_kernel_ms"].append(st["kernel_ms"])
            t["replay_walk_ms"].append(st["walk_ms"])
            t["replay_fold_ms"].append(st["fold_ms"])
            tape.vjp(up_p, up_g)
            st = tape.last_vjp_stats
            t["vjp_kernel_ms"].append(st["kernel_ms"])
            t["vjp_fold_ms"].append(st["fold_ms"])
            t["vjp_scatter_ms"].append(st["walk_ms"])
        torch.cuda.synchronize()
        row.update({key: summary(v) for key, v in t.items()})
        tape.close()
        print(json.dumps(row), flush=True)
        sc.close()


if __name__ == "__main__":
    main()
