"""Walk tape: record time, replay time and tape size against the full solve, on the SURVEY
section 8 configurations.  GPU box only.

    python3 tools/tape_timing.py [--pkg DIR] [--reps N] [--tag TAG] [--max-gb G] [configs...]  (default: B C D)
    python3 tools/tape_timing.py --summarize FILE.jsonl

One process times one library: the full solve's kernel_ms (wos_stats, HIP events) over --reps
repetitions after a warm-up and, where the package has WosScene.record, one recording
(kernel_ms of wos_tape_record, tape bytes and entries) and the replay's kernel_ms / walk_ms (the
replay kernel) / fold_ms, replay and full solve alternating call by call.  --pkg DIR imports wos_amd
from another checkout's package directory: run the parent commit's checkout and this one in
alternating processes, several rounds, all lines into one file (--tag names the leg), then
--summarize prints per config the medians over the rounds with their spread and the ratio
replay / parent solve.  A config whose tape would exceed --max-gb is reported as refused.
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def summary(xs):
    xs = sorted(xs)
    return {"median": xs[len(xs) // 2], "min": xs[0], "max": xs[-1]}


def summarize(path):
    rows = [json.loads(l) for l in open(path) if l.strip().startswith("{")]
    rows = [r for r in rows if "solve_kernel_ms" in r]
    for name in sorted({r["config"] for r in rows}):
        legs = {}
        for r in rows:
            if r["config"] == name:
                legs.setdefault(r["tag"], []).append(r)
        out = {"summary": name, "rounds": {t: len(v) for t, v in legs.items()}}
        for t, v in legs.items():
            out[f"{t}_solve_kernel_ms"] = summary([r["solve_kernel_ms"]["median"] for r in v])
            rep = [r for r in v if "replay_kernel_ms" in r]
            if rep:
                out[f"{t}_replay_kernel_ms"] = summary([r["replay_kernel_ms"]["median"] for r in rep])
                out[f"{t}_replay_walk_ms"] = summary([r["replay_walk_ms"]["median"] for r in rep])
                out[f"{t}_replay_fold_ms"] = summary([r["replay_fold_ms"]["median"] for r in rep])
                out[f"{t}_record_kernel_ms"] = summary([r["record_kernel_ms"] for r in rep])
                out["tape_bytes"], out["tape_entries"] = rep[0]["tape_bytes"], rep[0]["tape_entries"]
                out["max_entries_per_walk"] = rep[0]["max_entries_per_walk"]
        if "parent_solve_kernel_ms" in out and "new_replay_kernel_ms" in out:
            base = out["parent_solve_kernel_ms"]
            out["replay_over_parent_solve"] = {k: out["new_replay_kernel_ms"][k] / base["median"]
                                               for k in ("median", "min", "max")}
            out["record_over_parent_solve"] = out["new_record_kernel_ms"]["median"] / base["median"]
        print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pkg", default=os.path.join(REPO, "neural-monte-carlo-fluid-simulation_amd"))
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--tag", default="new")
    ap.add_argument("--max-gb", type=float, default=32.0)
    ap.add_argument("--summarize", metavar="FILE", default=None)
    ap.add_argument("configs", nargs="*", default=["B", "C", "D"])
    a = ap.parse_args()
    if a.summarize:
        return summarize(a.summarize)
    sys.path.insert(0, os.path.abspath(a.pkg))
    import numpy as np
    import torch
    from wos_amd import WosError, WosScene, solver_params, workloads

    dev = torch.device("cuda", 0)
    has_tape = hasattr(WosScene, "record")
    for name in a.configs:
        cfg = workloads.config_by_name(name)
        sc = WosScene(cfg["vertices"], cfg["prims"], cfg["source"], cfg["absorption"], watertight=True,
                      **cfg["scene_kw"])
        x = torch.from_numpy(np.ascontiguousarray(cfg["points"])).to(dev)
        prm = solver_params(cfg["solver"], cfg["output"])
        row = {"tag": a.tag, "config": name, "points": int(x.shape[0]), "walks": cfg["solver"]["nWalks"],
               "reps": a.reps}
        p0 = sc.solve(x, prm)[0]  # warm-up: code objects, workspace
        tape = None
        if has_tape:
            try:
                tape = sc.record(x, prm, max_bytes=int(a.max_gb * 2 ** 30))
            except WosError as e:
                row["tape_refused"] = str(e)
        if tape is not None:
            info = tape.info
            row.update(record_kernel_ms=tape.record_stats["kernel_ms"], tape_bytes=info["bytes"],
                       tape_entries=info["n_entries"], max_entries_per_walk=info["max_entries_per_walk"])
            p1 = tape.solve()[0]
            row["replay_bit_identical"] = bool(torch.equal(p0.view(torch.int32), p1.view(torch.int32)))
        solve, rk, rw, rf = [], [], [], []
        for _ in range(a.reps):
            solve.append(sc.solve(x, prm)[-1]["kernel_ms"])
            if tape is not None:
                st = tape.solve()[-1]
                rk.append(st["kernel_ms"])
                rw.append(st["walk_ms"])
                rf.append(st["fold_ms"])
        torch.cuda.synchronize()
        row["solve_kernel_ms"] = summary(solve)
        if tape is not None:
            row.update(replay_kernel_ms=summary(rk), replay_walk_ms=summary(rw), replay_fold_ms=summary(rf))
            tape.close()
        print(json.dumps(row), flush=True)
        sc.close()


if __name__ == "__main__":
    main()
