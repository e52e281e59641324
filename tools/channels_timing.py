"""Cost of C source channels on one set of walks (wos_solve_channels) against C sequential
one-channel solves, on the SURVEY section 8 configurations.  GPU box only.

    python3 tools/channels_timing.py [--pkg DIR] [--reps N] [--tag TAG] [--out FILE] [configs...]   (default: B D)

Per config and C = 1..4, after a warm-up of every leg, the legs alternate solve by solve on the
same geometry and points:
  multi       one solve of a scene holding the (C, ...) source  (ch0 = f, ch1 = f reversed,
              ch2 = 0, ch3 = -f)
  sequential  C wos_solve calls on a one-channel scene, the source replaced in between
              (wos_scene_set_source on the device); the times of the C solves are summed
Reported per leg: median, min and max over the repetitions of kernel_ms, first_ball_ms, walk_ms
and fold_ms (wos_stats: device time, HIP events).  --pkg DIR imports wos_amd from another
checkout's package directory (the yardstick is the sequential leg of the parent commit: run this
script once per checkout, alternating, in one GPU visit); a package without channels runs the
sequential leg only.  One JSON line per config and C, appended to --out if given.
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("kernel_ms", "first_ball_ms", "walk_ms", "fold_ms")


def summary(xs):
    xs = sorted(xs)
    return {"median": xs[len(xs) // 2], "min": xs[0], "max": xs[-1]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pkg", default=os.path.join(REPO, "neural-monte-carlo-fluid-simulation_amd"))
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--tag", default="")
    ap.add_argument("--out", default="")
    ap.add_argument("configs", nargs="*", default=["B", "D"])
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.pkg))
    import numpy as np
    import torch
    from wos_amd import WosScene, solver_params, workloads
    from wos_amd import _lib

    dev = torch.device("cuda", 0)
    has_channels = hasattr(_lib, "MAX_CHANNELS")
    for name in a.configs:
        cfg = workloads.config_by_name(name)
        f = np.ascontiguousarray(cfg["source"], np.float32)
        rev = np.ascontiguousarray(f[tuple(slice(None, None, -1) for _ in f.shape)])
        chans = torch.from_numpy(np.stack([f, rev, np.zeros_like(f), -f])).to(dev)
        x = torch.from_numpy(np.ascontiguousarray(cfg["points"])).to(dev)
        prm = solver_params(cfg["solver"], cfg["output"])
        single = WosScene(cfg["vertices"], cfg["prims"], chans[0], cfg["absorption"], watertight=True,
                          **cfg["scene_kw"])
        multi = WosScene(cfg["vertices"], cfg["prims"], chans[0], cfg["absorption"], watertight=True,
                         **cfg["scene_kw"]) if has_channels else None

        def sequential(c):
            tot = dict.fromkeys(KEYS, 0.0)
            for k in range(c):
                single.set_source(chans[k])
                st = single.solve(x, prm)[-1]
                for key in KEYS:
                    tot[key] += st[key]
            return tot

        def together(c):
            return multi.solve(x, prm)[-1]  # its source was set for this C

        for c in (1, 2, 3, 4):
            legs = {"sequential": sequential}
            if has_channels:
                multi.set_source(chans[:c])
                legs["multi"] = together
            for fn in legs.values():  # warm-up: code objects, workspace
                fn(c)
            t = {leg: {key: [] for key in KEYS} for leg in legs}
            for _ in range(a.reps):
                for leg, fn in legs.items():
                    st = fn(c)
                    for key in KEYS:
                        t[leg][key].append(st[key])
            torch.cuda.synchronize()
            line = json.dumps({"tag": a.tag, "config": name, "channels": c, "points": int(x.shape[0]),
                               "walks": cfg["solver"]["nWalks"], "reps": a.reps,
                               **{leg: {key: summary(v) for key, v in d.items()} for leg, d in t.items()}})
            print(line, flush=True)
            if a.out:
                with open(a.out, "a") as fh:
                    fh.write(line + "\n")
        single.close()
        if multi is not None:
            multi.close()


if __name__ == "__main__":
    main()
