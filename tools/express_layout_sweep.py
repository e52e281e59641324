"""Sweep of the express layout and the length-hint thresholds on config B (bench.py's default workload, through
the same workloads.config_by_name("B"): karman, 65 398 points x 128 walks), one process; --shard N: on its stride-N
shard (points 0, N, 2N, ... at their global RNG indices, as bench.py --full times it):
    python3 tools/express_layout_sweep.py [--solo 0,64,80,96] [--xmin 24,32,40] [--epw 4,8,16] [--stripe 0,1]
                                          [--placement 0,1] [--hint-min 24] [--warm 3] [--diag [--set 24,16,96,0,0]]
Per combination: a cold solve (the workspace's caches dropped), then `warm` hinted solves; one line with the mean
warm walk-kernel, first-ball-span and total kernel time, the cold walk kernel, the hint counts and the sha-256
(first 16 digits) of p, grad, n_est and steps of the last solve, which must be the same on every line.
--diag: three blocking solves (a -DWOS_DIAG=1 library prints its counters after each), at the library's defaults
or at --set express_min,epw,solo_min,stripe,placement.
"""
import argparse
import hashlib
import itertools
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "neural-monte-carlo-fluid-simulation_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from wos_amd import (WosScene, length_hint_stats, release_caches, set_express_layout, set_length_hints,  # noqa: E402
                     solver_params, workloads)


def ints(s):
    return [int(v) for v in s.split(",")]


ap = argparse.ArgumentParser()
ap.add_argument("--solo", type=ints, default=[0, 64, 80, 96])
ap.add_argument("--xmin", type=ints, default=[24, 32, 40])
ap.add_argument("--epw", type=ints, default=[4, 8, 16])
ap.add_argument("--stripe", type=ints, default=[0, 1])
ap.add_argument("--placement", type=ints, default=[0, 1])
ap.add_argument("--warm", type=int, default=3)
ap.add_argument("--hint-min", type=int, default=24, help="walks listed (lowered to express_min where that is lower)")
ap.add_argument("--shard", type=int, default=1)
ap.add_argument("--diag", action="store_true")
ap.add_argument("--set", type=ints, default=None)
args = ap.parse_args()

cfg = workloads.config_by_name("B")
dev = torch.device("cuda", 0)
sc = WosScene(cfg["vertices"], cfg["prims"], torch.from_numpy(cfg["source"]).to(dev), cfg["absorption"], watertight=True,
              device=0, **cfg["scene_kw"])
x = torch.from_numpy(np.ascontiguousarray(cfg["points"][0::args.shard])).to(dev)
prm = solver_params(cfg["solver"], cfg["output"])


def solve():
    p, g, st, n, steps = sc.solve(x, prm, counts=True, index_base=0, index_stride=args.shard)
    torch.cuda.synchronize()
    h = hashlib.sha256()
    for a in (p, g, n, steps):
        h.update(a.cpu().numpy().tobytes())
    return st, h.hexdigest()[:16], length_hint_stats(0)


if args.diag:
    if args.set:
        set_length_hints(min(args.hint_min, args.set[0]), args.set[0], args.set[1], -1, 0)
        set_express_layout(*args.set[2:5])
    for k in range(3):
        print("diag solve", k, file=sys.stderr, flush=True)
        st, sha, hint = solve()
        print(f"  walk_ms {st['walk_ms']:.3f} {sha} {hint}", file=sys.stderr, flush=True)
    sys.exit(0)

tag = "B" if args.shard == 1 else f"B/{args.shard}"
solve()  # (the process's first solve: module load, workspace allocation)
print("# express_min epw solo_min stripe placement | warm walk_ms fb_ms kernel_ms (means) | cold walk_ms | sha | hints")
for xmin, epw, solo, stripe, placement in itertools.product(args.xmin, args.epw, args.solo, args.stripe, args.placement):
    release_caches(0)
    set_length_hints(min(args.hint_min, xmin), xmin, epw, -1, 0)
    set_express_layout(solo, stripe, placement)
    cold, sha0, _ = solve()
    w = [solve() for _ in range(args.warm)]
    assert all(s == sha0 for _, s, _ in w), "outputs differ"
    mean = lambda k: sum(st[k] for st, _, _ in w) / len(w)  # noqa: E731
    print(f"{tag} {xmin} {epw} {solo} {stripe} {placement} | {mean('walk_ms'):.4f} {mean('first_ball_ms'):.4f} "
          f"{mean('kernel_ms'):.4f} | {cold['walk_ms']:.4f} | {sha0} | {w[-1][2]}", flush=True)
