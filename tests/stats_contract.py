"""The deterministic part of wos_stats for every entry point that fills one
(tests/test_gpu_stats_contract.py compares it with tests/golden/stats_contract.json).

One karman scene (bvc_cases.case("karman"), the scene of channel_cases' tests), 70 points: 69 of
the workload's random points (one full block of 64 and a partial one) and the cylinder's centre,
which lies outside the domain.  Two walk counts under wos_set_max_batch_tasks(2^16), the smallest
cap the library accepts:
    w6     6 walks per point: 420 tasks, one batch (the cap cannot go below 2^16 tasks, so 70
           points of 6 walks never split);
    w1024  1024 walks per point: 64 points fill a batch, so the 70 points split into 64 + 6.
Per walk count, in turn: wos_solve (host and device pointers), wos_solve_var, wos_tape_record,
wos_tape_solve, wos_tape_vjp, wos_tape_vjp_indexed, then with two source channels
wos_solve_channels and wos_tape_solve, and every async-capable call once more with
WOS_PTRS_DEVICE | WOS_ASYNC followed by wos_solve_stats on its ticket (the stats the call itself
returned are kept too: a ticket and nothing else).  Last, at the default cap, wos_bvc on the
karman scene at bvc_cases' settings and on bvc_cases.junction_square at the small settings of
test_gpu_bvc.py (its Dirichlet solves' counters are summed into the call's).

    python tests/stats_contract.py --write --parent <commit> [--out <file>]

writes the fixture.  It is run on the GPU with WOS_LIB_PATH naming a library built from the
parent of the change under test, never against the code under test; <commit> is that parent's
hash and is recorded in the fixture.
"""
import ctypes as C
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "stats_contract.json")

COUNTERS = ("walk_steps", "wasted_steps", "walks_recorded", "walks_escaped", "walks_max_length", "walks_rr",
            "walks_dirichlet", "points_estimated", "rejection_iters")
SHAPE = ("walk_launches", "first_ball_blocks_per_cu", "walk_blocks_per_cu", "walk_lds_bytes", "star_grid",
         "geom_global", "dir_grid")
TIMES = ("kernel_ms", "first_ball_ms", "walk_ms", "fold_ms")
N_POINTS = 70
WALKS = (6, 1024)
BATCH_CAP = 2 ** 16


def deterministic(st):
    """What of a stats dict (_lib.Stats.as_dict) does not depend on the clock."""
    d = {k: int(st[k]) for k in COUNTERS + SHAPE}
    d["ticket_zero"] = int(st["ticket"]) == 0
    for k in TIMES:
        v = float(st[k])
        assert v >= 0.0 and np.isfinite(v), (k, v)
        d[k] = "positive" if v > 0.0 else "zero"
    return d


def points():
    from wos_amd import workloads
    pts = workloads.karman_points(1024)[:N_POINTS].copy()
    centre, _ = workloads.karman_obstacle(workloads.scene_size(workloads.KARMAN_OBJ))
    pts[10] = centre  # inside the cylinder: outside the domain
    return np.ascontiguousarray(pts, np.float32)


def _walk_calls(out, tag, sc, c, n_walks):
    import torch

    import channel_cases as cc
    from wos_amd import _lib, solver_params
    L = _lib.load()
    prm = solver_params(dict(c["solver"], nWalks=n_walks), c["output"])
    x = points()
    n, dim = x.shape
    xd = torch.from_numpy(x).cuda()
    cells = int(np.prod(c["source"].shape))
    side = torch.cuda.Stream()
    DEV, ASYNC = _lib.WOS_PTRS_DEVICE, _lib.WOS_PTRS_DEVICE | _lib.WOS_ASYNC

    def host(ch):
        return {"p": np.empty(ch * n, np.float32), "g": np.empty(ch * n * dim, np.float32),
                "pv": np.empty(ch * n, np.float32), "gv": np.empty(ch * n * dim, np.float32),
                "n": np.empty(n, np.int32), "s": np.empty(n, np.int32), "up": np.ones(ch * n, np.float32),
                "ug": np.ones(ch * n * dim, np.float32), "gs": np.empty(ch * cells, np.float32)}

    def dev(ch):
        return {k: torch.from_numpy(a).cuda() for k, a in host(ch).items()}

    def hp(b, k):
        return b[k].ctypes.data

    def dp(b, k):
        return b[k].data_ptr()

    def call(name, fn, *args):
        st = _lib.Stats()
        rc = fn(*[C.byref(st) if a is Ellipsis else a for a in args])
        assert rc == 0, (name, L.wos_last_error())
        out[f"{tag}/{name}"] = deterministic(st.as_dict())
        return st

    def call_async(name, fn, *args):
        torch.cuda.synchronize()
        st = call(name + "_async", fn, *args)
        later = _lib.Stats()
        assert L.wos_solve_stats(sc._h, st.ticket, C.byref(later)) == 0, (name, L.wos_last_error())
        assert later.ticket == st.ticket
        out[f"{tag}/{name}_async_stats"] = deterministic(later.as_dict())

    s = side.cuda_stream
    b, d = host(1), dev(1)
    call("solve_host", L.wos_solve, sc._h, C.byref(prm), x.ctypes.data, n, 0, 1, hp(b, "p"), hp(b, "g"), hp(b, "n"),
         hp(b, "s"), ..., None, 0)
    call("solve_dev", L.wos_solve, sc._h, C.byref(prm), xd.data_ptr(), n, 0, 1, dp(d, "p"), dp(d, "g"), dp(d, "n"),
         dp(d, "s"), ..., None, DEV)
    call("solve_var", L.wos_solve_var, sc._h, C.byref(prm), x.ctypes.data, n, 0, 1, hp(b, "p"), hp(b, "g"),
         hp(b, "pv"), hp(b, "gv"), hp(b, "n"), hp(b, "s"), ..., None, 0)
    h = C.c_void_p()
    call("tape_record", L.wos_tape_record, sc._h, C.byref(prm), x.ctypes.data, n, 0, 1, 0, C.byref(h), ..., None, 0)
    try:
        call("tape_solve", L.wos_tape_solve, h, sc._h, 1, hp(b, "p"), hp(b, "g"), hp(b, "pv"), hp(b, "gv"),
             hp(b, "n"), hp(b, "s"), ..., None, 0)
        call("tape_vjp", L.wos_tape_vjp, h, sc._h, 1, hp(b, "up"), hp(b, "ug"), hp(b, "gs"), ..., None, 0)
        assert L.wos_tape_index_build(h, 0) == 0, L.wos_last_error()
        call("tape_vjp_indexed", L.wos_tape_vjp_indexed, h, sc._h, 1, hp(b, "up"), hp(b, "ug"), hp(b, "gs"), ...,
             None, 0)
        call_async("solve", L.wos_solve, sc._h, C.byref(prm), xd.data_ptr(), n, 0, 1, dp(d, "p"), dp(d, "g"),
                   dp(d, "n"), dp(d, "s"), ..., s, ASYNC)
        call_async("solve_var", L.wos_solve_var, sc._h, C.byref(prm), xd.data_ptr(), n, 0, 1, dp(d, "p"), dp(d, "g"),
                   dp(d, "pv"), dp(d, "gv"), dp(d, "n"), dp(d, "s"), ..., s, ASYNC)
        call_async("tape_solve", L.wos_tape_solve, h, sc._h, 1, dp(d, "p"), dp(d, "g"), dp(d, "pv"), dp(d, "gv"),
                   dp(d, "n"), dp(d, "s"), ..., s, ASYNC)
        call_async("tape_vjp", L.wos_tape_vjp, h, sc._h, 1, dp(d, "up"), dp(d, "ug"), dp(d, "gs"), ..., s, ASYNC)
        call_async("tape_vjp_indexed", L.wos_tape_vjp_indexed, h, sc._h, 1, dp(d, "up"), dp(d, "ug"), dp(d, "gs"),
                   ..., s, ASYNC)
        # two channels on the same grid: the tape (one set of walks) replays them too
        sc.set_source(cc.channels(c["source"], 2))
        b2, d2 = host(2), dev(2)
        call("solve_channels", L.wos_solve_channels, sc._h, C.byref(prm), x.ctypes.data, n, 0, 1, 2, hp(b2, "p"),
             hp(b2, "g"), hp(b2, "pv"), hp(b2, "gv"), hp(b2, "n"), hp(b2, "s"), ..., None, 0)
        call("tape_solve_channels", L.wos_tape_solve, h, sc._h, 2, hp(b2, "p"), hp(b2, "g"), hp(b2, "pv"),
             hp(b2, "gv"), hp(b2, "n"), hp(b2, "s"), ..., None, 0)
        call_async("solve_channels", L.wos_solve_channels, sc._h, C.byref(prm), xd.data_ptr(), n, 0, 1, 2,
                   dp(d2, "p"), dp(d2, "g"), dp(d2, "pv"), dp(d2, "gv"), dp(d2, "n"), dp(d2, "s"), ..., s, ASYNC)
        torch.cuda.synchronize()
    finally:
        L.wos_tape_destroy(h)
        sc.set_source(c["source"])


def collect():
    """{call: deterministic stats} of every call above, on device 0 through the loaded library."""
    import torch
    assert torch.cuda.is_available(), "needs a GPU"  # before the library opens the device, like conftest's gpu
    import bvc_cases
    from wos_amd import WosScene, bvc_params, set_max_batch_tasks, solver_params
    out = {}
    c = bvc_cases.case("karman")
    sc = WosScene(c["vertices"], c["prims"], c["source"], c["absorption"], watertight=True)
    prev = set_max_batch_tasks(BATCH_CAP)
    try:
        for w in WALKS:
            _walk_calls(out, f"w{w}", sc, c, w)
    finally:
        set_max_batch_tasks(prev)
    out["bvc/karman"] = deterministic(
        sc.bvc(solver_params(c["solver"], c["output"]), bvc_params(c["solver"], c["output"]))[2]["stats"])
    sc.close()
    j = bvc_cases.junction_square()
    small = dict(j["solver"], boundaryCacheSize=128, nWalksForCachedGradientEstimates=32,
                 nWalksForCachedSolutionEstimates=16)
    jout = dict(j["output"], gridRes=16)
    sj = WosScene(j["vertices"], j["prims"], j["source"], j["absorption"], watertight=True, **j["kw"])
    out["bvc/junction"] = deterministic(sj.bvc(solver_params(small, jout), bvc_params(small, jout))[2]["stats"])
    sj.close()
    return out


def main():
    import argparse
    ap = argparse.ArgumentParser(description="write tests/golden/stats_contract.json from the parent commit's library")
    ap.add_argument("--write", action="store_true", required=True)
    ap.add_argument("--parent", required=True, help="hash of the commit WOS_LIB_PATH's library was built from")
    ap.add_argument("--out", default=FIXTURE)
    a = ap.parse_args()
    if not os.environ.get("WOS_LIB_PATH"):
        sys.exit("WOS_LIB_PATH must name a library built from the parent commit, never the code under test")
    sys.path[:0] = [HERE, os.path.join(os.path.dirname(HERE), "neural-monte-carlo-fluid-simulation_amd")]
    doc = {"parent_commit": a.parent, "n_points": N_POINTS, "walks": list(WALKS), "batch_cap": BATCH_CAP,
           "calls": collect()}
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote {len(doc['calls'])} calls to {a.out}")


if __name__ == "__main__":
    main()
