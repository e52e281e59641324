"""The ordered kernel launches of the C ABI's main paths, to compare two builds of the library
(profiles/r10_capi_split.md § Launches): (kernel name, grid, block, LDS) per dispatch.

    rocprofv3 --kernel-trace --output-format csv -d DIR_A -o kt -- python3 tools/launch_trace.py run   # WOS_LIB_PATH: build A
    rocprofv3 --kernel-trace --output-format csv -d DIR_B -o kt -- python3 tools/launch_trace.py run   # build B
    python3 tools/launch_trace.py compare DIR_A DIR_B [--list OUT.txt]

Each trace is a run of its own: no counters, no other tracing.  `run` makes, with host pointers
only (no torch kernels in the trace): one config-B solve on 4 096 points, one two-channel solve,
one tape record + replay + both adjoints (the index build between them), and one wos_bvc at the
settings of tests/bvc_cases.py karman.  `compare` exits 1 unless the two lists are identical.
LDS is the dispatch's whole LDS_Block_Size; the kernels' static LDS is the same on both sides
when their code objects are, so the column compares the dynamic part.
"""
import csv
import glob
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "neural-monte-carlo-fluid-simulation_amd"), os.path.join(REPO, "tests")):
    sys.path.insert(0, p)


def run():
    import numpy as np

    import bvc_cases
    import channel_cases
    from wos_amd import WosScene, bvc_params, solver_params, workloads
    cfg = workloads.config_by_name("B")
    pts = np.ascontiguousarray(cfg["points"][:4096])
    prm = solver_params(cfg["solver"], cfg["output"])
    sc = WosScene(cfg["vertices"], cfg["prims"], cfg["source"], cfg["absorption"], watertight=True)
    sc.solve(pts, prm)
    tape = sc.record(pts, prm)
    tape.solve()
    up = np.ones(pts.shape[0], np.float32)
    tape.vjp(up, None)
    tape.vjp(up, None, deterministic=True)
    sc.set_source(channel_cases.channels(cfg["source"], 2))
    sc.solve(pts, prm)
    tape.close()
    sc.close()
    c = bvc_cases.case("karman")
    sb = WosScene(c["vertices"], c["prims"], c["source"], c["absorption"], watertight=True)
    sb.bvc(solver_params(c["solver"], c["output"]), bvc_params(c["solver"], c["output"]))
    sb.close()
    print("launch_trace: done")


def launches(d):
    files = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        sys.exit(f"launch_trace: no *kernel_trace.csv under {d}")
    rows = []
    for f in files:
        with open(f, newline="") as fh:
            rows += list(csv.DictReader(fh))
    rows.sort(key=lambda r: int(r["Dispatch_Id"]))
    return [(r["Kernel_Name"], tuple(int(r[f"Grid_Size_{a}"]) for a in "XYZ"),
             tuple(int(r[f"Workgroup_Size_{a}"]) for a in "XYZ"), int(r["LDS_Block_Size"])) for r in rows]


def compare(da, db, list_out=None):
    a, b = launches(da), launches(db)
    if list_out:
        with open(list_out, "w") as f:
            for name, grid, block, lds in a:
                f.write(f"{name.split('(')[0]}\t{grid}\t{block}\t{lds}\n")
    names = sorted({x[0].split("(")[0].split("<")[0] for x in a})
    print(f"launch_trace: {len(a)} dispatches in {da}, {len(b)} in {db}, {len(names)} distinct kernels")
    for i, (x, y) in enumerate(zip(a, b)):
        if x != y:
            print(f"launch_trace: first difference at dispatch {i}:\n  {x}\n  {y}")
            return 1
    if len(a) != len(b):
        print("launch_trace: one list is a prefix of the other")
        return 1
    print("launch_trace: identical")
    return 0


if __name__ == "__main__":
    if len(sys.argv) == 2 and sys.argv[1] == "run":
        run()
    elif len(sys.argv) in (4, 6) and sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3], sys.argv[5] if len(sys.argv) == 6 and sys.argv[4] == "--list" else None))
    else:
        sys.exit(__doc__)
