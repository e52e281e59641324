"""The ordered kernel launches of the C ABI's main paths, to compare two builds of the library
(profiles/r10_capi_split.md § Launches): (kernel name, grid, block, LDS) per dispatch.

    rocprofv3 --kernel-trace --output-format csv -d DIR_A -o kt -- python3 tools/launch_trace.py run   # WOS_LIB_PATH: build A
    rocprofv3 --kernel-trace --output-format csv -d DIR_B -o kt -- python3 tools/launch_trace.py run   # build B
    python3 tools/launch_trace.py compare DIR_A DIR_B [--list OUT.txt]

Each trace is a run of its own: no counters, no other tracing.  `run` makes, with host pointers
only (no torch kernels in the trace): one config-B solve on 4 096 points, one two-channel solve,
one tape record + replay + both adjoints (the index build between them), one wos_bvc at the
settings of tests/bvc_cases.py karman, and the fused SIREN's entry points (siren()).  `compare`
exits 1 unless the two lists are identical; two neighbours that changed places are listed and passed
over, for the reader to judge (profiles/siren_host_split.md: the zero fill of wos_siren_vjp).
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
    siren()
    print("launch_trace: done")


def siren():
    """The fused SIREN's entry points through the C ABI (profiles/siren_host_split.md § Launches): a
    (2, 64, 1) net and 45 points on host pointers -- wos_siren_eval, wos_siren_vjp, wos_siren_fit with
    gradients and loss only, wos_adam_step with clipping -- then four iterations each of
    wos_siren_fit_run and wos_siren_fit_run_batches on device buffers filled by hipMemcpy."""
    import ctypes as C

    import numpy as np

    from wos_amd import _lib
    L = _lib.load()
    with open("/proc/self/maps") as f:  # the HIP runtime that the library itself runs on
        hip = C.CDLL(next(line.split()[-1] for line in f if "libamdhip64" in line))
    d, H, n, K = 2, 64, 45, 4
    rng = np.random.default_rng(7)
    shapes = [(H, d), (H, H), (d, H)]
    W = [rng.uniform(-0.1, 0.1, s).astype(np.float32) for s in shapes]
    B = [rng.uniform(-0.1, 0.1, s[0]).astype(np.float32) for s in shapes]
    x = rng.uniform(-1, 1, (K * n, d)).astype(np.float32)
    t = rng.uniform(-1, 1, (K * n, d)).astype(np.float32)
    arr = lambda ptrs: (C.c_void_p * len(ptrs))(*ptrs)  # noqa: E731
    host = lambda a: a.ctypes.data  # noqa: E731
    ok = lambda rc: rc == 0 or sys.exit(f"launch_trace: {L.wos_last_error().decode()}")  # noqa: E731

    def net(ptr):
        return _lib.SirenNet(d, d, H, 1, 30.0, arr([ptr(a) for a in W]), arr([ptr(a) for a in B]))
    hn = net(host)
    u, jac, div = np.empty((n, d), np.float32), np.empty((n, d, d), np.float32), np.empty(n, np.float32)
    ok(L.wos_siren_eval(C.byref(hn), host(x), n, host(u), host(jac), host(div), 0, 0, None))
    GW, GB = [np.empty_like(a) for a in W], [np.empty_like(a) for a in B]
    gw, gb = arr([host(a) for a in GW]), arr([host(a) for a in GB])
    ok(L.wos_siren_vjp(C.byref(hn), host(x), n, host(u), host(jac), host(div), gw, gb, 0, 0, 0, None))
    loss = np.empty(1, np.float32)
    ok(L.wos_siren_fit(C.byref(hn), host(x), n, host(t), None, host(loss), gw, gb, 0, 0, 0, None))
    ok(L.wos_siren_fit(C.byref(hn), host(x), n, host(t), None, host(loss), None, None, 0, 0, 0, None))
    P = [a.copy() for a in W + B]
    total = sum(a.size for a in P)
    m, v, norm = np.zeros(total, np.float32), np.zeros(total, np.float32), np.empty(1, np.float32)
    opt = _lib.AdamParams(1e-4, 0.9, 0.999, 1e-8, 0.1)
    ok(L.wos_adam_step(len(P), (C.c_int64 * len(P))(*[a.size for a in P]), arr([host(a) for a in P]),
                       arr([host(a) for a in GW + GB]), host(m), host(v), 1, C.byref(opt), host(norm), 0, 0, None))

    def dev(a):
        p = C.c_void_p()
        assert hip.hipMalloc(C.byref(p), C.c_size_t(a.nbytes)) == 0
        assert hip.hipMemcpy(p, C.c_void_p(host(a)), C.c_size_t(a.nbytes), 1) == 0  # hipMemcpyHostToDevice
        return p.value
    on = {id(a): dev(a) for a in W + B}
    dn = net(lambda a: on[id(a)])
    dx, dt, dm, dv = dev(x), dev(t), dev(np.zeros(total, np.float32)), dev(np.zeros(total, np.float32))
    dl, ds = dev(np.zeros(K, np.float32)), dev(np.zeros(2, np.int64))
    idx = rng.integers(0, K * n, (K, n)).astype(np.int64)
    flags = _lib.WOS_PTRS_DEVICE
    ok(L.wos_siren_fit_run(C.byref(dn), dx, dt, None, K * n, dev(idx), K, n, dm, dv, 0, C.byref(opt), -1.0, 0, dl, ds, 0,
                           flags, 0, None))
    offsets = (C.c_int64 * (K + 1))(0, 1, 34, 99, 180)  # 1, 33, 65 and 81 rows: a plan of its own per iteration
    ok(L.wos_siren_fit_run_batches(C.byref(dn), dx, dt, None, offsets, K, dm, dv, K, C.byref(opt), -1.0, 0, dl, ds, 0, flags,
                                   0, None))


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
    swaps, i = 0, 0
    while i < min(len(a), len(b)):
        if a[i] != b[i]:
            if a[i:i + 2] != b[i:i + 2][::-1]:
                print(f"launch_trace: first difference at dispatch {i}:\n  {a[i]}\n  {b[i]}")
                return 1
            print(f"launch_trace: dispatches {i} and {i + 1} are swapped:\n  {a[i]}\n  {a[i + 1]}")
            swaps, i = swaps + 1, i + 1
        i += 1
    if len(a) != len(b):
        print("launch_trace: one list is a prefix of the other")
        return 1
    print("launch_trace: identical" + (f" apart from {swaps} swapped neighbours (listed above)" if swaps else ""))
    return 0


if __name__ == "__main__":
    if len(sys.argv) == 2 and sys.argv[1] == "run":
        run()
    elif len(sys.argv) in (4, 6) and sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3], sys.argv[5] if len(sys.argv) == 6 and sys.argv[4] == "--list" else None))
    else:
        sys.exit(__doc__)
