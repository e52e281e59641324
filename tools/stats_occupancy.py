"""first_ball_blocks_per_cu / walk_blocks_per_cu / walk_lds_bytes as wos_stats reports them for the
solves of profiles/r9_kernel_variants.md § Occupancy (B, C and D are the bench configs' scenes and
solver settings, C and D on 16 384 of their points; BVC is tests/bvc_cases.py karman).

    [WOS_LIB_PATH=<another build>] python3 tools/stats_occupancy.py

Prints one line per solve; run it once per library and compare (profiles/r10_capi_split.md).
"""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "neural-monte-carlo-fluid-simulation_amd"), os.path.join(REPO, "tests")):
    sys.path.insert(0, p)


def main():
    import numpy as np

    import bvc_cases
    import channel_cases
    from wos_amd import WosScene, bvc_params, solver_params, workloads

    def show(name, st):
        print(f"{name}: {st['first_ball_blocks_per_cu']} / {st['walk_blocks_per_cu']} / {st['walk_lds_bytes']}")

    for name, cap in (("B", None), ("C", 16384), ("D", 16384)):
        cfg = workloads.config_by_name(name)
        pts = np.ascontiguousarray(cfg["points"][:cap])
        sc = WosScene(cfg["vertices"], cfg["prims"], cfg["source"], cfg["absorption"], watertight=True,
                      **cfg["scene_kw"])
        show(f"{name} default", sc.solve(pts, solver_params(cfg["solver"], cfg["output"]))[2])
        if name == "B":
            show("B robust", sc.solve(pts, solver_params(dict(cfg["solver"], robustFloatSemantics=True),
                                                         cfg["output"]))[2])
        if name != "C":
            sc.set_source(channel_cases.channels(cfg["source"], 4))
            show(f"{name} four channels", sc.solve(pts, solver_params(cfg["solver"], cfg["output"]))[2])
        sc.close()
    c = bvc_cases.case("karman")
    sb = WosScene(c["vertices"], c["prims"], c["source"], c["absorption"], watertight=True)
    for tag, extra in (("BVC karman", {}), ("BVC robust karman", {"robustFloatSemantics": True})):
        prm = solver_params(dict(c["solver"], **extra), c["output"])
        show(tag, sb.bvc(prm, bvc_params(c["solver"], c["output"]), samples=False)[2]["stats"])
    sb.close()


if __name__ == "__main__":
    main()
