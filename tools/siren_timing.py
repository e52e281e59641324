"""Fused SIREN source: PressureProjector.source_from_network (wos_siren_eval, csrc/wos_siren.hip)
beside PressureProjector.source_from_velocity (PyTorch autograd: one forward and `dim` backward
passes) on the reference's grids.  GPU box only.

    python3 tools/siren_timing.py [--out profiles/siren_timing.jsonl] [--rounds 3] [--seconds 0.5]
    python3 tools/siren_timing.py --summarize profiles/siren_timing.jsonl

Cases: net2x128_2d -- 2 hidden layers of 128 on sample_uniform_2d(1000, karman), the 401 x 1002
grid behind profiles/r1d_projection_timing.json's siren_divergence_ms; net3x256_2d -- the
reference's 2D network (src/2d/config.json: 3 x 256, 2 -> 2) on the same grid; net3x256_3d -- its
3D network (3 -> 3) on sample_uniform_3d(80, cube), the 82^3 grid.
The two legs alternate within a round in one process; each is warmed up, then repeated for at
least --seconds of work between two device events, the second followed by a synchronise; the
figure is that time over the repetitions, i.e. a whole call (grid sampling, kernel(s), negation,
the allocator) as a time-stepper pays it.  hidden_gemm_flop counts the hidden layers' products for
value and tangents alone, points x L x H^2 x (1 + d_in) x 2; whole_call_tflops divides it by the
whole call's time and whole_call_share_of_peak by the 157.3 TF f32-MFMA peak as well -- a rate of
the whole call, not of the kernel.  peak_alloc_mb is torch's peak allocated memory over one call
beyond what was allocated before it; the fused leg's packed weights (L x H^2 floats) come from the
HIP runtime's stream-ordered pool and are added to its figure.  For the kernel alone:
    rocprofv3 --kernel-trace --stats -d DIR -- python3 tools/siren_timing.py --no-torch --rounds 1
--summarize prints per case and leg the median over the rounds with min and max, and whether the
fused leg's slowest round beat the torch leg's fastest.
"""
import argparse
import json
import math
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "neural-monte-carlo-fluid-simulation_amd"))

PEAK_F32_MFMA_TFLOPS = 157.3


def hidden_gemm_flop(points, d_in, hidden, n_hidden):
    return points * n_hidden * hidden * hidden * (1 + d_in) * 2


def summary(xs):
    xs = sorted(xs)
    return {"median": xs[len(xs) // 2], "min": xs[0], "max": xs[-1]}


def summarize(path):
    rows = [json.loads(l) for l in open(path) if l.strip().startswith("{")]
    rows = [r for r in rows if "case" in r and "fused_ms" in r and "torch_ms" in r]
    for case in sorted({r["case"] for r in rows}):
        v = [r for r in rows if r["case"] == case]
        fused, old = summary([r["fused_ms"] for r in v]), summary([r["torch_ms"] for r in v])
        flop = v[0]["hidden_gemm_flop"]
        out = {"summary": case, "rounds": len(v), "points": v[0]["points"], "fused_ms": fused, "torch_ms": old,
               "torch_over_fused": old["median"] / fused["median"],
               "fused_slowest_beats_torch_fastest": fused["max"] < old["min"],
               "hidden_gemm_flop": flop,
               "whole_call_tflops": flop / (fused["median"] * 1e-3) / 1e12,
               "whole_call_share_of_peak": flop / (fused["median"] * 1e-3) / 1e12 / PEAK_F32_MFMA_TFLOPS,
               "torch_whole_call_tflops": flop / (old["median"] * 1e-3) / 1e12,
               "peak_alloc_mb": {"fused": v[0]["fused_peak_alloc_mb"], "torch": v[0]["torch_peak_alloc_mb"]}}
        print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "siren_timing.jsonl"))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--seconds", type=float, default=0.5, help="least device time of work per leg and round")
    ap.add_argument("--summarize", metavar="FILE", default=None)
    ap.add_argument("--cases", nargs="*", default=None)
    ap.add_argument("--no-torch", action="store_true",
                    help="the fused leg only, nothing written to --out: for a kernel trace")
    a = ap.parse_args()
    if a.summarize:
        return summarize(a.summarize)
    import torch
    from wos_amd import projection as pj
    from wos_amd import workloads

    if not torch.cuda.is_available():
        sys.exit("siren_timing.py measures on the GPU: none is visible")
    dev = torch.device("cuda", 0)
    karman = workloads.karman_config(n_walks=8, n_points=64)
    cube = workloads.cube_config(res=4, n_walks=8)
    proj2 = pj.PressureProjector(dict(karman["scene"]), karman["solver"], karman["output"],
                                 torch.from_numpy(karman["points"]).to(dev))
    proj3 = pj.PressureProjector(dict(cube["scene"]), cube["solver"], cube["output"],
                                 torch.from_numpy(cube["points"]).to(dev))
    size2, size3 = workloads.scene_size(workloads.KARMAN_OBJ, 2), workloads.scene_size(workloads.CUBE_OBJ, 3)
    torch.manual_seed(11)
    cases = [("net2x128_2d", proj2, pj.Siren(2, 2, 2, 128).to(dev), 1000, size2),
             ("net3x256_2d", proj2, pj.Siren(2, 2, 3, 256).to(dev), 1000, size2),
             ("net3x256_3d", proj3, pj.Siren(3, 3, 3, 256).to(dev), 80, size3)]
    if a.cases:
        cases = [c for c in cases if c[0] in a.cases]

    def timed(fn):
        for _ in range(2):  # warm-up: code objects, hipBLASLt's choice, the allocator's blocks
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        reps = max(3, int(math.ceil(a.seconds * 1e3 / max(e0.elapsed_time(e1), 1e-3))))
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / reps, reps

    def peak_mb(fn):
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated(dev)
        torch.cuda.reset_peak_memory_stats(dev)
        fn()
        torch.cuda.synchronize()
        return (torch.cuda.max_memory_allocated(dev) - base) / 2 ** 20

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    f = None if a.no_torch else open(a.out, "a")
    for rnd in range(a.rounds):
        for name, proj, net, res, size in cases:
            lin = net.net[0]
            d_in, hidden, n_hidden = lin.in_features, lin.out_features, (len(net.net) - 3) // 2

            def fused():
                return proj.source_from_network(net, res, size)

            def old():
                return proj.source_from_velocity(net, res, size)

            new_div = fused()
            points = new_div.numel()
            fused_ms, fused_reps = timed(fused)
            row = {"case": name, "round": rnd, "points": points, "d_in": d_in, "hidden": hidden,
                   "hidden_layers": n_hidden, "grid": list(new_div.shape), "fused_ms": fused_ms,
                   "fused_reps": fused_reps}
            if a.no_torch:
                print(json.dumps(row), flush=True)
                continue
            torch_ms, torch_reps = timed(old)
            flop = hidden_gemm_flop(points, d_in, hidden, n_hidden)
            old_div = old()
            row.update({"torch_ms": torch_ms, "torch_reps": torch_reps, "hidden_gemm_flop": flop,
                        "whole_call_tflops": flop / (fused_ms * 1e-3) / 1e12,
                        "whole_call_share_of_peak": flop / (fused_ms * 1e-3) / 1e12 / PEAK_F32_MFMA_TFLOPS,
                        "fused_peak_alloc_mb": peak_mb(fused) + n_hidden * hidden * hidden * 4 / 2 ** 20,
                        "torch_peak_alloc_mb": peak_mb(old),
                        "max_abs_diff": float((new_div - old_div).abs().max()),
                        "max_abs_div": float(old_div.abs().max())})
            line = json.dumps(row)
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()
    if f is not None:
        f.close()


if __name__ == "__main__":
    main()
