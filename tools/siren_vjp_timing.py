"""Training through the SIREN source: PressureProjector.source_from_network(differentiable=True)
and its fused backward (wos_siren_vjp, csrc/wos_siren_vjp.hip) beside
source_from_velocity(create_graph=True) and its second-order autograd backward, on the grids of
tools/siren_timing.py.  GPU box only.

    python3 tools/siren_vjp_timing.py [--out profiles/siren_vjp_timing.jsonl] [--rounds 3] [--seconds 0.5]
    python3 tools/siren_vjp_timing.py --summarize profiles/siren_vjp_timing.jsonl

Cases: net2x128_2d and net3x256_2d on the 401 x 1002 grid, net3x256_3d on the 82^3 grid (see
tools/siren_timing.py).  A step is the source (-div u on the grid, attached to the weights) plus
the backward of sum(g * div) for a fixed random g, which fills every parameter's .grad: what a
training step pays around the Monte-Carlo part.  Leg `torch` is the autograd path, leg `fused`
the two kernels.  The legs alternate within a round in one process; each is warmed up, then
repeated for at least --seconds of work between two device events, the second followed by a
synchronise.  peak_alloc_mb is torch's peak allocated memory over one step beyond what was
allocated before it; the fused leg's workspace (the stash, the partial sums and the two packed
copies of the weights) comes from the HIP runtime's stream-ordered pool, is reported as
fused_workspace_mb and is added to the fused leg's figure.  max_rel_diff compares the two legs'
gradients per tensor, max |a - b| / max |b|, and reports the largest.
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

DEFAULT_STASH = 256 << 20  # wos_siren_vjp's stash cap with workspace_bytes = 0


def workspace_bytes(points, d_in, d_out, hidden, n_hidden, compute_units):
    """The temporary one wos_siren_vjp call takes (csrc/wos_siren.h siren_vjp_plan, wos_capi_siren.cpp)."""
    c = 1 + d_in
    tile = (2 * n_hidden + 1) * hidden * c * 32 * 4
    tiles_all = (points + 31) // 32
    tiles = min(tiles_all, DEFAULT_STASH // tile)
    resident = compute_units * max(1, (160 * 1024 - 4096) // (((hidden + 3) * c * 32 + d_in * 32) * 4))
    if tiles < tiles_all and tiles > resident:
        tiles -= tiles % resident
    part = d_out * hidden + d_out + (n_hidden + 1) * hidden + hidden * d_in
    slices = (tiles * c + 15) // 16 if n_hidden else 0
    return (tiles * tile + tiles * part * 4 + slices * n_hidden * hidden * hidden * 4
            + 2 * n_hidden * hidden * hidden * 4 + hidden * 4)


def summary(xs):
    xs = sorted(xs)
    return {"median": xs[len(xs) // 2], "min": xs[0], "max": xs[-1]}


def summarize(path):
    rows = [json.loads(l) for l in open(path) if l.strip().startswith("{")]
    rows = [r for r in rows if "case" in r and "fused_ms" in r and "torch_ms" in r]
    for case in sorted({r["case"] for r in rows}):
        v = [r for r in rows if r["case"] == case]
        fused, old = summary([r["fused_ms"] for r in v]), summary([r["torch_ms"] for r in v])
        print(json.dumps({"summary": case, "rounds": len(v), "points": v[0]["points"], "fused_ms": fused, "torch_ms": old,
                          "torch_over_fused": old["median"] / fused["median"],
                          "fused_slowest_beats_torch_fastest": fused["max"] < old["min"],
                          "peak_alloc_mb": {"fused": v[0]["fused_peak_alloc_mb"], "torch": v[0]["torch_peak_alloc_mb"]},
                          "fused_workspace_mb": v[0]["fused_workspace_mb"],
                          "max_rel_diff": max(r["max_rel_diff"] for r in v)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "siren_vjp_timing.jsonl"))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--seconds", type=float, default=0.5, help="least device time of work per leg and round")
    ap.add_argument("--summarize", metavar="FILE", default=None)
    ap.add_argument("--cases", nargs="*", default=None)
    a = ap.parse_args()
    if a.summarize:
        return summarize(a.summarize)
    import torch
    from wos_amd import projection as pj
    from wos_amd import workloads

    if not torch.cuda.is_available():
        sys.exit("siren_vjp_timing.py measures on the GPU: none is visible")
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
    with open(a.out, "a") as f:
        for rnd in range(a.rounds):
            for name, proj, net, res, size in cases:
                lin = net.net[0]
                d_in, hidden, n_hidden = lin.in_features, lin.out_features, (len(net.net) - 3) // 2
                d_out = net.net[-1].out_features
                params = [p for p in net.parameters()]
                shape = tuple(proj.source_from_network(net, res, size).shape)
                g = torch.randn(shape, device=dev, generator=torch.Generator(dev).manual_seed(5))

                def step(source):
                    for p in params:
                        p.grad = None
                    (g * source()).sum().backward()

                def fused():
                    step(lambda: proj.source_from_network(net, res, size, differentiable=True))

                def old():
                    step(lambda: proj.source_from_velocity(net, res, size, create_graph=True))

                def grads():
                    return [torch.zeros_like(p) if p.grad is None else p.grad.clone() for p in params]

                fused_ms, fused_reps = timed(fused)
                got = grads()
                torch_ms, torch_reps = timed(old)
                want = grads()
                rel = max(float((x - y).abs().max() / y.abs().max()) for x, y in zip(got, want) if float(y.abs().max()) > 0)
                points = int(g.numel())
                ws = workspace_bytes(points, d_in, d_out, hidden, n_hidden,
                                     torch.cuda.get_device_properties(dev).multi_processor_count)
                row = {"case": name, "round": rnd, "points": points, "d_in": d_in, "hidden": hidden,
                       "hidden_layers": n_hidden, "grid": list(shape), "fused_ms": fused_ms, "fused_reps": fused_reps,
                       "torch_ms": torch_ms, "torch_reps": torch_reps, "fused_workspace_mb": ws / 2 ** 20,
                       "fused_peak_alloc_mb": peak_mb(fused) + ws / 2 ** 20, "torch_peak_alloc_mb": peak_mb(old),
                       "max_rel_diff": rel}
                line = json.dumps(row)
                print(line, flush=True)
                f.write(line + "\n")
                f.flush()


if __name__ == "__main__":
    main()
