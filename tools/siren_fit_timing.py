"""One iteration of the time-stepper's velocity fit (_project_velocity, src/2d/models/model_split.py:
274-283) three ways: today's PressureProjector.projection_loss, the existing fused pieces, and the
fused fit step (wos_siren_fit, csrc/wos_siren_fit.hip).  GPU box only.

    python3 tools/siren_fit_timing.py [--out profiles/siren_fit_timing.jsonl] [--rounds 3] [--seconds 0.5]
    python3 tools/siren_fit_timing.py --summarize profiles/siren_fit_timing.jsonl

Cases: net3x256_2d -- the reference's 2D network (src/2d/config.json: 3 x 256, 2 -> 2); net3x256_3d
-- its 3D network (3 -> 3); net2x128_2d -- 2 hidden layers of 128; each plain and through the
karman wrap of query_velocity (inlet clamp and wall weight).  An iteration is what one pass of the
training loop pays before Adam: the draw of 16 384 sample indices (the reference's
sample_resolution^2), the no-grad evaluation of the previous network for the target, the loss, and
the backward into every parameter's .grad.  Legs:
    a  projection_loss + backward: torch modules and autograd, the yardstick
    b  siren.eval for the target, siren.apply(value=True) + a torch loss + backward (wos_siren_eval,
       wos_siren_vjp)
    c  projection_fit_loss + backward (wos_siren_eval for the target, wos_siren_fit)
The legs alternate within a round in one process; each is warmed up, then repeated for at least
--seconds of work between two device events, the second followed by a synchronise.  peak_alloc_mb
is torch's peak allocated memory over one iteration beyond what was allocated before it; the
workspace the fused calls take from the HIP runtime's stream-ordered pool (packed weights, stash,
partial sums) is reported as workspace_mb and added.  max_rel_diff compares legs b and c with leg
a per gradient tensor, max |x - a| / max |a|, and reports the largest.  For leg c's kernels alone:
    rocprofv3 --kernel-trace --stats -d DIR -- python3 tools/siren_fit_timing.py --legs c --rounds 1 --out /dev/null
--summarize prints per case the median over the rounds with min and max of every leg, and whether
leg c's slowest round beat the fastest round of both other legs.
"""
import argparse
import json
import math
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "neural-monte-carlo-fluid-simulation_amd"))

DEFAULT_STASH = 256 << 20  # the stash cap with workspace_bytes = 0
LDS_MAX = 160 * 1024 - 4096
N_SAMPLES = 128 * 128


def _tiles(points, tile_bytes, resident):
    tiles_all = (points + 31) // 32
    tiles = min(tiles_all, DEFAULT_STASH // tile_bytes)
    if tiles < tiles_all and tiles > resident:
        tiles -= tiles % resident
    return tiles


def fit_workspace_bytes(points, d_in, d_out, hidden, n_hidden, compute_units):
    """The temporary one wos_siren_fit call with gradients takes (csrc/wos_siren.h siren_fit_plan)."""
    tile = (2 * n_hidden + 1) * hidden * 32 * 4
    tiles = _tiles(points, tile, compute_units * max(1, LDS_MAX // (((hidden + 7) * 32 + d_in * 32) * 4)))
    part = d_out * hidden + d_out + (n_hidden + 1) * hidden + hidden * d_in
    slices = (tiles + 15) // 16 if n_hidden else 0
    return (tiles * tile + tiles * part * 4 + slices * n_hidden * hidden * hidden * 4 + tiles * 4
            + 2 * n_hidden * hidden * hidden * 4 + hidden * 4)


def vjp_workspace_bytes(points, d_in, d_out, hidden, n_hidden, compute_units):
    """The temporary one wos_siren_vjp call takes (csrc/wos_siren.h siren_vjp_plan)."""
    c = 1 + d_in
    tile = (2 * n_hidden + 1) * hidden * c * 32 * 4
    tiles = _tiles(points, tile, compute_units * max(1, LDS_MAX // (((hidden + 3) * c * 32 + d_in * 32) * 4)))
    part = d_out * hidden + d_out + (n_hidden + 1) * hidden + hidden * d_in
    slices = (tiles * c + 15) // 16 if n_hidden else 0
    return (tiles * tile + tiles * part * 4 + slices * n_hidden * hidden * hidden * 4
            + 2 * n_hidden * hidden * hidden * 4 + hidden * 4)


def summary(xs):
    xs = sorted(xs)
    return {"median": xs[len(xs) // 2], "min": xs[0], "max": xs[-1]}


def summarize(path):
    rows = [json.loads(l) for l in open(path) if l.strip().startswith("{")]
    rows = [r for r in rows if "case" in r and all(f"{k}_ms" in r for k in "abc")]
    for case in sorted({r["case"] for r in rows}):
        v = [r for r in rows if r["case"] == case]
        ms = {k: summary([r[f"{k}_ms"] for r in v]) for k in "abc"}
        print(json.dumps({"summary": case, "rounds": len(v), "points": v[0]["points"],
                          "a_projection_loss_ms": ms["a"], "b_apply_ms": ms["b"], "c_fit_ms": ms["c"],
                          "a_over_c": ms["a"]["median"] / ms["c"]["median"],
                          "b_over_c": ms["b"]["median"] / ms["c"]["median"],
                          "c_slowest_beats_fastest_of_both": ms["c"]["max"] < min(ms["a"]["min"], ms["b"]["min"]),
                          "peak_alloc_mb": {k: v[0][f"{k}_peak_alloc_mb"] for k in "abc"},
                          "workspace_mb": {k: v[0][f"{k}_workspace_mb"] for k in "bc"},
                          "max_rel_diff": {k: max(r[f"{k}_max_rel_diff"] for r in v) for k in "bc"}}), flush=True)


def karman_wrap(size, eps=0.1, inlet_vel=0.5):
    """query_velocity's karman branch without an obstacle (src/2d/models/base.py:169-180), out of place."""
    import torch

    def wrap(x, u):
        inlet = (x[..., 0] >= size[0]) & (x[..., 0] <= size[0] + eps)
        ux = torch.where(inlet, torch.full_like(u[..., 0], inlet_vel), u[..., 0])
        w = (torch.min(torch.abs(x[..., 1] - size[2]).clamp(min=0, max=eps),
                       torch.abs(x[..., 1] - size[3]).clamp(min=0, max=eps)) / eps).detach()
        return torch.stack([ux, w * u[..., 1]] + [u[..., k] for k in range(2, u.shape[-1])], dim=-1)
    return wrap


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "siren_fit_timing.jsonl"))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--seconds", type=float, default=0.5, help="least device time of work per leg and round")
    ap.add_argument("--summarize", metavar="FILE", default=None)
    ap.add_argument("--cases", nargs="*", default=None)
    ap.add_argument("--legs", default="abc", help="the legs to run (a trace run takes `c` alone)")
    a = ap.parse_args()
    if a.summarize:
        return summarize(a.summarize)
    import torch
    from wos_amd import projection as pj
    from wos_amd import siren, workloads

    if not torch.cuda.is_available():
        sys.exit("siren_fit_timing.py measures on the GPU: none is visible")
    dev = torch.device("cuda", 0)
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    karman = workloads.karman_config(n_walks=8, n_points=65536)
    cube = workloads.cube_config(res=40, n_walks=8)
    proj2 = pj.PressureProjector(dict(karman["scene"]), karman["solver"], karman["output"],
                                 torch.from_numpy(karman["points"]).to(dev))
    proj3 = pj.PressureProjector(dict(cube["scene"]), cube["solver"], cube["output"],
                                 torch.from_numpy(cube["points"]).to(dev))
    size2, size3 = workloads.scene_size(workloads.KARMAN_OBJ, 2), workloads.scene_size(workloads.CUBE_OBJ, 3)
    torch.manual_seed(11)
    nets = [("net3x256_2d", proj2, (2, 2, 3, 256), size2), ("net3x256_3d", proj3, (3, 3, 3, 256), size3),
            ("net2x128_2d", proj2, (2, 2, 2, 128), size2)]
    cases = []
    for name, proj, shape, size in nets:
        net, prev = pj.Siren(*shape).to(dev), pj.Siren(*shape).to(dev).requires_grad_(False)
        cases.append((name + "_plain", proj, net, prev, None))
        cases.append((name + "_karman", proj, net, prev, karman_wrap([float(s) for s in size])))
    if a.cases:
        cases = [c for c in cases if c[0] in a.cases]

    def timed(fn):
        for _ in range(3):  # warm-up: code objects, hipBLASLt's choice, the allocator's blocks
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

    if a.out != os.devnull:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        for rnd in range(a.rounds):
            for name, proj, net, prev, wrap in cases:
                lin = net.net[0]
                d_in, hidden, n_hidden = lin.in_features, lin.out_features, (len(net.net) - 3) // 2
                d_out = net.net[-1].out_features
                params = list(net.parameters())
                n = proj.samples.shape[0]
                grad_p = 0.1 * torch.randn((n, d_in), device=dev, generator=torch.Generator(dev).manual_seed(5))
                gen = torch.Generator(dev)
                velocity = (lambda x: wrap(x, net(x))) if wrap else net
                velocity_prev = (lambda x: wrap(x, prev(x))) if wrap else prev

                def leg_a():
                    return proj.projection_loss(velocity, velocity_prev, grad_p, N_SAMPLES, generator=gen)

                def leg_b():
                    hi = n - 1 if proj.dim == 2 else n
                    idx = torch.randint(0, hi, (N_SAMPLES,), device=dev, generator=gen)
                    x = proj.samples[idx]
                    with torch.no_grad():
                        u_prev = siren.eval(prev, x)
                        target = (wrap(x, u_prev) if wrap else u_prev) - grad_p[idx]
                    u = siren.apply(net, x, value=True)
                    return torch.mean(((wrap(x, u) if wrap else u) - target) ** 2)

                def leg_c():
                    return proj.projection_fit_loss(net, prev, grad_p, N_SAMPLES, wrap=wrap, generator=gen)

                legs = {"a": leg_a, "b": leg_b, "c": leg_c}

                def step(k):
                    def run():
                        for p in params:
                            p.grad = None
                        gen.manual_seed(9)  # every leg and repetition fits the same samples
                        legs[k]().backward()
                    return run

                pack_b = n_hidden * hidden * hidden * 4  # wos_siren_eval's packed weights, freed before the next call
                ws = {"b": max(vjp_workspace_bytes(N_SAMPLES, d_in, d_out, hidden, n_hidden, cus), pack_b),
                      "c": max(fit_workspace_bytes(N_SAMPLES, d_in, d_out, hidden, n_hidden, cus), pack_b)}
                row = {"case": name, "round": rnd, "points": N_SAMPLES, "d_in": d_in, "hidden": hidden,
                       "hidden_layers": n_hidden, "wrap": wrap is not None}
                grads = {}
                for k in a.legs:
                    row[f"{k}_ms"], row[f"{k}_reps"] = timed(step(k))
                    grads[k] = [p.grad.clone() for p in params]
                    row[f"{k}_peak_alloc_mb"] = peak_mb(step(k)) + ws.get(k, 0) / 2 ** 20
                    if k in ws:
                        row[f"{k}_workspace_mb"] = ws[k] / 2 ** 20
                for k in "bc":
                    if k in grads and "a" in grads:
                        row[f"{k}_max_rel_diff"] = max(float((x - y).abs().max() / y.abs().max())
                                                       for x, y in zip(grads[k], grads["a"]) if float(y.abs().max()) > 0)
                line = json.dumps(row)
                print(line, flush=True)
                f.write(line + "\n")
                f.flush()


if __name__ == "__main__":
    main()
