"""The velocity fit through a wrap that mixes the velocity's components (wos_amd.projection.slip_wrap:
the reference's jpipe branch, src/2d/models/base.py:191-222), the route it had before the fit step
took a matrix per point against the fused one, by tools/siren_fit_timing.py's method.  GPU box only.

    python3 tools/siren_fit_matrix_timing.py [--out profiles/siren_fit_matrix_timing.jsonl] [--rounds 3] [--seconds 0.5]
    python3 tools/siren_fit_matrix_timing.py --summarize profiles/siren_fit_matrix_timing.jsonl

Cases: net3x256_2d, net3x256_3d and net2x128_2d as in siren_fit_timing.py, each through a slip wrap
around a circle (a sphere in 3D) in the middle of the scene, the weight rising from 0 on it to 1 a
quarter of the scene's height away.  An iteration fits 16 384 samples.  Legs:
    a  one iteration before Adam on the route without the matrix form: siren.eval for the target,
       siren.apply(value=True), the wrap and the loss in torch, backward (wos_siren_eval, wos_siren_vjp)
    b  the same through projection_fit_loss + backward (wos_siren_eval, wos_siren_fit with a matrix per
       point; the wrap's matrix is built from d_out + 1 calls of it)
    la the training loop around leg a with torch.optim.Adam, per iteration
    lb PressureProjector.fit_projection (wos_siren_fit_run), per iteration over --iters iterations, the
       pool's target and matrices included
The legs alternate within a round in one process; each is warmed up, then repeated for at least
--seconds of work between two device events, the second followed by a synchronise.  max_rel_diff
compares leg b's gradients with leg a's per tensor, max |x - a| / max |a|, and reports the largest.
--summarize prints per case the median over the rounds with min and max of every leg, and whether
the fused leg's slowest round beat the other route's fastest, for the step and for the loop.
"""
import argparse
import copy
import json
import math
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "neural-monte-carlo-fluid-simulation_amd"))

N_SAMPLES = 128 * 128
LEGS = ("a", "b", "la", "lb")


def summary(xs):
    xs = sorted(xs)
    return {"median": xs[len(xs) // 2], "min": xs[0], "max": xs[-1]}


def summarize(path):
    rows = [json.loads(l) for l in open(path) if l.strip().startswith("{")]
    rows = [r for r in rows if "case" in r and all(f"{k}_ms" in r for k in LEGS)]
    for case in sorted({r["case"] for r in rows}):
        v = [r for r in rows if r["case"] == case]
        ms = {k: summary([r[f"{k}_ms"] for r in v]) for k in LEGS}
        print(json.dumps({"summary": case, "rounds": len(v), "points": v[0]["points"], "loop_iters": v[0]["loop_iters"],
                          "a_apply_ms": ms["a"], "b_fit_ms": ms["b"], "la_python_loop_ms": ms["la"],
                          "lb_fit_projection_ms": ms["lb"],
                          "a_over_b": ms["a"]["median"] / ms["b"]["median"],
                          "la_over_lb": ms["la"]["median"] / ms["lb"]["median"],
                          "b_slowest_beats_a_fastest": ms["b"]["max"] < ms["a"]["min"],
                          "lb_slowest_beats_la_fastest": ms["lb"]["max"] < ms["la"]["min"],
                          "max_rel_diff": max(r["b_max_rel_diff"] for r in v)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "siren_fit_matrix_timing.jsonl"))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--seconds", type=float, default=0.5, help="least device time of work per leg and round")
    ap.add_argument("--iters", type=int, default=256, help="iterations of one loop leg (fit_projection's iters_per_call)")
    ap.add_argument("--summarize", metavar="FILE", default=None)
    ap.add_argument("--cases", nargs="*", default=None)
    a = ap.parse_args()
    if a.summarize:
        return summarize(a.summarize)
    import torch
    from wos_amd import projection as pj
    from wos_amd import siren, workloads

    if not torch.cuda.is_available():
        sys.exit("siren_fit_matrix_timing.py measures on the GPU: none is visible")
    dev = torch.device("cuda", 0)
    karman = workloads.karman_config(n_walks=8, n_points=65536)
    cube = workloads.cube_config(res=40, n_walks=8)
    proj2 = pj.PressureProjector(dict(karman["scene"]), karman["solver"], karman["output"],
                                 torch.from_numpy(karman["points"]).to(dev))
    proj3 = pj.PressureProjector(dict(cube["scene"]), cube["solver"], cube["output"],
                                 torch.from_numpy(cube["points"]).to(dev))
    size2, size3 = workloads.scene_size(workloads.KARMAN_OBJ, 2), workloads.scene_size(workloads.CUBE_OBJ, 3)

    def slip(size):
        d = len(size) // 2
        centre = torch.tensor([0.5 * (float(size[2 * k]) + float(size[2 * k + 1])) for k in range(d)], device=dev)
        height = min(float(size[2 * k + 1]) - float(size[2 * k]) for k in range(d))
        radius, eps = 0.2 * height, 0.25 * height

        def normal(x):
            r = x - centre
            return r / torch.sqrt((r * r).sum(-1, keepdim=True))

        def weight(x):
            r = x - centre
            return ((torch.sqrt((r * r).sum(-1)) - radius) / eps).clamp(min=0, max=1)
        return pj.slip_wrap(normal, weight)

    torch.manual_seed(11)
    cases = []
    for name, proj, shape, size in (("net3x256_2d", proj2, (2, 2, 3, 256), size2), ("net3x256_3d", proj3, (3, 3, 3, 256), size3),
                                    ("net2x128_2d", proj2, (2, 2, 2, 128), size2)):
        cases.append((name + "_slip", proj, pj.Siren(*shape).to(dev), pj.Siren(*shape).to(dev).requires_grad_(False), slip(size)))
    if a.cases:
        cases = [c for c in cases if c[0] in a.cases]

    def timed(fn, per=1):
        for _ in range(3 if per == 1 else 1):  # warm-up: code objects, hipBLASLt's choice, the allocator's blocks
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
        return e0.elapsed_time(e1) / reps / per, reps

    if a.out != os.devnull:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        for rnd in range(a.rounds):
            for name, proj, net0, prev, wrap in cases:
                lin = net0.net[0]
                d_in, hidden, n_hidden = lin.in_features, lin.out_features, (len(net0.net) - 3) // 2
                n = proj.samples.shape[0]
                hi = n - 1 if proj.dim == 2 else n
                grad_p = 0.1 * torch.randn((n, d_in), device=dev, generator=torch.Generator(dev).manual_seed(5))
                gen = torch.Generator(dev)
                net = copy.deepcopy(net0)  # the loop legs train: every leg and round starts from the same weights
                params = list(net.parameters())

                def leg_a(net_=net):
                    idx = torch.randint(0, hi, (N_SAMPLES,), device=dev, generator=gen)
                    x = proj.samples[idx]
                    with torch.no_grad():
                        target = wrap(x, siren.eval(prev, x)) - grad_p[idx]
                    return torch.mean((wrap(x, siren.apply(net_, x, value=True)) - target) ** 2)

                def leg_b():
                    return proj.projection_fit_loss(net, prev, grad_p, N_SAMPLES, wrap=wrap, generator=gen)

                def step(leg):
                    def run():
                        for p in params:
                            p.grad = None
                        gen.manual_seed(9)  # every leg and repetition fits the same samples
                        leg().backward()
                    return run

                def loop_a():
                    mine = copy.deepcopy(net0)
                    opt = torch.optim.Adam(mine.parameters(), lr=1e-4)
                    gen.manual_seed(9)
                    for _ in range(a.iters):
                        opt.zero_grad(set_to_none=True)
                        leg_a(mine).backward()
                        opt.step()

                def loop_b():
                    mine = copy.deepcopy(net0)
                    gen.manual_seed(9)
                    proj.fit_projection(mine, prev, grad_p, N_SAMPLES, a.iters, wrap=wrap, generator=gen, iters_per_call=a.iters)

                row = {"case": name, "round": rnd, "points": N_SAMPLES, "d_in": d_in, "hidden": hidden,
                       "hidden_layers": n_hidden, "loop_iters": a.iters}
                grads = {}
                for k, leg in (("a", leg_a), ("b", leg_b)):
                    row[f"{k}_ms"], row[f"{k}_reps"] = timed(step(leg))
                    grads[k] = [p.grad.clone() for p in params]
                row["la_ms"], row["la_reps"] = timed(loop_a, per=a.iters)
                row["lb_ms"], row["lb_reps"] = timed(loop_b, per=a.iters)
                row["b_max_rel_diff"] = max(float((x - y).abs().max() / y.abs().max())
                                            for x, y in zip(grads["b"], grads["a"]) if float(y.abs().max()) > 0)
                line = json.dumps(row)
                print(line, flush=True)
                f.write(line + "\n")
                f.flush()


if __name__ == "__main__":
    main()
