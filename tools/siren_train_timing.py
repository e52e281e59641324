"""One iteration of the projection fit's training loop (_project_velocity in _training_loop,
src/2d/models/model_split.py:274-283, base.py:130-152), optimiser included, four ways.  GPU box only.

    python3 tools/siren_train_timing.py [--out profiles/siren_train_timing.jsonl] [--rounds 3] [--seconds 0.5]
    python3 tools/siren_train_timing.py --summarize profiles/siren_train_timing.jsonl

Cases: net3x256_2d plain and through the karman wrap, net3x256_3d, net2x128_2d; the pool is config
B's karman sample set (the cube's for 3D), the batch 16 384.  Legs:
    a   the reference's loop on the fused fit step: projection_fit_loss, zero_grad, backward,
        torch.optim.Adam.step(), loss.item()
    a2  the same without .item()
    b   on the pool's precomputed target: index draw, three gathers, siren.fit, siren.adam_step
    c   PressureProjector.fit_projection with iters_per_call = 256 (wos_siren_fit_run); its once-per-call
        evaluation of the previous network over the whole pool is included
and, per case, the optimiser step alone: siren.adam_step against torch.optim.Adam.step() (torch's
default implementation, named in the record) on the same gradients.  The legs alternate within a
round in one process, each on its own copy of the network; each is warmed up, then repeated for at
least --seconds of work between two device events, the second followed by a synchronise.  For leg
c's kernels alone:
    rocprofv3 --kernel-trace --stats -d DIR -- python3 tools/siren_train_timing.py --legs c --rounds 1 --out /dev/null
--summarize prints per case the median over the rounds with min and max of every leg, and whether
leg c's slowest round beat the fastest round of every other leg.
"""
import argparse
import copy
import json
import math
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "neural-monte-carlo-fluid-simulation_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

N_SAMPLES = 128 * 128
LEGS = ("a", "a2", "b", "c")


def summary(xs):
    xs = sorted(xs)
    return {"median": xs[len(xs) // 2], "min": xs[0], "max": xs[-1]}


def summarize(path):
    rows = [json.loads(l) for l in open(path) if l.strip().startswith("{")]
    rows = [r for r in rows if "case" in r and all(f"{k}_ms" in r for k in LEGS)]
    for case in sorted({r["case"] for r in rows}):
        v = [r for r in rows if r["case"] == case]
        ms = {k: summary([r[f"{k}_ms"] for r in v]) for k in LEGS + ("adam_fused", "adam_torch")}
        others = min(ms[k]["min"] for k in ("a", "a2", "b"))
        print(json.dumps({"summary": case, "rounds": len(v), "batch": v[0]["batch"], "pool": v[0]["pool"],
                          "a_reference_loop_ms": ms["a"], "a2_without_item_ms": ms["a2"], "b_fit_and_adam_step_ms": ms["b"],
                          "c_fit_projection_ms": ms["c"], "a_over_c": ms["a"]["median"] / ms["c"]["median"],
                          "b_over_c": ms["b"]["median"] / ms["c"]["median"],
                          "c_slowest_beats_fastest_of_every_other": ms["c"]["max"] < others,
                          "adam_step_fused_ms": ms["adam_fused"], "adam_step_torch_ms": ms["adam_torch"],
                          "torch_adam": v[0]["torch_adam"]}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "siren_train_timing.jsonl"))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--seconds", type=float, default=0.5, help="least device time of work per leg and round")
    ap.add_argument("--summarize", metavar="FILE", default=None)
    ap.add_argument("--cases", nargs="*", default=None)
    ap.add_argument("--legs", default=",".join(LEGS + ("adam",)),
                    help="the legs to run, comma-separated; adam: the optimiser step alone (a trace run takes `c` alone)")
    a = ap.parse_args()
    if a.summarize:
        return summarize(a.summarize)
    import torch
    from siren_fit_timing import karman_wrap
    from wos_amd import projection as pj
    from wos_amd import siren, workloads

    if not torch.cuda.is_available():
        sys.exit("siren_train_timing.py measures on the GPU: none is visible")
    legs_wanted = [k for k in a.legs.split(",") if k]
    dev = torch.device("cuda", 0)
    karman = workloads.karman_config(n_walks=8, n_points=65536)
    cube = workloads.cube_config(res=40, n_walks=8)
    proj2 = pj.PressureProjector(dict(karman["scene"]), karman["solver"], karman["output"],
                                 torch.from_numpy(karman["points"]).to(dev))
    proj3 = pj.PressureProjector(dict(cube["scene"]), cube["solver"], cube["output"],
                                 torch.from_numpy(cube["points"]).to(dev))
    size2 = workloads.scene_size(workloads.KARMAN_OBJ, 2)
    torch.manual_seed(11)
    cases = []
    for name, proj, shape, wrap in (("net3x256_2d_plain", proj2, (2, 2, 3, 256), None),
                                    ("net3x256_2d_karman", proj2, (2, 2, 3, 256), karman_wrap([float(s) for s in size2])),
                                    ("net3x256_3d_plain", proj3, (3, 3, 3, 256), None),
                                    ("net2x128_2d_plain", proj2, (2, 2, 2, 128), None)):
        cases.append((name, proj, pj.Siren(*shape).to(dev), pj.Siren(*shape).to(dev).requires_grad_(False), wrap))
    if a.cases:
        cases = [c for c in cases if c[0] in a.cases]

    def timed(fn, unit=1):
        """ms per iteration of fn(k), which runs k * unit iterations."""
        fn(3)  # warm-up: code objects, the allocator's blocks, the stream-ordered pool
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn(1)
        e1.record()
        e1.synchronize()
        reps = max(3, int(math.ceil(a.seconds * 1e3 / max(e0.elapsed_time(e1), 1e-3))))
        e0.record()
        fn(reps)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / (reps * unit), reps * unit

    if a.out != os.devnull:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        for rnd in range(a.rounds):
            for name, proj, net0, prev, wrap in cases:
                n, d = proj.samples.shape
                hi = n - 1 if proj.dim == 2 else n
                grad_p = 0.1 * torch.randn((n, d), device=dev, generator=torch.Generator(dev).manual_seed(5))
                gen = torch.Generator(dev).manual_seed(9)
                with torch.no_grad():
                    u_prev = siren.eval(prev, proj.samples)
                    scale, target = None, u_prev - grad_p
                    if wrap is not None:
                        scale, offset = siren.diagonal_wrap(wrap, proj.samples, d)
                        target = wrap(proj.samples, u_prev) - grad_p - offset

                def reference_loop(item):
                    net = copy.deepcopy(net0).requires_grad_(True)
                    opt = torch.optim.Adam(net.parameters(), lr=1e-4)

                    def run(k):
                        for _ in range(k):
                            loss = proj.projection_fit_loss(net, prev, grad_p, N_SAMPLES, wrap=wrap, generator=gen)
                            opt.zero_grad()
                            loss.backward()
                            opt.step()
                            if item:
                                loss.item()
                    return run

                def leg_b():
                    net = copy.deepcopy(net0).requires_grad_(False)
                    state = siren.AdamState(net)

                    def run(k):
                        for _ in range(k):
                            idx = torch.randint(0, hi, (N_SAMPLES,), device=dev, generator=gen)
                            _, gw, gb = siren.fit(net, proj.samples[idx], target[idx], None if scale is None else scale[idx])
                            siren.adam_step(net, (gw, gb), state)
                    return run

                def leg_c():
                    net = copy.deepcopy(net0).requires_grad_(False)
                    state = siren.AdamState(net)

                    def run(k):
                        proj.fit_projection(net, prev, grad_p, N_SAMPLES, 256 * k, state=state, wrap=wrap, generator=gen,
                                            iters_per_call=256)
                    return run

                def adam_alone(fused):
                    net = copy.deepcopy(net0).requires_grad_(not fused)
                    p = siren.pack(net)
                    grads = [torch.randn_like(t) for t in p.weights + p.biases]
                    nl = len(p.weights)
                    if fused:
                        state = siren.AdamState(net)
                        return lambda k: [siren.adam_step(net, (grads[:nl], grads[nl:]), state) for _ in range(k)]
                    params = [m.weight for m in net.net if hasattr(m, "weight")] + [m.bias for m in net.net if hasattr(m, "bias")]
                    for t, g in zip(params, grads):
                        t.grad = g
                    opt = torch.optim.Adam(params, lr=1e-4)
                    return lambda k: [opt.step() for _ in range(k)]

                legs = {"a": (reference_loop(True), 1), "a2": (reference_loop(False), 1), "b": (leg_b(), 1), "c": (leg_c(), 256)}
                d0 = torch.optim.Adam([torch.zeros(1, device=dev, requires_grad=True)]).defaults
                row = {"case": name, "round": rnd, "batch": N_SAMPLES, "pool": int(n), "d_in": int(d), "wrap": wrap is not None,
                       "torch_adam": f"torch {torch.__version__} default: foreach={d0.get('foreach')} fused={d0.get('fused')} "
                                     "(None, None: the foreach implementation on CUDA tensors)"}
                for k in legs_wanted:
                    if k == "adam":
                        row["adam_fused_ms"], _ = timed(adam_alone(True))
                        row["adam_torch_ms"], _ = timed(adam_alone(False))
                    else:
                        row[f"{k}_ms"], row[f"{k}_iters"] = timed(*legs[k])
                line = json.dumps(row)
                print(line, flush=True)
                f.write(line + "\n")
                f.flush()


if __name__ == "__main__":
    main()
