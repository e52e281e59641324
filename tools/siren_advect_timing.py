"""One iteration of the advection fit's training loop (_advect_velocity in _training_loop,
src/2d/models/model_split.py:88-120, base.py:130-152), optimiser included, four ways.  GPU box only.

    python3 tools/siren_advect_timing.py [--out profiles/siren_advect_timing.jsonl] [--rounds 3] [--seconds 0.5]
    python3 tools/siren_advect_timing.py --summarize profiles/siren_advect_timing.jsonl

Cases: net3x256_2d plain, net3x256_2d through the karman wrap with the samples inside a disk dropped
(keep), net3x256_3d, net2x128_2d, each with the previous network alone and with network_tilde (the
reference's `flag` branch); 16 384 fresh points per iteration.  Legs:
    a   the reference's loop on the fused fit step: draw (and filter), advection_fit_loss, zero_grad,
        backward, torch.optim.Adam.step(), loss.item()
    a2  the same without .item()
    b   the same pieces per iteration from Python with the fused optimiser: draw (and filter), the
        backtrack, clamp and target in torch around siren.eval, siren.fit, siren.adam_step
    c   wos_amd.projection.fit_advection with iters_per_call = 256 (wos_siren_fit_run_batches)
The legs alternate within a round in one process, each on its own copy of the network; each is warmed
up, then repeated for at least --seconds of work between two device events, the second followed by a
synchronise.  c_peak_alloc_mb is torch's peak allocation over one block of 256 iterations (the
library's stream-ordered workspace is not torch's and not in it).  --package DIR measures the package
of another checkout (legs a, a2 and b exist before fit_advection does).  For leg c's kernels alone:
    rocprofv3 --kernel-trace --stats -d DIR -- python3 tools/siren_advect_timing.py --legs c --rounds 1 --out /dev/null
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

N_SAMPLES = 128 * 128
LEGS = ("a", "a2", "b", "c")
DT = 0.05


def summary(xs):
    xs = sorted(xs)
    return {"median": xs[len(xs) // 2], "min": xs[0], "max": xs[-1]}


def summarize(path):
    rows = [json.loads(l) for l in open(path) if l.strip().startswith("{")]
    rows = [r for r in rows if "case" in r and all(f"{k}_ms" in r for k in LEGS)]
    for case in sorted({r["case"] for r in rows}):
        v = [r for r in rows if r["case"] == case]
        ms = {k: summary([r[f"{k}_ms"] for r in v]) for k in LEGS}
        others = min(ms[k]["min"] for k in ("a", "a2", "b"))
        print(json.dumps({"summary": case, "rounds": len(v), "batch": v[0]["batch"], "mean_kept": v[0]["mean_kept"],
                          "a_reference_loop_ms": ms["a"], "a2_without_item_ms": ms["a2"], "b_fit_and_adam_step_ms": ms["b"],
                          "c_fit_advection_ms": ms["c"], "a_over_c": ms["a"]["median"] / ms["c"]["median"],
                          "b_over_c": ms["b"]["median"] / ms["c"]["median"],
                          "c_slowest_beats_fastest_of_every_other": ms["c"]["max"] < others,
                          "c_peak_alloc_mb": max(r["c_peak_alloc_mb"] for r in v)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "siren_advect_timing.jsonl"))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--seconds", type=float, default=0.5, help="least device time of work per leg and round")
    ap.add_argument("--summarize", metavar="FILE", default=None)
    ap.add_argument("--cases", nargs="*", default=None)
    ap.add_argument("--legs", default=",".join(LEGS), help="the legs to run, comma-separated (a trace run takes `c` alone)")
    ap.add_argument("--package", default=os.path.join(REPO, "neural-monte-carlo-fluid-simulation_amd"),
                    help="the directory that holds wos_amd (another checkout's, to measure legs a, a2 and b there)")
    ap.add_argument("--label", default="head", help="recorded with every row")
    a = ap.parse_args()
    if a.summarize:
        return summarize(a.summarize)
    import torch
    from siren_fit_timing import karman_wrap  # puts this checkout's package on the path: --package goes in front of it
    sys.path.insert(0, os.path.abspath(a.package))
    from wos_amd import projection as pj
    from wos_amd import siren, workloads

    if not torch.cuda.is_available():
        sys.exit("siren_advect_timing.py measures on the GPU: none is visible")
    legs_wanted = [k for k in a.legs.split(",") if k]
    dev = torch.device("cuda", 0)
    size2 = [float(s) for s in workloads.scene_size(workloads.KARMAN_OBJ, 2)]
    size3 = [float(s) for s in workloads.scene_size(workloads.CUBE_OBJ, 3)]
    cx, cy, r = size2[0] + 0.25 * (size2[1] - size2[0]), 0.5 * (size2[2] + size2[3]), 0.125 * (size2[3] - size2[2])

    def outside_disk(x):
        return (x[..., 0] - cx) ** 2 + (x[..., 1] - cy) ** 2 > r * r
    torch.manual_seed(11)
    cases = []
    for name, shape, size, wrap, keep in (("net3x256_2d_plain", (2, 2, 3, 256), size2, None, None),
                                          ("net3x256_2d_karman_keep", (2, 2, 3, 256), size2, karman_wrap(size2), outside_disk),
                                          ("net3x256_3d_plain", (3, 3, 3, 256), size3, None, None),
                                          ("net2x128_2d_plain", (2, 2, 2, 128), size2, None, None)):
        nets = [pj.Siren(*shape).to(dev)] + [pj.Siren(*shape).to(dev).requires_grad_(False) for _ in range(2)]
        for with_tilde in (False, True):
            cases.append((name + ("_tilde" if with_tilde else ""), size, nets[0], nets[1], nets[2] if with_tilde else None,
                          wrap, keep))
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
            for name, size, net0, prev, tilde, wrap, keep in cases:
                d = len(size) // 2
                gen = torch.Generator(dev).manual_seed(9)

                def draw():
                    x = torch.rand(N_SAMPLES, d, device=dev, generator=gen)
                    for c in range(d):
                        x[..., c] = x[..., c] * (size[2 * c + 1] - size[2 * c]) + size[2 * c]
                    return x if keep is None else x[keep(x)]

                def reference_loop(item):
                    net = copy.deepcopy(net0).requires_grad_(True)
                    opt = torch.optim.Adam(net.parameters(), lr=1e-4)

                    def run(k):
                        for _ in range(k):
                            loss = pj.advection_fit_loss(net, prev, draw(), DT, size, network_tilde=tilde, wrap=wrap)
                            opt.zero_grad()
                            loss.backward()
                            opt.step()
                            if item:
                                loss.item()
                    return run

                def leg_b():
                    net = copy.deepcopy(net0).requires_grad_(False)
                    state = siren.AdamState(net)

                    def query(n_, pts):
                        u = siren.eval(n_, pts)
                        return u if wrap is None else wrap(pts, u)

                    def run(k):
                        for _ in range(k):
                            x = draw()
                            back = x - query(prev, x) * DT
                            back = torch.stack([back[..., c].clamp(min=size[2 * c], max=size[2 * c + 1]) for c in range(d)], dim=-1)
                            target = query(prev, back)
                            if tilde is not None:
                                target = 2 * target - query(tilde, back)
                            scale = None
                            if wrap is not None:
                                scale, offset = siren.diagonal_wrap(wrap, x, d, check=False)
                                target = target - offset
                            _, gw, gb = siren.fit(net, x, target, scale)
                            siren.adam_step(net, (gw, gb), state)
                    return run

                def leg_c():
                    net = copy.deepcopy(net0).requires_grad_(False)
                    state = siren.AdamState(net)

                    def run(k):
                        pj.fit_advection(net, prev, DT, size, 256 * k, n_samples=N_SAMPLES, network_tilde=tilde, wrap=wrap,
                                         keep=keep, state=state, generator=gen, iters_per_call=256)
                    return run

                legs = {"a": (reference_loop(True), 1), "a2": (reference_loop(False), 1), "b": (leg_b(), 1), "c": (leg_c(), 256)}
                kept = N_SAMPLES if keep is None else float(sum(draw().shape[0] for _ in range(8))) / 8
                row = {"case": name, "round": rnd, "label": a.label, "batch": N_SAMPLES, "mean_kept": kept, "d_in": d,
                       "wrap": wrap is not None, "keep": keep is not None, "tilde": tilde is not None,
                       "torch": torch.__version__}
                for k in legs_wanted:
                    row[f"{k}_ms"], row[f"{k}_iters"] = timed(*legs[k])
                    if k == "c":
                        torch.cuda.synchronize()
                        torch.cuda.reset_peak_memory_stats(dev)
                        legs["c"][0](1)
                        torch.cuda.synchronize()
                        row["c_peak_alloc_mb"] = torch.cuda.max_memory_allocated(dev) / 2 ** 20
                line = json.dumps(row)
                print(line, flush=True)
                f.write(line + "\n")
                f.flush()


if __name__ == "__main__":
    main()
