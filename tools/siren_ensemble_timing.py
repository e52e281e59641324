"""The fit loops of an ensemble, one member after the other against all members in one device loop
(wos_siren_fit_run_ensemble, wos_siren_fit_run_batches_ensemble; DESIGN.md "Ensemble fit loops").
GPU box only.

    python3 tools/siren_ensemble_timing.py [--out profiles/siren_ensemble_timing.jsonl] [--rounds 3] [--seconds 0.5]
    python3 tools/siren_ensemble_timing.py --summarize profiles/siren_ensemble_timing.jsonl

Cases: the reference's networks, net2x128 2 -> 2 (karman, karman3d), net5x64 3 -> 3 (smoke3d, smoke_obs,
vortex_collide) and net3x256 2 -> 2 at 16 384 points per iteration, net6x64 2 -> 2 at 4 096
(taylorgreen); E = 2 and 4 members.  Legs, each a call of 64 iterations:
    a    E calls of siren.fit_run, one member after the other
    b    one call of siren.fit_run_ensemble
    ab   E calls of siren.fit_run_batches
    bb   one call of siren.fit_run_batches_ensemble
    s    one member through siren.fit_run            (the single-network entry point)
    s1   one member through siren.fit_run_ensemble   (E = 1 through the new one)
The legs alternate within a round in one process, each on its own copies of the networks; each is
warmed up, then repeated for at least --seconds of work between two device events, the second followed
by a synchronise.  Every figure is milliseconds per iteration AND MEMBER.  --package DIR measures the
package of another checkout (the parent commit's has legs a, ab and s only: that pins that the
single-network path did not get slower), --label names its rows.  For leg b's kernels alone:
    rocprofv3 --kernel-trace --stats -d DIR -- python3 tools/siren_ensemble_timing.py --legs b --cases net2x128 \\
        --members 4 --rounds 1 --out /dev/null
--summarize prints per case and E the median over the rounds with min and max of every leg, (b)'s time
over (a)'s, whether (b)'s slowest round beat (a)'s fastest, and the parent's rows beside this checkout's.
"""
import argparse
import copy
import json
import math
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LEGS = ("a", "b", "ab", "bb", "s", "s1")
ITERS = 64
# name: (d_in, d_out, hidden layers, hidden, points per iteration)
CASES = {"net2x128": (2, 2, 2, 128, 16384), "net5x64": (3, 3, 5, 64, 16384), "net6x64": (2, 2, 6, 64, 4096),
         "net3x256": (2, 2, 3, 256, 16384)}
N_POOL = 65536


def summary(xs):
    xs = sorted(xs)
    return {"median": xs[len(xs) // 2], "min": xs[0], "max": xs[-1]}


def summarize(path):
    rows = [json.loads(l) for l in open(path) if l.strip().startswith("{")]
    rows = [r for r in rows if "case" in r and "members" in r]
    for case in CASES:
        for E in sorted({r["members"] for r in rows if r["case"] == case}):
            out = {"summary": case, "members": E}
            for label in sorted({r["label"] for r in rows}):
                v = [r for r in rows if r["case"] == case and r["members"] == E and r["label"] == label]
                ms = {k: summary([r[f"{k}_ms"] for r in v]) for k in LEGS if v and all(f"{k}_ms" in r for r in v)}
                if not ms:
                    continue
                out[label] = {"rounds": len(v), **{f"{k}_ms_per_iter_member": ms[k] for k in ms}}
                for one, ens in (("a", "b"), ("ab", "bb"), ("s", "s1")):
                    if one in ms and ens in ms:
                        out[label][f"{ens}_over_{one}"] = ms[ens]["median"] / ms[one]["median"]
                        out[label][f"{ens}_slowest_beats_{one}_fastest"] = ms[ens]["max"] < ms[one]["min"]
            print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "siren_ensemble_timing.jsonl"))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--seconds", type=float, default=0.5, help="least device time of work per leg and round")
    ap.add_argument("--summarize", metavar="FILE", default=None)
    ap.add_argument("--cases", nargs="*", default=None)
    ap.add_argument("--members", nargs="*", type=int, default=[2, 4])
    ap.add_argument("--legs", default=",".join(LEGS), help="the legs to run, comma-separated (a trace run takes `b` alone)")
    ap.add_argument("--package", default=os.path.join(REPO, "neural-monte-carlo-fluid-simulation_amd"),
                    help="the directory that holds wos_amd (another checkout's, to measure legs a, ab and s there)")
    ap.add_argument("--label", default="head", help="recorded with every row")
    a = ap.parse_args()
    if a.summarize:
        return summarize(a.summarize)
    import torch
    sys.path.insert(0, os.path.abspath(a.package))
    from wos_amd import projection as pj
    from wos_amd import siren

    if not torch.cuda.is_available():
        sys.exit("siren_ensemble_timing.py measures on the GPU: none is visible")
    legs_wanted = [k for k in a.legs.split(",") if k]
    dev = torch.device("cuda", 0)
    torch.manual_seed(11)

    def timed(fn, iters):
        """ms per iteration of fn(k), which runs k calls of `iters` iterations."""
        fn(2)  # warm-up: code objects, the allocator's blocks, the stream-ordered pool
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn(1)
        e1.record()
        e1.synchronize()
        reps = max(2, int(math.ceil(a.seconds * 1e3 / max(e0.elapsed_time(e1), 1e-3))))
        e0.record()
        fn(reps)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / (reps * iters), reps * iters

    if a.out != os.devnull:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        for rnd in range(a.rounds):
            for name, (d, d_out, L, H, batch) in CASES.items():
                if a.cases and name not in a.cases:
                    continue
                for E in a.members:
                    nets0 = [pj.Siren(d, d_out, L, H).to(dev).requires_grad_(False) for _ in range(E)]
                    pool = torch.rand(N_POOL, d, device=dev)
                    pool_t = [torch.randn(N_POOL, d_out, device=dev) for _ in range(E)]
                    pool_s = [torch.rand(N_POOL, d_out, device=dev) + 0.5 for _ in range(E)]
                    idx = torch.randint(0, N_POOL, (ITERS, batch), device=dev)
                    x = torch.rand(ITERS * batch, d, device=dev)
                    rows_t = [torch.randn(ITERS * batch, d_out, device=dev) for _ in range(E)]
                    rows_s = [torch.rand(ITERS * batch, d_out, device=dev) + 0.5 for _ in range(E)]
                    counts = [batch] * ITERS

                    def members(n=E):
                        nets = [copy.deepcopy(m) for m in nets0[:n]]
                        return nets, [siren.AdamState(m) for m in nets]

                    def leg(which):
                        n = 1 if which in ("s", "s1") else E
                        nets, states = members(n)

                        def run(k):
                            for _ in range(k):
                                if which in ("a", "s"):
                                    for e in range(n):
                                        siren.fit_run(nets[e], states[e], pool, pool_t[e], pool_s[e], idx)
                                elif which in ("b", "s1"):
                                    siren.fit_run_ensemble(nets, states, pool, pool_t[:n], pool_s[:n], idx)
                                elif which == "ab":
                                    for e in range(n):
                                        siren.fit_run_batches(nets[e], states[e], x, rows_t[e], rows_s[e], counts)
                                else:
                                    siren.fit_run_batches_ensemble(nets, states, x, rows_t, rows_s, counts)
                        return run, n
                    row = {"case": name, "round": rnd, "label": a.label, "members": E, "batch": batch, "d_in": d, "d_out": d_out,
                           "hidden": H, "hidden_layers": L, "iters_per_call": ITERS, "torch": torch.__version__}
                    for k in legs_wanted:
                        run, n = leg(k)
                        ms, iters = timed(run, ITERS)
                        row[f"{k}_ms"], row[f"{k}_iters"] = ms / n, iters  # per iteration and member
                    line = json.dumps(row)
                    print(line, flush=True)
                    f.write(line + "\n")
                    f.flush()


if __name__ == "__main__":
    main()
