"""Geometry queries: the device time of WosScene.query (wos_scene_query, csrc/wos_query.hip)
beside a chunked torch-on-device brute force -- the best a caller could do without leaving the
device before the query existed.  GPU box only.

    python3 tools/query_timing.py [--out profiles/query_timing.jsonl] [--rounds 3] [--reps 50]
    python3 tools/query_timing.py --summarize profiles/query_timing.jsonl

Scenes: karman (geometry_1cyl_long_open.obj, 80 segments) and the engine outline (647 segments).
Points: the grid sample_uniform_2d(1000, size, with_boundary=True) gives over the scene's bounding
box (what get_divergence's query_velocity evaluates the obstacle SDF on) and 16 384 random points.
Every figure is HIP-event time of `reps` back-to-back calls on one stream divided by reps, after a
warm-up, with distance, signed distance, state and closest point all asked for; the legs
alternate within a round.  query_us is WosScene.query as a caller uses it: four torch.empty and one
ctypes call per query, so for a short kernel it is the host's rate of enqueueing, not the
kernel's time.  enqueue_only_us calls wos_scene_query directly on buffers allocated once: the
stream stays full whenever the kernel outlasts one ctypes call, and the figure is then the kernel
plus the gap between launches.  For the kernel alone, trace one case:
    rocprofv3 --kernel-trace --stats -d DIR -- python3 tools/query_timing.py --no-torch --rounds 1 --cases CASE
The brute force computes distance, closest point and the segment-normal
sign (no vertex normals, no state word); its largest |distance - query's| is recorded as a sanity
check.  --summarize prints per case and leg the median over the rounds with min and max.
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "neural-monte-carlo-fluid-simulation_amd"))


def summary(xs):
    xs = sorted(xs)
    return {"median": xs[len(xs) // 2], "min": xs[0], "max": xs[-1]}


def summarize(path):
    rows = [json.loads(l) for l in open(path) if l.strip().startswith("{")]
    rows = [r for r in rows if "case" in r and "query_us" in r]
    for case in sorted({r["case"] for r in rows}):
        v = [r for r in rows if r["case"] == case]
        out = {"summary": case, "rounds": len(v), "points": v[0]["points"], "segments": v[0]["segments"],
               "query_us": summary([r["query_us"] for r in v]),
               "enqueue_only_us": summary([r["enqueue_only_us"] for r in v]) if all("enqueue_only_us" in r for r in v) else None,
               "torch_us": summary([r["torch_us"] for r in v]),
               "max_abs_dist_diff": max(r["max_abs_dist_diff"] for r in v)}
        out["torch_over_query"] = out["torch_us"]["median"] / out["query_us"]["median"]
        print(json.dumps(out), flush=True)


def torch_brute_force(seg_a, seg_u, x, chunk):
    """Distance, segment-normal sign and closest point of x [N, 2] to segments a + t u, chunked
    over the points so that the [chunk, S] intermediates stay bounded."""
    import torch
    c2 = (seg_u * seg_u).sum(-1)
    inv = torch.where(c2 > 0, 1.0 / c2, torch.zeros_like(c2))  # a zero-length segment is its first end
    d_out, s_out, c_out = [], [], []
    for s in range(0, x.shape[0], chunk):
        q = x[s:s + chunk]
        w = q[:, None, :] - seg_a[None]
        t = ((w * seg_u[None]).sum(-1) * inv[None]).clamp(0.0, 1.0)
        cp = seg_a[None] + t[..., None] * seg_u[None]
        r = q[:, None, :] - cp
        d2 = (r * r).sum(-1)
        best = d2.argmin(1)
        rows = torch.arange(q.shape[0], device=q.device)
        rb, ub = r[rows, best], seg_u[best]
        d = d2[rows, best].sqrt()
        sign = torch.where(rb[:, 0] * ub[:, 1] - rb[:, 1] * ub[:, 0] > 0, 1.0, -1.0)
        d_out.append(d)
        s_out.append(sign * d)
        c_out.append(cp[rows, best])
    return torch.cat(d_out), torch.cat(s_out), torch.cat(c_out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "query_timing.jsonl"))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--chunk", type=int, default=65536, help="points per chunk of the torch brute force")
    ap.add_argument("--summarize", metavar="FILE", default=None)
    ap.add_argument("--cases", nargs="*", default=None, help="only these cases (e.g. karman_random16384)")
    ap.add_argument("--no-torch", action="store_true",
                    help="the query legs only, nothing written to --out: for a kernel trace of one case")
    a = ap.parse_args()
    if a.summarize:
        return summarize(a.summarize)
    import numpy as np
    import torch
    from wos_amd import WosScene, load_obj, workloads
    from wos_amd.projection import sample_uniform_2d

    if not torch.cuda.is_available():
        sys.exit("query_timing.py measures on the GPU: none is visible")
    dev = torch.device("cuda", 0)
    scenes = {"karman": load_obj(workloads.KARMAN_OBJ, 2), "engine": load_obj(workloads.ENGINE_OBJ, 2, False, True)}
    cases = []
    for name, (v, ix) in scenes.items():
        sc = WosScene(v, ix, np.zeros((4, 4), np.float32), 350.0, watertight=True)
        size = (float(v[:, 0].min()), float(v[:, 0].max()), float(v[:, 1].min()), float(v[:, 1].max()))
        grid = sample_uniform_2d(1000, size, with_boundary=True, device=dev).reshape(-1, 2).contiguous()
        gen = torch.Generator(device=dev).manual_seed(4)
        u = torch.rand(16384, 2, device=dev, generator=gen)
        rnd = (u * torch.tensor([size[1] - size[0], size[3] - size[2]], device=dev) +
               torch.tensor([size[0], size[2]], device=dev)).contiguous()
        seg_a = torch.from_numpy(v[ix[:, 0]]).to(dev)
        seg_u = torch.from_numpy(v[ix[:, 1]] - v[ix[:, 0]]).to(dev)
        cases += [(f"{name}_grid1000", sc, grid, seg_a, seg_u), (f"{name}_random16384", sc, rnd, seg_a, seg_u)]

    def timed(fn):
        fn()  # warm-up: code objects, the allocator's blocks
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.reps):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / a.reps

    from wos_amd import _lib
    L = _lib.load()

    def enqueue_only(sc, x):
        """wos_scene_query itself: outputs allocated once, one ctypes call per query, WOS_ASYNC."""
        n = int(x.shape[0])
        d, sd = torch.empty(n, device=dev), torch.empty(n, device=dev)
        cp, st = torch.empty(n, 2, device=dev), torch.empty(n, dtype=torch.int32, device=dev)
        s = torch.cuda.current_stream(dev).cuda_stream
        args = (sc._h, 0, 0.0, x.data_ptr(), n, d.data_ptr(), sd.data_ptr(), cp.data_ptr(), st.data_ptr(), s,
                _lib.WOS_PTRS_DEVICE | _lib.WOS_ASYNC)

        def fn():
            if L.wos_scene_query(*args) != 0:
                raise RuntimeError(L.wos_last_error().decode())
        fn.keep = (d, sd, cp, st)
        return fn

    if a.cases:
        cases = [c for c in cases if c[0] in a.cases]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        for rnd_i in range(a.rounds):
            for name, sc, x, seg_a, seg_u in cases:
                q_us = timed(lambda: sc.query(x, closest=True))
                e_us = timed(enqueue_only(sc, x))
                if a.no_torch:
                    print(json.dumps({"case": name, "round": rnd_i, "query_us": q_us, "enqueue_only_us": e_us}), flush=True)
                    continue
                t_us = timed(lambda: torch_brute_force(seg_a, seg_u, x, a.chunk))
                d, _, _, _ = sc.query(x, closest=True)
                bd, _, _ = torch_brute_force(seg_a, seg_u, x, a.chunk)
                row = {"case": name, "round": rnd_i, "points": int(x.shape[0]), "segments": int(seg_a.shape[0]),
                       "reps": a.reps, "query_us": q_us, "enqueue_only_us": e_us, "torch_us": t_us,
                       "max_abs_dist_diff": float((d - bd).abs().max())}
                line = json.dumps(row)
                print(line, flush=True)
                f.write(line + "\n")
                f.flush()


if __name__ == "__main__":
    main()
