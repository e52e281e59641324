"""Scenes, items and float64 references shared by the two pins of the walk step's geometry
queries: test_geometry_oracle_cpu.py (the oracle's exports against float64) and
test_gpu_geometry_probe.py (the device forms against the oracle).  Test infrastructure only."""
import functools
import json
import os

import numpy as np

import kat_cases
import objparse
from wos_amd import workloads

f32, f64 = np.float32, np.float64
EPS = float(np.finfo(f32).eps)  # kFltEps / FEPS
U = 2.0 ** -24                  # unit roundoff of float32
FLT_MAX = float(np.finfo(f32).max)
MARGIN = 1e-3                   # the decision margin of the float64 references


def record(section, key, value):
    """With WOS_GEOMETRY_PROFILE=<file> in the environment the two tests write what they measured
    into that JSON file (profiles/geometry_probe.json was made so); otherwise nothing is written."""
    path = os.environ.get("WOS_GEOMETRY_PROFILE")
    if not path:
        return
    data = {}
    if os.path.exists(path):
        with open(path) as f:
            data = json.load(f)
    data.setdefault(section, {})[key] = value
    with open(path, "w") as f:
        json.dump(data, f, indent=1, sort_keys=True)
        f.write("\n")


# ---- scenes ------------------------------------------------------------------------------------------
def open_box():
    """scenes/cube.obj without its first two triangles: boundary edges next to a missing face."""
    v, ix = objparse.load(workloads.CUBE_OBJ, 3)
    return v, ix[2:]


@functools.lru_cache(maxsize=None)
def scene(name):
    """(vertices, prims, kwargs of WosScene / OracleScene) of a named geometry."""
    kw = {"watertight": True}
    if name == "lshape":
        c = kat_cases.lshape2d(res=4, npts=1, near_corner=0)
        v, ix = c["vertices"], c["prims"]
    elif name == "lshape_origin":
        # the L-shape moved so that its reflex vertex, the one candidate, is (0, 0): the view x - 0 is
        # exact, so float32 points can put d^2 on either neighbour of prec^2
        c = kat_cases.lshape2d(res=4, npts=1, near_corner=0)
        v, ix = c["vertices"] - np.float32(1.0), c["prims"]
    elif name == "box":
        v, ix = workloads.box_2d(1.0)
    elif name == "karman":
        v, ix = objparse.load(workloads.KARMAN_OBJ, 2)
    elif name in ("engine", "engine_flip"):
        c = workloads.engine_config(n_points=1, flip=name == "engine_flip")
        v, ix = c["vertices"], c["prims"]
    elif name == "obstacle":  # config C: the unit box with a 64-segment Dirichlet circle
        c = workloads.dirichlet_obstacle_config(res=48)
        v, ix = c["vertices"], c["prims"]
        kw.update(dvertices=c["dvertices"], dprims=c["dprims"], dirichlet_value=0.0)
    elif name == "circle4096":
        v, ix = workloads.box_2d(1.0)
        dv, dix = workloads.circle_2d((0.5, 0.35), 0.1, 4096)
        kw.update(dvertices=dv, dprims=dix, dirichlet_value=1.0)
    elif name == "cube":
        v, ix = objparse.load(workloads.CUBE_OBJ, 3)
    elif name == "cube_dirichlet":  # the unit cube inside the reference's cube, as a Dirichlet mesh
        v, ix = objparse.load(workloads.CUBE_OBJ, 3)
        kw.update(dvertices=(0.5 * v).astype(f32), dprims=ix[:, ::-1].copy(), dirichlet_value=0.0)
    elif name == "open_box":
        v, ix = open_box()
        kw = {"watertight": False}
    elif name == "lprism":
        c = kat_cases.lprism3d(res=4, npts=1, near_corner=0)
        v, ix = c["vertices"], c["prims"]
    elif name == "cube7":
        v, ix = workloads.subdivided_cube(7)
    elif name == "gear":  # more than 512 reflex vertices: over 64 silhouette groups, a hierarchy over them
        c = workloads.gear_config(n_teeth=480)
        v, ix = c["vertices"], c["prims"]
    elif name == "gear_prism":
        # the 160-tooth gear's outline extruded over z in [0, 0.2] without caps: reflex edges and
        # boundary edges next to a missing face, over 64 groups of triangles and of candidates
        c = workloads.gear_config(n_teeth=160)
        v2, s = c["vertices"], c["prims"]
        n = len(v2)
        v = np.concatenate([np.c_[v2, np.zeros(n)], np.c_[v2, np.full(n, 0.2)]])
        ix = np.concatenate([[(a, b, b + n), (a, b + n, a + n)] for a, b in s])
        kw = {"watertight": False}
    else:
        raise KeyError(name)
    return np.ascontiguousarray(v, f32), np.ascontiguousarray(ix, np.int32), kw


def source(dim):
    return np.zeros((4,) * dim, f32)


def oracle_scene(oracle, name):
    v, ix, kw = scene(name)
    return oracle.OracleScene(v, ix, source(v.shape[1]), 350.0, **kw)


def wos_scene(name):
    from wos_amd import WosScene
    v, ix, kw = scene(name)
    return WosScene(v, ix, source(v.shape[1]), 350.0, **kw)


def bbox(name):
    v, _, kw = scene(name)
    pts = v if "dvertices" not in kw else np.concatenate([v, kw["dvertices"]])
    return pts.min(0).astype(f64), pts.max(0).astype(f64)


def diameter(name):
    lo, hi = bbox(name)
    return float(np.linalg.norm(hi - lo))


# ---- random items --------------------------------------------------------------------------------------
def random_points(name, n, rng, pad=0.15):
    """uniform over the bounding box grown by `pad` of its extent, both sides"""
    lo, hi = bbox(name)
    e = (hi - lo) * pad
    return rng.uniform(lo - e, hi + e, (n, lo.size)).astype(f32)


def random_dirs(dim, n, rng):
    """unit directions from float32 sincos"""
    ph = rng.uniform(0, 2 * np.pi, n).astype(f32)
    if dim == 2:
        return np.stack([np.cos(ph), np.sin(ph)], -1).astype(f32)
    z = rng.uniform(-1, 1, n).astype(f32)
    r = np.sqrt(np.maximum(f32(0), f32(1) - z * z), dtype=f32)
    return np.stack([r * np.cos(ph), r * np.sin(ph), z], -1).astype(f32)


def random_lengths(name, n, rng, min_r=1e-3, flt_max_every=16):
    """log-uniform from minR / 2 to the scene diameter, every flt_max_every-th FLT_MAX"""
    t = np.exp(rng.uniform(np.log(min_r / 2), np.log(diameter(name)), n)).astype(f32)
    t[::flt_max_every] = f32(FLT_MAX)
    return t


# ---- float64 references -----------------------------------------------------------------------------------
def _decided(margins):
    """A primitive is robustly decided when every acceptance margin clears MARGIN (accepted) or
    one of them fails by MARGIN (rejected): (accepted, robust)."""
    m = np.stack(margins, -1)
    acc = (m >= 0).all(-1)
    return acc, np.where(acc, (m >= MARGIN).all(-1), (m <= -MARGIN).any(-1))


def ray64(v, ix, o, d, tmax):
    """The first hit of n rays in float64: found, d, p, unit normal, keep and the derived bound on
    |d32 - d64| of the winning primitive (see test_geometry_oracle_cpu's docstring)."""
    V = v.astype(f64)
    o, d, tmax = o.astype(f64), d.astype(f64), tmax.astype(f64)
    n, dim = o.shape
    pa = V[ix[:, 0]][None]
    if dim == 2:
        vv = (V[ix[:, 1]] - V[ix[:, 0]])[None]
        u = pa - o[:, None]
        d0, d1 = d[:, None, 0], d[:, None, 1]
        s_det = np.abs(d0 * vv[..., 1]) + np.abs(d1 * vv[..., 0])
        det = d0 * vv[..., 1] - d1 * vv[..., 0]
        t = (u[..., 0] * d1 - u[..., 1] * d0) / det
        s_num = np.abs(u[..., 0] * vv[..., 1]) + np.abs(u[..., 1] * vv[..., 0])
        dist = (u[..., 0] * vv[..., 1] - u[..., 1] * vv[..., 0]) / det
        inside = [t, 1 - t]
        pts = pa + t[..., None] * vv
        nrm = np.stack([vv[..., 1], -vv[..., 0]], -1) + 0 * t[..., None]
        chain = 8.0  # 8/3 over the three roundings of a term's chain
    else:
        v1 = (V[ix[:, 1]] - V[ix[:, 0]])[None]
        v2 = (V[ix[:, 2]] - V[ix[:, 0]])[None]
        s = o[:, None] - pa
        dd = d[:, None]
        pp = np.cross(dd, v2)
        det = (v1 * pp).sum(-1)
        s_det = (np.abs(v1) * _abs_cross(dd, v2)).sum(-1)
        vb = (s * pp).sum(-1) / det
        q = np.cross(s, v1)
        wb = (dd * q).sum(-1) / det
        dist = (v2 * q).sum(-1) / det
        s_num = (np.abs(v2) * _abs_cross(s, v1)).sum(-1)
        inside = [vb, wb, 1 - vb - wb]
        pts = pa + v1 * vb[..., None] + v2 * wb[..., None]
        nrm = np.cross(v1, v2) + 0 * vb[..., None]
        chain = 20.0  # 8/3 over the seven roundings of a term's chain
    rel = np.abs(det) / np.maximum(s_det, 1e-300)
    parallel_ok = (np.abs(det) > EPS) & (rel >= MARGIN)
    acc, robust = _decided(inside + [dist, tmax[:, None] - dist])
    acc = acc & (np.abs(det) > EPS)
    key = np.where(acc, dist, np.inf)
    order = np.sort(key, axis=1)
    win = key.argmin(1)
    found = np.isfinite(order[:, 0])
    with np.errstate(invalid="ignore"):  # inf - inf where nothing is hit
        gap_ok = ~found | (order[:, 1] - order[:, 0] >= MARGIN) if key.shape[1] > 1 else np.ones(n, bool)
    keep = (parallel_ok & robust).all(1) & gap_ok
    r = np.arange(n)
    dw, detw = dist[r, win], np.abs(det[r, win])
    bound = chain * U * (s_num[r, win] / detw + np.abs(dw) * (1 + s_det[r, win] / detw))
    nw = nrm[r, win]
    nw = nw / np.linalg.norm(nw, axis=-1, keepdims=True)
    return {"found": found, "d": dw, "p": pts[r, win], "n": nw, "keep": keep, "bound": bound}


def _abs_cross(a, b):
    """the sums of absolute values of the terms of a x b, per component"""
    a, b = np.abs(a), np.abs(b)
    return np.stack([a[..., 1] * b[..., 2] + a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] + a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] + a[..., 1] * b[..., 0]], -1)


def _unit(x):
    return x / np.linalg.norm(x, axis=-1, keepdims=True)


def candidates64(v, ix, double_sided=False):
    """The silhouette candidates of computeSilhouettes in float64, in the oracle's order:
    2D (p, n0, n1, miss), 3D (pa, pb, n0, n1, miss)."""
    V = v.astype(f64)
    dim = V.shape[1]
    out = []
    if dim == 2:
        nxt, prv = {}, {}
        for a, b in ix:
            nxt[int(a)], prv[int(b)] = int(b), int(a)
        seen = set()
        for seg in ix:
            for vi in map(int, seg):
                if vi in seen:
                    continue
                seen.add(vi)
                n0 = n1 = np.zeros(2)
                if vi in nxt:
                    s = V[nxt[vi]] - V[vi]
                    n0 = _unit(np.array([s[1], -s[0]]))
                if vi in prv:
                    s = V[vi] - V[prv[vi]]
                    n1 = _unit(np.array([s[1], -s[0]]))
                both = vi in nxt and vi in prv
                if both and not double_sided and n0[0] * n1[1] - n1[0] * n0[1] < 1e-3:
                    continue
                out.append((V[vi], V[vi], n0, n1, not both))
    else:
        edge, order = {}, []
        for tri in ix:
            for j in range(3):
                i, jn, k = int(tri[j - 1]), int(tri[j]), int(tri[(j + 1) % 3])
                e = (min(jn, k), max(jn, k))
                if e not in edge:
                    edge[e] = [-1, e[0], e[1], -1]
                    order.append(e)
                edge[e][0 if jn < k else 3] = i
        for e in order:
            i0, a, b, i3 = edge[e]
            n0 = n1 = np.zeros(3)
            if i3 != -1:
                n0 = _unit(np.cross(V[b] - V[a], V[i3] - V[a]))
            if i0 != -1:
                n1 = _unit(np.cross(V[a] - V[b], V[i0] - V[b]))
            both = i3 != -1 and i0 != -1
            if both and not double_sided:
                ang = np.arctan2(_unit(V[b] - V[a]) @ np.cross(n0, n1), n0 @ n1)
                if ang < 1e-3:
                    continue
            out.append((V[a], V[b], n0, n1, not both))
    if not out:
        return None
    return tuple(np.array([c[k] for c in out]) for k in range(5))


def star64(v, ix, x, max_r, flip, min_r=1e-3, prec=1e-3, double_sided=False):
    """computeStarRadius in float64 and whether every candidate's decisions clear MARGIN relative
    to their thresholds: (radius, keep)."""
    x, max_r = x.astype(f64), max_r.astype(f64)
    n = x.shape[0]
    base = np.maximum(max_r, min_r)
    cand = candidates64(v, ix, double_sided)
    trivial = (min_r > max_r) | (min_r * min_r >= np.where(max_r < FLT_MAX, max_r, 1e30) ** 2)
    if cand is None:
        return np.where(min_r > max_r, max_r, base), np.ones(n, bool)
    pa, pb, n0, n1, miss = cand
    e = pb - pa
    ee = (e * e).sum(-1)
    t = np.where(ee > 0, ((x[:, None] - pa[None]) * e[None]).sum(-1) / np.where(ee > 0, ee, 1.0), 0.0)
    view = x[:, None] - (pa[None] + np.clip(t, 0, 1)[..., None] * e[None])
    d = np.linalg.norm(view, axis=-1)
    u = view / np.maximum(d, 1e-300)[..., None]
    dot0, dot1 = (u * n0[None]).sum(-1), (u * n1[None]).sum(-1)
    sign = np.where(np.asarray(flip)[:, None] != 0, -1.0, 1.0)  # the query passes !flipNormalOrientation
    sil = np.where(np.abs(dot0) <= prec, sign * dot1 > prec, np.where(np.abs(dot1) <= prec, sign * dot0 > prec,
                                                                     dot0 * dot1 < 0))
    sil = sil | miss[None]
    # the thresholds every decision compares with: each must be cleared by a relative MARGIN
    far = lambda a, b: np.abs(a - b) >= MARGIN * np.maximum(np.abs(b), 1e-30)
    robust = (far(np.abs(dot0), prec) & far(np.abs(dot1), prec) & (np.abs(dot0 * dot1) >= MARGIN * prec * prec) |
              miss[None])
    robust = robust & far(d, prec) & (d > prec) & far(d, max_r[:, None]) & far(d, min_r)
    ok = sil & (d <= max_r[:, None])
    key = np.where(ok, d, np.inf)
    # the first candidate within minR ends the scan, else the closest
    within = ok & (d <= min_r)
    first = np.where(within.any(1), within.argmax(1), key.argmin(1))
    r = np.arange(n)
    found = np.isfinite(key[r, first])
    order = np.sort(key, axis=1)
    with np.errstate(invalid="ignore"):
        gap_ok = ~found | within.any(1) | (key.shape[1] < 2) | \
            (order[:, min(1, key.shape[1] - 1)] - order[:, 0] >= MARGIN * order[:, 0])
    rad = np.where(found, np.maximum(key[r, first], min_r), base)
    rad = np.where(min_r > max_r, max_r, np.where(trivial, base, rad))
    return rad, trivial | (robust.all(1) & gap_ok)


def seg_dist64(v, ix, q):
    a, b = v[ix[:, 0]].astype(f64), v[ix[:, 1]].astype(f64)
    s = b - a
    t = np.clip(((q[:, None] - a[None]) * s[None]).sum(-1) / (s * s).sum(-1)[None], 0, 1)
    return np.linalg.norm(q[:, None] - (a[None] + t[..., None] * s[None]), axis=-1).min(1)


def tri_dist64(v, ix, q):
    """float64 distance to the nearest triangle: the plane distance where the projection falls
    inside, else the nearest edge."""
    out = np.full(q.shape[0], np.inf)
    V = v.astype(f64)
    for t in ix:
        a, b, c = V[t[0]], V[t[1]], V[t[2]]
        n = _unit(np.cross(b - a, c - a))
        h = (q - a) @ n
        p = q - h[:, None] * n
        inside = np.ones(q.shape[0], bool)
        edge = np.full(q.shape[0], np.inf)
        for e0, e1 in ((a, b), (b, c), (c, a)):
            inside &= np.cross(e1 - e0, p - e0) @ n >= 0
            s = e1 - e0
            tt = np.clip(((q - e0) @ s) / (s @ s), 0, 1)
            edge = np.minimum(edge, np.linalg.norm(q - (e0 + tt[:, None] * s), axis=1))
        out = np.minimum(out, np.where(inside, np.abs(h), edge))
    return out


def dirichlet64(name, x):
    """computeDistToDirichlet in float64: the Dirichlet mesh, or the far-corner form without one"""
    v, ix, kw = scene(name)
    x = x.astype(f64)
    if "dvertices" in kw:
        return (seg_dist64 if v.shape[1] == 2 else tri_dist64)(kw["dvertices"], kw["dprims"], x)
    lo, hi = v.min(0).astype(f64) - EPS, v.max(0).astype(f64) + EPS
    return np.linalg.norm(np.minimum(lo - x, x - hi), axis=-1)


# ---- adversarial items (float32, built on the host) ---------------------------------------------------------
def _na(x, k=1, up=True):
    """x moved k float32 steps up or down"""
    x = np.asarray(x, f32).copy()
    for _ in range(k):
        x = np.nextafter(x, f32(np.inf if up else -np.inf))
    return x


def _pick(n, k):
    """up to k indices spread over range(n)"""
    return np.unique(np.linspace(0, n - 1, min(n, k)).astype(int))


def host_bbox(name):
    """pmin, pmax as prepare_scene forms them (float32, FLT_EPSILON pad) and the culling pad"""
    v, _, kw = scene(name)
    pts = v if "dvertices" not in kw else np.concatenate([v, kw["dvertices"]])
    pmin, pmax = (pts.min(0) - f32(EPS)).astype(f32), (pts.max(0) + f32(EPS)).astype(f32)
    span = f32((pmax - pmin).max())
    return pmin, pmax, f32(f32(1e-4) * span + f32(1e-6))


def group_boxes(pts_per_item, pad):
    """the padded boxes of groups of 8 consecutive items (each item: [k, dim] points): lo, hi float32"""
    lo, hi = [], []
    for g0 in range(0, len(pts_per_item), 8):
        q = np.concatenate(pts_per_item[g0:g0 + 8]).astype(f32)
        lo.append(q.min(0) - pad)
        hi.append(q.max(0) + pad)
    return np.array(lo, f32), np.array(hi, f32)


def grid_lines(name, targets, n_dprims=None):
    """Coordinates on the cell boundaries and outer faces of the star grid (every resolution
    build_star_grid may settle on) or of the Dirichlet grid, with their float32 neighbours:
    a list of (axis, coordinate)."""
    pmin, pmax, _ = host_bbox(name)
    dim = pmin.size
    span = float((pmax - pmin).max())
    gpad = 1e-3 * span + 1e-6
    glo = pmin.astype(f64) - gpad
    gext = (pmax.astype(f64) + gpad) - glo
    out = []
    for target in targets:
        h = (np.prod(gext) / target) ** (1.0 / dim)
        for k in range(dim):
            n = max(1, int(np.ceil(gext[k] / h)))
            gmin, inv = f32(glo[k]), f32(n / gext[k])
            for i in sorted({0, 1, n // 2, n - 1, n}):
                c = f32(f64(gmin) + i / f64(inv))
                out += [(k, c), (k, _na(c)), (k, _na(c, 2)), (k, _na(c, 1, False)), (k, _na(c, 2, False))]
    return out


def _rot(u):
    return np.stack([-u[..., 1], u[..., 0]], -1)


@np.errstate(invalid="ignore", divide="ignore")
def ray_items(name, rng, n_random=768, limit=3100):
    """[n, 2 dim + 1] float32 rays: random ones, then the adversarial families of the probe's test
    (the tmax bands of known hits are added by the caller, from the oracle's own d)."""
    v, ix, _ = scene(name)
    dim = v.shape[1]
    diam = f32(diameter(name))
    V = v.astype(f64)
    o = [random_points(name, n_random, rng)]
    d = [random_dirs(dim, n_random, rng)]
    t = [random_lengths(name, n_random, rng)]

    def add(oo, dd, tt=None):
        oo, dd = np.atleast_2d(np.asarray(oo, f32)), np.atleast_2d(np.asarray(dd, f32))
        m = max(len(oo), len(dd))
        o.append(np.broadcast_to(oo, (m, dim)))
        d.append(np.broadcast_to(dd, (m, dim)))
        t.append(np.full(m, FLT_MAX if tt is None else tt, f32))

    # aimed at vertices, and at the float32 neighbours of the origin and of the aim
    for vi in _pick(len(v), 48):
        src = random_points(name, 2, rng)
        for s in src:
            aim = (V[vi] - s.astype(f64))
            u = (aim / np.linalg.norm(aim)).astype(f32)
            add(s, u)
            add(s, u, diam)
            for k in range(dim):
                for up in (True, False):
                    s2 = s.copy(); s2[k] = _na(s[k], 1, up)
                    add(s2, u)
                    u2 = u.copy(); u2[k] = _na(u[k], 1, up)
                    add(s, u2)
        # exactly through the vertex along an axis (t = 0 / t = 1, shared vertices and edges)
        for k in range(dim):
            for sgn in (-1.0, 1.0):
                s = v[vi].copy(); s[k] = f32(s[k] - sgn * f32(0.25) * diam)
                e = np.zeros(dim, f32); e[k] = sgn
                add(s, e)
    # origins on a primitive's line or plane (ud, uv, vn, wn, dn exactly 0 or a few ulps off)
    for p in _pick(len(ix), 48):
        a = V[ix[p, 0]]
        e1 = V[ix[p, 1]] - a
        e2 = V[ix[p, 2]] - a if dim == 3 else 0 * e1
        for s1, s2 in ((-0.5, 0.0), (0.25, 0.25), (1.5, 0.0), (0.5, 0.0), (0.0, 0.0), (1.0, 0.0)):
            s = (a + s1 * e1 + s2 * e2).astype(f32)
            dirs = random_dirs(dim, 2, rng)
            inplane = (e1 / np.linalg.norm(e1)).astype(f32)
            for u in (dirs[0], dirs[1], inplane, -inplane):
                add(s, u)
                for k in range(dim):
                    s2_ = s.copy(); s2_[k] = _na(s[k], 1, bool(k & 1))
                    add(s2_, u)
    # nearly parallel: |dv|, |det| at {0.5, 0.99, 1, 1.01, 2} kFltEps
    for p in _pick(len(ix), 32):
        a = V[ix[p, 0]]
        e1 = V[ix[p, 1]] - a
        if dim == 2:
            nrm, scale = _rot(e1) / np.linalg.norm(e1), np.linalg.norm(e1)
            tang = e1 / np.linalg.norm(e1)
        else:
            e2 = V[ix[p, 2]] - a
            c = np.cross(e1, e2)
            nrm, scale = c / np.linalg.norm(c), np.linalg.norm(c)
            tang = (0.3 * e1 + 0.4 * e2) / np.linalg.norm(0.3 * e1 + 0.4 * e2)
        s = (a + 0.5 * e1 + (0.2 * (V[ix[p, 2]] - a) if dim == 3 else 0) + 0.05 * float(diam) * nrm - 0.3 * float(diam) * tang)
        for kk in (0.5, 0.99, 1.0, 1.01, 2.0, 8.0, 64.0):
            for sgn in (-1.0, 1.0):
                u = tang + sgn * kk * EPS / scale * nrm
                add(s.astype(f32), (u / np.linalg.norm(u)).astype(f32))
    # axis-parallel directions with exact +0.0 and -0.0 components (rcp = +-inf, 0 inf slabs)
    pts = np.concatenate([random_points(name, 12, rng), v[_pick(len(v), 12)]])
    for s in pts:
        for k in range(dim):
            for sgn in (-1.0, 1.0):
                for z in (0.0, -0.0):
                    e = np.full(dim, z, f32); e[k] = sgn
                    add(s, e)
                    add(s, e, f32(0.3) * diam)
    # origins exactly on a padded group-box face
    _, _, pad = host_bbox(name)
    lo, hi = group_boxes([v[ix[p]] for p in range(len(ix))], pad)
    for g in _pick(len(lo), 24):
        for k in range(dim):
            for face in (lo[g, k], hi[g, k]):
                s = rng.uniform(lo[g], hi[g]).astype(f32); s[k] = face
                for u in random_dirs(dim, 2, rng):
                    add(s, u)
                e = np.zeros(dim, f32); e[(k + 1) % dim] = 1.0
                add(s, e)
                e = np.zeros(dim, f32); e[k] = 1.0
                add(s, e)
    # a known primitive's midpoint from close by, every (group, slot) position: the solo winner's lane
    if len(ix) >= 64:
        for l in range(64):
            p = (l * 9) % len(ix)
            a = V[ix[p]].mean(0)
            e1 = V[ix[p, 1]] - V[ix[p, 0]]
            nrm = _rot(e1) if dim == 2 else np.cross(e1, V[ix[p, 2]] - V[ix[p, 0]])
            nrm = nrm / np.linalg.norm(nrm)
            for sgn in (-1.0, 1.0):
                add((a + sgn * 0.02 * float(diam) * nrm).astype(f32), (-sgn * nrm).astype(f32))
    return _finite_capped(np.concatenate([np.concatenate(o), np.concatenate(d), np.concatenate(t)[:, None]], 1), limit)


def _finite_capped(items, limit):
    """the finite rows (a degenerate primitive of the mesh gives none), thinned evenly to `limit`"""
    items = items.astype(f32)
    items = items[np.isfinite(items).all(1)]
    return items[_pick(len(items), limit)]


def tmax_bands(rays, found, d, limit=192):
    """rays with a known hit at the oracle's own d: tmax at d, one ulp either side, d / 1.00001, d 1.00001"""
    dim = (rays.shape[1] - 1) // 2
    hit = np.flatnonzero((found != 0) & (d > 0))
    hit = hit[_pick(len(hit), limit)] if len(hit) else hit
    out = []
    for tt in (d[hit], _na(d[hit]), _na(d[hit], 1, False), (d[hit] / f32(1.00001)).astype(f32),
               (d[hit] * f32(1.00001)).astype(f32)):
        r = rays[hit].copy()
        r[:, 2 * dim] = tt
        out.append(r)
    return np.concatenate(out) if len(hit) else rays[:0]


def _f32_dist(x, c):
    """|x - c| as the kernels form it in float32 (2D candidates)"""
    w = (x - c).astype(f32)
    acc = w[..., 0] * w[..., 0]
    for k in range(1, w.shape[-1]):
        acc = acc + w[..., k] * w[..., k]
    return np.sqrt(acc, dtype=f32)


@np.errstate(invalid="ignore", divide="ignore")
def star_items(name, rng, n_random=768, min_r=1e-3, prec=1e-3, limit=4096):
    """[n, dim + 2] float32 star queries (x, maxR, flip): random ones, then the adversarial families."""
    v, ix, kw = scene(name)
    dim = v.shape[1]
    diam = float(diameter(name))
    x = [random_points(name, n_random, rng)]
    r = [random_lengths(name, n_random, rng, min_r)]
    noflip = []  # rows built for flipNormalOrientation = 0

    def add(xx, rr):
        xx = np.atleast_2d(np.asarray(xx, f32))
        x.append(xx)
        r.append(np.broadcast_to(np.asarray(rr, f32), (len(xx),)).copy())

    cand = candidates64(v, ix, kw.get("double_sided", False))
    if cand is not None:
        pa, pb, n0, n1, miss = cand
        for s in _pick(len(pa), 40):
            mid = 0.5 * (pa[s] + pb[s])
            if dim == 2:
                frame = lambda n: (n, _rot(n))
                around = lambda: (lambda a: np.array([np.cos(a), np.sin(a)]))(rng.uniform(0, 2 * np.pi))
            else:
                e = (pb[s] - pa[s]) / np.linalg.norm(pb[s] - pa[s])
                frame = lambda n: (n, np.cross(e, n))
                b1 = np.cross(e, [0.3, 0.5, 0.8]); b1 /= np.linalg.norm(b1)
                around = lambda: (lambda a: np.cos(a) * b1 + np.sin(a) * np.cross(e, b1))(rng.uniform(0, 2 * np.pi))
            # at distance prec (1 +- delta) from the candidate
            for dl in (0.0, 1e-7, 1e-5, 9e-5, 1.1e-4):
                for sgn in (-1.0, 1.0):
                    add((mid + prec * (1 + sgn * dl) * around()).astype(f32), [diam, FLT_MAX][int(sgn > 0)])
            # at d = minR, and maxR = d +- one ulp
            for rad in (min_r, 0.03 * diam, 0.2 * diam):
                xs = (mid + rad * around()).astype(f32)
                dd = _f32_dist(xs, mid.astype(f32))
                for mr in (dd, _na(dd), _na(dd, 1, False), f32(rad)):
                    add(xs, mr)
            # dot0 or dot1 at +-prec +- delta
            for nn in (n0[s], n1[s]):
                if not nn.any():
                    continue
                a_ax, b_ax = frame(nn)
                for dl in (0.0, 1e-7, 9e-6, 1.1e-5, 1e-4):
                    for sd in (-1.0, 1.0):
                        for sp in (-1.0, 1.0):
                            for sb in (-1.0, 1.0):
                                a = sp * (prec + sd * dl)
                                u = a * a_ax + sb * np.sqrt(1 - a * a) * b_ax
                                add((mid + 0.05 * diam * u).astype(f32), FLT_MAX if sb > 0 else diam)
        # a candidate at the origin (2D): d^2 on prec^2 and its float32 neighbours from every side, where
        # the exact test's d > prec and silhouette_class2's band on d^2 must agree
        p2 = f32(prec) * f32(prec)
        band = {float(p2), float(_na(p2)), float(_na(p2, 2)), float(_na(p2, 1, False))}
        for s in range(len(pa)):
            if dim != 2 or pa[s].any():
                continue
            for th in np.linspace(0, 2 * np.pi, 64, endpoint=False) + 0.013:
                x0, x1 = f32(prec * np.cos(th)), f32(prec * np.sin(th))
                k = 0 if abs(x0) >= abs(x1) else 1
                steps = (np.array([x0, x1], f32)[k].view(np.int32) + np.arange(-300, 301)).astype(np.int32).view(f32)
                other = f32(x1 if k == 0 else x0)
                d2 = (steps * steps + other * other).astype(f32)
                for q in np.flatnonzero(np.isin(d2.astype(f64), list(band)))[:6]:
                    xs = np.array([steps[q], other] if k == 0 else [other, steps[q]], f32)
                    noflip.append(sum(len(a) for a in x))
                    add(xs, diam)
        # 3D: on the line of an edge beyond its ends, where the bounding-sphere bound dm - hr of
        # star_candidate's early-out is attained, maxR a few 1e-6 above the distance
        for s in (_pick(len(pa), 64) if dim == 3 else []):
            e = pb[s] - pa[s]
            ln = np.linalg.norm(e)
            for end, sg in ((pb[s], 1.0), (pa[s], -1.0)):
                for far in (1e-3, 1e-2, 0.1, 1.0):
                    xs = (end + sg * far * e).astype(f32)
                    dd = np.linalg.norm(xs.astype(f64) - end)
                    for up in (1e-6, 1e-5, 3e-5, 1e-4):
                        add(xs, f32(dd * (1 + up)))
        # on a group's bounding sphere +- 1.01 prec; maxR at the padded-box distance (1 +- 1e-5)
        _, _, pad = host_bbox(name)
        items = [np.stack([pa[s], pb[s]]) if dim == 3 else pa[s][None] for s in range(len(pa))]
        lo, hi = group_boxes(items, pad)
        for g in _pick(len(lo), 24):
            c = 0.5 * (lo[g].astype(f64) + hi[g].astype(f64))
            q = np.concatenate(items[8 * g:8 * g + 8]).astype(f32).astype(f64)
            rho = np.linalg.norm(q - c, axis=1).max() + float(pad)
            for sgn in (-1.0, 0.0, 1.0):
                for _ in range(3):
                    u = random_dirs(dim, 1, rng)[0].astype(f64)
                    add((c + (rho + sgn * 1.01 * prec) * u).astype(f32), [diam, FLT_MAX, 0.5 * diam][int(sgn) + 1])
            for _ in range(3):
                xs = (c + (rho + rng.uniform(0.02, 0.3) * diam) * random_dirs(dim, 1, rng)[0]).astype(f32)
                e = np.maximum(np.maximum(lo[g] - xs, xs - hi[g]), f32(0))
                bd = np.sqrt((e.astype(f64) ** 2).sum())
                for fac in (1 - 1e-5, 1.0, 1 + 1e-5, 1 - 5e-6, 1 + 5e-6):
                    add(xs, f32(bd * fac))
    # on the star grid's cell boundaries and outer faces
    for k, c in grid_lines(name, [4096 >> j for j in range(7)]):
        xs = random_points(name, 1, rng)[0]
        xs[k] = c
        add(xs, diam)
    xs = np.concatenate(x)
    flip = (rng.random(len(xs)) < 0.25).astype(f32)
    flip[noflip] = 0.0
    return _finite_capped(np.concatenate([xs, np.concatenate(r)[:, None], flip[:, None]], 1), limit)


def dirichlet_items(name, rng, n_random=768):
    """[n, dim] float32 points: random ones, the Dirichlet mesh's vertices and midpoints (exact ties
    between the primitives of a vertex), the Dirichlet grid's cell boundaries and outer faces."""
    v, ix, kw = scene(name)
    dv, dix = kw["dvertices"].astype(f32), kw["dprims"]
    x = [random_points(name, n_random, rng), dv[_pick(len(dv), 256)]]
    x.append(dv[dix[_pick(len(dix), 256)]].astype(f64).mean(1).astype(f32))
    near = dv[rng.integers(0, len(dv), 256)] + rng.normal(size=(256, dv.shape[1])).astype(f32) * f32(0.02 * diameter(name))
    x.append(near.astype(f32))
    if dv.shape[1] == 2:
        nd = len(dix)
        target = 16384 if nd <= 512 else (4096 if nd <= 4096 else 1024)
        for k, c in grid_lines(name, [target]):
            for _ in range(4):
                xs = random_points(name, 1, rng)[0]
                xs[k] = c
                x.append(xs[None])
    return np.concatenate(x).astype(f32)
