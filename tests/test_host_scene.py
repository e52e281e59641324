"""CPU checks of the culling records the kernels rely on for exactness
(csrc/wos_host_scene.cpp, built here with plain g++ through tests/native/host_scene_shim.cpp):

* every primitive / silhouette candidate lies inside its group's padded box;
* every adjacent normal of a group lies inside the group's normal cone, every
  candidate inside its bounding sphere;
* soundness of the cone test (wos_kernel.hip cone_culled): for random query points,
  a group the test culls never holds a candidate the exact silhouette test
  (isWideSilhouetteVertex, wide_query_operations.h:328-358) accepts.

The cone test checked here is a numpy float64 restatement; the device function itself, with its
rsq and approximate sqrt, is checked beside the exact test by tests/test_gpu_geometry_probe.py.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import objparse
from wos_amd import workloads

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "neural-monte-carlo-fluid-simulation_amd", "csrc")
KGROUP = 8


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("hs") / "libhs.so")
    subprocess.run(["g++", "-std=c++17", "-O1", "-fPIC", "-shared", "-ffp-contract=off", "-I", CSRC,
                    os.path.join(HERE, "native", "host_scene_shim.cpp"), os.path.join(CSRC, "wos_host_scene.cpp"),
                    os.path.join(CSRC, "wos_fcpw_bvh.cpp"),
                    "-o", out], check=True)
    return C.CDLL(out)


def prepare(shim, v, ix, dim, double_sided=False):
    v = np.ascontiguousarray(v, np.float32)
    ix = np.ascontiguousarray(ix, np.int32)
    cap = 64 * (ix.shape[0] + 16) * 4
    bufs = [np.zeros(cap, np.float32) for _ in range(4)]
    counts = np.zeros(4, np.int32)
    f = C.POINTER(C.c_float)
    rc = shim.hs_prepare(dim, v.ctypes.data_as(f), v.shape[0], ix.ctypes.data_as(C.POINTER(C.c_int)), ix.shape[0],
                         int(double_sided), *[x for b in bufs for x in (b.ctypes.data_as(f), cap)],
                         counts.ctypes.data_as(C.POINTER(C.c_int)))
    assert rc == 0, rc
    npr, nsil, npg, nsg = counts.tolist()
    ps, ss = (4, 8) if dim == 2 else (9, 16)
    return dict(prim=bufs[0][:npr * ps].reshape(npr, ps), sil=bufs[1][:nsil * ss].reshape(nsil, ss),
                pg=bufs[2][:npg * 8].reshape(npg, 8), sg=bufs[3][:nsg * 16].reshape(nsg, 16))


def scenes():
    out = []
    cfg = workloads.karman_config(n_walks=8)
    out.append(("karman", 2) + objparse.load(cfg["obj"], 2))
    g = workloads.gear_config()
    out.append(("gear", 2, g["vertices"], g["prims"]))
    c = workloads.cube_config(res=2, n_walks=8)
    v, ix = objparse.load(c["obj"], 3)
    out.append(("cube", 3, v, ix))
    out.append(("open_box", 3, v, ix[2:]))  # two faces' triangles removed: open edges -> silhouettes
    return out


@pytest.mark.parametrize("name,dim,v,ix", scenes(), ids=[s[0] for s in scenes()])
def test_group_boxes_contain_members(shim, name, dim, v, ix):
    r = prepare(shim, v, ix, dim)
    prim, sil, pg, sg = r["prim"], r["sil"], r["pg"], r["sg"]
    assert pg.shape[0] == (prim.shape[0] + KGROUP - 1) // KGROUP
    for p in range(prim.shape[0]):
        B = pg[p // KGROUP]
        if dim == 2:
            pts = [prim[p, 0:2], prim[p, 0:2] + prim[p, 2:4]]  # record holds [pa, pb - pa]
        else:
            pts = [prim[p, 0:3], prim[p, 3:6], prim[p, 6:9]]
        for q in pts:
            assert np.all(q >= B[0:dim]) and np.all(q <= B[4:4 + dim]), (name, p)
    for s in range(sil.shape[0]):
        B = sg[s // KGROUP]
        pts = [sil[s, 0:2]] if dim == 2 else [sil[s, 0:3], sil[s, 3:6]]
        for q in pts:
            assert np.all(q >= B[0:dim]) and np.all(q <= B[4:4 + dim])
            assert np.linalg.norm(q.astype(np.float64) - B[8:8 + dim]) <= B[11]


@pytest.mark.parametrize("name,dim,v,ix", scenes(), ids=[s[0] for s in scenes()])
def test_normal_cones_contain_normals(shim, name, dim, v, ix):
    r = prepare(shim, v, ix, dim)
    sil, sg = r["sil"], r["sg"]
    o0, o1, om = (2, 4, 6) if dim == 2 else (6, 9, 12)
    for gi in range(sg.shape[0]):
        B = sg[gi]
        members = sil[gi * KGROUP:(gi + 1) * KGROUP]
        if np.any(members[:, om] != 0):
            assert B[15] != 0  # a candidate next to a missing primitive disables culling
        if B[15] != 0:
            continue
        alpha = np.arctan2(B[3], B[7])
        for S in members:
            for o in (o0, o1):
                n = S[o:o + dim].astype(np.float64)
                ang = np.arccos(np.clip(n @ B[12:12 + dim] / np.linalg.norm(n), -1, 1))
                assert ang <= alpha + 1e-6


def cone_culled(B, x, prec, dim):
    """numpy float64 restatement of wos_kernel.hip cone_culled"""
    if B[15] != 0:
        return False
    rho = B[11]
    w = x - B[8:8 + dim]
    D2 = w @ w
    lim = rho + 1.01 * prec + 1e-6
    if not D2 > lim * lim:
        return False
    invD = 1 / np.sqrt(D2)
    sinb = rho * invD
    cosb = np.sqrt(max(0.0, 1 - sinb * sinb))
    sina, cosa = B[3], B[7]
    cosg, sing = cosa * cosb - sina * sinb, sina * cosb + cosa * sinb
    cost = np.clip((w @ B[12:12 + dim]) * invD, -1, 1)
    sint = np.sqrt(max(0.0, 1 - cost * cost))
    thr = prec + 1e-3
    if sint * cosg + cost * sing > 1e-3 and cost * cosg - sint * sing > thr:
        return True
    return sint * cosg - cost * sing > 1e-3 and cost * cosg + sint * sing < -thr


def silhouette_2d(S, x, prec, flip=True):
    """isWideSilhouetteVertex (float64 evaluation of the kernel's is_silhouette<2>)"""
    sign = 1.0 if flip else -1.0
    view = x - S[0:2]
    d = np.linalg.norm(view)
    n0, n1 = S[2:4].astype(np.float64), S[4:6].astype(np.float64)
    if not d > prec:
        return sign * (n0[0] * n1[1] - n0[1] * n1[0]) > prec
    u = view / d
    d0, d1 = u @ n0, u @ n1
    if abs(d0) <= prec:
        return sign * d1 > prec
    if abs(d1) <= prec:
        return sign * d0 > prec
    return d0 * d1 < 0


def _grid_check(shim, v, ix, dim, pts, double_sided=False, prec=1e-3, min_r=1e-3, budget=16384):
    v = np.ascontiguousarray(v, np.float32)
    ix = np.ascontiguousarray(ix, np.int32)
    pts = np.ascontiguousarray(pts, np.float32)
    info = np.zeros(10, np.int32)
    f = C.POINTER(C.c_float)
    shim.hs_star_grid_check.restype = C.c_int
    bad = shim.hs_star_grid_check(dim, v.ctypes.data_as(f), v.shape[0], ix.ctypes.data_as(C.POINTER(C.c_int)),
                                  ix.shape[0], int(double_sided), C.c_float(prec), C.c_float(min_r),
                                  pts.ctypes.data_as(f), pts.shape[0], budget, info.ctypes.data_as(C.POINTER(C.c_int)))
    return bad, dict(zip(["ok", "ncell", "list_len", "bytes", "n0", "n1", "n2", "checked", "max_list"], info[:9]))


def _grid_points(v, dim, sil_pts, n=6000, seed=5):
    """uniform points over the bbox (+5 % band), points within 1e-4..3e-2 of every
    silhouette candidate, and points on a fine lattice (cell boundaries)"""
    rng = np.random.default_rng(seed)
    lo, hi = v.min(0), v.max(0)
    span = (hi - lo).max()
    out = [rng.uniform(lo - 0.05 * span, hi + 0.05 * span, (n, dim))]
    for q in sil_pts:
        r = np.exp(rng.uniform(np.log(1e-4), np.log(3e-2), (40, 1)))
        d = rng.normal(size=(40, dim))
        out.append(q + r * d / np.linalg.norm(d, axis=1, keepdims=True))
    g = np.linspace(0.0, 1.0, 41 if dim == 2 else 13)
    mesh = np.stack(np.meshgrid(*([g] * dim), indexing="ij"), -1).reshape(-1, dim)
    out.append(lo + mesh * (hi - lo))
    return np.concatenate(out).astype(np.float32)


@pytest.mark.parametrize("name,dim,v,ix", scenes(), ids=[s[0] for s in scenes()])
@pytest.mark.parametrize("double_sided", [False, True])
def test_star_grid_lists_decide_the_full_scan(shim, name, dim, v, ix, double_sided):
    """The star-radius grid (wos_host_scene.cpp build_star_grid) must give, for every
    point of its cells, the same computeStarRadius as the full sequential scan over
    all silhouette candidates -- bit for bit, both normal orientations."""
    r = prepare(shim, v, ix, dim, double_sided)
    sil_pts = r["sil"][:, 0:dim] if dim == 2 else 0.5 * (r["sil"][:, 0:3] + r["sil"][:, 3:6])
    pts = _grid_points(np.asarray(v, np.float64), dim, sil_pts)
    bad, info = _grid_check(shim, v, ix, dim, pts, double_sided)
    if r["sil"].shape[0] == 0 or r["sil"].shape[0] > 255:  # no grid: the kernel scans groups
        assert not info["ok"]
        return
    assert info["ok"], info
    assert info["bytes"] <= 16384
    assert info["checked"] > 0.8 * pts.shape[0], info
    assert bad == 0, (bad, info)


@pytest.mark.parametrize("prec,min_r", [(1e-3, 1e-3), (1e-2, 0.05), (1e-4, 1e-4)])
def test_star_grid_other_settings(shim, prec, min_r):
    s = [t for t in scenes() if t[0] == "karman"][0]
    r = prepare(shim, s[2], s[3], 2)
    pts = _grid_points(np.asarray(s[2], np.float64), 2, r["sil"][:, 0:2], n=4000, seed=11)
    bad, info = _grid_check(shim, s[2], s[3], 2, pts, prec=prec, min_r=min_r)
    assert info["ok"] and bad == 0, (bad, info)
    # the lists are short: far fewer candidates than the 44 of a full scan
    assert info["list_len"] / info["ncell"] < 12, info


@pytest.mark.parametrize("name", ["karman", "gear"])
def test_cone_culling_is_sound(shim, name):
    s = [t for t in scenes() if t[0] == name][0]
    r = prepare(shim, s[2], s[3], 2)
    sil, sg = r["sil"], r["sg"]
    lo, hi = s[2].min(0) - 0.2, s[2].max(0) + 0.2
    rng = np.random.default_rng(3)
    culled = 0
    for x in rng.uniform(lo, hi, (3000, 2)):
        for gi in range(sg.shape[0]):
            if not cone_culled(sg[gi].astype(np.float64), x, 1e-3, 2):
                continue
            culled += 1
            for S in sil[gi * KGROUP:(gi + 1) * KGROUP]:
                for flip in (True, False):
                    assert not (S[6] != 0 or silhouette_2d(S, x, 1e-3, flip)), (name, gi, x)
    assert culled > 1000  # the test culls a real share of the groups


# ---- group hierarchy (wos_scene.h DevTree) -----------------------------------------
KTREE_LEVELS, KTREE_MIN = 8, 64


def _tree(shim, groups, stride):
    groups = np.ascontiguousarray(groups, np.float32)
    n = groups.shape[0]
    cap = 8 * (n + 64)
    nodes = np.zeros(cap, np.float32)
    meta = np.zeros(1 + 2 * (KTREE_LEVELS + 1), np.int32)
    f = C.POINTER(C.c_float)
    rc = shim.hs_group_tree(groups.ctypes.data_as(f), stride, n, nodes.ctypes.data_as(f), cap,
                            meta.ctypes.data_as(C.POINTER(C.c_int)))
    assert rc >= 0
    levels = int(meta[0])
    cnt = meta[1:2 + KTREE_LEVELS].tolist()
    off = meta[2 + KTREE_LEVELS:].tolist()
    return levels, cnt, off, nodes[:rc].reshape(-1, 8)


def _tree_next(levels, cnt, L, i, limit, node_ok, leaf_ok):
    """Python restatement of wos_device.h tree_next (the kernel's stackless cursor)."""
    while L >= 0:
        if (i << (3 * L)) >= limit:
            return -1, L, i
        ok = leaf_ok(i) if L == 0 else node_ok(L, i)
        if ok and L > 0:
            L, i = L - 1, i << 3
            continue
        found = i if ok else -1
        i += 1
        while L < levels and ((i & 7) == 0 or i >= cnt[L]):
            i, L = ((i - 1) >> 3) + 1, L + 1
        if L == levels and i >= cnt[L]:
            L = -1
        if found >= 0:
            return found, L, i
    return -1, L, i


@pytest.mark.parametrize("ngroups", [10, 64, 65, 200, 513, 4099])
def test_group_tree_contains_and_traverses(shim, ngroups):
    """node boxes contain their children; the cursor, walked window by window like
    ray_hit_wave / star_radius_wave, emits exactly the flat scan's accepted groups in
    increasing order (box-overlap tests: a group's ancestors contain its box)"""
    rng = np.random.default_rng(ngroups)
    c = np.cumsum(rng.normal(0, 1, (ngroups, 2)), 0)        # spatially coherent, like a boundary polyline
    half = rng.uniform(0.1, 1.0, (ngroups, 2))
    groups = np.zeros((ngroups, 16), np.float32)             # silhouette-group stride (box in the first 8)
    groups[:, 0:2], groups[:, 4:6] = c - half, c + half
    levels, cnt, off, nodes = _tree(shim, groups, 16)
    assert cnt[0] == ngroups
    if ngroups <= KTREE_MIN:
        assert levels == 0
        return
    assert levels >= 1 and cnt[levels] <= 8

    def box(L, i):
        return groups[i, :8] if L == 0 else nodes[off[L] + i]

    for L in range(1, levels + 1):
        assert cnt[L] == (cnt[L - 1] + 7) // 8
        for i in range(cnt[L]):
            B = box(L, i)
            for ch in range(8 * i, min(8 * i + 8, cnt[L - 1])):
                C_ = box(L - 1, ch)
                assert np.all(C_[0:3] >= B[0:3]) and np.all(C_[4:7] <= B[4:7])
    for trial in range(20):
        q = rng.uniform(c.min(0), c.max(0))
        r = rng.uniform(0.5, 8.0)

        def overlaps(B):
            return np.all(B[0:2] <= q + r) and np.all(B[4:6] >= q - r)

        want = [g for g in range(ngroups) if overlaps(groups[g, :8])]
        got, L, i = [], levels, 0
        while L >= 0:
            g0 = i << (3 * L)
            limit = g0 + 16
            while True:
                g, L, i = _tree_next(levels, cnt, L, i, limit, lambda L_, i_: overlaps(box(L_, i_)),
                                     lambda i_: overlaps(groups[i_, :8]))
                if g < 0:
                    break
                assert g0 <= g < limit
                got.append(g)
        assert got == want, trial


@pytest.mark.parametrize("case", ["dirichlet_obstacle", "engine"])
def test_dirichlet_grid_lists_hold_the_nearest_segments(shim, case):
    """The Dirichlet-distance cell grid (wos_host_scene.cpp build_dirichlet_grid): at random
    points and points on and next to the Dirichlet segments, every segment the float scan
    could pick (true distance within 1e-6 relative of the nearest) is on the point's cell
    list, so the kernel's list scan returns the full scan's distance."""
    rng = np.random.default_rng(7)
    if case == "engine":
        import engine_pin as ep
        U = ep.upstream_scene()
        (nv, nix), (dv, dix) = U["neumann"], U["dirichlet"]
    else:
        c = workloads.dirichlet_obstacle_config(n_walks=4, res=8)
        nv, nix, dv, dix = c["vertices"], c["prims"], c["dvertices"], c["dprims"]
    nv, dv = np.ascontiguousarray(nv, np.float32), np.ascontiguousarray(dv, np.float32)
    nix, dix = np.ascontiguousarray(nix, np.int32), np.ascontiguousarray(dix, np.int32)
    allv = np.concatenate([nv, dv])
    lo, hi = allv.min(0), allv.max(0)
    pts = [rng.uniform(lo, hi, (20000, 2))]
    a, b = dv[dix[:, 0]], dv[dix[:, 1]]
    t = rng.uniform(0, 1, (len(dix), 8, 1))
    on = a[:, None, :] + t * (b - a)[:, None, :]
    pts.append(on.reshape(-1, 2))
    pts.append((on + rng.normal(0, 1e-3 * float((hi - lo).max()), on.shape)).reshape(-1, 2))
    pts.append(np.concatenate([a, b]))
    pts = np.ascontiguousarray(np.concatenate(pts), np.float32)
    info = np.zeros(8, np.int32)
    f, i = C.POINTER(C.c_float), C.POINTER(C.c_int)
    bad = shim.hs_dir_grid_check(nv.ctypes.data_as(f), nv.shape[0], nix.ctypes.data_as(i), nix.shape[0],
                                 dv.ctypes.data_as(f), dv.shape[0], dix.ctypes.data_as(i), dix.shape[0],
                                 pts.ctypes.data_as(f), pts.shape[0], info.ctypes.data_as(i))
    assert info[0] == 1, info  # the grid is built
    assert info[6] > 0.9 * pts.shape[0], info
    assert bad == 0, (bad, info)
    assert info[3] <= 256 and info[2] <= 16 * info[1], info  # short lists
