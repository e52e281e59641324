"""Geometry queries on the GPU (include/wos.h "Geometry queries", csrc/wos_query.hip):
wos_scene_query against the CPU oracle's point_info bit for bit, the state word against a recorded
tape's pstate, the closest point against float64 geometry, the interface (numpy, torch on a side
stream, the raw C ABI, every refusal), and MeshSDF / PressureProjector.sample_state on top of it."""
import ctypes as C
import functools

import numpy as np
import pytest

import objparse
import variance_cases as vc
from test_gpu_parity import assert_bits_equal
from wos_amd import _lib, workloads

pytestmark = pytest.mark.gpu

EST, MASKP, MASKG, INSIDE = _lib.STATE_ESTIMATED, _lib.STATE_MASK_P, _lib.STATE_MASK_GRAD, _lib.STATE_INSIDE


# ---- scenes ---------------------------------------------------------------------------------------
def _karman_geometry():
    return objparse.load(workloads.KARMAN_OBJ, 2)


def _karman_points():
    """300 points: 200 of config B's, 50 outside the box or inside the cylinder, 50 ON the mesh --
    vertices (the t <= eps normal branches, exact ties between the two segments of a vertex) and
    segment midpoints."""
    cfg = workloads.karman_config(n_walks=2)
    v, ix = _karman_geometry()
    size = workloads.scene_size(workloads.KARMAN_OBJ)
    c, r = workloads.karman_obstacle(size)
    rng = np.random.default_rng(21)
    ang = rng.uniform(0, 2 * np.pi, 25)
    inside_cyl = np.stack([c[0] + 0.9 * r * rng.random(25) * np.cos(ang), c[1] + 0.9 * r * rng.random(25) * np.sin(ang)], -1)
    out = np.stack([rng.uniform(size[0], size[1], 25), rng.choice([-1.0, 1.0], 25) * rng.uniform(0.61, 1.2, 25)], -1)
    mid = (0.5 * (v[ix[:25, 0]] + v[ix[:25, 1]])).astype(np.float32)
    pts = np.concatenate([cfg["points"][:200], inside_cyl, out, v[::max(1, len(v) // 25)][:25], mid])
    return np.ascontiguousarray(pts, np.float32)


def _box_points(v, n, seed, pad=0.15):
    """n uniform points over the mesh's bounding box grown by `pad` of its extent: both sides."""
    lo, hi = v.min(0), v.max(0)
    e = (hi - lo) * pad
    return np.random.default_rng(seed).uniform(lo - e, hi + e, (n, v.shape[1])).astype(np.float32)


def _circle_dirichlet():
    """Config C's box with its Dirichlet disk as a 4 096-segment circle: 512 groups, the scene
    builds a hierarchy over them and the records (16 384 floats) do not fit the kernel's LDS."""
    v, ix = workloads.box_2d(1.0)
    dv, dix = workloads.circle_2d((0.5, 0.35), 0.1, 4096)
    return v, ix, dv, dix


@functools.lru_cache(maxsize=None)
def _case(name):
    """(vertices, prims, scene kwargs, points) of a named geometry."""
    kw = {"watertight": True}
    if name == "karman":
        v, ix = _karman_geometry()
        pts = _karman_points()
    elif name == "karman1000":
        v, ix = _karman_geometry()
        pts = workloads.karman_config(n_walks=2)["points"][:1000]
    elif name in ("engine", "engine_flip"):
        cfg = workloads.engine_config(n_points=200, flip=name == "engine_flip")
        v, ix, pts = cfg["vertices"], cfg["prims"], cfg["points"]
    elif name == "gear":
        cfg = workloads.gear_config()
        v, ix = cfg["vertices"], cfg["prims"]
        assert (ix.shape[0] + 7) // 8 > 16  # more than 16 groups: closest_lane's culled scan
        pts = _box_points(v, 200, 5)
    elif name == "circle4096":
        v, ix, dv, dix = _circle_dirichlet()
        kw.update(dvertices=dv, dprims=dix, dirichlet_value=1.0)
        rng = np.random.default_rng(9)
        near = np.float32([0.5, 0.35]) + rng.normal(size=(64, 2)) * 0.08
        pts = np.concatenate([_box_points(v, 64, 6, pad=0.1), near]).astype(np.float32)
    elif name == "gear6000":
        cfg = workloads.gear_config(n_teeth=6000)
        v, ix = cfg["vertices"], cfg["prims"]
        assert ix.shape[0] * 4 > 4096  # beyond the kernel's LDS staging: global-memory path
        pts = _box_points(v, 128, 7)
    elif name == "cube":
        v, ix = objparse.load(workloads.CUBE_OBJ, 3)
        pts = _box_points(v, 200, 8, pad=0.25)
    elif name == "cube24":
        v, ix = workloads.subdivided_cube(24)
        pts = _box_points(v, 64, 10, pad=0.25)
    elif name == "open_box":  # the cube without its first two triangles, not watertight: inside is always 1
        v, ix = objparse.load(workloads.CUBE_OBJ, 3)
        ix = ix[2:]
        kw = {"watertight": False}
        pts = _box_points(v, 64, 12, pad=0.25)
    elif name == "double_sided":
        v, ix = objparse.load(workloads.CUBE_OBJ, 3)
        ix = ix[2:]
        kw = {"watertight": True, "double_sided": True}
        pts = _box_points(v, 64, 13, pad=0.25)
    else:
        raise KeyError(name)
    return np.ascontiguousarray(v, np.float32), np.ascontiguousarray(ix, np.int32), kw, np.ascontiguousarray(pts)


def _source(dim):
    return np.zeros((4,) * dim, np.float32)


def _scene(name):
    from wos_amd import WosScene
    v, ix, kw, _ = _case(name)
    return WosScene(v, ix, _source(v.shape[1]), 350.0, **kw)


@functools.lru_cache(maxsize=None)
def _oracle_info(name):
    """The oracle's point_info of the case's points, once per session: dirichlet_dist,
    neumann_dist, signed_neumann_dist float32 and inside int32."""
    import oracle_lib
    v, ix, kw, pts = _case(name)
    okw = {k: kw[k] for k in ("dvertices", "dprims", "dirichlet_value", "watertight", "double_sided") if k in kw}
    osc = oracle_lib.OracleScene(v, ix, _source(v.shape[1]), 350.0, **okw)
    info = [oracle_lib.point_info(osc, p) for p in pts]
    return {k: np.array([i[k] for i in info], np.int32 if k == "inside" else np.float32)
            for k in ("dirichlet_dist", "neumann_dist", "signed_neumann_dist", "inside")}


def _check_against_oracle(name, got, ref, which="neumann"):
    d, sd, state = got[:3]
    if which == "neumann":
        assert_bits_equal(d, ref["neumann_dist"])
        assert_bits_equal(sd, ref["signed_neumann_dist"])
    else:
        assert_bits_equal(d, ref["dirichlet_dist"])
        assert_bits_equal(np.abs(sd), ref["dirichlet_dist"])
    np.testing.assert_array_equal((state >> 3) & 1, ref["inside"], err_msg=name)


# ---- 1. bit for bit against the oracle --------------------------------------------------------------
@pytest.mark.parametrize("name", ["karman", "engine", "engine_flip", "gear", "circle4096", "gear6000", "cube", "cube24",
                                  "open_box", "double_sided"])
def test_query_matches_oracle(gpu, oracle, name):
    pts = _case(name)[3]
    ref = _oracle_info(name)
    sc = _scene(name)
    got = sc.query(pts)
    _check_against_oracle(name, got, ref)
    inside = (got[2] >> 3) & 1
    if name == "open_box":
        assert inside.all()
    else:
        assert 0 < inside.sum() < pts.shape[0], "the points must lie on both sides"
    if name == "circle4096":
        gd = sc.query(pts, which="dirichlet")
        _check_against_oracle(name, gd, ref, which="dirichlet")
        np.testing.assert_array_equal(gd[2], got[2])  # the state does not depend on `which`
        assert (gd[1] < 0).any() and (gd[1] > 0).any()
    sc.close()


def test_karman_sign_and_special_points(gpu, oracle):
    """signed_dist is the solver's: negative on the domain side; the points ON the mesh have
    distance 0 (vertices, exactly) and agree with the oracle there too (covered above)."""
    v, ix, _, pts = _case("karman")
    sc = _scene("karman")
    d, sd, state = sc.query(pts)
    interior = pts[:200]
    assert (sd[:200] < 0).all() and (state[:200] & INSIDE).all() and interior.shape[0] == 200
    assert not (state[200:250] & INSIDE).any() and (sd[200:250] > 0).all()
    # the vertices: 0 from the segment that starts there (a + 0 u), a + 1 (b - a) may round off b
    assert (d[250:275] <= 2.0 ** -21).all() and (d[250:275] == 0).any()
    d1, sd1, _ = sc.query(np.array([[0.0, 0.60349 - 0.028]], np.float32))  # 0.028 below the upper wall
    assert abs(sd1[0] + 0.028) < 1e-5 and d1[0] == -sd1[0]
    sc.close()


@pytest.mark.parametrize("n", [1, 257, 1000])
def test_query_partial_wave_block_and_several_blocks(gpu, oracle, n):
    pts = _case("karman1000")[3]
    ref = _oracle_info("karman1000")
    sc = _scene("karman1000")
    d, sd, state, cp = sc.query(pts[:n], closest=True)
    assert d.shape == sd.shape == state.shape == (n,) and cp.shape == (n, 2) and state.dtype == np.int32
    _check_against_oracle(f"n={n}", (d, sd, state), {k: a[:n] for k, a in ref.items()})
    sc.close()


# ---- 2. the state word --------------------------------------------------------------------------------
def _host_inside(sd_n, sd_d, watertight=True):
    """insideDomain (fcpw_scene_loader.h:642-648) from the two signed distances."""
    if not watertight:
        return np.ones(sd_n.shape, bool)
    return np.where(np.abs(sd_d) < np.abs(sd_n), sd_d < 0, sd_n < 0)


def test_state_equals_tape_pstate_karman_mask(gpu):
    """mask 1e-2 with points on both sides of it, next to the walls and to the cylinder."""
    from wos_amd import WosScene, solver_params
    c = vc.case("karman_w2")
    size = workloads.scene_size(workloads.KARMAN_OBJ)
    cen, r = workloads.karman_obstacle(size)
    extra = np.array([[0.0, 0.595], [0.0, 0.585], [0.3, -0.592], [0.3, -0.58], [cen[0] + r + 0.004, cen[1]],
                      [cen[0] + r + 0.03, cen[1]], [cen[0], cen[1] - r - 0.006], [cen[0], cen[1] - r - 0.02]], np.float32)
    pts = np.ascontiguousarray(np.concatenate([c["points"], extra]))
    mask = 1e-2
    sc = WosScene(c["vertices"], c["prims"], c["source"], c["absorption"], watertight=True)
    prm = solver_params(c["solver"], dict(c["output"], boundaryDistanceMask=mask))
    tape = sc.record(pts, prm)
    pstate = tape.read("pstate")
    d, sd, state = sc.query(pts, boundary_distance_mask=mask)
    np.testing.assert_array_equal(state & 7, pstate & 7)
    np.testing.assert_array_equal(sc.query_state(pts, mask), state)
    est = (state & EST) != 0
    assert (est & ((state & MASKP) != 0)).any() and (est & ((state & (MASKP | MASKG)) == 0)).any()
    assert ((state & EST) == 0).any()
    # the extras alternate: within the mask distance, beyond it
    np.testing.assert_array_equal((state[-8:] & MASKP) != 0, [True, False] * 4)
    np.testing.assert_array_equal((state & INSIDE) != 0, sd < 0)  # no Dirichlet geometry: the Neumann side decides
    np.testing.assert_array_equal((state & MASKP) != 0, d < np.float32(mask))
    # another mask, another word: the default 0 masks nothing that is inside
    s0 = sc.query_state(pts)
    assert not (s0[est] & (MASKP | MASKG)).any()
    tape.close()
    sc.close()


def test_state_equals_tape_pstate_dirichlet_shell(gpu):
    from wos_amd import WosScene, solver_params
    c = vc.case("dirichlet_w40")
    rng = np.random.default_rng(3)
    ang = rng.uniform(0, 2 * np.pi, 24)
    rad = 0.1 + rng.uniform(-8e-4, 8e-4, 24)  # the disk's epsilon shell, both sides of the circle
    shell = np.float32([0.5, 0.35]) + np.stack([rad * np.cos(ang), rad * np.sin(ang)], -1)
    pts = np.ascontiguousarray(np.concatenate([c["points"], shell]), np.float32)
    sc = WosScene(c["vertices"], c["prims"], c["source"], c["absorption"], watertight=True, **c["kw"])
    prm = solver_params(dict(c["solver"], nWalks=2), c["output"])
    tape = sc.record(pts, prm)
    pstate = tape.read("pstate")
    mask = c["output"]["boundaryDistanceMask"]
    dn, sdn, state = sc.query(pts, boundary_distance_mask=mask)
    dd, sdd, state_d = sc.query(pts, which="dirichlet", boundary_distance_mask=mask)
    np.testing.assert_array_equal(state & 7, pstate & 7)
    np.testing.assert_array_equal(state, state_d)
    inside = _host_inside(sdn, sdd)
    np.testing.assert_array_equal((state & INSIDE) != 0, inside)
    assert inside[-24:].any() and not inside[-24:].all()  # the shell points straddle the circle
    assert ((state & MASKP) != 0).any()
    tape.close()
    sc.close()


@pytest.mark.parametrize("name", ["open_box", "double_sided", "cube"])
def test_state_inside_rule_3d(gpu, name):
    v, ix, kw, pts = _case(name)
    sc = _scene(name)
    d, sd, state = sc.query(pts, boundary_distance_mask=0.05)
    inside = _host_inside(sd, np.full_like(sd, np.inf), kw["watertight"])  # no Dirichlet mesh: the far corner, never nearer
    np.testing.assert_array_equal((state & INSIDE) != 0, inside)
    est = inside | bool(kw.get("double_sided"))
    np.testing.assert_array_equal((state & EST) != 0, est)
    np.testing.assert_array_equal((state & MASKP) != 0, d < np.float32(0.05))
    np.testing.assert_array_equal((state & MASKG) != 0, (~est) | (d < np.float32(0.05)))
    sc.close()


# ---- 3. the closest point -----------------------------------------------------------------------------
def _seg_dist64(v, ix, q):
    a, b = v[ix[:, 0]].astype(np.float64), v[ix[:, 1]].astype(np.float64)
    s = b - a
    t = np.clip(((q[:, None] - a[None]) * s[None]).sum(-1) / (s * s).sum(-1)[None], 0, 1)
    return np.linalg.norm(q[:, None] - (a[None] + t[..., None] * s[None]), axis=-1).min(1)


def _tri_dist64(v, ix, q):
    """float64 distance to the nearest triangle: the plane distance where the projection falls
    inside, else the nearest edge."""
    out = np.full(q.shape[0], np.inf)
    V = v.astype(np.float64)
    for t in ix:
        a, b, c = V[t[0]], V[t[1]], V[t[2]]
        n = np.cross(b - a, c - a)
        n /= np.linalg.norm(n)
        h = (q - a) @ n
        p = q - h[:, None] * n
        inside = np.ones(q.shape[0], bool)
        for e0, e1 in ((a, b), (b, c), (c, a)):
            inside &= np.cross(e1 - e0, p - e0) @ n >= 0
        edge = np.full(q.shape[0], np.inf)
        for e0, e1 in ((a, b), (b, c), (c, a)):
            s = e1 - e0
            tt = np.clip(((q - e0) @ s) / (s @ s), 0, 1)
            edge = np.minimum(edge, np.linalg.norm(q - (e0 + tt[:, None] * s), axis=1))
        out = np.minimum(out, np.where(inside, np.abs(h), edge))
    return out


@pytest.mark.parametrize("name", ["karman", "gear", "cube", "circle4096"])
def test_closest_point(gpu, name):
    v, ix, kw, pts = _case(name)
    dim = v.shape[1]
    sc = _scene(name)
    for which, vv, ii in (("neumann", v, ix),) + ((("dirichlet", kw["dvertices"], kw["dprims"]),) if "dprims" in kw else ()):
        d, sd, state, cp = sc.query(pts, which=which, closest=True)
        assert cp.shape == (pts.shape[0], dim) and cp.dtype == np.float32
        # the same float32 operations as the kernel: one rounding per square and add, plus the root
        r = pts - cp
        acc = r[:, 0] * r[:, 0]
        for k in range(1, dim):
            acc = acc + r[:, k] * r[:, k]
        re = np.sqrt(acc, dtype=np.float32)
        err = np.abs(re.astype(np.float64) - d.astype(np.float64))
        print(f"{name}/{which}: max |recomputed - dist| / dist = {np.max(err / np.maximum(d, 1e-30)):.3e}")
        assert (err <= (dim + 2) * 2.0 ** -24 * d.astype(np.float64)).all()
        # on the mesh: the few float32 roundings of a + t (b - a)
        on = (_seg_dist64 if dim == 2 else _tri_dist64)(vv, ii, cp.astype(np.float64))
        bound = 8 * 2.0 ** -24 * max(float(np.abs(vv).max()), float(np.abs(cp).max()))
        print(f"{name}/{which}: max distance of closest from the mesh = {on.max():.3e} (bound {bound:.3e})")
        assert (on <= bound).all()
    sc.close()


# ---- 4. the interface ---------------------------------------------------------------------------------
def test_torch_side_stream_equals_numpy(gpu):
    import torch
    v, ix, _, pts = _case("karman")
    sc = _scene("karman")
    ref = sc.query(pts, boundary_distance_mask=1e-3, closest=True)
    x = torch.from_numpy(pts).cuda()
    side = torch.cuda.Stream()
    for stream in (None, side, side.cuda_stream):
        got = sc.query(x, boundary_distance_mask=1e-3, closest=True, stream=stream)
        assert all(t.is_cuda and t.device == x.device for t in got)
        if stream is not None:
            side.synchronize()
        d, sd, state, cp = (t.cpu().numpy() for t in got)
        assert_bits_equal(d, ref[0])
        assert_bits_equal(sd, ref[1])
        np.testing.assert_array_equal(state, ref[2])
        assert_bits_equal(cp.ravel(), ref[3].ravel())
        assert got[2].dtype == torch.int32
    # a CPU tensor goes the host way
    h = sc.query(torch.from_numpy(pts), closest=False)
    assert isinstance(h[0], np.ndarray) and len(h) == 3
    assert_bits_equal(h[0], ref[0])
    sc.close()


def test_c_abi_optional_outputs_async_and_empty(gpu):
    import torch
    L = _lib.load()
    v, ix, _, pts = _case("karman")
    n = pts.shape[0]
    sc = _scene("karman")
    ref = sc.query(pts, boundary_distance_mask=1e-3, closest=True)
    full = {"dist": ref[0], "signed_dist": ref[1], "closest": ref[3], "state": ref[2]}
    names = ("dist", "signed_dist", "closest", "state")

    def host(skip):
        out = {k: np.full_like(full[k], 77) for k in names if k not in skip}
        rc = L.wos_scene_query(sc._h, 0, 1e-3, pts.ctypes.data, n, *[out[k].ctypes.data if k in out else None for k in names],
                               None, 0)
        assert rc == 0, L.wos_last_error()
        return out

    for skip in [()] + [(k,) for k in names] + [("dist", "signed_dist", "closest"), ("signed_dist", "closest", "state")]:
        for k, a in host(skip).items():
            assert a.tobytes() == full[k].tobytes(), (skip, k)
    # device pointers, WOS_ASYNC on a side stream: returns at once, ordered on the stream
    x = torch.from_numpy(pts).cuda()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    for skip in [()] + [(k,) for k in names]:
        out = {k: torch.full(full[k].shape, 77, dtype=torch.int32 if k == "state" else torch.float32, device="cuda")
               for k in names if k not in skip}
        side.wait_stream(torch.cuda.current_stream())
        rc = L.wos_scene_query(sc._h, 0, 1e-3, x.data_ptr(), n, *[out[k].data_ptr() if k in out else None for k in names],
                               side.cuda_stream, _lib.WOS_PTRS_DEVICE | _lib.WOS_ASYNC)
        assert rc == 0, L.wos_last_error()
        side.synchronize()
        for k, t in out.items():
            assert t.cpu().numpy().tobytes() == full[k].tobytes(), (skip, k)
    # device pointers without WOS_ASYNC: done when the call returns
    st = torch.full((n,), 77, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    assert L.wos_scene_query(sc._h, 0, 1e-3, x.data_ptr(), n, None, None, None, st.data_ptr(), side.cuda_stream,
                             _lib.WOS_PTRS_DEVICE) == 0
    assert st.cpu().numpy().tobytes() == full["state"].tobytes()
    # n == 0: succeeds without a launch, whatever the point pointer
    one = np.zeros(1, np.float32)
    assert L.wos_scene_query(sc._h, 0, 0.0, None, 0, one.ctypes.data, None, None, None, None, 0) == 0
    assert one[0] == 0
    e = sc.query(np.zeros((0, 2), np.float32), closest=True)
    assert [a.shape for a in e] == [(0,), (0,), (0,), (0, 2)]
    et = sc.query(torch.zeros((0, 2), device="cuda"))
    assert all(t.is_cuda and t.shape == (0,) for t in et)
    sc.close()


def test_refusals(gpu):
    from wos_amd import WosError
    L = _lib.load()
    v, ix, _, pts = _case("karman")
    sc = _scene("karman")
    d = np.zeros(pts.shape[0], np.float32)
    s = np.zeros(pts.shape[0], np.int32)

    def call(which, dist, sd, cp, state, scene=sc, n=pts.shape[0], p=pts.ctypes.data):
        rc = L.wos_scene_query(scene._h if scene is not None else None, which, 0.0, p, n, dist, sd, cp, state, None, 0)
        return rc, L.wos_last_error().decode()

    for which in (-1, 2):
        rc, msg = call(which, d.ctypes.data, None, None, None)
        assert rc == -1 and "which" in msg and str(which) in msg
    rc, msg = call(0, None, None, None, None)
    assert rc == -1 and "no output" in msg
    cp = np.zeros((pts.shape[0], 2), np.float32)
    for args in ((d.ctypes.data, None, None), (None, d.ctypes.data, None), (None, None, cp.ctypes.data)):
        rc, msg = call(1, *args, s.ctypes.data)  # karman holds no Dirichlet boundary
        assert rc == -1 and "no Dirichlet boundary" in msg
    rc, msg = call(1, None, None, None, s.ctypes.data)  # state alone needs none
    assert rc == 0
    np.testing.assert_array_equal(s, sc.query_state(pts))
    rc, msg = call(0, d.ctypes.data, None, None, None, scene=None)
    assert rc == -1 and "null scene" in msg
    rc, msg = call(0, d.ctypes.data, None, None, None, n=-1)
    assert rc == -1 and "negative" in msg
    rc, msg = call(0, d.ctypes.data, None, None, None, p=None)
    assert rc == -1 and "null point" in msg
    with pytest.raises(WosError, match="no Dirichlet boundary"):
        sc.query(pts, which="dirichlet")
    with pytest.raises(WosError, match="'neumann' or 'dirichlet'"):
        sc.query(pts, which="robin")
    with pytest.raises(WosError, match=r"points must be \[N,2\]"):
        sc.query(np.zeros((4, 3), np.float32))
    sc.close()


def test_solve_unchanged_by_queries(gpu):
    """A query reads geometry only: the solve before and the solve after return the same bits,
    also with a query enqueued on another stream in between."""
    import torch
    from wos_amd import WosScene, solver_params
    c = vc.case("karman_w40")
    sc = WosScene(c["vertices"], c["prims"], c["source"], c["absorption"], watertight=True)
    prm = solver_params(c["solver"], c["output"])
    x = torch.from_numpy(c["points"]).cuda()
    p0, g0, _ = sc.solve(x, prm)
    side = torch.cuda.Stream()
    q1 = sc.query(x, stream=side, closest=True)
    q2 = sc.query(c["points"], which="neumann")
    p1, g1, _ = sc.solve(x, prm)
    side.synchronize()
    assert_bits_equal(p0.cpu().numpy(), p1.cpu().numpy())
    assert_bits_equal(g0.cpu().numpy().ravel(), g1.cpu().numpy().ravel())
    assert_bits_equal(q1[0].cpu().numpy(), q2[0])
    sc.close()


# ---- 5. MeshSDF and the projector -----------------------------------------------------------------------
def _direction64(v, ix, x, clearance):
    """float64 (x - closest) / |x - closest| of 2D points (0 where the distance is 0), the
    distance, and which points are at least `clearance` away from a tie -- a place where the
    closest point jumps to another part of the mesh.  Moving x by `clearance` changes every
    distance by at most that, so x is clear if no segment comes within 2 clearance of the best
    distance with a closest point that is not on the best segment itself (one that is -- the
    shared vertex of a neighbour -- can never be nearer than the best segment: no tie there)."""
    a, b = v[ix[:, 0]].astype(np.float64), v[ix[:, 1]].astype(np.float64)
    x = x.astype(np.float64)
    s = b - a
    ss = np.where((s * s).sum(-1) > 0, (s * s).sum(-1), 1.0)
    t = np.clip(((x[:, None] - a[None]) * s[None]).sum(-1) / ss[None], 0, 1)
    cp = a[None] + t[..., None] * s[None]
    d = np.linalg.norm(x[:, None] - cp, axis=-1)
    best = d.argmin(1)
    rows = np.arange(x.shape[0])
    cpb, db = cp[rows, best], d[rows, best]
    ab, sb = a[best], s[best]
    tb = np.clip(((cp - ab[:, None]) * sb[:, None]).sum(-1) / ss[best][:, None], 0, 1)
    off_best = np.linalg.norm(cp - (ab[:, None] + tb[..., None] * sb[:, None]), axis=-1) > 1e-9
    clear = ~((d - db[:, None] < 2 * clearance) & off_best).any(1)
    return (x - cpb) / np.where(db > 0, db, 1.0)[:, None], db, clear


def test_meshsdf_values_and_gradient(gpu):
    import torch
    from wos_amd.projection import MeshSDF, divergence
    v, ix = _karman_geometry()
    sc = _scene("karman")
    pts = workloads.karman_config(n_walks=2)["points"][:600]
    outside = _case("karman")[3][200:250]
    allp = np.ascontiguousarray(np.concatenate([pts, outside]))
    _, sd, _ = sc.query(allp)
    x = torch.from_numpy(allp).cuda().requires_grad_(True)
    for positive, sign in (("inside", -1.0), ("outside", 1.0)):
        sdf = MeshSDF(sc, positive)
        val = sdf(x)
        assert val.is_cuda and val.shape == (allp.shape[0],)
        assert_bits_equal(val.detach().cpu().numpy(), (np.float32(sign) * sd))
        (g,) = torch.autograd.grad(val.sum(), x)
        g = g.cpu().numpy().astype(np.float64)
        np.testing.assert_allclose(np.linalg.norm(g, axis=1), 1.0, atol=4 * 2.0 ** -24)
        # every point at least 1e-3 away from a tie, however near the boundary: direction and sign
        dir64, d64, clear = _direction64(v, ix, allp, 1e-3)
        assert clear.sum() > 500 and (d64[clear] < 0.02).sum() > 20 and (d64[clear] < 2e-3).any()
        want = sign * np.sign(sd)[:, None] * dir64
        err = np.abs(g - want).max(1)
        k = np.argmax(err * clear)
        print(f"MeshSDF({positive}): max |backward - float64 direction| = {err[k]:.3e} (at distance {d64[k]:.3e}) over "
              f"{clear.sum()} tie-clear points, nearest at {d64[clear].min():.3e}")
        assert (err[clear] <= 1e-5).all()
        assert ((g * want).sum(1)[clear] > 0.999).all()  # the sign, said on its own
    # the reference's two input shapes: (N, 2) above, the (H, W, 2) grid here, through divergence()
    grid = torch.from_numpy(workloads.uniform_grid_2d(24, workloads.scene_size(workloads.KARMAN_OBJ))).cuda()
    grid.requires_grad_(True)
    sdf = MeshSDF(sc, "inside")
    c = torch.tensor([0.75, -1.25], device="cuda")
    val = sdf(grid)
    assert val.shape == grid.shape[:-1]
    div = divergence(sdf(grid)[..., None] * c, grid)
    (gd,) = torch.autograd.grad(val.sum(), grid)
    np.testing.assert_allclose(div[..., 0].detach().cpu().numpy(), (gd * c).sum(-1).cpu().numpy(), rtol=0, atol=1e-6)
    flat = grid.detach().reshape(-1, 2).cpu().numpy()
    dir64, d64, clear = _direction64(v, ix, flat, 1e-3)
    _, sdg, _ = sc.query(flat)
    want = (-np.sign(sdg)[:, None] * dir64 * c.cpu().numpy().astype(np.float64)).sum(-1)
    got = div.detach().reshape(-1).cpu().numpy().astype(np.float64)
    print(f"divergence term: max error {np.abs(got - want)[clear].max():.3e} over {clear.sum()} of {clear.size} grid points")
    # |c|_1 = 2 times the 1e-5 above; the grid's boundary rows lie on (or within 1e-7 of) the walls
    assert clear.sum() > 200 and (d64[clear] < 1e-6).any() and (np.abs(got - want)[clear] <= 2e-5).all()
    on = d64 == 0
    assert (got[on] == 0).all()  # 0 where the distance is 0
    # the second derivative is refused, not silently dropped
    (g1,) = torch.autograd.grad((sdf(grid) ** 2).sum(), grid, create_graph=True)
    with pytest.raises(RuntimeError, match="once_differentiable"):
        g1.sum().backward()
    sc.close()


def test_shim_sdf_and_projector_sample_state(gpu):
    import torch
    import zombie_bindings
    from wos_amd import projection as pj
    cfg = workloads.karman_config(n_walks=2, n_points=300)
    scene_cfg = dict(workloads.SCENE_BASE, boundary=workloads.KARMAN_OBJ)
    extra = _case("karman")[3][200:300]  # outside, inside the cylinder, on the mesh
    samples = torch.from_numpy(np.ascontiguousarray(np.concatenate([cfg["points"], extra]))).cuda()
    proj = pj.PressureProjector(scene_cfg, cfg["solver"], dict(cfg["output"], boundaryDistanceMask=1e-2), samples,
                                reuse_walks=True)
    state = proj.sample_state()
    assert state.is_cuda and state.dtype == torch.int32 and state.shape == (samples.shape[0],)
    div = torch.from_numpy(cfg["source"]).cuda()
    p, g = proj.solve(div)
    pstate = proj._tape.read("pstate")
    np.testing.assert_array_equal(state.cpu().numpy() & 7, pstate & 7)
    s = state.cpu().numpy()
    assert ((s & EST) != 0).any() and ((s & EST) == 0).any() and ((s & MASKP) != 0).any()
    # what the state promises is what the solve returns: masked or not estimated samples come back as 0
    gz = (g.cpu().numpy() == 0).all(1)
    assert gz[((s & EST) == 0) | ((s & MASKG) != 0)].all()
    sub = samples[:17]
    np.testing.assert_array_equal(proj.sample_state(sub).cpu().numpy(), s[:17])
    # the shim's pass-through
    zs = zombie_bindings.Scene(scene_cfg, np.zeros((4, 4), np.float32))
    _, sd, _ = zs._scene.query(samples)
    assert_bits_equal(zs.sdf(samples).cpu().numpy(), -sd.cpu().numpy())
    assert_bits_equal(zs.sdf(samples, positive="outside").cpu().numpy(), sd.cpu().numpy())
    assert_bits_equal(zs.sdf(samples.cpu().numpy()), -sd.cpu().numpy())
