"""The walk step's three geometry queries on the device, pinned directly (wos_selftest_geometry).

Every walk step asks for a star radius (star_radius_wave), a first ray hit (ray_hit_wave) and the
distance to the Dirichlet boundary (dirichlet_dist_step).  Each is a stack of shortcuts in front of
the reference's sequential scan -- box and cone culls, rcp / rsq pre-filters with margins, cell
lists -- under several execution regimes chosen by how many lanes of a wave query.  The probe runs,
per item, the plain scan, the per-lane culled form and the wave-cooperative form as shipped, on the
scene planned as a solve plans it, under caller-chosen lane masks; and every shortcut beside the
exact test over every primitive, candidate and group (a soundness word, fired / declined counts).

Asserted, per scene, schedule and kind, over random and adversarial items (geometry_cases.py):
  1. the three device forms are equal bit for bit;
  2. they equal the oracle's sequential scans bit for bit (oracle_ray_hits, oracle_star_radii,
     oracle_dirichlet_dists, themselves pinned against float64 in test_geometry_oracle_cpu.py);
  3. neither the lane mask nor the schedule changes a bit (the soundness words and counts do not
     depend on the mask either);
  4. the Dirichlet distance and projection equal wos_scene_query's dist and closest;
  5. every soundness bit is 0;
  6. each regime and each shortcut the case was built for was entered, fired and declined (the
     regime from the probe's branch tag, not from a diagnostics build);
  7. the refusals, by status and message.
Not built here: the winner's lane position in the solo ray reduction is spread by aiming at
primitives of many (group, slot) positions, but which lane it lands on is not asserted.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import geometry_cases as gc
from test_gpu_parity import assert_bits_equal
from wos_amd import WosError, _lib

pytestmark = pytest.mark.gpu

GG, NO_STAR, NO_DIR = _lib.SCHED_GEOM_GLOBAL, _lib.SCHED_NO_STAR_GRID, _lib.SCHED_NO_DIR_GRID
ALL64 = 0xFFFFFFFFFFFFFFFF
INVALID = -1  # include/wos.h WOS_E_INVALID


# ---- lane masks: the same items under every one --------------------------------------------------------
def _masks(n, kind):
    """n items as waves of (a) all 64 lanes, (b) alternating lanes, (c) two lanes, (d) one lane at
    positions 0, 37 and 63 in turn."""
    def fill(pattern_of):
        out, left, w = [], n, 0
        while left > 0:
            bits = [b for b in range(64) if (pattern_of(w) >> b) & 1][:left]
            out.append(sum(1 << b for b in bits))
            left -= len(bits)
            w += 1
        return np.array(out, np.uint64)
    return {"all": fill(lambda w: ALL64), "alternating": fill(lambda w: 0x5555555555555555),
            "two": fill(lambda w: (1 << 5) | (1 << 40)), "one": fill(lambda w: 1 << (0, 37, 63)[w % 3])}


# ---- items and their oracle answers, once per (scene, kind) ----------------------------------------------
@functools.lru_cache(maxsize=None)
def _reference(name, kind, prec=1e-3):
    import oracle_lib
    # a multiple of 64 items, so that no mask set ends in a wave of another regime
    whole_waves = lambda a: np.ascontiguousarray(a[:len(a) // 64 * 64])
    osc = gc.oracle_scene(oracle_lib, name)
    dim = gc.scene(name)[0].shape[1]
    rng = np.random.default_rng(sum(map(ord, name + kind)))
    if kind == "ray":
        rays = gc.ray_items(name, rng)
        found, d, _, _ = oracle_lib.ray_hits(osc, rays[:, :dim], rays[:, dim:2 * dim], rays[:, 2 * dim])
        items = whole_waves(np.concatenate([rays, gc.tmax_bands(rays, found, d)]))
        ref = oracle_lib.ray_hits(osc, items[:, :dim], items[:, dim:2 * dim], items[:, 2 * dim])
    elif kind == "star":
        items = whole_waves(gc.star_items(name, rng, prec=prec))
        ref = oracle_lib.star_radii(osc, items[:, :dim], items[:, dim], items[:, dim + 1].astype(np.int32), prec=prec)
    else:
        items = whole_waves(gc.dirichlet_items(name, rng))
        ref = oracle_lib.dirichlet_dists(osc, items)
    assert 0 < len(items) <= 4096 and np.isfinite(items).all()
    for a in (ref if isinstance(ref, tuple) else (ref,)):
        a.setflags(write=False)
    items.setflags(write=False)
    return items, ref


def _check_forms(kind, dim, out, ref):
    """assertions 1 and 2 on one probe result"""
    if kind == "ray":
        found, d, p, nrm = ref
        for form in range(3):
            np.testing.assert_array_equal(out[:, form, 0] != 0, found != 0, err_msg=f"found, form {form}")
            assert_bits_equal(out[:, form, 1], d)
            assert_bits_equal(np.ascontiguousarray(out[:, form, 2:2 + dim]), p)
            assert_bits_equal(np.ascontiguousarray(out[:, form, 5:5 + dim]), nrm)
    elif kind == "star":
        for form in range(3):
            assert_bits_equal(np.ascontiguousarray(out[:, form, 0]), ref)
    else:
        dist, proj = ref
        for form in range(3):
            assert_bits_equal(np.ascontiguousarray(out[:, form, 0]), dist)
        for form in range(2):  # dirichlet_dist_step returns the distance alone
            assert_bits_equal(np.ascontiguousarray(out[:, form, 1:1 + dim]), proj)


def _fired_declined(counts, what):
    s = _lib.GEO_COUNT[what]
    return int(counts[:, s].sum()), int(counts[:, s + 1].sum())


# (scene, schedule, kind): the regimes asserted (per mask set) and the shortcuts that must fire and decline
R, S, D = "ray", "star", "dirichlet"
CASES = [
    ("lshape", 0, R), ("box", 0, R), ("lshape", 0, S), ("lshape_origin", 0, S), ("lshape_origin", NO_STAR, S),
    ("karman", 0, R), ("karman", 0, S), ("karman", NO_STAR, S),
    ("engine", 0, R), ("engine", 0, S), ("engine_flip", 0, R), ("engine_flip", 0, S),
    ("engine", GG, R), ("engine", GG, S),
    ("gear", GG, R), ("gear", GG, S), ("gear_prism", GG, R), ("gear_prism", GG, S),
    ("obstacle", 0, D), ("obstacle", NO_DIR, D), ("circle4096", 0, D),
    ("cube", 0, R), ("cube", 0, S), ("open_box", 0, R), ("open_box", 0, S), ("cube_dirichlet", 0, D),
    ("lprism", 0, R), ("lprism", 0, S), ("cube7", GG, R), ("cube7", GG, S),
]


def _expect_regimes(name, sched, kind, plan, tags, n_prims):
    """assertion 6, regimes: the tags each mask set must show, from how the scene was planned"""
    L = _lib
    seen = {m: set(int(t) for t in np.unique(tags[m])) for m in tags}
    if kind == R:
        small = n_prims <= (24 if plan["dim"] == 2 else 16)
        tree = plan["geom_global"] and plan["ptree"] > 0
        multi = L.GEO_RAY_TREE if tree else (L.GEO_RAY_LANE_SCAN if small else L.GEO_RAY_LIST)
        for m in ("all", "alternating", "two"):
            assert seen[m] == {multi}, (m, seen[m])
        assert seen["one"] == {L.GEO_RAY_TREE if tree else L.GEO_RAY_SOLO}
        if sched & GG:
            assert plan["geom_global"] == 1 and tree
        if name in ("lshape", "box", "cube", "open_box"):
            assert small and not plan["geom_global"]
    elif kind == S:
        base = {m: {t & 0xFF for t in seen[m]} - {L.GEO_STAR_NONE} for m in seen}
        scan = L.GEO_STAR_TREE if (plan["geom_global"] and plan["stree"] > 0) else L.GEO_STAR_GROUPS
        if plan["n_silhouettes"] == 0:
            return
        if plan["star_grid"]:
            assert not sched & NO_STAR
            assert L.GEO_STAR_SOLO_CELL in base["one"] and L.GEO_STAR_CELL_LISTS in base["all"]
            assert scan in base["all"] and scan in base["one"]  # points outside the grid
            assert any(t & L.GEO_STAR_MIXED for t in seen["all"]), "no wave mixed lanes inside and outside the grid"
        else:
            for m in base:
                assert base[m] == {scan}, (m, base[m])
        if name == "karman":
            assert bool(plan["star_grid"]) == (sched == 0) and not plan["geom_global"]
        if name in ("gear", "gear_prism"):  # the silhouette-group hierarchy, 2D and 3D
            assert plan["stree"] > 0 and scan == L.GEO_STAR_TREE and not plan["star_grid"]
    else:
        if plan["dir_grid"]:
            assert not sched & NO_DIR and plan["dim"] == 2
            for m in seen:
                assert seen[m] == {L.GEO_DIR_GRID, L.GEO_DIR_GRID_MISS}, (m, seen[m])
        else:
            scan = L.GEO_DIR_TREE if plan["dtree"] > 0 else L.GEO_DIR_CULLED
            assert seen["one"] == {L.GEO_DIR_SOLO}
            for m in ("all", "alternating", "two"):
                assert seen[m] == {scan}, (m, seen[m])
        if name == "obstacle":
            assert bool(plan["dir_grid"]) == (sched == 0)
        if name == "circle4096":  # its cell lists are too long for a grid: the hierarchy, or one lane's scan
            assert plan["dtree"] > 0 and not plan["dir_grid"]


# the shortcuts that must have fired and declined, and where
MUST_FIRE = {
    ("karman", R): ["ray_box", "ray_prefilter"], ("engine", R): ["ray_box", "ray_prefilter"],
    ("cube7", R): ["ray_box", "ray_prefilter"], ("lshape", R): ["ray_prefilter"], ("cube", R): ["ray_prefilter"],
    ("karman", S): ["ball_box", "cone", "star_early"], ("engine", S): ["ball_box", "cone", "star_early"],
    ("open_box", S): ["star_early"], ("lprism", S): ["ball_box", "cone", "star_early"],
    ("gear", R): ["ray_box", "ray_prefilter"], ("gear", S): ["ball_box", "cone", "star_early"],
    # (every candidate group of the open prism holds a boundary edge, so its cone never culls)
    ("gear_prism", R): ["ray_box", "ray_prefilter"], ("gear_prism", S): ["ball_box", "star_early"],
    ("lshape_origin", S): ["ball_box", "cone", "star_early"],
    ("obstacle", D): ["dir_box"], ("circle4096", D): ["dir_box"],
}


# silhouettePrecision 1e-3 everywhere, and once 1.25e-3: there fl(sqrt(d^2)) is still prec at the float32
# successor of prec^2 (at 1e-3 it is not), so the upper edge of silhouette_class2's band on d^2 decides
CASES = [c + (1e-3,) for c in CASES] + [("lshape_origin", 0, S, 1.25e-3)]


@pytest.mark.parametrize("name,sched,kind,prec", CASES, ids=[f"{n}-{s}-{k}-{p:g}" for n, s, k, p in CASES])
def test_probe(gpu, oracle, name, sched, kind, prec):
    items, ref = _reference(name, kind, prec)
    v, ix, kw = gc.scene(name)
    dim = v.shape[1]
    sc = gc.wos_scene(name)
    try:
        res = {m: sc.selftest_geometry(kind, items, masks, schedule=sched, silhouette_precision=prec)
               for m, masks in _masks(len(items), kind).items()}
    except WosError as e:  # a device error leaves the context unusable: nothing more runs on it
        pytest.exit(f"wos_selftest_geometry {name}/{sched}/{kind}: {e}", returncode=3)
    first = res["all"]
    plan = dict(first["plan"], dim=dim)
    summary = {"items": len(items), "plan": first["plan"],
               "tags": {m: {str(t): int(c) for t, c in zip(*np.unique(r["tags"], return_counts=True))} for m, r in res.items()},
               "sound_bits_set": int(np.count_nonzero(first["sound"])),
               "fired_declined": {w: _fired_declined(first["counts"], w) for w in _lib.GEO_COUNT},
               "class2_012": [int(first["counts"][:, _lib.GEO_C_CLASS + k].sum()) for k in range(3)]}
    key = f"{name}/{sched}/{kind}" + ("" if prec == 1e-3 else f"/prec={prec:g}")
    print(f"{key}: {summary}")
    gc.record("probe", key, summary)
    for m, r in res.items():
        assert r["plan"] == first["plan"]
        _check_forms(kind, dim, r["out"], ref)                                   # 1, 2 (and with them 3)
        np.testing.assert_array_equal(r["sound"], first["sound"], err_msg=m)      # 3
        np.testing.assert_array_equal(r["counts"], first["counts"], err_msg=m)
        bad = np.flatnonzero(r["sound"])
        assert bad.size == 0, f"{m}: soundness bits {np.unique(r['sound'][bad])} at items {bad[:8]}: {items[bad[:8]]}"  # 5
    if kind == D:                                                                 # 4
        d, _, _, cp = sc.query(items, which="dirichlet", closest=True)
        assert_bits_equal(d, ref[0])
        assert_bits_equal(cp, ref[1])
    _expect_regimes(name, sched, kind, plan, {m: r["tags"] for m, r in res.items()}, len(ix))  # 6
    for what in MUST_FIRE.get((name, kind), []):
        fired, declined = _fired_declined(first["counts"], what)
        assert fired > 0 and declined > 0, f"{what}: fired {fired}, declined {declined}"
    if (name, kind) in (("karman", S), ("lshape_origin", S)):
        assert all(c > 0 for c in summary["class2_012"]), summary["class2_012"]
    if kind == S and plan["star_grid"]:
        assert first["counts"][:, _lib.GEO_C_CELL_LEN].max() > 0
    sc.close()


def test_refusals(gpu):
    L = _lib.load()
    sc = gc.wos_scene("box")
    items = np.zeros((2, 5), np.float32)
    items[:, 2] = 1.0
    out = np.zeros((2, 3, 8), np.float32)
    tags, sound, counts = np.zeros(2, np.int32), np.zeros(2, np.uint32), np.zeros((2, 16), np.uint32)
    masks = np.array([3], np.uint64)

    def call(scene=sc._h, kind=_lib.GEO_RAY, it=items.ctypes.data, n=2, m=masks, o=out.ctypes.data):
        rc = L.wos_selftest_geometry(scene, 0, 1e-3, 1e-3, kind, it, n, m.ctypes.data if m is not None else None,
                                     0 if m is None else m.size, o, tags.ctypes.data, sound.ctypes.data,
                                     counts.ctypes.data, None)
        return rc, L.wos_last_error().decode()

    assert call()[0] == 0
    for bad in (dict(scene=None), dict(it=None), dict(m=None), dict(o=None)):
        rc, msg = call(**bad)
        assert rc == INVALID and "null argument" in msg, (bad, rc, msg)
    rc, msg = call(kind=7)
    assert rc == INVALID and "kind must be" in msg and "got 7" in msg
    rc, msg = call(kind=_lib.GEO_DIRICHLET)
    assert rc == INVALID and "no Dirichlet boundary" in msg
    for m in (np.array([1], np.uint64), np.array([7], np.uint64), np.array([1, 2, 4], np.uint64)):
        rc, msg = call(m=m)
        assert rc == INVALID and "set bits sum to" in msg and "n = 2" in msg
    rc, msg = call(n=0, m=np.zeros(0, np.uint64))
    assert rc == 0
    with pytest.raises(WosError, match="kind must be"):
        sc.selftest_geometry(9, items, masks)
    sc.close()
