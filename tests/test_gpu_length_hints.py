"""Length hints (include/wos.h wos_set_length_hints; DESIGN.md, Length hints): the second solve of the
same walks starts the walks its predecessor found long first, in express waves.  A scheduling hint only,
so every case is "bit-identical to the solve without it" -- plus the getter's word that express walks
were in fact started (or, for a stale or foreign list, that none were).

Scenes: the ring of points 2e-3 outside karman's cylinder at roulette threshold 0.01 (walks of several
hundred steps, tests/test_gpu_tape.py) and the karman points themselves at 32 walks; hint_min and
express_min are lowered so that a few hundred points exercise what config B does with 8.4 M walks."""
import numpy as np
import pytest

import variance_cases as vc
from test_gpu_parity import assert_bits_equal

pytestmark = pytest.mark.gpu

COUNTERS = ("walk_steps", "wasted_steps", "walks_recorded", "walks_escaped", "walks_max_length", "walks_rr",
            "walks_dirichlet", "points_estimated", "rejection_iters")
OFF = 0x40  # WOS_SCHED_NO_LENGTH_HINTS


def _ring(radius_off=2e-3, n=300):
    from wos_amd import workloads
    ctr, r = workloads.karman_obstacle(workloads.scene_size(workloads.KARMAN_OBJ))
    th = np.linspace(0, 2 * np.pi, n, endpoint=False)
    return np.stack([ctr[0] + (r + radius_off) * np.cos(th), ctr[1] + (r + radius_off) * np.sin(th)], 1)


def _case(name):
    from wos_amd import workloads
    if name == "ring":
        c = vc.case("karman_w40")
        c["solver"] = dict(c["solver"], russianRouletteThreshold=0.01)
        cfg = workloads.karman_config(n_walks=40)
        c["points"] = np.ascontiguousarray(np.concatenate([cfg["points"][:64], cfg["points"][6241:6242], _ring()]),
                                           np.float32)
    else:  # karman's own points (two of them outside the domain), 32 walks, 2 walk-kernel blocks and a ragged one
        c = vc.case("karman_w40")
        cfg = workloads.karman_config(n_walks=32)
        c["solver"] = dict(cfg["solver"])
        c["points"] = np.ascontiguousarray(np.concatenate([cfg["points"][:330], cfg["points"][6241:6242],
                                                           vc.karman_points()[-10:]]), np.float32)
    return c


def _scene(c, absorption=None):
    from wos_amd import WosScene
    return WosScene(c["vertices"], c["prims"], c["source"], c["absorption"] if absorption is None else absorption,
                    watertight=True, **c["kw"])


def _prm(c, schedule=0, seed=None, **flags):
    from wos_amd import solver_params
    return solver_params(dict(c["solver"], **flags), c["output"], seed=seed, schedule=schedule)


def _solve(sc, c, prm, pts=None, **idx):
    import torch
    from wos_amd import length_hint_stats
    x = torch.from_numpy(c["points"] if pts is None else pts).cuda()
    p, g, pv, gv, st, n, steps = sc.solve(x, prm, variance=True, counts=True, **idx)
    torch.cuda.synchronize()
    return {"p": p.cpu().numpy(), "g": g.cpu().numpy(), "pv": pv.cpu().numpy(), "gv": gv.cpu().numpy(),
            "n": n.cpu().numpy(), "steps": steps.cpu().numpy(), "st": st, "hint": length_hint_stats(0)}


def _same(a, b, msg=""):
    for k in ("p", "g", "pv", "gv"):
        assert a[k].shape == b[k].shape, (msg, k)
        assert_bits_equal(a[k].ravel(), b[k].ravel())
    for k in ("n", "steps"):
        np.testing.assert_array_equal(a[k], b[k], err_msg=f"{msg} {k}")
    for k in COUNTERS:
        assert a["st"][k] == b["st"][k], (msg, k)


@pytest.fixture(autouse=True)
def _tuning(gpu):
    """A cold workspace and the small scenes' thresholds: list walks of >= 8 steps, express from 16."""
    from wos_amd import release_caches, set_length_hints
    release_caches(0)
    set_length_hints(8, 16, 2, -1, 0)
    yield
    set_length_hints()


_REF = {}


def _ref(name, oracle=None):
    """The case without hints (computed once, never changed) and the CPU oracle on every 7th point."""
    if name not in _REF:
        c = _case(name)
        sc = _scene(c)
        r = _solve(sc, c, _prm(c, OFF))
        sc.close()
        assert r["hint"] == {"claimed": 0, "overflow": 0, "listed": 0, "express": 0}
        _REF[name] = [c, r, None]
    if oracle is not None and _REF[name][2] is None:
        c = _REF[name][0]
        osc = oracle.OracleScene(c["vertices"], c["prims"], c["source"], c["absorption"], watertight=True, **c["kw"])
        _REF[name][2] = oracle.solve(osc, oracle.make_params(c["solver"], c["output"]),
                                     np.ascontiguousarray(c["points"][::7]), index_base=0, index_stride=7)
    return _REF[name]


def _warm(sc, c, prm, **kw):
    """cold then hinted solve; the hinted one did start express walks"""
    cold = _solve(sc, c, prm, **kw)
    assert cold["hint"]["claimed"] == 0 and cold["hint"]["express"] == 0 and cold["hint"]["listed"] > 0, cold["hint"]
    hot = _solve(sc, c, prm, **kw)
    assert hot["hint"]["express"] > 0 and hot["hint"]["claimed"] == hot["hint"]["express"], hot["hint"]
    return cold, hot


# ---- 1. hinted == unhinted ------------------------------------------------------------------------
@pytest.mark.parametrize("prio", [0, 3])
@pytest.mark.parametrize("per_wave", [1, 4])
@pytest.mark.parametrize("name", ["ring", "karman"])
def test_hinted_equals_unhinted(gpu, oracle, name, per_wave, prio):
    from wos_amd import set_length_hints
    c, ref, (po, go, no, so, _) = _ref(name, oracle)
    set_length_hints(8, 16, per_wave, -1, prio)
    sc = _scene(c)
    cold, hot = _warm(sc, c, _prm(c))
    sc.close()
    print(name, per_wave, prio, hot["hint"])
    _same(cold, ref, "cold")
    _same(hot, ref, "hinted")
    assert_bits_equal(hot["p"][::7], po)
    assert_bits_equal(hot["g"][::7].ravel(), go.ravel())
    np.testing.assert_array_equal(hot["n"][::7], no)
    np.testing.assert_array_equal(hot["steps"][::7], so)


# ---- 2. stale and foreign lists -------------------------------------------------------------------
def test_stale_and_foreign_hints_are_ignored(gpu):
    c, ref, _ = _ref("ring")
    sc = _scene(c)
    prm = _prm(c)
    _, hot = _warm(sc, c, prm)
    _same(hot, ref)

    def foreign(msg, scene=sc, pts=None, idx=None, **flags):
        idx = idx or {}
        got = _solve(scene, c, _prm(c, **flags), pts=pts, **idx)
        assert got["hint"]["claimed"] == 0 and got["hint"]["express"] == 0, (msg, got["hint"])
        _same(got, _solve(scene, c, _prm(c, OFF, **flags), pts=pts, **idx), msg)

    # the same number of other points: only the device's checksum can tell
    other = c["points"].copy()
    other[65:] = _ring(2.5e-3).astype(np.float32)
    foreign("other points", pts=other)
    assert _solve(sc, c, prm, pts=other)["hint"]["claimed"] > 0  # (their own list is used)
    _solve(sc, c, prm)  # back to the first points: cold
    assert _solve(sc, c, prm)["hint"]["claimed"] > 0
    # the host key, field by field as the solve sees it
    foreign("seed", seed=12345)
    _solve(sc, c, prm)
    foreign("index_base", idx={"index_base": 5})
    _solve(sc, c, prm)
    foreign("index_stride", idx={"index_stride": 3})
    _solve(sc, c, prm)
    foreign("maxWalkLength", maxWalkLength=100)
    _solve(sc, c, prm)
    sc2 = _scene(c, absorption=300.0)
    foreign("absorption", scene=sc2)
    sc2.close()
    # and the first set again: cold, then hinted, identical
    _, hot = _warm(sc, c, prm)
    _same(hot, ref, "back")
    sc.close()


# ---- 3. a list too small ----------------------------------------------------------------------------
def test_list_overflow_is_counted(gpu):
    from wos_amd import set_length_hints
    c, ref, _ = _ref("ring")
    set_length_hints(1, 16, 2, 8, 0)
    sc = _scene(c)
    cold = _solve(sc, c, _prm(c))
    assert cold["hint"]["listed"] == 8 and cold["hint"]["overflow"] > 1000, cold["hint"]
    hot = _solve(sc, c, _prm(c))
    # a list that overflowed is never used (include/wos.h): no express walks, and the overflow counted again
    assert hot["hint"]["claimed"] == hot["hint"]["express"] == 0 and hot["hint"]["overflow"] > 1000, hot["hint"]
    sc.close()
    _same(cold, ref)
    _same(hot, ref)


# ---- 4. the reference's fresh Scene per projection ------------------------------------------------
def test_fresh_scene_per_projection(gpu):
    c, ref, _ = _ref("ring")
    sc = _scene(c)
    cold = _solve(sc, c, _prm(c))
    sc.close()
    sc = _scene(c)
    hot = _solve(sc, c, _prm(c))
    sc.close()
    assert cold["hint"]["claimed"] == 0 and hot["hint"]["claimed"] == hot["hint"]["express"] > 0, hot["hint"]
    _same(hot, ref)


# ---- 5. two solves in flight ------------------------------------------------------------------------
@pytest.mark.parametrize("two_streams", [False, True])
def test_two_solves_in_flight(gpu, two_streams):
    import torch
    from wos_amd import length_hint_stats
    c, ref, _ = _ref("ring")
    sc = _scene(c)
    x = torch.from_numpy(c["points"]).cuda()
    streams = [torch.cuda.Stream(), torch.cuda.Stream() if two_streams else None]
    streams[1] = streams[1] or streams[0]
    torch.cuda.synchronize()
    outs = [sc.solve(x, _prm(c), counts=True, sync=False, stream=streams[k % 2]) for k in range(3)]
    stats = [sc.solve_stats(o[2]["ticket"]) for o in outs]
    torch.cuda.synchronize()
    h = length_hint_stats(0)
    assert h["claimed"] == h["express"] > 0, h
    sc.close()
    for (p, g, _, n, steps), st in zip(outs, stats):
        assert_bits_equal(p.cpu().numpy(), ref["p"])
        assert_bits_equal(g.cpu().numpy().ravel(), ref["g"].ravel())
        np.testing.assert_array_equal(n.cpu().numpy(), ref["n"])
        np.testing.assert_array_equal(steps.cpu().numpy(), ref["steps"])
        for k in COUNTERS:
            assert st[k] == ref["st"][k], k


# ---- 6. wos_release_caches drops the list ----------------------------------------------------------
def test_release_caches_drops_hints(gpu):
    from wos_amd import release_caches
    c, ref, _ = _ref("ring")
    sc = _scene(c)
    _warm(sc, c, _prm(c))
    release_caches(0)
    _, hot = _warm(sc, c, _prm(c))  # cold again (asserted), then hinted
    sc.close()
    _same(hot, ref)


# ---- 7. the workspace's other users -----------------------------------------------------------------
def test_tape_and_bvc_after_hinted_solve(gpu, oracle):
    import bvc_cases
    import test_gpu_bvc
    import test_gpu_tape
    c, ref, _ = _ref("ring")
    sc = _scene(c)
    _warm(sc, c, _prm(c))
    t = vc.case("karman_w2")
    test_gpu_tape._record_replay_equals_fresh(t, test_gpu_tape._prm(t), msg="tape after hints")
    test_gpu_bvc.test_bvc_bit_exact(gpu, oracle, bvc_cases.NAMES[0])
    got = _solve(sc, c, _prm(c))  # whatever the others left of the list: the same result
    sc.close()
    assert got["hint"]["claimed"] == got["hint"]["express"]
    _same(got, ref)


# ---- 8. degenerate batches --------------------------------------------------------------------------
def test_degenerate_batches(gpu):
    from wos_amd import set_length_hints, workloads
    c, _, _ = _ref("ring")
    sc = _scene(c)
    ctr, r = workloads.karman_obstacle(workloads.scene_size(workloads.KARMAN_OBJ))
    outside = np.ascontiguousarray(np.concatenate([_ring(-0.5 * r, 70), _ring(-0.9 * r, 7)]), np.float32)
    for msg, pts in (("all outside", outside), ("one point", c["points"][64:65])):
        off = _solve(sc, c, _prm(c, OFF), pts=pts)
        for k in range(3):
            got = _solve(sc, c, _prm(c), pts=pts)
            assert got["hint"]["claimed"] == got["hint"]["express"], (msg, got["hint"])
            _same(got, off, msg)
        if msg == "all outside":
            assert got["st"]["points_estimated"] == 0 and got["hint"]["listed"] == 0
    # no walk long enough for the list: the next solve builds an empty express list
    set_length_hints(60000, 60000, 2, -1, 0)
    off = _solve(sc, c, _prm(c, OFF))
    for k in range(2):
        got = _solve(sc, c, _prm(c))
        assert got["hint"] == {"claimed": 0, "overflow": 0, "listed": 0, "express": 0}
        _same(got, off, "empty list")
    sc.close()
