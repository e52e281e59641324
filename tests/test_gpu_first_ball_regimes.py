"""Full solves against the oracle at the walk counts where wos_first_ball_kernel changes its
code: points per wave (4, 3, 2, 1), the four shuffles, the packed 3D one-pass shuffle, the pair
loop's passes, LDS-staged and global jump constants (tests/test_lhs_cpu.py asserts that the
sweep of tests/lhs_cases.py visits every such plan and both sides of every switch).

The query points spell out every estimated / unestimated pattern of a wave's pack, then a tail
that leaves the last pack -- and the last queue grab -- running past n; point indices start at 3
with stride 7.  p, grad p, n_est, steps and the counters must equal the oracle's bit for bit
(test_gpu_parity._compare).  The twins run the other first-ball instantiations (four channels,
robust float semantics), the replay cases the indices whose shuffle draws reject, and the last
two the jump table's regrowth and the refusal beyond the LDS budget."""
import numpy as np
import pytest

import channel_cases as cc
import lhs_cases
import objparse
import wos_amd
from test_gpu_parity import _compare, _pair, assert_bits_equal
from wos_amd import WosScene, selftest_lhs_plan, solver_params, workloads

pytestmark = pytest.mark.gpu

INDEX_BASE, INDEX_STRIDE = 3, 7


@pytest.fixture(scope="module")
def scenes(gpu, oracle):
    """dim -> (cfg, oracle scene, GPU scene, estimated points, unestimated points)"""
    out = {}
    cfg = workloads.karman_config(n_walks=128, n_points=2048)
    osc, sc = _pair(cfg, oracle)
    c, r = workloads.karman_obstacle(workloads.scene_size(workloads.KARMAN_OBJ))
    # (inside the obstacle, outside the domain: the unestimated points of test_gpu_parity.py)
    unest = np.array([[c[0], c[1]], [-100.0, -100.0], [c[0] + r * 0.5, c[1]], [100.0, 50.0]], np.float32)
    pts = cfg["points"]
    # away from the channel walls: the long near-wall walks are test_lone_walks_bit_exact's
    est = np.ascontiguousarray(pts[0.6035 - np.abs(pts[:, 1]) > 0.05][:80])
    out[2] = (cfg, osc, sc, est, unest)
    cfg = workloads.cube_config(res=5, n_walks=64)
    osc, sc = _pair(cfg, oracle, dim=3)
    unest = np.array([[2.0, 0.0, 0.0], [0.0, -3.0, 0.5]], np.float32)
    out[3] = (cfg, osc, sc, np.ascontiguousarray(cfg["points"][:80]), unest)
    yield out
    for v in out.values():
        v[2].close()


def pattern_points(P, est, unest, short=False):
    """Every estimated / unestimated pattern of a pack of P points one after another (slot s
    of pack k is point k P + s: the kernel hands points out in order from 0), then one more
    estimated point; P = 1: estimated and unestimated points mixed.  (points, estimated mask)"""
    if P == 1:
        mask = [1, 0, 1, 1, 0] if short else [1, 0, 1, 1, 0, 0, 1, 1, 1, 0, 1]
    else:
        mask = [(m >> s) & 1 for m in range(1 << P) for s in range(P)] + [1]
    pts, ne, nu = [], 0, 0
    for m in mask:
        if m:
            pts.append(est[ne])
            ne += 1
        else:
            pts.append(unest[nu % len(unest)])
            nu += 1
    return np.ascontiguousarray(np.stack(pts), np.float32), np.array(mask, bool)


def _case_points(scenes, dim, nw, anti):
    plan = selftest_lhs_plan(lhs_cases.n_pairs_of(nw, anti), dim)
    P, grab = plan["points_per_wave"], plan["point_grab"]
    _, _, _, est, unest = scenes[dim]
    pts, mask = pattern_points(P, est, unest, short=nw >= 384)
    n = pts.shape[0]
    # the last pack and the last queue grab run past n
    assert n % (grab * P) != 0 and (P == 1 or n % P != 0)
    return pts, mask


def _cfg(scenes, dim, nw, anti=True, **solver):
    base = scenes[dim][0]
    s = dict(base["solver"], nWalks=nw, **solver)
    if not anti:
        s["disableGradientAntitheticVariates"] = True
    return {"solver": s, "output": base["output"]}


@pytest.mark.parametrize("dim,nw,anti", lhs_cases.sweep_cases())
def test_regime_bit_exact(gpu, oracle, scenes, dim, nw, anti):
    _, osc, sc, _, _ = scenes[dim]
    pts, mask = _case_points(scenes, dim, nw, anti)
    _, _, st = _compare(oracle, osc, sc, _cfg(scenes, dim, nw, anti), pts, index_base=INDEX_BASE,
                        index_stride=INDEX_STRIDE)
    assert st["points_estimated"] == int(mask.sum())  # the patterns are the intended ones
    assert st["walks_recorded"] > 0


@pytest.mark.parametrize("nw", [34, 130])
@pytest.mark.parametrize("dim", [2, 3])
def test_four_channel_twin(gpu, scenes, dim, nw):
    """wos_first_ball_kernel<DIM, false, 4>: each channel of the four-channel solve equals
    the single-channel solve of the same source, GPU against GPU."""
    cfg, _, sc1, _, _ = scenes[dim]
    pts, _ = _case_points(scenes, dim, nw, True)
    prm = solver_params(_cfg(scenes, dim, nw)["solver"], cfg["output"])
    v, ix = objparse.load(cfg["obj"], dim)
    src4 = cc.channels(cfg["source"], 4)
    sc4 = WosScene(v, ix, src4, float(cfg["scene"]["absorptionCoeff"]), watertight=True)
    try:
        p4, g4, st4, ne4, sp4 = sc4.solve(pts, prm, counts=True, index_base=INDEX_BASE, index_stride=INDEX_STRIDE)
        assert p4.shape == (4, pts.shape[0])
        for k in range(4):
            sc1.set_source(src4[k])
            p1, g1, st1, ne1, sp1 = sc1.solve(pts, prm, counts=True, index_base=INDEX_BASE, index_stride=INDEX_STRIDE)
            assert_bits_equal(p4[k], p1)
            assert_bits_equal(g4[k], g1)
            np.testing.assert_array_equal(ne4, ne1)
            np.testing.assert_array_equal(sp4, sp1)
            assert st4["walk_steps"] == st1["walk_steps"] and st4["rejection_iters"] == st1["rejection_iters"]
    finally:
        sc1.set_source(cfg["source"])
        sc4.close()


@pytest.mark.parametrize("nw", [34, 130])
@pytest.mark.parametrize("dim", [2, 3])
def test_robust_twin(gpu, scenes, dim, nw):
    """wos_first_ball_kernel<DIM, true>: on karman and the unit cube (mu R <= 60) the robust
    solve equals the default one bit for bit (as test_robust_identical_below_threshold)."""
    cfg, _, sc, _, _ = scenes[dim]
    pts, _ = _case_points(scenes, dim, nw, True)
    kw = dict(counts=True, index_base=INDEX_BASE, index_stride=INDEX_STRIDE)
    p0, g0, st0, ne0, sp0 = sc.solve(pts, solver_params(_cfg(scenes, dim, nw)["solver"], cfg["output"]), **kw)
    p1, g1, st1, ne1, sp1 = sc.solve(pts, solver_params(_cfg(scenes, dim, nw, robustFloatSemantics=True)["solver"],
                                                        cfg["output"]), **kw)
    assert_bits_equal(p0, p1)
    assert_bits_equal(g0, g1)
    np.testing.assert_array_equal(ne0, ne1)
    np.testing.assert_array_equal(sp0, sp1)
    assert st0["walk_steps"] == st1["walk_steps"] > 0 and st0["rejection_iters"] == st1["rejection_iters"]


@pytest.mark.parametrize("nstrat,dims", sorted(lhs_cases.REPLAY))
def test_replay_solves_bit_exact(gpu, oracle, scenes, nstrat, dims):
    """Three points whose middle index rejects in its shuffle draws (tests/test_lhs_cpu.py):
    in a pack one slot replays its partners and the others do not."""
    dim = dims + 1
    _, osc, sc, est, _ = scenes[dim]
    for idx in lhs_cases.REPLAY[(nstrat, dims)]:
        _compare(oracle, osc, sc, _cfg(scenes, dim, nstrat), est[:3], index_base=idx - 1, index_stride=1)


def test_jump_table_regrowth(gpu, oracle, scenes):
    """2100 walks draw 4200 stratified values and as many partners: past the jump table's
    first 4096 entries, so the table is rebuilt; the solve equals the oracle, and the 128-walk
    solve made before it repeats bit for bit on the new table."""
    _, osc, sc, est, _ = scenes[2]
    wos_amd.release_caches(0)  # the table starts over, whatever ran before in this process
    before = _compare(oracle, osc, sc, _cfg(scenes, 2, 128), est[:16])
    _compare(oracle, osc, sc, _cfg(scenes, 2, 2100), est[:2], index_base=INDEX_BASE, index_stride=INDEX_STRIDE)
    p, g, st = sc.solve(est[:16], solver_params(_cfg(scenes, 2, 128)["solver"], scenes[2][0]["output"]))
    assert_bits_equal(p, before[0])
    assert_bits_equal(g, before[1])
    assert st["walk_steps"] == before[2]["walk_steps"]


def test_walks_beyond_lds_budget_refused(gpu, oracle, scenes):
    """The smallest nWalks whose four waves of stratified samples exceed the dynamic LDS budget
    (from wos_selftest_lhs_plan's formula) returns WOS_E_CAPACITY naming the first-ball kernel;
    the solve after it still equals the solve before.  Two walks fewer -- the most that fit --
    still solve, bit for bit with the oracle."""
    cfg, osc, sc, est, _ = scenes[2]

    def fits(n_pairs):
        plan = selftest_lhs_plan(n_pairs, 2)
        return 4 * plan["wave_lds_bytes"] <= plan["lds_budget"]

    lo, hi = 1, 1 << 16  # fits(lo), not fits(hi)
    assert fits(lo) and not fits(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if fits(mid) else (lo, mid)
    prm = solver_params(_cfg(scenes, 2, 128)["solver"], cfg["output"])
    p0, g0, st0 = sc.solve(est[:16], prm)
    with pytest.raises(wos_amd.WosError, match=r"\(-4\).*first-ball kernel"):
        sc.solve(est[:2], solver_params(_cfg(scenes, 2, 2 * hi)["solver"], cfg["output"]))
    _compare(oracle, osc, sc, _cfg(scenes, 2, 2 * lo), est[:2], index_base=INDEX_BASE, index_stride=INDEX_STRIDE)
    p1, g1, st1 = sc.solve(est[:16], prm)
    assert_bits_equal(p1, p0)
    assert_bits_equal(g1, g0)
    assert st1["walk_steps"] == st0["walk_steps"] > 0
