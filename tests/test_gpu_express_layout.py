"""Express layout (include/wos.h wos_set_express_layout; DESIGN.md, Length hints): which wave starts which express
walk -- a wave each for the longest (solo_min), the others striped or in blocks, the express wave rotating or pinned
to the workgroup's lowest SIMD.  Scheduling only, so every case is "bit-identical to the solve without hints", with
the getter's word that every entry of the express list was started exactly as often as it is listed.

The scenes, the unhinted references and the helpers are tests/test_gpu_length_hints.py's; tuning 8 / 16 as there."""
import numpy as np
import pytest

import test_gpu_length_hints as lh

pytestmark = pytest.mark.gpu

LAYOUTS = [(solo_min, stripe, placement) for solo_min in (0, 1, 24) for stripe in (0, 1) for placement in (0, 1)]


@pytest.fixture(autouse=True)
def _tuning(gpu):
    from wos_amd import release_caches, set_express_layout, set_length_hints
    release_caches(0)
    set_length_hints(8, 16, 2, -1, 0)
    set_express_layout()
    yield
    set_length_hints()
    set_express_layout()


def _workgroups(n_points, n_walks=40):
    """of the walk grid: one per 64 walks ("ring" runs 40 to a point; so few points never reach the resident-block cap)"""
    return (n_points * n_walks + 63) // 64


def _check_tier(tier, hint, per_wave, solo_min, n16, n24, wg):
    """The solo tier the build kernel formed (wos_express_layout_stats) against the walks themselves: n16 and n24 are
    the walks of >= 16 and >= 24 steps, each counted by a solve that lists exactly those, wg the walk grid's
    workgroups.  The express candidates are the n16 walks, so under solo_min = 1 all of them are the tier's; one claim
    per workgroup cuts the tier to wg entries, then the list to what the other claims hold."""
    express, solo, below = hint["express"], tier["solo"], tier["claims_below"]
    want_solo = min({0: 0, 1: n16, 24: n24}[solo_min], wg)
    assert solo == want_solo, (tier, hint, n16, n24, wg)
    assert express == min(n16, want_solo + (wg - want_solo) * per_wave), (tier, hint, n16, n24, wg)
    assert below == (express - solo + per_wave - 1) // per_wave and solo + below <= wg, (tier, hint, wg)


@pytest.mark.parametrize("per_wave", [1, 4, 64])
@pytest.mark.parametrize("name", ["ring", "karman"])
def test_every_layout_equals_unhinted(gpu, name, per_wave):
    from wos_amd import express_layout_stats, set_express_layout, set_length_hints
    c, ref, _ = lh._ref(name)
    set_length_hints(8, 16, per_wave, -1, 0)
    sc = lh._scene(c)
    prm = lh._prm(c)
    cold, hot = lh._warm(sc, c, prm)
    lh._same(cold, ref, "cold")
    lh._same(hot, ref, "default layout")
    # the walks of >= 16 and of >= 24 steps, counted: solves that list those alone; then one that lists from 8 again
    set_length_hints(16, 16, per_wave, -1, 0)
    n16 = lh._solve(sc, c, prm)["hint"]["listed"]
    set_length_hints(24, 24, per_wave, -1, 0)
    n24 = lh._solve(sc, c, prm)["hint"]["listed"]
    set_length_hints(8, 16, per_wave, -1, 0)
    lh._solve(sc, c, prm)
    wg = _workgroups(c["points"].shape[0], 40 if name == "ring" else 32)
    assert 0 < n24 < n16, (n24, n16)
    for solo_min, stripe, placement in LAYOUTS:
        set_express_layout(solo_min, stripe, placement)
        got = lh._solve(sc, c, prm)  # the list its predecessor left: hinted, whatever layout that one ran with
        tier = express_layout_stats(0)
        print(name, per_wave, (solo_min, stripe, placement), got["hint"], tier)
        assert got["hint"]["express"] > 0 and got["hint"]["claimed"] == got["hint"]["express"], got["hint"]
        _check_tier(tier, got["hint"], per_wave, solo_min, n16, n24, wg)
        lh._same(got, ref, f"layout {solo_min} {stripe} {placement}")
    sc.close()


@pytest.mark.parametrize("per_wave", [1, 4, 64])
@pytest.mark.parametrize("pts", ["first40", "last3"])
def test_one_round_cap_truncates_tier_and_list(gpu, pts, per_wave):
    """A walk grid of a few workgroups: one claim per workgroup holds fewer walks than are long, so the build kernel
    cuts the solo tier, then the list.  first40: the first 40 points of "ring" (25 workgroups); last3: three points of
    the ring itself, 2 workgroups and walks of several hundred steps, so under solo_min = 1 the tier is cut for sure."""
    from wos_amd import set_express_layout, set_length_hints
    c, _, _ = lh._ref("ring")
    p = np.ascontiguousarray(c["points"][:40] if pts == "first40" else c["points"][-3:])
    wg = _workgroups(len(p))
    set_length_hints(8, 16, per_wave, -1, 0)
    sc = lh._scene(c)
    off = lh._solve(sc, c, lh._prm(c, lh.OFF), pts=p)
    prm = lh._prm(c)
    cold, hot = lh._warm(sc, c, prm, pts=p)
    lh._same(cold, off, "cold")
    lh._same(hot, off, "default layout")
    for solo_min, stripe, placement in LAYOUTS:
        set_express_layout(solo_min, stripe, placement)
        got = lh._solve(sc, c, prm, pts=p)
        h = got["hint"]
        print(pts, wg, per_wave, (solo_min, stripe, placement), h)
        assert h["express"] > 0 and h["claimed"] == h["express"], h
        # one claim per workgroup: a walk each in the solo tier, per_wave below it
        assert h["express"] <= wg * (1 if solo_min == 1 else per_wave), (h, wg)
        if pts == "last3" and solo_min == 1:
            assert h["listed"] > wg and h["express"] == wg, (h, wg)  # more long walks than workgroups: cut
        lh._same(got, off, f"layout {solo_min} {stripe} {placement}")
    sc.close()


def test_simd_ids(gpu):
    from wos_amd import selftest_simd_ids
    ids, raw = selftest_simd_ids(0)
    print("SIMD of waves 0..3 of one workgroup:", ids, "hardware id registers:", [hex(r) for r in raw])
    assert len(ids) == 4 and all(0 <= s <= 3 for s in ids), ids
    # (which SIMD a wave lands on is the hardware's choice: nothing more to assert)
