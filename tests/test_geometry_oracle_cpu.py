"""The oracle's batched geometry exports against float64 (no GPU).

oracle_ray_hits, oracle_star_radii and oracle_dirichlet_dists (oracle/wos_oracle.h) are the
references the device probe of the walk step's geometry queries is compared with bit for bit
(test_gpu_geometry_probe.py), so they are pinned here first: the same expressions in numpy
float64 on about 2 000 random items per scene of karman, the L-shape, the cube and the L-prism
(the Dirichlet distance also on config C's circle and on a cube-in-cube, which have a Dirichlet
mesh).  The bounds are derived, not measured; the measured maxima are printed and recorded beside
them in profiles/geometry_probe.json.

Which items are compared.  A float32 scan and a float64 scan agree only where no decision of either
sits on its threshold, so an item is compared when every primitive or candidate is robustly decided
by the float64 evaluation -- a condition on the inputs, and at least half of the random items of
every scene must meet it.  With MARGIN = 1e-3:
  * rays: for every primitive |dv| (2D) or |det| (3D) exceeds kFltEps and is at least MARGIN times
    the sum of the absolute values of its terms (the cancellation in the denominator is bounded by
    1 / MARGIN; an absolute margin would drop every ray of karman, whose cylinder segments are
    4e-3 long); and the primitive is either accepted with each of t, 1 - t (2D), v, w, 1 - v - w
    (3D), d, tmax - d at least MARGIN, or rejected by one of them being at most -MARGIN; and the
    second-best accepted d lies MARGIN above the best.
  * star radii: for every candidate |dot0| and |dot1| differ from prec, d from prec, minR and maxR
    by a relative MARGIN, dot0 dot1 from 0 by MARGIN prec^2, d > prec, and the closest accepted
    candidate is closer than the next by a relative MARGIN.
  * Dirichlet distances: every item (a minimum of continuous functions has no decision to flip).

The bounds, with u = 2^-24.
  * 2D ray, d = uv / dv with uv = u0 v1 - u1 v0, u = P - o, dv = dir0 v1 - dir1 v0.  Each term of uv
    passes three roundings (the subtraction P - o, the product, the difference), each term of dv two
    (v is stored), the reciprocal and the product with it add two: to first order
    |d32 - d64| <= u (3 (|u0 v1| + |u1 v0|) / |dv| + |d| (2 + 2 (|dir0 v1| + |dir1 v0|) / |dv|)),
    and with a factor 8 / 3 over it
        |d32 - d64| <= 8 u ((|u0 v1| + |u1 v0|) / |dv| + |d| (1 + (|dir0 v1| + |dir1 v0|) / |dv|)).
  * 3D ray, d = v2 . (s x v1) / det, det = v1 . (dir x v2).  Each term of either triple product
    passes seven roundings (two subtractions forming its operands, product and difference of the
    cross product, product and two additions of the dot product), so with S(a, b, c) the sum of the
    absolute values of the six terms of a . (b x c) and the same 8 / 3
        |d32 - d64| <= 20 u (S(v2, s, v1) / |det| + |d| (1 + S(v1, dir, v2) / |det|)).
  * distances (star radius, Dirichlet distance): test_closest_point's bound 8 u max |coordinate|, the
    coordinates being those of the mesh and of the query point.
"""
import numpy as np
import pytest

import geometry_cases as gc

SCENES = ["karman", "lshape", "cube", "lprism"]
N_ITEMS = 2000
SEEDS = {"karman": 11, "lshape": 12, "cube": 13, "lprism": 14, "obstacle": 15, "cube_dirichlet": 16}


def _report(kind, name, kept, n, err, bound):
    """prints the measured maximum beside its bound (and records it: geometry_cases.record)"""
    k = int(np.argmax(err / bound))
    rec = {"items": n, "compared": kept, "max_error": float(err.max()), "worst_error": float(err[k]),
           "worst_bound": float(bound[k]), "worst_error_over_bound": float(err[k] / bound[k])}
    print(f"{kind}/{name}: {rec}")
    gc.record("float64", f"{kind}/{name}", rec)


@pytest.mark.parametrize("name", SCENES)
def test_ray_hits_against_float64(oracle, name):
    v, ix, _ = gc.scene(name)
    rng = np.random.default_rng(SEEDS[name])
    o = gc.random_points(name, N_ITEMS, rng)
    d = gc.random_dirs(v.shape[1], N_ITEMS, rng)
    tmax = gc.random_lengths(name, N_ITEMS, rng)
    found, dist, p, nrm = oracle.ray_hits(gc.oracle_scene(oracle, name), o, d, tmax)
    ref = gc.ray64(v, ix, o, d, tmax)
    keep = ref["keep"]
    assert keep.sum() * 2 >= N_ITEMS, f"{name}: only {keep.sum()} of {N_ITEMS} rays clear every margin"
    np.testing.assert_array_equal(found[keep] != 0, ref["found"][keep])
    hit = keep & ref["found"]
    assert hit.sum() > 100 and (keep & ~ref["found"]).sum() > 100
    err = np.abs(dist[hit].astype(np.float64) - ref["d"][hit])
    _report("ray", name, int(keep.sum()), N_ITEMS, err, ref["bound"][hit])
    assert (err <= ref["bound"][hit]).all()
    # the hit point lies on the ray at d, the normal is the primitive's: a few roundings each
    scale = max(float(np.abs(v).max()), float(np.abs(o).max()))
    on_ray = o[hit].astype(np.float64) + ref["d"][hit, None] * d[hit].astype(np.float64)
    assert (np.abs(p[hit] - on_ray).max(-1) <= ref["bound"][hit] + 8 * gc.U * (scale + ref["d"][hit])).all()
    assert (np.abs(nrm[hit] - ref["n"][hit]).max(-1) <= 8 * gc.U).all()
    # a miss reports zeros
    assert not dist[found == 0].any() and not p[found == 0].any() and not nrm[found == 0].any()


@pytest.mark.parametrize("name", SCENES)
def test_star_radii_against_float64(oracle, name):
    v, ix, _ = gc.scene(name)
    rng = np.random.default_rng(SEEDS[name] + 100)
    x = gc.random_points(name, N_ITEMS, rng)
    max_r = gc.random_lengths(name, N_ITEMS, rng)
    flip = (rng.random(N_ITEMS) < 0.25).astype(np.int32)
    got = oracle.star_radii(gc.oracle_scene(oracle, name), x, max_r, flip)
    ref, keep = gc.star64(v, ix, x, max_r, flip)
    assert keep.sum() * 2 >= N_ITEMS, f"{name}: only {keep.sum()} of {N_ITEMS} points clear every margin"
    finite = keep & (ref < 1e30)
    np.testing.assert_array_equal(got[keep & ~finite], np.float32(gc.FLT_MAX))
    err = np.abs(got[finite].astype(np.float64) - ref[finite])
    bound = 8 * gc.U * max(float(np.abs(v).max()), float(np.abs(x).max()))
    _report("star", name, int(keep.sum()), N_ITEMS, err, np.full(err.shape, bound))
    assert (err <= bound).all()
    if gc.candidates64(v, ix) is not None:  # the candidates decided some radii, maxR the others
        below = finite & (ref < np.maximum(max_r, 1e-3) * (1 - 1e-6))
        assert below.sum() > 20 and (finite & ~below).sum() > 20


@pytest.mark.parametrize("name", SCENES + ["obstacle", "cube_dirichlet"])
def test_dirichlet_dists_against_float64(oracle, name):
    v, ix, kw = gc.scene(name)
    rng = np.random.default_rng(SEEDS[name] + 200)
    x = gc.random_points(name, N_ITEMS, rng)
    dist, proj = oracle.dirichlet_dists(gc.oracle_scene(oracle, name), x)
    ref = gc.dirichlet64(name, x)
    err = np.abs(dist.astype(np.float64) - ref)
    bound = 8 * gc.U * max(float(np.abs(v).max()), float(np.abs(x).max()))
    _report("dirichlet", name, N_ITEMS, N_ITEMS, err, np.full(err.shape, bound))
    assert (err <= bound).all()
    if "dvertices" in kw:  # the projection lies on the mesh, at the distance
        dist64 = gc.seg_dist64 if v.shape[1] == 2 else gc.tri_dist64
        assert (dist64(kw["dvertices"], kw["dprims"], proj.astype(np.float64)) <= bound).all()
        assert (np.abs(np.linalg.norm(x.astype(np.float64) - proj, axis=-1) - ref) <= bound).all()
    else:
        np.testing.assert_array_equal(proj, x)
