"""The certified shortcuts of the Yukawa rejection sampler against its exact test, draw by draw.

rejectionSampleGreensFn accepts iff u < T(r).  The kernels decide most iterations without
the exact T (csrc/wos_device.h): rej_fast_decide / rej_fast_decide3 (float approximations with
an error band), rej_quick_bound (per-ball certain reject) and rej_xreject3 (radius-dependent
certain reject, 3D).  Each promises the exact test's decision.  wos_selftest_rejection runs
the shipped functions on a ball (R, lambda) at the radius draw r = x R and returns, for each
of them, its edge over the 2^23 values u_k = k 2^-23 a stream can draw -- every predicate
compares u with values that do not depend on u, so an edge describes its decision at every
draw.  With

    a   draws the fast test accepts           r0  first draw the fast test rejects
    e   draws the exact test accepts          q   first draw the per-ball bound rejects
    e3  the same for rej_exact_decide3        xr  first draw the radius bound rejects

the shortcuts are sound iff a <= e <= min(r0, q, xr) and e3 == e, for every ball and radius:
a failure names a concrete (R, lambda, x, k).
"""
import json
import sys

import numpy as np
import pytest

from test_rejection_bounds import _thresholds_2d, _thresholds_3d
from wos_amd import _lib, selftest_rejection

pytestmark = pytest.mark.gpu

f32 = np.float32
N23 = 1 << 23
INVALID = -1  # include/wos.h WOS_E_INVALID
A, R0, E, E3, Q, XR = range(6)
LAMBDAS = [1e-2, 1.0, 10.0, 50.0, 350.0, 2000.0, 1e4]
# non-robust 3D balls whose exp_fast(-mu r) goes denormal, then 0
MUR_3D_EXTRA = [80.5, 85.0, 87.5, 88.5, 95.0, 104.0, 110.0]


def _grid(v):
    """v rounded to a multiple of 2^-23 in [0, 1]"""
    return np.clip(np.round(np.asarray(v, np.float64) * N23), 0, N23) / N23


def _sweep(dim):
    """Items (ball index, R, lambda, x) as float32 arrays, ball after ball."""
    rng = np.random.default_rng(20 + dim)
    x_common = np.concatenate([_grid(rng.uniform(0.0, 1.0, 150)), _grid(1.0 - np.logspace(-7, -2, 30)),
                               [2.0 ** -23, 0.5, 0.0]])
    mur_all = np.geomspace(2e-4, 79.9, 120)
    if dim == 3:
        mur_all = np.concatenate([mur_all, MUR_3D_EXTRA])
    ball, Rs, lams, xs = [], [], [], []
    nb = 0
    for lam in LAMBDAS:
        for mur in mur_all:
            R = mur / np.sqrt(lam)
            if not (1e-4 <= R <= 3.0):
                continue
            x = np.concatenate([x_common, _grid([min(1.0, 0.6 / mur), min(1.0, 1.0 / mur)])])
            ball.append(np.full(x.size, nb))
            Rs.append(np.full(x.size, R))
            lams.append(np.full(x.size, lam))
            xs.append(x)
            nb += 1
    return (np.concatenate(ball), np.concatenate(Rs).astype(f32), np.concatenate(lams).astype(f32),
            np.concatenate(xs).astype(f32))


@pytest.fixture(scope="module", params=[2, 3])
def probe(request, gpu):
    dim = request.param
    ball, R, lam, x = _sweep(dim)
    edges, vals, flags = selftest_rejection(dim, R, lam, x)
    return {"dim": dim, "ball": ball, "R": R, "lam": lam, "x": x, "edges": edges.astype(np.int64),
            "vals": vals, "flags": flags}


def _mur(p):
    """mu R and mu r in the kernels' float order"""
    sl = np.sqrt(p["lam"])
    return (p["R"] * sl).astype(f32), ((p["x"] * p["R"]).astype(f32) * sl).astype(f32)


def _worst(p, bad, by):
    i = np.flatnonzero(bad)[np.argmax(by[bad])]
    return {"R": float(p["R"][i]), "lam": float(p["lam"][i]), "x": float(p["x"][i]), "x_2^23": int(round(float(p["x"][i]) * N23)),
            "edges(a,r0,e,e3,q,xr)": p["edges"][i].tolist(), "nrm,bound,invNB": p["vals"][i].tolist()}


def test_sweep_size(probe):
    assert 1.0e5 < probe["R"].size < 1.3e5


def test_shortcuts_never_contradict_exact_test(probe):
    """a <= e <= min(r0, q, xr), for every item, the balls with a non-positive norm included:
    no draw is accepted by the fast test or rejected by a shortcut against the exact test."""
    ed = probe["edges"]
    a, r0, e, q, xr = ed[:, A], ed[:, R0], ed[:, E], ed[:, Q], ed[:, XR]
    acc = a > e               # draws e .. a - 1: accepted by the fast test, rejected by the exact one
    rej = np.minimum(np.minimum(r0, q), xr) < e   # draws rejected by a shortcut, accepted by the exact test
    report = {}
    if acc.any():
        report["fast accepts what exact rejects"] = (int(acc.sum()), _worst(probe, acc, a - e))
    for name, col in (("fast", r0), ("quick", q), ("xreject3", xr)):
        b = col < e
        if b.any():
            report[name + " rejects what exact accepts"] = (int(b.sum()), _worst(probe, b, e - col))
    print(f"dim {probe['dim']}: {int(acc.sum())} items with a > e, {int(rej.sum())} with a reject below e, "
          f"of {a.size}")
    assert not report, report


def test_exact_variants_agree_and_edges_are_edges(probe):
    ed = probe["edges"]
    np.testing.assert_array_equal(ed[:, E3], ed[:, E])
    bad = probe["flags"] != 0
    assert not bad.any(), (int(bad.sum()), _worst(probe, bad, probe["flags"]))
    if probe["dim"] == 2:
        assert (ed[:, XR] == N23).all()


def _same_bits(got, want):
    got, want = np.asarray(got, f32), np.asarray(want, f32)
    gn, wn = np.isnan(got), np.isnan(want)
    np.testing.assert_array_equal(gn, wn)
    np.testing.assert_array_equal(got[~gn].view(np.uint32), want[~wn].view(np.uint32))


def _count_below(T):
    """number of draws k 2^-23, k = 0 .. 2^23 - 1, below T (none below a NaN)"""
    T = np.asarray(T, np.float64)
    with np.errstate(invalid="ignore"):
        c = np.ceil(np.clip(np.nan_to_num(T, nan=0.0), 0.0, 1.0) * N23)
    return c.astype(np.int64)


def test_probe_measures_the_shipped_exact_path(probe, oracle):
    """norm, bound, 1 / (norm bound) and the exact accept count equal the oracle-math model of
    tests/test_rejection_bounds.py bit for bit, on every 7th ball with all of its x."""
    thresholds = _thresholds_2d if probe["dim"] == 2 else _thresholds_3d
    nb = int(probe["ball"].max()) + 1
    for b in range(0, nb, 7):
        sel = np.flatnonzero(probe["ball"] == b)
        R, lam = probe["R"][sel[0]], probe["lam"][sel[0]]
        T, _, (_, inv_nb, nrm, bound) = thresholds(R, lam, probe["x"][sel])
        _same_bits(probe["vals"][sel], np.tile(np.array([nrm, bound, inv_nb], f32), (sel.size, 1)))
        np.testing.assert_array_equal(probe["edges"][sel, E], _count_below(T), err_msg=f"ball R={R} lam={lam}")


def test_undecided_regimes_stay_undecided(probe):
    """2D balls with mu R >= 80 and 3D radius draws with mu r > 88 (exp_fast gives 0) are left to
    the exact test at every draw: the fast tests rely on comparisons with a non-finite band being
    false.  The sweep stops below mu R = 80 in 2D, so that regime gets balls of its own."""
    if probe["dim"] == 2:
        x = np.concatenate([_grid(np.linspace(0.0, 1.0, 41)), _grid(1.0 - np.logspace(-7, -2, 12))]).astype(f32)
        mur_big = np.repeat(np.array([80.0, 80.5, 88.0, 120.0, 300.0]), x.size)
        for lam in (350.0, 2000.0, 1e4):
            R = (mur_big / np.sqrt(lam)).astype(f32)
            lams = np.full(R.size, lam, f32)
            ed, _, _ = selftest_rejection(2, R, lams, np.tile(x, 5))
            und = (R * np.sqrt(lams)).astype(f32) >= 80.0
            assert und.sum() >= 4 * x.size
            assert (ed[und, A] == 0).all() and (ed[und, R0] == N23).all()
        return
    ed = probe["edges"]
    _, mur = _mur(probe)
    und = mur > 88.0
    assert und.sum() > 100
    assert (ed[und, A] == 0).all() and (ed[und, R0] == N23).all()


def _band_stats(p):
    ed = p["edges"]
    muR, mur = _mur(p)
    nrm, inv_nb = p["vals"][:, 0], p["vals"][:, 2]
    ok = (muR < 80.0) & (mur > 0) & (nrm > 0) & np.isfinite(inv_nb)
    a, r0, e = ed[ok, A], ed[ok, R0], ed[ok, E]
    share = (r0 - a) / N23
    # the band's centre is the fast threshold: how far from it the exact edge lies, in half bands
    # (1 would be a draw decided wrongly); bands clipped by the ends of the draw range say nothing
    inside = (a > 0) & (r0 < N23)
    off = np.abs(e - 0.5 * (a + r0)) / np.maximum(0.5 * (r0 - a), 0.5)
    out = {"items": int(ok.sum()), "undecided_share_mean": float(share.mean()), "undecided_share_max": float(share.max()),
           "undecided_everywhere_fraction": float(np.mean((a == 0) & (r0 == N23)))}
    # (a band of 16 draws resolves the offset to 1/16; the wider ones say how much of it is the grid)
    for width in (16, 256):
        w = inside & ((r0 - a) >= width)
        out[f"bands_of_{width}_draws_or_more"] = int(w.sum())
        out[f"exact_edge_offset_over_half_band_max_{width}"] = float(off[w].max()) if w.any() else 0.0
    return out


def test_shortcuts_stay_useful(probe):
    """soundness must not be bought with a wide band: over the balls the fast tests are meant for,
    the band leaves under 1e-3 of the draws to the exact test on average, and at most 1 % of the
    items are undecided at every draw"""
    s = _band_stats(probe)
    print(f"dim {probe['dim']}: {s}")
    assert s["undecided_share_mean"] < 1e-3, s
    assert s["undecided_everywhere_fraction"] <= 0.01, s


def test_refusals_and_empty(gpu):
    L = _lib.load()
    one = np.ones(1, f32)
    ed, va, fl = np.zeros(6, np.int32), np.zeros(3, f32), np.zeros(1, np.int32)
    good = [one.ctypes.data, one.ctypes.data, one.ctypes.data, 1, ed.ctypes.data, va.ctypes.data, fl.ctypes.data]
    assert L.wos_selftest_rejection(2, *good, 0) == _lib.WOS_OK
    for dim in (1, 4, 0, -2):
        assert L.wos_selftest_rejection(dim, *good, 0) == INVALID
    for k in (0, 1, 2, 4, 5, 6):
        args = list(good)
        args[k] = None
        assert L.wos_selftest_rejection(3, *args, 0) == INVALID, k
    neg = list(good)
    neg[3] = -1
    assert L.wos_selftest_rejection(3, *neg, 0) == INVALID
    for dim in (2, 3):
        e0, v0, f0 = selftest_rejection(dim, [], [], [])
        assert e0.shape == (0, 6) and v0.shape == (0, 3) and f0.shape == (0,)


if __name__ == "__main__":
    # the measured band of both dimensions as JSON, with the package directory on PYTHONPATH:
    #   python tests/test_gpu_rejection.py profiles/rejection_band.json
    out = {}
    for d in (2, 3):
        ball, R, lam, x = _sweep(d)
        edges, vals, flags = selftest_rejection(d, R, lam, x)
        out[f"{d}d"] = _band_stats({"edges": edges.astype(np.int64), "vals": vals, "R": R, "lam": lam, "x": x})
    with open(sys.argv[1], "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
