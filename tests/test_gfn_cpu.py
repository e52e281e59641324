"""The Green's-function model against itself, the truth table against the model, and the CPU
oracle's members (oracle_gfn: the gfn_* and fs2_* functions of every oracle solve) against the
truth under the derived bounds (tests/gfn_model.py; DESIGN.md "Green's-function probe").
The device probe is held against the same table in tests/test_gpu_gfn.py.
"""
import os
import sys

import mpmath as mp
import numpy as np
import pytest

import gfn_cases as C
import gfn_model as M
import oracle_lib

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_gfn_truth as G  # noqa: E402

mpf = mp.mpf


@pytest.fixture
def dps30():
    """The derivative and quadrature self-checks run at 30 digits (mp.diff and mp.quad of integer-order
    Bessel functions at 50 take minutes); they assert 15 or more, the probe needs 8."""
    with mp.workdps(30):
        yield


# a dozen (lambda, R, r): mu R from 1e-3 to 300, r near the pole, mid-ball and near the sphere
POINTS = [(1e-2, 0.01, 0.003), (1e-2, 3.0, 2.9), (1.0, 1.5, 0.4), (1.0, 0.2, 0.1999), (50.0, 0.7, 1e-3),
          (50.0, 2.0, 1.0), (350.0, 0.3, 0.1), (350.0, 1.0, 0.99), (1e4, 0.05, 0.02), (1e4, 1.0, 0.5),
          (1e4, 3.0, 2.5), (350.0, 0.011, 0.0001)]


@pytest.mark.parametrize("d", [2, 3])
@pytest.mark.parametrize("l", [0, 1])
def test_mode_solves_the_radial_equation(d, l, dps30):
    """g'' + (d-1)/r g' - (l (l + d - 2) / r^2 + lambda) g = 0, g(R) = 0, and the pole's strength:
    r^(d-1) G_0'(r) -> -1/|S^(d-1)|, r^(d-1) G_1(r) -> 1/|S^(d-1)| (grad_x of the free-space pole)."""
    A = M.sphere_area(d)
    for lam, R, r in POINTS:
        lam, R, r = mpf(lam), mpf(R), mpf(r)
        for la in (lam, mpf(0)):
            g = M._G(d, l, R, la)
            g1, g2 = mp.diff(g, r), mp.diff(g, r, 2)
            res = g2 + (d - 1) / r * g1 - (l * (l + d - 2) / r ** 2 + la) * g(r)
            assert abs(res) <= mpf(10) ** -18 * (abs(g2) + abs(la * g(r))), (d, l, lam, R, r)
            assert abs(g(R)) <= mpf(10) ** -25 * abs(g(R / 2))
            eps = R * mpf(10) ** -14
            if l == 0:
                assert abs(eps ** (d - 1) * mp.diff(g, eps) * A + 1) < mpf(10) ** -15
            else:
                assert abs(eps ** (d - 1) * g(eps) * A - 1) < mpf(10) ** -15


@pytest.mark.parametrize("d", [2, 3])
def test_members_closed_form_vs_derived(d, dps30):
    """Every member the truth table takes in closed form equals its definition by mp.diff / mp.quad of
    G_0 and G_1 (norm = the integral of G_0 over the ball)."""
    for lam, R, r in POINTS[::2]:
        for la in (mpf(lam), mpf(0)):
            R, r = mpf(R), mpf(r)
            mu = mp.sqrt(la)
            a = M.members(d, la, R, r, mu, mu * r, mu * R, mu * r)
            b = M.derived_members(d, r, R, la)
            for k, v in b.items():
                assert abs(a[k] - v) <= mpf(10) ** -18 * abs(v), (d, la, R, r, k)


@pytest.mark.parametrize("d", [2, 3])
def test_yukawa_members_tend_to_harmonic(d):
    for _, R, r in POINTS:
        R, r = mpf(R), mpf(r)
        la = mpf(10) ** -20
        mu = mp.sqrt(la)
        y = M.members(d, la, R, r, mu, mu * r, mu * R, mu * r)
        h = M.members(d, 0, R, r, 0, 0, 0, 0)
        for k in ("ev", "gn", "pk", "norm", "dpk", "pkg"):
            assert abs(y[k] - h[k]) <= mpf(10) ** -17 * abs(h[k]), (d, R, r, k)


@pytest.mark.parametrize("d", [2, 3])
def test_harmonic_dipole_is_the_pole_gradient(d, dps30):
    """G_1 is grad_x G(x, y) at x = c: checked on the method-of-images Green's function, whose
    gradient with respect to the pole at the centre is G_1(|y|) y / |y|."""
    R = mpf("1.3")
    y = [mpf("0.3"), mpf("-0.4"), mpf("0.5")][:d]
    r = mp.sqrt(sum(t * t for t in y))
    for k in range(d):
        def f(t, k=k):
            x = [mpf(0)] * d
            x[k] = t
            return M.images_green(d, x, y, R)
        # (the pole sits at the centre: a one-sided limit is the derivative, the function is smooth in x)
        g = mp.diff(f, mpf(0), h=mpf(10) ** -12, direction=1)
        assert abs(g - M.mode_harmonic(d, 1, r, R) * y[k] / r) < mpf(10) ** -10


def test_free_space_closed_form_vs_derived(dps30):
    for lam, _, r in POINTS[::3]:
        for la in (mpf(lam), mpf(0)):
            r = mpf(r)
            mu = mp.sqrt(la)
            a, b = M.fs_scalars(la, r, mu, mu * r), M.fs_derived(la, r)
            for k, v in b.items():
                assert abs(a[k] - v) <= mpf(10) ** -15 * abs(v), (la, r, k)


# ---- the rounding count of every shipped expression -------------------------------------------------
# (k, a): the float (scaled members: double) roundings and the A&S Bessel values on the expression's
# longest path -- a sum over the factors of a product or quotient, a maximum over the terms of a sum
# -- counted from csrc/wos_device.h (Gfn) and csrc/wos_bvc.hip (FreeSpace2) by gfn_model.bounds, which
# mirrors them node by node; "h" harmonic, "y" Yukawa reference members, "s" scaled members.
ROUNDINGS = {
    (2, "h"): {"ev": (3, 0), "gn": (4, 0), "pk": (1, 0), "norm": (2, 0), "pkg": (3, 0), "dpk": (0, 0), "exy": (3, 0),
               "fsG": (2, 0), "fsg": (3, 0), "fsc": (5, 0)},
    (2, "y"): {"A0": (1, 1), "A1": (1, 1), "B0": (1, 1), "B1": (1, 1), "ev": (7, 3), "gn": (9, 3), "pk": (4, 1),
               "norm": (8, 1), "pkg": (5, 1), "dpk": (7, 3), "exy": (8, 3), "fsG": (2, 1), "fsg": (4, 1), "fsc": (14, 1)},
    (2, "s"): {"A0": (1, 1), "A1": (1, 1), "B0": (1, 1), "B1": (1, 1), "ev": (13, 3), "gn": (15, 3), "pk": (5, 1),
               "norm": (9, 1), "pkg": (8, 1), "dpk": (13, 3), "exy": (14, 3), "fsG": (2, 1), "fsg": (4, 1), "fsc": (14, 1)},
    (3, "h"): {"ev": (3, 0), "gn": (5, 0), "pk": (1, 0), "norm": (2, 0), "pkg": (3, 0), "dpk": (0, 0), "exy": (3, 0)},
    (3, "y"): {"A0": (1, 0), "A1": (7, 0), "B0": (4, 0), "B1": (9, 0), "ev": (20, 0), "gn": (29, 0), "pk": (10, 0),
               "norm": (14, 0), "pkg": (12, 0), "dpk": (21, 0), "exy": (21, 0)},
    (3, "s"): {"ev": (15, 0), "gn": (28, 0), "pk": (9, 0), "norm": (13, 0), "pkg": (12, 0), "dpk": (20, 0), "exy": (16, 0)},
}


def _representative(d, kind):
    T = C.table()
    X, k = T[f"X{d}"], T[f"kind{d}"]
    if kind == "s":
        return int(np.flatnonzero((k == 1) & (X > 100) & (X < 200))[5])
    return int(np.flatnonzero((k == 0) & (X > 1) & (X < 3))[5])


def roundings(d, kind):
    i = _representative(d, kind)
    b = M.bounds(d, {"h": 0, "y": 1, "s": 2}[kind], C.table()[f"items{d}"][i])
    return {s: (e.k, e.a) for s, e in b.items()}


@pytest.mark.parametrize("d", [2, 3])
@pytest.mark.parametrize("kind", ["h", "y", "s"])
def test_rounding_counts(d, kind):
    got = roundings(d, kind)
    want = ROUNDINGS[(d, kind)]
    assert {s: got[s] for s in want} == want


# ---- the table is the model's ------------------------------------------------------------------------
@pytest.mark.parametrize("d", [2, 3])
def test_truth_table_is_the_models(d):
    """The committed items are the generator's, and every 37th row of every table equals the model
    recomputed (truth to the last bit of its double, bound and range flag exactly)."""
    T = C.table()
    items, kind = G.make_items(d)
    assert np.array_equal(items.view(np.uint32), T[f"items{d}"].view(np.uint32))
    assert np.array_equal(kind, T[f"kind{d}"])
    assert tuple(T["slots"]) == G.SLOTS
    rows_h = np.flatnonzero(kind != 1)
    idx2 = T[f"idx2{d}"]
    assert np.array_equal(idx2, np.flatnonzero(T[f"X{d}"] > C.ROBUST_MUR))
    for mode, rows, tt, ee in ((0, rows_h, T[f"th{d}"], T[f"eh{d}"]), (1, np.arange(len(items)), T[f"ty{d}"], T[f"e1{d}"]),
                               (2, idx2, None, T[f"e2{d}"])):
        for j in range(0, len(rows), 37):
            i = rows[j]
            tv, ev, ov, ts = G.row_values((d, mode, items[i], int(kind[i])))
            assert np.array_equal(ev, ee[j], equal_nan=True), (d, mode, i)
            if mode == 1:
                assert np.array_equal(ov, T[f"out1{d}"][j]), (d, mode, i)
            if tt is not None:
                assert np.array_equal(tv, tt[j], equal_nan=True), (d, mode, i)
            else:
                assert np.array_equal(ts, T[f"tys{d}"][i], equal_nan=True), (d, mode, i)


# ---- the oracle against the truth ---------------------------------------------------------------------
def oracle_report(d, mode):
    T = C.table()
    return C.compare(d, mode, oracle_lib.gfn(d, mode, T[f"items{d}"][C.rows_of(d, mode)]))


@pytest.mark.parametrize("d", [2, 3])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_oracle_members_within_bounds(d, mode):
    C.check_report(d, mode, oracle_report(d, mode))


def test_oracle_gfn_refusals():
    L = oracle_lib.lib()
    it = np.zeros(C.table()["items2"].shape[1], np.float32)
    out = np.zeros(32, np.float32)
    assert L.oracle_gfn(2, 0, it.ctypes.data, 0, out.ctypes.data) == 0
    assert L.oracle_gfn(2, 0, None, 1, out.ctypes.data) == -1
    assert L.oracle_gfn(2, 0, it.ctypes.data, -1, out.ctypes.data) == -1
    for dim, mode in ((1, 0), (4, 0), (2, 3), (2, -1)):
        assert L.oracle_gfn(dim, mode, it.ctypes.data, 1, out.ctypes.data) == -2
