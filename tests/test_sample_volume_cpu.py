"""The source sample on the CPU: the oracle's plain loop (oracle_sample_volume, the reference's
sampleVolume + rejectionSampleGreensFn) against the independent model of
tests/sample_volume_model.py -- the replay bit for bit, the accept decisions against the
mathematics, and the accepted radius's distribution (DESIGN.md "Source-sample probe").  No GPU."""
import math

import numpy as np
import pytest

import gfn_model
import oracle_lib
import sample_volume_cases as C
import sample_volume_model as M

IN_BAND_CAP = 1e-3
DKW_DELTA = 1e-9

_ref = {}


def reference(name, dim):
    """The oracle's result on a case, computed once and shared (never modified)."""
    if (name, dim) not in _ref:
        items, seeds, robust = C.case(name, dim)
        r = oracle_lib.sample_volume(dim, items, seeds, robust)
        for v in r.values():
            v.setflags(write=False)
        _ref[(name, dim)] = r
    return _ref[(name, dim)]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_stream_closed_form_against_stepping():
    s = M.seed_state(12345)
    t = s
    for k in range(1, 2050):
        t = (t * M.MULT + M.INC) & M.M64
        if k in (1, 2, 3, 255, 256, 257, 1999, 2000, 2049):
            assert M.advance(s, k) == t
    # the vector draw and the scalar draw agree, and draws lie on the 2^-23 grid below 1
    st = np.array([M.advance(s, k) for k in range(64)], np.uint64)
    v = M._draw_v(st)
    assert all(v[k] == M.draw(int(st[k])) for k in range(64))
    assert (v < 1).all() and (v * 2.0 ** 23 == np.round(v * 2.0 ** 23)).all()


def test_model_threshold_against_50_digit_green():
    """float64 is enough: T of the model against gfn_model's 50-digit members, including the scaled
    forms' range and the balls whose norm cancels."""
    mp = gfn_model.mp
    for dim in (2, 3):
        for R, lam in ((0.004, 10.0), (0.0002, 350.0), (0.4, 50.0), (3.2, 350.0), (4.5, 350.0)):
            sl, X, bound = M.float_ball(dim, R, lam, True)
            for frac in (0.01, 0.3, 0.9, 0.999):
                r = np.float32(frac * R)
                x = np.float32(r * sl)
                m = gfn_model.members(dim, mp.mpf(float(np.float32(lam))), mp.mpf(float(np.float32(R))), mp.mpf(float(r)),
                                      mp.mpf(float(sl)), mp.mpf(float(x)), mp.mpf(float(X)), mp.mpf(float(x)))
                T = m["ev"] * gfn_model.sphere_area(dim) * mp.mpf(float(r)) ** (dim - 1) / m["norm"] / mp.mpf(float(bound))
                Tm, _ = M.threshold(dim, R, lam, True, np.array([r]))
                assert abs(Tm[0] - float(T)) <= 1e-9 * abs(float(T)), (dim, R, lam, frac)


@pytest.mark.parametrize("dim", (2, 3))
@pytest.mark.parametrize("name", C.FAMILIES)
def test_replay_bit_for_bit(name, dim):
    items, seeds, _ = C.case(name, dim)
    ref = reference(name, dim)
    for i in range(items.shape[0]):
        k = int(ref["iters"][i])
        state, r, out = M.replay(dim, items[i], seeds[i], k)
        assert state == int(ref["state"][i]), (name, dim, i)
        if r is None:
            assert k == 0
            continue
        assert 1 <= k <= M.LIMIT
        assert bits(r) == bits(ref["r"][i]), (name, dim, i)
        assert (bits(out) == bits(ref["out"][i])).all(), (name, dim, i)


@pytest.mark.parametrize("dim", (2, 3))
@pytest.mark.parametrize("name", C.FAMILIES)
def test_accept_decisions_against_the_mathematics(name, dim):
    items, seeds, robust = C.case(name, dim)
    ref = reference(name, dim)
    if name == "harmonic" and dim == 3:
        assert (ref["iters"] == 0).all()  # the closed form: no loop
        return
    j = M.judge(dim, items, seeds, ref["iters"])
    share = j["in_band"] / max(1, j["iterations"])
    print(f"{name} {dim}D: {j['iterations']} iterations, {j['in_band']} in band ({share:.2e}, cap {IN_BAND_CAP:.0e}), "
          f"{j['limit']} loops at the limit, {j['unbounded_norm']} of {j['balls']} balls without a norm bound")
    assert j["bad"] == [], j["bad"]
    assert share <= IN_BAND_CAP


@pytest.mark.parametrize("dim", (2, 3))
def test_slow_case_holds_long_loops_and_loops_at_the_limit(dim):
    it = reference("slow", dim)["iters"]
    assert (it > C.LONG_ITERS).sum() >= C.SLOW_MIN_LONG
    assert (it == C.LIMIT).sum() >= C.SLOW_MIN_LIMIT


@pytest.mark.parametrize("dim", (2, 3))
@pytest.mark.parametrize("mu_r", C.DISTRIBUTION_MU_R)
def test_accepted_radius_distribution(mu_r, dim):
    items, seeds = C.distribution_ball(dim, mu_r)
    r = oracle_lib.sample_volume(dim, items, seeds)
    n = items.shape[0]
    at_limit = int((r["iters"] == M.LIMIT).sum())
    assert at_limit == 0
    bound = math.sqrt(math.log(2 / DKW_DELTA) / (2 * n))
    assert abs(bound - 0.0128) < 1e-4
    d, active = M.dkw_distance(dim, items[0, 0], items[0, 1], True, r["r"])
    print(f"{dim}D mu R = {mu_r}: DKW distance {d:.5f} (bound {bound:.5f}), heuristic bound exceeded: {active}")
    assert d <= bound
