"""The source sample on the device, pinned directly (wos_selftest_sample_volume): the shipped
wave-cooperative sample_volume_wave against the sequential sample_volume on every field, bit for
bit; the sequential form against the oracle's plain loop; the canaries; the regime every lane mask
was built for; the slow balls' counts (DESIGN.md "Source-sample probe").  Cases and masks:
tests/sample_volume_cases.py; the CPU half: tests/test_sample_volume_cpu.py."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib
import sample_volume_cases as SC
import sample_volume_model as M
from wos_amd import _lib, selftest_sample_volume

pytestmark = pytest.mark.gpu

# (fb, need_pdf) as shipped: the walk step's call and the first balls' call; each with both Gfn forms
CALLS = ((False, False), (True, True))
PDF0 = np.float32(-1234.5)  # the probe's canary value of pdf (csrc/wos_selftest.hip)

_plans, _ref, _runs = {}, {}, {}


def plan(dim, fb):
    if (dim, fb) not in _plans:
        _plans[(dim, fb)] = selftest_sample_volume(dim, np.zeros((0, _lib.SV_ITEM), np.float32), np.zeros(0, np.uint32),
                                                   np.zeros(0, np.uint64), fb=fb)["plan"]
    return _plans[(dim, fb)]


def mask_sets():
    return SC.mask_sets([plan(d, fb) for d in (2, 3) for fb in (False, True)])


def reference(name, dim, rb):
    """The oracle's loop on a case, once (read-only)."""
    if (name, dim, rb) not in _ref:
        items, seeds, _ = SC.case(name, dim)
        r = oracle_lib.sample_volume(dim, items, seeds, rb)
        for v in r.values():
            v.setflags(write=False)
        _ref[(name, dim, rb)] = r
    return _ref[(name, dim, rb)]


def variants(name, dim):
    """(fb, need_pdf, rb) a case runs under: the robust kernels' case under rb alone."""
    only_rb = SC.case(name, dim)[2]
    return [(fb, pdf, rb) for fb, pdf in CALLS for rb in (False, True) if rb or not only_rb]


def run(name, dim, fb, pdf, rb):
    """{mask set: (masks, items used, probe result)} of one case and variant, once."""
    key = (name, dim, fb, pdf, rb)
    if key not in _runs:
        items, seeds, _ = SC.case(name, dim)
        out = {}
        for ms, pattern in mask_sets().items():
            masks, used = SC.tile(pattern, items.shape[0])
            out[ms] = (masks, used, selftest_sample_volume(dim, items, seeds, masks, fb=fb, rb=rb, need_pdf=pdf))
        _runs[key] = out
    return _runs[key]


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def expected_tags(name, dim, fb, rb, masks, used, iters):
    items = SC.case(name, dim)[0][:used]
    p = plan(dim, fb)
    balls, inv = np.unique(items[:, :3], axis=0, return_inverse=True)
    fast = np.array([M.on_fast_path(dim, b[0], b[1], bool(b[2]), rb) for b in balls])[inv.reshape(-1)]
    wave, _ = SC.wave_of_item(masks)
    nc = np.bincount(wave, weights=fast, minlength=len(masks)).astype(int)[wave]
    dense = (p["own"] > 0) & (nc >= p["own_min"])
    tag = np.where(dense, np.where(iters <= p["own"], _lib.SV_DENSE_OWN, _lib.SV_DENSE_COOP), _lib.SV_SPARSE)
    tag = np.where(nc == 1, _lib.SV_SOLO, tag)
    # the function's own trace: a lane publishes its stream iff it enters a cooperative generation
    tag = np.where(np.isin(tag, (_lib.SV_SPARSE, _lib.SV_DENSE_COOP)), tag | _lib.SV_PUBLISHED, tag)
    return np.where(fast, tag, _lib.SV_FALLBACK), fast, wave


CASES = [(n, d) + v for n in SC.FAMILIES for d in (2, 3) for v in variants(n, d)]


@pytest.mark.parametrize("name,dim,fb,pdf,rb", CASES)
def test_cooperative_equals_sequential_equals_oracle(name, dim, fb, pdf, rb):
    items, seeds, _ = SC.case(name, dim)
    ref = reference(name, dim, rb)
    closed = dim == 3 and name == "harmonic"  # the 3D harmonic closed form: no loop, pdf always written
    for ms, (masks, used, res) in run(name, dim, fb, pdf, rb).items():
        at = (name, dim, fb, pdf, rb, ms)
        assert used > 0, at
        u = slice(0, used)
        # (a) the cooperative form is the sequential form: a scheduling defect shows here first
        for f in ("iters", "state", "r", "out", "pdf"):
            a, b = bits(res[f][u, 0]), bits(res[f][u, 1])
            bad = np.flatnonzero((a != b).reshape(used, -1).any(axis=1))
            assert bad.size == 0, (at, "cooperative != sequential", f, bad[:8], res["tags"][bad[:8]])
        # (b) the sequential form is the oracle's plain loop
        for f in ("iters", "state", "r", "out") + (("pdf",) if pdf or closed else ()):
            a, b = bits(res[f][u, 1]), bits(np.ascontiguousarray(ref[f][u]))
            bad = np.flatnonzero((a != b).reshape(used, -1).any(axis=1))
            assert bad.size == 0, (at, "sequential != oracle", f, bad[:8])
        if not pdf and not closed:
            assert (bits(res["pdf"][u]) == bits(PDF0)).all(), at
        # (c) no canary: clear lanes untouched, pdf untouched where the caller does not need it.  The closed
        # form alone writes pdf unasked (sample_volume, as the reference does; the walk step discards it)
        wave, lane = SC.wave_of_item(masks)
        can = res["canary"].copy()
        if closed and not pdf:
            assert (can[wave, lane] == _lib.SV_CANARY["pdf"]).all(), at
            can[wave, lane] = 0
        assert not can.any(), (at, np.argwhere(can)[:8], can[can != 0][:8])
        # (d) every lane took the regime its wave's sampling lanes call for
        exp, _, _ = expected_tags(name, dim, fb, rb, masks, used, res["iters"][u, 0])
        assert (res["tags"][u] == exp).all(), (at, np.flatnonzero(res["tags"][u] != exp)[:8])


@pytest.mark.parametrize("dim", (2, 3))
@pytest.mark.parametrize("fb,pdf", CALLS)
def test_mask_sets_enter_their_regimes(dim, fb, pdf):
    """On the ordinary balls every lane samples cooperatively, so the mask alone sets the regime."""
    p = plan(dim, fb)
    runs = run("ordinary", dim, fb, pdf, False)
    tags = {ms: r[2]["tags"][:r[1]] & ~_lib.SV_PUBLISHED for ms, r in runs.items()}
    for l in (0, 37, p["wave"] - 1):
        assert (tags[f"solo_{l}"] == _lib.SV_SOLO).all()
    for ms in ("lanes_2", "lanes_3", f"lanes_{p['own_min'] - 1}", "alternating"):
        assert (tags[ms] == _lib.SV_SPARSE).all(), ms
    if p["own"] > 0:
        for ms in (f"lanes_{p['own_min']}", "all", "empty_between"):
            assert np.isin(tags[ms], (_lib.SV_DENSE_OWN, _lib.SV_DENSE_COOP)).all(), ms
            assert (tags[ms] == _lib.SV_DENSE_COOP).any(), ms
            assert (tags[ms] == _lib.SV_DENSE_OWN).any(), ms
    # the masks at which `per` goes from 1 to 2 exist for this instantiation's block size
    n = p["wave"] // p["bmin"] + 1
    assert f"lanes_{n}" in tags and f"lanes_{n - 1}" in tags
    # three lanes take B = wave / 3 below the cap, two lanes reach it
    assert p["wave"] // 3 < p["bcap"] <= p["wave"] // 2


@pytest.mark.parametrize("dim,rb", ((2, False), (2, True), (3, True)))
@pytest.mark.parametrize("fb,pdf", CALLS)
def test_mixed_waves_sample_beside_fallback_lanes(dim, rb, fb, pdf):
    for ms, (masks, used, res) in run("mixed", dim, fb, pdf, rb).items():
        wave, _ = SC.wave_of_item(masks)
        t = res["tags"][:used] & ~_lib.SV_PUBLISHED
        per_wave = np.bincount(wave)
        for w in np.flatnonzero(per_wave >= 2):
            tw = t[wave == w]
            assert (tw == _lib.SV_FALLBACK).any() and (tw != _lib.SV_FALLBACK).any(), (ms, w, tw)


@pytest.mark.parametrize("dim,rb", ((2, False), (2, True), (3, True)))
@pytest.mark.parametrize("fb,pdf", CALLS)
def test_dense_waves_hold_fallback_lanes(dim, rb, fb, pdf):
    """Three lanes in four sample: a full wave runs the own generation beside lanes on the sequential loop."""
    p = plan(dim, fb)
    masks, used, res = run("mixed_dense", dim, fb, pdf, rb)["all"]
    wave, _ = SC.wave_of_item(masks)
    t = res["tags"][:used] & ~_lib.SV_PUBLISHED
    assert p["own"] > 0 and 3 * p["wave"] // 4 >= p["own_min"]
    for w in range(len(masks)):
        tw = t[wave == w]
        assert (tw == _lib.SV_FALLBACK).sum() == p["wave"] // 4, w
        assert np.isin(tw[tw != _lib.SV_FALLBACK], (_lib.SV_DENSE_OWN, _lib.SV_DENSE_COOP)).all(), w
    assert (t == _lib.SV_DENSE_OWN).any() and (t == _lib.SV_DENSE_COOP).any()


@pytest.mark.parametrize("dim", (2, 3))
def test_harmonic_balls_are_all_fallback(dim):
    for fb, pdf, rb in variants("harmonic", dim):
        for ms, (masks, used, res) in run("harmonic", dim, fb, pdf, rb).items():
            assert (res["tags"][:used] == _lib.SV_FALLBACK).all(), (fb, rb, ms)  # (and nothing published)


@pytest.mark.parametrize("dim", (2, 3))
@pytest.mark.parametrize("fb,pdf", CALLS)
def test_slow_balls_leave_the_lds_jump_table_and_reach_the_limit(dim, fb, pdf):
    p = plan(dim, fb)
    assert p["jump_lds"] <= SC.LONG_ITERS and p["limit"] == SC.LIMIT
    for ms in ("all", "solo_37", "lanes_3"):
        masks, used, res = run("slow", dim, fb, pdf, False)[ms]
        assert used == SC.case("slow", dim)[0].shape[0] or ms != "all"
        it = res["iters"][:used, 0]
        scale = used / SC.case("slow", dim)[0].shape[0]
        assert (it > SC.LONG_ITERS).sum() >= SC.SLOW_MIN_LONG * scale, ms
        assert (it == SC.LIMIT).sum() >= SC.SLOW_MIN_LIMIT * scale, ms
        assert it.max() <= SC.LIMIT


def test_refusals():
    L = _lib.load()
    INVALID = -1  # include/wos.h WOS_E_INVALID
    n = 4
    it = np.zeros((n, _lib.SV_ITEM), np.float32)
    it[:, 0], it[:, 1], it[:, 2], it[:, 6] = 0.5, 50.0, 1, 1
    seeds = np.arange(n, dtype=np.uint32)
    masks = np.array([0xF], np.uint64)
    out = np.zeros((n, 2, _lib.SV_OUT), np.float32)
    state = np.zeros((n, 2), np.uint64)
    iters = np.zeros((n, 2), np.uint32)
    tags = np.zeros(n, np.int32)
    canary = np.zeros((1, 64), np.uint32)
    ptrs = [it, seeds, masks, out, state, iters, tags, canary]

    def call(dim=2, variant=0, n_=n, null=None, m=masks):
        a = [None if k == null else x.ctypes.data for k, x in enumerate(ptrs)]
        a[2] = None if null == 2 else m.ctypes.data
        return L.wos_selftest_sample_volume(dim, variant, 0, a[0], a[1], n_, a[2], m.size, a[3], a[4], a[5], a[6], a[7],
                                            None, 0)

    assert call() == _lib.WOS_OK
    assert (iters[:, 0] == iters[:, 1]).all() and (iters[:, 0] > 0).all()
    assert call(n_=0, m=np.zeros(1, np.uint64)) == _lib.WOS_OK
    for k in range(len(ptrs)):
        assert call(null=k) == INVALID, k
    assert call(n_=-1) == INVALID
    for dim in (1, 4):
        assert call(dim=dim) == INVALID
    assert call(variant=4) == INVALID
    assert call(m=np.array([0x1F], np.uint64)) == INVALID  # five lanes, four items
    assert call(m=np.array([0x3], np.uint64)) == _lib.WOS_OK  # fewer lanes than items: the rest unused
    r = selftest_sample_volume(3, it[:0], seeds[:0], masks[:0])
    assert r["iters"].shape == (0, 2) and r["plan"]["limit"] == 1000
