"""The walk tape's cell-sorted index and the atomic-free adjoint over it on the GPU (include/wos.h
"Walk tape adjoint, indexed", csrc/wos_tape_index.hip): wos_tape_index_build against the host
model of tests/tape_index_model.py, wos_selftest_tape_rowsum bit for bit against the model's
restatement of the reduction order, wos_tape_vjp_indexed against tape_adjoint_model.adjoint within
the bound test_gpu_tape_adjoint.py derives (it holds for any summation order), and the
determinism the feature is for.  Scenes, grids, upstreams and helpers are those of
test_gpu_tape_adjoint.py."""
import ctypes as C

import numpy as np
import pytest

import tape_adjoint_model as tm
import tape_index_model as im
import test_gpu_tape_adjoint as ta
import variance_cases as vc
from test_gpu_parity import assert_bits_equal

pytestmark = pytest.mark.gpu

GRID = ta.GRID


def _bits(a, b):
    a = a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)
    b = b.cpu().numpy() if hasattr(b, "cpu") else np.asarray(b)
    assert a.shape == b.shape
    assert_bits_equal(a.ravel(), b.ravel())


# ---- 1. the sum kernels on hand-built rows, bit for bit ---------------------------------------
def _tile():
    from wos_amd import _lib
    tile = C.c_int32(0)
    _lib.load().wos_selftest_tape_rowsum(None, 0, None, None, None, None, 0, 0, None, C.byref(tile), 0)  # refused
    return int(tile.value)


def _selftest_against_model(row, id, w, T, seed):
    from wos_amd import selftest_tape_rowsum
    rng = np.random.default_rng(seed)
    a, c = rng.standard_normal((4, T)).astype(np.float32), rng.standard_normal((4, T)).astype(np.float32)
    four, tile = selftest_tape_rowsum(row, id, w, a, c)
    assert four.shape == (4, row.size - 1) and four.dtype == np.float32 and tile == _tile()
    for ch in range(4):
        one, _ = selftest_tape_rowsum(row, id, w, a[ch], c[ch])
        assert_bits_equal(one, im.rowsum(row, id, w, a[ch], c[ch], tile))
        assert_bits_equal(four[ch], one)  # a channel's order does not depend on the channel count
    two, _ = selftest_tape_rowsum(row, id, w, a[:2], c[:2])
    assert_bits_equal(two.ravel(), four[:2].ravel())
    return four


def test_selftest_rows_of_every_kind(gpu):
    tile = _tile()
    assert tile >= 256 and tile % im.CHUNK == 0
    rng = np.random.default_rng(11)
    row, id, w = im.selftest_rows(rng, tile)
    k = np.diff(row.astype(np.int64))
    assert k[0] == 0 and k[-1] == 0 and row[-1] % tile != 0
    assert np.any(row[:-1][k > 0] % tile == 0) and np.any(row[1:][k > 0] % tile == 0)  # starts / ends on a boundary
    assert np.any(id >> 31) and not np.all(id >> 31)
    out = _selftest_against_model(row, id, w, 300, 12)
    assert not np.any(out[:, k == 0]) and np.all(out[:, k > 0] != 0)


def test_selftest_one_row_holds_every_term(gpu):
    tile = _tile()
    rng = np.random.default_rng(13)
    n = 5 * tile + 13
    id, w = im.random_terms(rng, n, 77)
    for row in (np.array([0, n], np.uint32), np.array([0, 0, n, n], np.uint32)):
        _selftest_against_model(row, id, w, 77, 14)


def test_selftest_no_terms_gives_exact_zero(gpu):
    from wos_amd import selftest_tape_rowsum
    row = np.zeros(6, np.uint32)
    empty = np.zeros(0, np.uint32)
    a = np.ones((4, 3), np.float32)
    out, _ = selftest_tape_rowsum(row, empty, empty.astype(np.float32), a, a)
    assert out.shape == (4, 5) and not np.any(out.view(np.uint32))


def test_selftest_refusals(gpu):
    from wos_amd import WosError, selftest_tape_rowsum
    a = np.ones(3, np.float32)
    ok_row, ok_id, ok_w = np.array([0, 1, 2], np.uint32), np.array([0, 2], np.uint32), np.ones(2, np.float32)
    selftest_tape_rowsum(ok_row, ok_id, ok_w, a, a)
    for row, id in ((np.array([1, 1, 2], np.uint32), ok_id), (np.array([0, 2, 1], np.uint32), ok_id[:1]),
                    (ok_row, np.array([0, 3], np.uint32)), (ok_row, np.array([0, 3 | im.FIRST], np.uint32))):
        with pytest.raises(WosError):
            selftest_tape_rowsum(row, id, ok_w[:id.size], a, a)
    with pytest.raises(WosError):
        selftest_tape_rowsum(ok_row, ok_id, ok_w, np.ones((5, 3), np.float32), np.ones((5, 3), np.float32))


# ---- 2. the index on real tapes -----------------------------------------------------------------
def _two_segment_case():
    """The recording of test_gpu_tape_adjoint.test_vjp_across_batches."""
    from wos_amd import workloads
    c = vc.case("karman_w128")
    c["solver"] = dict(c["solver"], nWalks=64)
    c["points"] = np.ascontiguousarray(workloads.karman_config(n_walks=64)["points"][:1100])
    return c


def _ring_case():
    """The ring of test_gpu_tape_adjoint.test_vjp_long_walks_cross_chunks."""
    from wos_amd import workloads
    c = vc.case("karman_w40")
    c["solver"] = dict(c["solver"], russianRouletteThreshold=0.01)
    cfg = workloads.karman_config(n_walks=40)
    ctr, r = workloads.karman_obstacle(workloads.scene_size(workloads.KARMAN_OBJ))
    th = np.linspace(0, 2 * np.pi, 1500, endpoint=False)
    ring = np.stack([ctr[0] + (r + 2e-3) * np.cos(th), ctr[1] + (r + 2e-3) * np.sin(th)], 1)
    c["points"] = np.ascontiguousarray(np.concatenate([cfg["points"][:64], cfg["points"][6241:6242], ring]), np.float32)
    return c


def _check_index(tape, cells):
    """read_index equals the model's row, id, w and cell exactly; index_info adds up."""
    before = tape.info
    assert tape.index_info["built"] == 0 and tape.index_info["n_cells"] == cells
    tape.build_index()
    assert tape.info == before, "wos_tape_get_info reports what it reported before (bytes without the index)"
    segs = tm.read_segments(tape)
    n_terms, longest, rows = 0, 0, []
    for s, seg in enumerate(segs):
        row, id, w, cell = im.index(seg, cells)
        np.testing.assert_array_equal(tape.read_index("row", s), row)
        np.testing.assert_array_equal(tape.read_index("id", s), id)
        assert_bits_equal(tape.read_index("w", s), w)
        np.testing.assert_array_equal(tape.read_index("cell", s), cell)
        n_terms += int(row[-1])
        longest = max(longest, int(np.diff(row.astype(np.int64)).max()))
        rows.append(np.diff(row.astype(np.int64)))
    info = tape.index_info
    assert info["built"] == 1 and info["n_segments"] == len(segs) and info["n_terms"] == n_terms > 0
    assert info["max_terms_per_cell"] == longest and info["n_cells"] == cells and info["tile_terms"] == _tile()
    assert info["bytes"] >= 12 * n_terms + 4 * (cells + 1) * len(segs)
    return rows


INDEX_CASES = {
    "karman_long_rows": ("karman_w40", {}, None),
    "karman_sparse_grid": ("karman_w40", {}, (37, 53)),
    "cube3d": ("cube3d_w24", {}, None),
    "dirichlet": ("dirichlet_w40", {}, None),
    "dropped_walks": ("karman_w40", {"maxWalkLength": 3}, None),
}


@pytest.mark.parametrize("label", list(INDEX_CASES))
def test_index_against_model(gpu, label):
    name, flags, grid = INDEX_CASES[label]
    c = vc.case(name)
    shape = grid or GRID[c["dim"]]
    src = np.random.default_rng(1).standard_normal(shape).astype(np.float32)
    sc = ta._scene(c, source=src)
    tape = sc.record(c["points"], ta._prm(c, **flags), **ta._idx(c))
    k = _check_index(tape, int(np.prod(shape)))[0]
    if label == "karman_long_rows":
        assert k.max() > tape.index_info["tile_terms"], "rows that cross tiles"
    if label == "karman_sparse_grid":
        assert np.any(k == 0) and np.any(k == 1)
    if label == "dropped_walks":
        rec = (tape.read("code") & 1) != 0
        assert 0 < rec.sum() < rec.size
    tape.close()
    sc.close()


def test_index_of_two_segments(gpu):
    from wos_amd import set_max_batch_tasks
    c = _two_segment_case()
    sc = ta._scene(c)
    prev = set_max_batch_tasks(2 ** 16)
    try:
        tape = sc.record(c["points"], ta._prm(c))
    finally:
        set_max_batch_tasks(prev)
    assert tape.segments == [1024, 76]
    rows = _check_index(tape, 35)
    assert len(rows) == 2 and rows[1].sum() > 0
    tape.close()
    sc.close()


# ---- 3. the gradient ---------------------------------------------------------------------------
def _check_det(tape, c, flags=None, msg=""):
    """test_gpu_tape_adjoint._check_vjp with deterministic=True: within the derived bound of the
    float64 model (the bound holds for any summation order), dead rows without effect."""
    dim, n = c["dim"], c["points"].shape[0]
    cells = int(np.prod(GRID[dim]))
    segs, prm = ta._model(tape, c, flags)
    P, G = ta._upstream(n, dim)
    ref, M, k = tm.adjoint(segs, P, G, prm, cells)
    tol = tm.tolerance(M, k, prm["wpp"])
    vjp = lambda p, g: tape.vjp(p, g, deterministic=True)
    got = vjp(P, G)
    assert got.shape == GRID[dim] and tape.index_info["built"] == 1
    assert np.count_nonzero(ref) > cells // 3, "the case must reach the grid"
    ta._within(got, ref, tol, msg)
    ps = np.concatenate([s["pstate"] for s in segs])
    est = (ps & tm.EST) != 0
    dead_p, dead_g = ~est | ((ps & tm.MASK_P) != 0), ~est | ((ps & tm.MASK_G) != 0)
    P1, G1, P0, G0 = P.copy(), G.copy(), P.copy(), G.copy()
    P1[dead_p], G1[dead_g] = 1e3, -1e3
    P0[dead_p], G0[dead_g] = 0.0, 0.0
    ta._within(vjp(P1, G1), ref, tol, msg + " dead rows perturbed")
    zeroed = vjp(P0, G0)
    ta._within(zeroed, ref, tol, msg + " dead rows zeroed")
    once = k <= 1
    assert_bits_equal(zeroed.ravel()[once], vjp(P1, G1).ravel()[once])
    only_dead_p = np.where(dead_p, P1, 0).astype(np.float32)
    only_dead_g = np.where(dead_g[:, None], G1, 0).astype(np.float32)
    assert not np.any(vjp(only_dead_p, only_dead_g)), "dead rows alone give exactly zero"
    _bits(vjp(P, G), got)
    return {"ref": ref, "tol": tol, "got": got, "P": P, "G": G}


@pytest.mark.parametrize("label", list(ta.CASES))
def test_indexed_vjp_against_model(gpu, label):
    from wos_amd import _lib
    name, flags, sched = ta.CASES[label]
    c = vc.case(name)
    sc = ta._scene(c)
    tape = sc.record(c["points"], ta._prm(c, schedule=_lib.SCHED_GEOM_GLOBAL if sched else 0, **flags), **ta._idx(c))
    _check_det(tape, c, flags, label)
    tape.close()
    sc.close()


def test_indexed_vjp_long_walks(gpu):
    c = _ring_case()
    sc = ta._scene(c)
    tape = sc.record(c["points"], ta._prm(c))
    info = tape.info
    assert info["max_entries_per_walk"] > 2 * info["replay_chunk_entries"], info
    _check_det(tape, c, msg="long walks")
    tape.close()
    sc.close()


def test_indexed_vjp_across_batches(gpu):
    """One segment against two is compared within the bound only: the segments' sums are added in
    segment order, so the order of a cell's additions differs by construction."""
    from wos_amd import set_max_batch_tasks
    c = _two_segment_case()
    prm = ta._prm(c)
    sc = ta._scene(c)
    whole = sc.record(c["points"], prm)
    prev = set_max_batch_tasks(2 ** 16)
    try:
        split = sc.record(c["points"], prm)
        assert split.segments == [1024, 76] and whole.segments == [1100]
        r = _check_det(split, c, msg="two segments")
    finally:
        set_max_batch_tasks(prev)
    one = whole.vjp(r["P"], r["G"], deterministic=True)
    ta._within(one, r["ref"], r["tol"], "one segment, same bound")
    _bits(split.vjp(r["P"], r["G"], deterministic=True), r["got"])  # the batch cap of the call does not enter
    _bits(whole.vjp(r["P"], r["G"], deterministic=True), one)
    for t in (split, whole):
        t.close()
    sc.close()


def test_ignore_source_gives_exact_zero(gpu):
    c = vc.case("karman_w40")
    sc = ta._scene(c)
    tape = sc.record(c["points"], ta._prm(c, ignoreSource=True))
    P, G = ta._upstream(c["points"].shape[0], 2)
    got = tape.vjp(P, G, deterministic=True)
    assert got.shape == GRID[2] and not np.any(got.view(np.uint32))
    info = tape.index_info
    assert info["built"] == 1 and info["n_terms"] == 0 and info["max_terms_per_cell"] == 0
    assert not np.any(tape.read_index("row")) and tape.read_index("id").size == 0
    tape.close()
    sc.close()


# ---- 4. determinism -----------------------------------------------------------------------------
def test_determinism(gpu):
    import torch
    from wos_amd import _lib, release_caches
    L = _lib.load()
    c = vc.case("karman_w40")
    prm = ta._prm(c)
    n = c["points"].shape[0]
    P, G = ta._upstream(n, 2)
    sc = ta._scene(c)
    tape = sc.record(c["points"], prm)
    base = tape.vjp(P, G, deterministic=True)
    assert np.count_nonzero(base) > 35 // 3
    assert tape.index_info["max_terms_per_cell"] > tape.index_info["tile_terms"], "rows that cross tiles"
    for _ in range(2):
        _bits(tape.vjp(P, G, deterministic=True), base)
    # torch tensors on a side stream
    dP, dG = torch.from_numpy(P).cuda(), torch.from_numpy(G).cuda()
    side = torch.cuda.Stream()
    got = tape.vjp(dP, dG, stream=side, deterministic=True)
    assert got.is_cuda and tape.last_vjp_stats["kernel_ms"] > 0
    _bits(got, base)
    # WOS_ASYNC with device pointers: a ticket now, the statistics later
    dout = torch.full(GRID[2], float("nan"), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    st = _lib.Stats()
    assert L.wos_tape_vjp_indexed(tape._h, sc._h, 1, dP.data_ptr(), dG.data_ptr(), dout.data_ptr(), C.byref(st),
                                  side.cuda_stream, _lib.WOS_PTRS_DEVICE | _lib.WOS_ASYNC) == 0
    assert st.ticket > 0 and st.walks_recorded == 0
    full = sc.solve_stats(st.ticket)
    assert full["walks_recorded"] == tape.record_stats["walks_recorded"] and full["kernel_ms"] > 0
    assert full["fold_ms"] > 0 and full["walk_ms"] > 0
    _bits(dout, base)
    # the index survives release_caches
    release_caches()
    assert tape.index_info["built"] == 1
    _bits(tape.vjp(P, G, deterministic=True), base)
    # a second tape recorded from the same inputs
    twin = sc.record(c["points"], prm)
    _bits(twin.vjp(P, G, deterministic=True), base)
    twin.close()
    tape.close()
    sc.close()


def test_channels_bit_for_bit(gpu):
    """Channel ch of a four-channel call is the single-channel call with upstream ch."""
    c = vc.case("dirichlet_w40")
    dim, n = c["dim"], c["points"].shape[0]
    sc = ta._scene(c)
    tape = sc.record(c["points"], ta._prm(c))
    P, G = ta._upstream(n, dim, seed=8, nch=4)
    P[2], G[2] = 0.0, 0.0
    single = [tape.vjp(P[ch], G[ch], deterministic=True) for ch in range(4)]
    sc.set_source(ta._source(dim, seed=2, nch=4))
    got = tape.vjp(P, G, deterministic=True)
    assert got.shape == (4,) + GRID[dim] and np.any(got[0]) and not np.any(got[2])
    for ch in range(4):
        _bits(np.ascontiguousarray(got[ch]), single[ch])
    sc.set_source(ta._source(dim, seed=3, nch=2))
    two = tape.vjp(P[:2], G[:2], deterministic=True)
    _bits(np.ascontiguousarray(two), np.ascontiguousarray(got[:2]))
    tape.close()
    sc.close()


# ---- 5. refusals and the rest ------------------------------------------------------------------
def test_refusals_and_capacity(gpu):
    from wos_amd import WosError, _lib
    L = _lib.load()
    c = vc.case("karman_w40")
    prm = ta._prm(c)
    n = c["points"].shape[0]
    P, G = ta._upstream(n, 2)
    out = np.zeros(GRID[2], np.float32)
    sc = ta._scene(c)
    tape = sc.record(c["points"], prm)
    before = [a.copy() for a in tape.solve()[:2]]
    # the indexed vjp before the build, and the read
    assert L.wos_tape_vjp_indexed(tape._h, sc._h, 1, P.ctypes.data, G.ctypes.data, out.ctypes.data, None, None, 0) == -1
    assert b"wos_tape_vjp_indexed" in L.wos_last_error() and b"index" in L.wos_last_error()
    with pytest.raises(WosError):
        tape.read_index("row")
    with pytest.raises(WosError):
        tape.read_index("nothing")
    # a cap the build cannot meet: nothing is kept, the tape works as before
    with pytest.raises(WosError) as e:
        tape.build_index(max_bytes=1)
    assert f"({_lib.WOS_E_CAPACITY})" in str(e.value) and "wos_tape_index_build" in str(e.value), str(e.value)
    assert L.wos_tape_index_build(tape._h, 1) == _lib.WOS_E_CAPACITY == -4 and tape.index_info["built"] == 0 and tape.index_info["bytes"] == 0
    for a, b in zip(before, tape.solve()[:2]):
        _bits(a, b)
    segs, mprm = ta._model(tape, c)
    ref, M, k = tm.adjoint(segs, P, G, mprm, 35)
    tol = tm.tolerance(M, k, mprm["wpp"])
    ta._within(tape.vjp(P, G), ref, tol, "the atomic path after a refused build")
    tape.build_index()
    tape.build_index()  # idempotent
    info = tape.index_info
    assert info["built"] == 1
    tape.build_index(max_bytes=1)  # built already: nothing to allocate, nothing to refuse
    assert tape.index_info == info
    got = tape.vjp(P, G, deterministic=True)
    ta._within(got, ref, tol, "after a refused, then an uncapped build")
    ta._within(tape.vjp(P, G), ref, tol, "the atomic path beside the index")
    # a cap the index fits under
    capped = sc.record(c["points"], prm)
    capped.build_index(max_bytes=1 << 30)
    _bits(capped.vjp(P, G, deterministic=True), got)
    capped.close()
    # wos_tape_index_read out of range
    buf = np.zeros(8, np.uint32)
    nt = info["n_terms"]
    for seg, field, off, cnt in ((1, 0, 0, 1), (-1, 0, 0, 1), (0, 9, 0, 1), (0, -1, 0, 1), (0, 0, 36, 1), (0, 0, 0, 37),
                                 (0, 1, nt, 1), (0, 2, -1, 1), (0, 3, 0, nt + 1), (0, 1, 0, -1)):
        assert L.wos_tape_index_read(tape._h, seg, field, off, cnt, buf.ctypes.data) == -1, (seg, field, off, cnt)
        assert b"wos_tape_index_read" in L.wos_last_error()
    assert L.wos_tape_index_read(tape._h, 0, 0, 35, 1, buf.ctypes.data) == 0 and buf[0] == nt
    # the checks wos_tape_vjp makes
    assert L.wos_tape_vjp_indexed(tape._h, sc._h, 1, None, None, out.ctypes.data, None, None, 0) == -1
    assert b"both upstream" in L.wos_last_error()
    sc.set_source(ta._source(2)[:-1])
    with pytest.raises(WosError) as e:
        tape.vjp(P, G, deterministic=True)
    assert "source dims" in str(e.value)
    sc.set_source(ta._source(2))
    # a tape recorded without a source grid
    bare = ta._scene(c, source=None)
    bare_tape = bare.record(c["points"], prm)
    assert L.wos_tape_index_build(bare_tape._h, 0) == -1
    assert b"wos_tape_index_build" in L.wos_last_error() and b"null source" in L.wos_last_error()
    assert bare_tape.index_info["built"] == 0 and bare_tape.index_info["n_cells"] == 0
    bare_tape.close()
    bare.close()
    # the forward after an indexed backward is undisturbed
    for a, b in zip(before, tape.solve()[:2]):
        _bits(a, b)
    tape.close()
    tape.close()
    sc.close()


def test_projector_deterministic_backward(gpu):
    import torch
    proj, cfg = ta._projector(deterministic_backward=True)
    n = proj.samples.shape[0]
    w, v = (torch.from_numpy(a).cuda() for a in ta._upstream(n, 2, seed=7))
    grads = []
    for _ in range(2):
        div = torch.from_numpy(ta._source(2, seed=6)).cuda().requires_grad_(True)
        p, gp = proj.solve(div, differentiable=True)
        (torch.sum(w * p) + torch.sum(v * gp)).backward()
        grads.append(div.grad.cpu().numpy())
    assert proj._tape.index_info["built"] == 1
    _bits(grads[0], grads[1])
    _bits(proj._tape.vjp(w, v, deterministic=True), grads[0])
    segs = tm.read_segments(proj._tape)
    prm = tm.tape_prm(2, cfg["solver"], proj._tape.info["n_tasks"] // n)
    ref, M, k = tm.adjoint(segs, w.cpu().numpy(), v.cpu().numpy(), prm, 35)
    ta._within(grads[0], ref, tm.tolerance(M, k, prm["wpp"]), "div.grad, deterministic")
    plain, _ = ta._projector()
    assert plain.deterministic_backward is False
