"""The walk tape's adjoint on the GPU (include/wos.h "Walk tape adjoint", csrc/wos_tape.hip):
wos_tape_vjp against the host model of tests/tape_adjoint_model.py, built from WalkTape.read.

The yardstick is anchored without the new kernels: the model's float32 forward is bit for bit
tape.solve() (itself bit-exact to the oracle), and its float64 adjoint is that forward's transpose
(tests/test_tape_adjoint_cpu.py).  The source grids are the test's own and non-square -- (5, 7)
and (3, 4, 5) -- so a transposed index shows; geometry, points and parameters come from
tests/variance_cases.py.

The bound, per cell: |vjp - ref| <= (k + 2 wpp + 16) 2^-24 M with M the absolute mass of the
cell's terms and k their count (tape_adjoint_model.tolerance).  Derivation: every addend
a_j (thr nrm) carries three float roundings (a_j, the product thr nrm, their product), the
float atomic sum of k terms in any order at most k - 1 more relative to M, and a_j itself sums at
most 2 wpp terms (the device keeps those sums in double, so they cost one rounding, which the
allowance covers with room)."""
import ctypes as C

import numpy as np
import pytest

import channel_cases as cc
import tape_adjoint_model as tm
import variance_cases as vc
from test_gpu_parity import assert_bits_equal

pytestmark = pytest.mark.gpu

GRID = {2: (5, 7), 3: (3, 4, 5)}


def _source(dim, seed=1, nch=None):
    shape = GRID[dim] if nch is None else (nch,) + GRID[dim]
    return np.random.default_rng(seed).standard_normal(shape).astype(np.float32)


def _scene(c, source="own", **kw):
    from wos_amd import WosScene
    src = _source(c["dim"]) if isinstance(source, str) else source
    return WosScene(c["vertices"], c["prims"], src, c["absorption"], watertight=True, **dict(c["kw"], **kw))


def _prm(c, schedule=0, **flags):
    from wos_amd import solver_params
    return solver_params(dict(c["solver"], **flags), c["output"], schedule=schedule)


def _idx(c):
    return {"index_base": c["index_base"], "index_stride": c["index_stride"]}


def _wpp(tape):
    i = tape.info
    return i["n_tasks"] // i["n_points"]


def _upstream(n, dim, seed=5, nch=None):
    rng = np.random.default_rng(seed)
    lead = () if nch is None else (nch,)
    return rng.standard_normal(lead + (n,)).astype(np.float32), rng.standard_normal(lead + (n, dim)).astype(np.float32)


def _model(tape, c, flags=None):
    segs = tm.read_segments(tape)
    return segs, tm.tape_prm(c["dim"], dict(c["solver"], **(flags or {})), _wpp(tape))


def _within(got, ref, tol, msg):
    assert got.dtype == np.float32
    err = np.abs(got.ravel().astype(np.float64) - ref)
    worst = float(np.max(err / np.maximum(tol, 1e-300)))
    print(f"{msg}: max |vjp - ref| / bound = {worst:.3g}, max |ref| = {np.abs(ref).max():.3g}")
    assert np.all(np.isfinite(got)) and np.all(err <= tol), (msg, worst)


def _check_vjp(tape, c, flags=None, msg=""):
    """vjp(Y) within the bound of the model; the rows of dead outputs are exactly zero."""
    dim, n = c["dim"], c["points"].shape[0]
    cells = int(np.prod(GRID[dim]))
    segs, prm = _model(tape, c, flags)
    P, G = _upstream(n, dim)
    ref, M, k = tm.adjoint(segs, P, G, prm, cells)
    tol = tm.tolerance(M, k, prm["wpp"])
    got = tape.vjp(P, G)
    assert got.shape == GRID[dim]
    assert np.count_nonzero(ref) > cells // 3, "the case must reach the grid"
    _within(got, ref, tol, msg)
    # outputs the forward masks or does not estimate: their upstream does not matter
    ps = np.concatenate([s["pstate"] for s in segs])
    est = (ps & tm.EST) != 0
    dead_p, dead_g = ~est | ((ps & tm.MASK_P) != 0), ~est | ((ps & tm.MASK_G) != 0)
    P1, G1, P0, G0 = P.copy(), G.copy(), P.copy(), G.copy()
    P1[dead_p], G1[dead_g] = 1e3, -1e3
    P0[dead_p], G0[dead_g] = 0.0, 0.0
    _within(tape.vjp(P1, G1), ref, tol, msg + " dead rows perturbed")
    zeroed = tape.vjp(P0, G0)
    _within(zeroed, ref, tol, msg + " dead rows zeroed")
    once = k <= 1  # a single addend: no summation order
    assert_bits_equal(zeroed.ravel()[once], tape.vjp(P1, G1).ravel()[once])
    only_dead_p, only_dead_g = np.where(dead_p, P1, 0).astype(np.float32), np.where(dead_g[:, None], G1, 0).astype(np.float32)
    assert not np.any(tape.vjp(only_dead_p, only_dead_g)), "dead rows alone give exactly zero"
    return {"segs": segs, "prm": prm, "ref": ref, "tol": tol, "got": got, "ps": ps, "k": k}


# ---- 1. the model is the engine -------------------------------------------------------------
@pytest.mark.parametrize("name", ["karman_w40", "dirichlet_w40", "cube3d_w24"])
def test_model_forward_is_the_replay_bit_for_bit(gpu, name):
    c = vc.case(name)
    sc = _scene(c)
    tape = sc.record(c["points"], _prm(c), **_idx(c))
    p, g, _, n_est, _ = tape.solve(counts=True)
    segs, prm = _model(tape, c)
    mp, mg, mn = tm.forward(segs, _source(c["dim"]), prm, np.float32)
    assert_bits_equal(mp, p)
    assert_bits_equal(mg.ravel(), g.ravel())
    np.testing.assert_array_equal(mn, n_est)
    assert np.count_nonzero(p) > c["points"].shape[0] // 2
    tape.close()
    sc.close()


# ---- 2. the transpose against the float64 model ---------------------------------------------------
CASES = {
    "karman_w40": ("karman_w40", {}, 0),
    "karman_w2": ("karman_w2", {}, 0),
    "cv_off": ("karman_nocv_w40", {}, 0),
    "antithetic_off": ("karman_noanti_w40", {}, 0),
    "strided_keys": ("karman_idx_w40", {}, 0),
    "dirichlet_masked_shell": ("dirichlet_w40", {}, 0),
    "cube3d": ("cube3d_w24", {}, 0),
    "dropped_walks": ("karman_w40", {"maxWalkLength": 3}, 0),
    "geom_global": ("karman_w40", {}, "gg"),
}


@pytest.mark.parametrize("label", list(CASES))
def test_vjp_against_model(gpu, label):
    from wos_amd import _lib
    name, flags, sched = CASES[label]
    c = vc.case(name)
    sc = _scene(c)
    tape = sc.record(c["points"], _prm(c, schedule=_lib.SCHED_GEOM_GLOBAL if sched else 0, **flags), **_idx(c))
    if sched:
        assert tape.record_stats["geom_global"] == 1
    r = _check_vjp(tape, c, flags, label)
    if label == "dropped_walks":
        rec = np.concatenate([(s["code"] & 1) != 0 for s in r["segs"]])
        assert 0 < rec.sum() < rec.size
    if label == "dirichlet_masked_shell":
        assert np.any((r["ps"] & (tm.MASK_P | tm.MASK_G)) != 0)
    if label == "karman_w40":
        assert np.any((r["ps"] & tm.EST) == 0)
    tape.close()
    sc.close()


def test_vjp_long_walks_cross_chunks(gpu):
    """The ring of test_gpu_tape.test_replay_long_walks_cross_chunks: walks of more than two chunks."""
    from wos_amd import workloads
    c = vc.case("karman_w40")
    c["solver"] = dict(c["solver"], russianRouletteThreshold=0.01)
    cfg = workloads.karman_config(n_walks=40)
    ctr, r = workloads.karman_obstacle(workloads.scene_size(workloads.KARMAN_OBJ))
    th = np.linspace(0, 2 * np.pi, 1500, endpoint=False)
    ring = np.stack([ctr[0] + (r + 2e-3) * np.cos(th), ctr[1] + (r + 2e-3) * np.sin(th)], 1)
    c["points"] = np.ascontiguousarray(np.concatenate([cfg["points"][:64], cfg["points"][6241:6242], ring]), np.float32)
    sc = _scene(c)
    tape = sc.record(c["points"], _prm(c))
    info = tape.info
    assert info["max_entries_per_walk"] > 2 * info["replay_chunk_entries"], info
    _check_vjp(tape, c, msg="long walks")
    tape.close()
    sc.close()


def test_vjp_across_batches(gpu):
    from wos_amd import set_max_batch_tasks, workloads
    c = vc.case("karman_w128")
    c["solver"] = dict(c["solver"], nWalks=64)
    c["points"] = np.ascontiguousarray(workloads.karman_config(n_walks=64)["points"][:1100])
    prm = _prm(c)
    sc = _scene(c)
    whole = sc.record(c["points"], prm)
    prev = set_max_batch_tasks(2 ** 16)  # 1024 points per batch: two segments
    try:
        split = sc.record(c["points"], prm)
        assert split.segments == [1024, 76] and whole.segments == [1100]
        r = _check_vjp(split, c, msg="two segments")
        P, G = _upstream(1100, 2)
        _within(whole.vjp(P, G), r["ref"], r["tol"], "one segment, same bound")
    finally:
        set_max_batch_tasks(prev)
    _within(split.vjp(P, G), r["ref"], r["tol"], "two segments, default cap")
    for t in (split, whole):
        t.close()
    sc.close()


# ---- 3. end to end, the forward engine as the yardstick -------------------------------------------------
@pytest.mark.parametrize("nch", [1, 4])
def test_transpose_identity_against_the_forward_engine(gpu, nch):
    """|<Y, solve(f) - solve(0)> - <vjp(Y), f>| <= 2 sum |f| tol, both sides summed in float64.
    On karman the boundary data are zero, so solve(0) = 0 and every rounding of the forward is
    relative to terms the bound's mass holds."""
    c = vc.case("karman_w40")
    dim, n = c["dim"], c["points"].shape[0]
    cells = int(np.prod(GRID[dim]))
    multi = nch > 1
    f = _source(dim, seed=9, nch=nch if multi else None)
    sc = _scene(c, source=f)
    tape = sc.record(c["points"], _prm(c))
    P, G = _upstream(n, dim, seed=3, nch=nch if multi else None)
    p1, g1, _ = tape.solve()
    got = tape.vjp(P, G)
    assert got.shape == f.shape
    sc.set_source(np.zeros_like(f))
    p0, g0, _ = tape.solve()
    assert np.all(np.isfinite(got))
    segs, prm = _model(tape, c)
    f64 = lambda a: np.asarray(a, np.float64).reshape((nch, -1))
    lhs = np.sum(f64(P) * (f64(p1) - f64(p0)), 1) + np.sum(f64(G) * (f64(g1) - f64(g0)), 1)
    rhs = np.sum(f64(got) * f64(f), 1)
    for ch in range(nch):
        _, M, k = tm.adjoint(segs, f64(P)[ch], f64(G)[ch].reshape(n, dim), prm, cells)
        bound = 2 * np.sum(np.abs(f64(f)[ch]) * tm.tolerance(M, k, prm["wpp"]))
        print(f"C={nch} channel {ch}: lhs {lhs[ch]:.9g} rhs {rhs[ch]:.9g} |diff| {abs(lhs[ch] - rhs[ch]):.3g} bound {bound:.3g}")
        assert abs(lhs[ch]) > bound, "the identity must not hold trivially"
        assert abs(lhs[ch] - rhs[ch]) <= bound
    tape.close()
    sc.close()


# ---- 4. channels ---------------------------------------------------------------------------------------------
def test_channels_are_independent(gpu):
    c = vc.case("dirichlet_w40")
    dim, n = c["dim"], c["points"].shape[0]
    cells = int(np.prod(GRID[dim]))
    sc = _scene(c)
    tape = sc.record(c["points"], _prm(c))
    segs, prm = _model(tape, c)
    P, G = _upstream(n, dim, seed=8, nch=4)
    P[2], G[2] = 0.0, 0.0
    single = [tape.vjp(P[ch], G[ch]) for ch in range(4)]
    sc.set_source(_source(dim, seed=2, nch=4))
    got = tape.vjp(P, G)
    sc.set_source(_source(dim, seed=4, nch=4), dirichlet_values=cc.DIRICHLET_VALUES)
    other = tape.vjp(P, G)  # neither the source values nor the constants enter
    assert got.shape == (4,) + GRID[dim]
    for ch in range(4):
        ref, M, k = tm.adjoint(segs, P[ch], G[ch], prm, cells)
        tol = tm.tolerance(M, k, prm["wpp"])
        for arr, what in ((got[ch], "plane"), (single[ch], "one channel"), (other[ch], "other source and constants")):
            _within(np.ascontiguousarray(arr), ref, tol, f"channel {ch} {what}")
    assert not np.any(got[2]) and not np.any(single[2]) and np.any(got[0])
    tape.close()
    sc.close()


# ---- 5. ignoreSource --------------------------------------------------------------------------------------------
def test_ignore_source_gives_zero(gpu):
    c = vc.case("karman_w40")
    sc = _scene(c)
    tape = sc.record(c["points"], _prm(c, ignoreSource=True))
    P, G = _upstream(c["points"].shape[0], 2)
    got = tape.vjp(P, G)
    assert got.shape == GRID[2] and not np.any(got)
    tape.close()
    sc.close()


# ---- 6. refusals -----------------------------------------------------------------------------------------------
def test_refusals(gpu):
    from wos_amd import WalkTape, WosError, _lib
    L = _lib.load()
    c = vc.case("karman_w40")
    prm = _prm(c)
    n = c["points"].shape[0]
    P, G = _upstream(n, 2)
    sc = _scene(c)
    tape = sc.record(c["points"], prm)

    def refused(what, fn):
        with pytest.raises(WosError) as e:
            fn()
        assert "(-1)" in str(e.value) and what in str(e.value), str(e.value)

    other = _scene(c)
    alias = WalkTape(other, tape._h, n, None, {})
    refused("another scene", lambda: alias.vjp(P, G))
    alias._h = None
    other.close()
    sc.set_source(_source(2)[:-1])
    refused("source dims", lambda: tape.vjp(P, G))
    sc.set_source(_source(2, nch=2))
    out = np.zeros((2,) + GRID[2], np.float32)
    assert L.wos_tape_vjp(tape._h, sc._h, 1, P.ctypes.data, G.ctypes.data, out.ctypes.data, None, None, 0) == -1
    assert b"n_channels" in L.wos_last_error()
    sc.set_source(_source(2))
    assert L.wos_tape_vjp(tape._h, sc._h, 1, None, None, out.ctypes.data, None, None, 0) == -1
    assert b"both upstream" in L.wos_last_error()
    with pytest.raises(WosError):
        tape.vjp(None, None)
    with pytest.raises(WosError):
        tape.vjp(P[:-1], G)
    # a tape recorded without a source grid
    bare = _scene(c, source=None)
    bare_tape = bare.record(c["points"], prm)
    assert L.wos_tape_vjp(bare_tape._h, bare._h, 1, P.ctypes.data, G.ctypes.data, out.ctypes.data, None, None, 0) == -1
    assert b"null source" in L.wos_last_error()
    bare_tape.close()
    bare.close()
    # wos_tape_read out of range
    buf = np.zeros(8, np.float32)
    T = n * _wpp(tape)
    for seg, field, off, cnt in ((1, 0, 0, 1), (-1, 0, 0, 1), (0, 99, 0, 1), (0, -1, 0, 1), (0, 0, T, 1), (0, 0, -1, 1),
                                 (0, 0, 0, T + 1), (0, 0, 0, -1), (0, 13, n, 1), (0, 2, T + 1, 1), (0, 14, 0, 2),
                                 (0, 8, 2 * T, 1)):
        assert L.wos_tape_read(tape._h, seg, field, off, cnt, buf.ctypes.data) == -1, (seg, field, off, cnt)
        assert b"wos_tape_read" in L.wos_last_error()
    assert L.wos_tape_read(tape._h, 0, 8, 2 * T - 1, 1, buf.ctypes.data) == 0
    with pytest.raises(WosError):
        tape.read("nothing")
    # none of it disturbed the tape
    segs, mprm = _model(tape, c)
    ref, M, k = tm.adjoint(segs, P, G, mprm, 35)
    _within(tape.vjp(P, G), ref, tm.tolerance(M, k, mprm["wpp"]), "after the refusals")
    tape.close()
    sc.close()


# ---- 7. plumbing ------------------------------------------------------------------------------------------------------
def test_plumbing(gpu):
    import torch
    from wos_amd import _lib, release_caches
    L = _lib.load()
    c = vc.case("karman_w40")
    prm = _prm(c)
    n = c["points"].shape[0]
    P, G = _upstream(n, 2)
    sc = _scene(c)
    tape = sc.record(torch.from_numpy(c["points"]).cuda(), prm)
    segs, mprm = _model(tape, c)
    ref, M, k = tm.adjoint(segs, P, G, mprm, 35)
    tol = tm.tolerance(M, k, mprm["wpp"])
    before = [t.cpu().numpy() for t in tape.solve()[:2]]
    # torch tensors on a side stream
    side = torch.cuda.Stream()
    got = tape.vjp(torch.from_numpy(P).cuda(), torch.from_numpy(G).cuda(), stream=side)
    assert got.is_cuda and tuple(got.shape) == GRID[2] and got.dtype == torch.float32
    _within(got.cpu().numpy(), ref, tol, "torch, side stream")
    assert tape.last_vjp_stats["kernel_ms"] > 0 and tape.last_vjp_stats["walks_recorded"] == tape.record_stats["walks_recorded"]
    # the forward after a backward is undisturbed
    after = [t.cpu().numpy() for t in tape.solve()[:2]]
    for a, b in zip(before, after):
        assert_bits_equal(a.ravel(), b.ravel())
    # the C ABI: either upstream null
    out = np.full(GRID[2], np.nan, np.float32)
    zP, zG = np.zeros_like(P), np.zeros_like(G)
    for up_p, up_g, rp, rg in ((P, None, P, zG), (None, G, zP, G)):
        r1, M1, k1 = tm.adjoint(segs, rp, rg, mprm, 35)
        assert L.wos_tape_vjp(tape._h, sc._h, 1, up_p.ctypes.data if up_p is not None else None,
                              up_g.ctypes.data if up_g is not None else None, out.ctypes.data, None, None, 0) == 0
        _within(out, r1, tm.tolerance(M1, k1, mprm["wpp"]), "one upstream null")
        assert np.any(out)
    # WOS_ASYNC with device pointers: a ticket now, the statistics later; the output is overwritten
    dP, dG = torch.from_numpy(P).cuda(), torch.from_numpy(G).cuda()
    dout = torch.full(GRID[2], float("nan"), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    st = _lib.Stats()
    assert L.wos_tape_vjp(tape._h, sc._h, 1, dP.data_ptr(), dG.data_ptr(), dout.data_ptr(), C.byref(st),
                          side.cuda_stream, _lib.WOS_PTRS_DEVICE | _lib.WOS_ASYNC) == 0
    assert st.ticket > 0 and st.walks_recorded == 0
    full = sc.solve_stats(st.ticket)
    assert full["walks_recorded"] == tape.record_stats["walks_recorded"] and full["kernel_ms"] > 0
    assert full["fold_ms"] > 0 and full["walk_ms"] > 0
    _within(dout.cpu().numpy(), ref, tol, "async")
    release_caches()
    _within(tape.vjp(P, G), ref, tol, "after release_caches")
    after = [t.cpu().numpy() for t in tape.solve()[:2]]
    for a, b in zip(before, after):
        assert_bits_equal(a.ravel(), b.ravel())
    tape.close()
    sc.close()


# ---- 8. autograd ------------------------------------------------------------------------------------------------------------
def _projector(reuse=True, **kw):
    import torch
    from wos_amd import projection as pj
    from wos_amd import workloads
    cfg = workloads.karman_config(n_walks=32, n_points=300)
    scene_cfg = dict(workloads.SCENE_BASE, boundary=workloads.KARMAN_OBJ)
    samples = torch.from_numpy(cfg["points"]).cuda()
    return pj.PressureProjector(scene_cfg, cfg["solver"], cfg["output"], samples, reuse_walks=reuse, **kw), cfg


def test_projector_differentiable(gpu):
    import torch
    proj, cfg = _projector()
    plain, _ = _projector(reuse=False)
    n = proj.samples.shape[0]
    div = torch.from_numpy(_source(2, seed=6)).cuda().requires_grad_(True)
    w, v = (torch.from_numpy(a).cuda() for a in _upstream(n, 2, seed=7))
    p, gp = proj.solve(div, differentiable=True)
    assert p.requires_grad and gp.requires_grad
    (torch.sum(w * p) + torch.sum(v * gp)).backward()
    want = proj._tape.vjp(w, v).cpu().numpy()
    segs = tm.read_segments(proj._tape)
    prm = tm.tape_prm(2, cfg["solver"], proj._tape.info["n_tasks"] // n)
    ref, M, k = tm.adjoint(segs, w.cpu().numpy(), v.cpu().numpy(), prm, 35)
    tol = tm.tolerance(M, k, prm["wpp"])
    assert div.grad.shape == div.shape
    _within(div.grad.cpu().numpy(), ref, tol, "div.grad")
    _within(want, ref, tol, "tape.vjp")
    # the variances come along, not differentiable
    out = proj.solve(div, variance=True, differentiable=True)
    assert len(out) == 4 and out[0].requires_grad and not out[2].requires_grad and not out[3].requires_grad
    # differentiable=False: today's outputs, without a graph
    a = proj.solve(div)
    b = plain.solve(div.detach())
    for x, y, z in zip(a, b, (p, gp)):
        assert not x.requires_grad and x.grad_fn is None
        assert_bits_equal(x.cpu().numpy().ravel(), y.cpu().numpy().ravel())
        assert_bits_equal(x.cpu().numpy().ravel(), z.detach().cpu().numpy().ravel())
    with pytest.raises(ValueError):
        plain.solve(div, differentiable=True)
    grouped, _ = _projector(force_gather=True)
    with pytest.raises(ValueError):
        grouped.solve(div, differentiable=True)


def test_training_step_through_the_projection(gpu):
    import torch
    from wos_amd import projection as pj
    from wos_amd import workloads
    proj, cfg = _projector()
    torch.manual_seed(0)
    net = pj.Siren(2, 2, 1, 16).cuda()
    size = workloads.scene_size(workloads.KARMAN_OBJ)
    div = proj.source_from_velocity(net, 6, size, create_graph=True)
    assert div.requires_grad
    detached = proj.source_from_velocity(net, 6, size)
    assert not detached.requires_grad
    assert div.shape == detached.shape and torch.allclose(div.detach(), detached, rtol=1e-5, atol=1e-6)
    p, gp = proj.solve(div, differentiable=True)
    loss = torch.mean(gp ** 2) + torch.mean(p ** 2)
    loss.backward()
    # the divergence does not depend on the last layer's bias; every weight matrix gets a gradient
    weights = [m.weight.grad for m in net.net if isinstance(m, torch.nn.Linear)]
    assert len(weights) == 3
    for g in weights:
        assert g is not None and torch.all(torch.isfinite(g)) and torch.count_nonzero(g) > 0
    for q in net.parameters():
        assert q.grad is None or torch.all(torch.isfinite(q.grad))
