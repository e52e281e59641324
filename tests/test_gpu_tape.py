"""The walk tape on the GPU (include/wos.h "Walk tape", csrc/wos_tape.hip): a replay is bit for
bit the full solve of the same scene, points, indices, parameters and key with the scene's
current source -- in p, grad, p_var, grad_var, n_est and steps.  Every comparison is on uint32
views with NaNs at the same places.  Shapes come from tests/variance_cases.py (every fold
branch: 150 karman points in two blocks + 22, points outside, dropped walks)."""
import ctypes as C
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import channel_cases as cc
import variance_cases as vc
from test_gpu_parity import assert_bits_equal

pytestmark = pytest.mark.gpu

FLOATS, INTS = ("p", "g", "pv", "gv"), ("n", "steps")
COUNTERS = ("walk_steps", "wasted_steps", "walks_recorded", "walks_escaped", "walks_max_length", "walks_rr",
            "walks_dirichlet", "points_estimated", "rejection_iters")


def _out(t):
    p, g, pv, gv, st, n, steps = t
    return {"p": p, "g": g, "pv": pv, "gv": gv, "n": n, "steps": steps, "st": st}


def _same(a, b, msg=""):
    for k in FLOATS:
        assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype == np.float32, (msg, k)
        assert_bits_equal(np.ascontiguousarray(a[k]).ravel(), np.ascontiguousarray(b[k]).ravel())
    for k in INTS:
        np.testing.assert_array_equal(a[k], b[k], err_msg=f"{msg} {k}")


def _scene(c, source="own", **kw):
    from wos_amd import WosScene
    src = c["source"] if isinstance(source, str) else source
    return WosScene(c["vertices"], c["prims"], src, c["absorption"], watertight=True, **dict(c["kw"], **kw))


def _prm(c, schedule=0, **flags):
    from wos_amd import solver_params
    return solver_params(dict(c["solver"], **flags), c["output"], schedule=schedule)


def _idx(c):
    return {"index_base": c["index_base"], "index_stride": c["index_stride"]}


def _fresh(sc, c, prm):
    return _out(sc.solve(c["points"], prm, variance=True, counts=True, **_idx(c)))


def _replay(tape):
    return _out(tape.solve(variance=True, counts=True))


def _record_replay_equals_fresh(c, prm, sc=None, msg=""):
    own = sc is None
    sc = _scene(c) if own else sc
    ref = _fresh(sc, c, prm)
    tape = sc.record(c["points"], prm, **_idx(c))
    got = _replay(tape)
    _same(got, ref, msg)
    for k in COUNTERS:
        assert got["st"][k] == ref["st"][k] == tape.record_stats[k], k
    info = tape.info
    assert info["n_points"] == c["points"].shape[0] and info["dim"] == c["dim"] and info["bytes"] > 0
    tape.close()
    if own:
        sc.close()
    return ref, info


# ---- 1. same source -------------------------------------------------------------------------
SAME_SOURCE = ("karman_w128", "karman_w40", "karman_w2", "karman_noanti_w40", "karman_nocv_w40", "dirichlet_w40",
               "cube3d_w64", "cube3d_w24", "karman_idx_w40")


@pytest.mark.parametrize("name", SAME_SOURCE)
def test_replay_same_source(gpu, name):
    c = vc.case(name)
    ref, info = _record_replay_equals_fresh(c, _prm(c), msg=name)
    assert np.count_nonzero(ref["p"]) > c["points"].shape[0] // 2
    assert info["n_walks"] == c["solver"]["nWalks"] and info["n_entries"] > 0
    assert info["n_tasks"] == c["points"].shape[0] * (c["solver"]["nWalks"] // 2 * 2 if not c["solver"].get(
        "disableGradientAntitheticVariates") else c["solver"]["nWalks"])


# ---- 2. a new source, against the live oracle and a fresh solve ---------------------------------
@pytest.mark.parametrize("name", ["karman_w40", "dirichlet_w40", "cube3d_w24"])
def test_replay_new_source_vs_oracle(gpu, oracle, name):
    c = vc.case(name)
    prm = _prm(c)
    rev = cc.channels(c["source"], 2)[1]
    sc = _scene(c)
    first = _fresh(sc, c, prm)
    tape = sc.record(c["points"], prm, **_idx(c))
    sc.set_source(rev)
    got = _replay(tape)
    osc = oracle.OracleScene(c["vertices"], c["prims"], rev, c["absorption"], watertight=True, **c["kw"])
    po, go, no, so, _ = oracle.solve(osc, oracle.make_params(c["solver"], c["output"]), c["points"], **_idx(c))
    assert_bits_equal(got["p"], po)
    assert_bits_equal(got["g"].ravel(), go.ravel())
    np.testing.assert_array_equal(got["n"], no)
    np.testing.assert_array_equal(got["steps"], so)
    _same(got, _fresh(sc, c, prm), name + " reversed source")
    if name == "karman_w40":  # its field is not symmetric: the reversed source gives another p
        assert not np.array_equal(got["p"], first["p"])
    sc.set_source(c["source"])  # a tape is not consumed
    _same(_replay(tape), first, name + " source set back")
    tape.close()
    sc.close()


# ---- 3. walks longer than two chunks, groups larger than a slice ---------------------------------
def test_replay_long_walks_cross_chunks(gpu):
    """64 karman points, config B's point 6241 (1.25e-6 from the wall), and a ring of 1500 points
    2e-3 outside the cylinder, at 40 walks.  Karman's own roulette threshold (0.99) ends every walk
    within about 200 steps -- the 322 steps DESIGN reports for point 6241 are that point's sum
    over its walks, and with these points the longest recorded walk had 111 entries (190 ring
    points, measured) -- so the threshold is 0.01 here: the walks that creep along the cylinder's
    short segments then live for several hundred steps."""
    from wos_amd import workloads
    c = vc.case("karman_w40")
    c["solver"] = dict(c["solver"], russianRouletteThreshold=0.01)
    cfg = workloads.karman_config(n_walks=40)
    ctr, r = workloads.karman_obstacle(workloads.scene_size(workloads.KARMAN_OBJ))
    th = np.linspace(0, 2 * np.pi, 1500, endpoint=False)
    ring = np.stack([ctr[0] + (r + 2e-3) * np.cos(th), ctr[1] + (r + 2e-3) * np.sin(th)], 1)
    c["points"] = np.ascontiguousarray(np.concatenate([cfg["points"][:64], cfg["points"][6241:6242], ring]), np.float32)
    _, info = _record_replay_equals_fresh(c, _prm(c), msg="long walks")
    print("long walks:", info)
    chunk = info["replay_chunk_entries"]
    assert chunk >= 64
    # one walk spans more than two passes of its wave, so its 64-task group exceeds one LDS slice too
    assert info["max_entries_per_walk"] > 2 * chunk, info
    assert info["n_entries"] > info["max_entries_per_walk"]


# ---- 4. batches ---------------------------------------------------------------------------------
def test_replay_across_batches(gpu):
    from wos_amd import set_max_batch_tasks, workloads
    c = vc.case("karman_w128")
    c["solver"] = dict(c["solver"], nWalks=64)
    c["points"] = np.ascontiguousarray(workloads.karman_config(n_walks=64)["points"][:1100])
    prm = _prm(c)
    sc = _scene(c)
    ref = _fresh(sc, c, prm)
    whole = sc.record(c["points"], prm)
    prev = set_max_batch_tasks(2 ** 16)  # 1024 points per batch: two segments
    try:
        split = sc.record(c["points"], prm)
        got_split = _replay(split)
        got_whole = _replay(whole)  # a tape recorded at another cap replays under this one
    finally:
        set_max_batch_tasks(prev)
    _same(got_split, ref, "two segments")
    _same(got_whole, ref, "one segment")
    _same(_replay(split), ref, "two segments, default cap")
    assert got_split["st"]["walk_launches"] == 2 and got_whole["st"]["walk_launches"] == 1
    assert split.info["n_entries"] == whole.info["n_entries"]
    for t in (split, whole):
        t.close()
    sc.close()


# ---- 5. nothing or little to replay ---------------------------------------------------------------
@pytest.mark.parametrize("flags", [{"ignoreSource": True}, {"maxWalkLength": 3}, {"russianRouletteThreshold": 0.5}],
                         ids=lambda f: next(iter(f)))
def test_replay_degenerate_parameters(gpu, flags):
    c = vc.case("karman_w40")
    ref, info = _record_replay_equals_fresh(c, _prm(c, **flags), msg=str(flags))
    if "ignoreSource" in flags:
        assert info["n_entries"] == 0 and info["max_entries_per_walk"] == 0
    if "maxWalkLength" in flags:
        est = ref["n"] > 0
        assert np.any(ref["n"][est] < 40) and ref["st"]["walks_max_length"] > 0


def test_replay_null_source(gpu):
    c = vc.case("karman_w40")
    sc = _scene(c, source=None)
    ref, info = _record_replay_equals_fresh(c, _prm(c), sc=sc, msg="null source")
    assert info["source_dims"] == [0, 0, 0] and not np.any(ref["p"])
    sc.close()


# ---- 6. source-free terms ----------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
def test_replay_keeps_the_neumann_term(gpu, mode):
    import kat_cases
    k = kat_cases.disk2d_neumann_flux(10.0, mode, n_walks=32, npts=150)
    c = dict(k, index_base=0, index_stride=1)
    ref, _ = _record_replay_equals_fresh(c, _prm(c), msg=k["name"])
    assert np.count_nonzero(ref["p"]) > 100  # all of it from totalNeumann: the source is zero


def test_replay_keeps_image_valued_dirichlet_data(gpu):
    import engine_pin as ep
    from test_engine_pin import _hip_scene
    from wos_amd import solver_params
    U = ep.upstream_scene()
    sel = np.arange(0, U["pts"].shape[0], 13)
    c = {"points": np.ascontiguousarray(U["pts"][sel]), "dim": 2, "index_base": 0, "index_stride": 13}
    sc = _hip_scene(U)
    prm = solver_params(ep.WOST_SOLVER, ep.WOST_OUTPUT)
    assert prm.n_walks == 96
    ref, _ = _record_replay_equals_fresh(c, prm, sc=sc, msg="engine pin")
    assert ref["st"]["walks_dirichlet"] > 0 and np.count_nonzero(ref["p"]) > 500
    sc.close()


# ---- 7. schedule -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["karman_w40", "cube3d_w24"])
def test_record_with_global_geometry(gpu, name):
    from wos_amd import _lib
    c = vc.case(name)
    sc = _scene(c)
    ref = _fresh(sc, c, _prm(c))
    tape = sc.record(c["points"], _prm(c, schedule=_lib.SCHED_GEOM_GLOBAL), **_idx(c))
    assert tape.record_stats["geom_global"] == 1
    _same(_replay(tape), ref, name + " GG recording")
    tape.close()
    sc.close()


# ---- 8. channels -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["karman_w40", "dirichlet_w40", "cube3d_w24"])
def test_replay_channels(gpu, name):
    c = vc.case(name)
    prm = _prm(c)
    sc = _scene(c)
    scalar = _fresh(sc, c, prm)
    tape = sc.record(c["points"], prm, **_idx(c))  # recorded on the one-channel scene
    n = c["points"].shape[0]
    for nch in (2, 3, 4):
        gsets = [None] + ([cc.DIRICHLET_VALUES[:nch]] if name == "dirichlet_w40" else [])
        for gv in gsets:
            sc.set_source(cc.channels(c["source"], nch), dirichlet_values=gv)
            got = _replay(tape)
            assert got["p"].shape == (nch, n) and got["gv"].shape == (nch, n, c["dim"]) and got["n"].shape == (n,)
            _same(got, _fresh(sc, c, prm), f"{name} C={nch} g={gv}")
            if gv is None:
                _same({k: (got[k][0] if k in FLOATS else got[k]) for k in FLOATS + INTS}, scalar, "channel 0")
    sc.set_source(c["source"])
    got = _replay(tape)
    assert got["p"].shape == (n,)
    _same(got, scalar, name + " back to one channel")
    tape.close()
    # and a tape recorded while the scene holds several channels
    sc.set_source(cc.channels(c["source"], 3))
    tape = sc.record(c["points"], prm, **_idx(c))
    _same(_replay(tape), _fresh(sc, c, prm), name + " recorded with 3 channels")
    sc.set_source(c["source"])
    _same(_replay(tape), scalar, name + " recorded with 3 channels, replayed with one")
    tape.close()
    sc.close()


# ---- 9. refusals and hygiene --------------------------------------------------------------------------
def test_refusals_and_hygiene(gpu):
    from wos_amd import WosError, _lib, release_caches
    c = vc.case("karman_w40")
    prm = _prm(c)
    sc = _scene(c)
    ref = _fresh(sc, c, prm)
    tape = sc.record(c["points"], prm)
    L = _lib.load()

    def refused(code, what, fn):
        with pytest.raises(WosError) as e:
            fn()
        assert f"({code})" in str(e.value) and what in str(e.value), str(e.value)

    other = _scene(c)  # same geometry and source, another scene
    other_tape = WalkTapeOn(other, tape)
    refused(-1, "another scene", lambda: other_tape.solve())
    other.close()
    sc.set_source(c["source"][:-1])
    refused(-1, "source dims", lambda: tape.solve())
    sc.set_source(cc.channels(c["source"], 2))
    st = _lib.Stats()
    n = c["points"].shape[0]
    p, g = np.empty((2, n), np.float32), np.empty((2, n, 2), np.float32)
    assert L.wos_tape_solve(tape._h, sc._h, 1, p.ctypes.data, g.ctypes.data, None, None, None, None, C.byref(st), None,
                            0) == -1
    assert b"n_channels" in L.wos_last_error()
    sc.set_source(c["source"])
    refused(-1, "robust_float", lambda: sc.record(c["points"], _prm(c, robustFloatSemantics=True)))
    refused(-1, "nWalks", lambda: sc.record(c["points"], _prm(c, nWalks=0)))
    refused(-1, "maxWalkLength", lambda: sc.record(c["points"], _prm(c, maxWalkLength=-1)))
    refused(-4, "max_bytes", lambda: sc.record(c["points"], prm, max_bytes=4096))
    _same(_fresh(sc, c, prm), ref, "the scene still solves after a refused recording")
    _same(_replay(tape), ref)
    # the tape owns its memory: it outlives the caches, and closing twice is harmless
    release_caches()
    _same(_replay(tape), ref, "after release_caches")
    release_caches()
    tape.close()
    tape.close()
    sc.close()


class WalkTapeOn:
    """tape's handle presented with another scene (what a caller holding raw handles could do)."""

    def __init__(self, scene, tape):
        self.scene, self.tape = scene, tape

    def solve(self):
        from wos_amd import WalkTape
        t = WalkTape(self.scene, self.tape._h, self.tape._n, None, {})
        try:
            return t.solve()
        finally:
            t._h = None  # the handle stays the original tape's


# ---- 10. plumbing -----------------------------------------------------------------------------------------
def test_cuda_tensors_and_side_stream(gpu):
    import torch
    c = vc.case("karman_w40")
    prm = _prm(c)
    sc = _scene(c)
    tape_host = sc.record(c["points"], prm)
    x = torch.from_numpy(c["points"]).cuda()
    tape = sc.record(x, prm)
    rev = cc.channels(c["source"], 2)[1]
    side = torch.cuda.Stream()
    sc.set_source(torch.from_numpy(rev).cuda())  # on torch's current stream; the replay on `side` is ordered after it
    out = tape.solve(variance=True, counts=True, stream=side)
    assert all(t.is_cuda for t in out[:4] + out[5:])
    got = _out(tuple(t.cpu().numpy() if hasattr(t, "cpu") else t for t in out))
    ref = _fresh(sc, c, prm)
    _same(got, ref, "side stream")
    _same(_replay(tape_host), ref, "host tape")
    two = tape.solve()
    assert len(two) == 3 and two[0].is_cuda
    assert_bits_equal(two[0].cpu().numpy(), ref["p"])
    for t in (tape, tape_host):
        t.close()
    sc.close()


def test_c_abi_optional_pointers_and_async(gpu):
    import torch
    from wos_amd import _lib
    L = _lib.load()
    c = vc.case("karman_w40")
    prm = _prm(c)
    sc = _scene(c)
    ref = _fresh(sc, c, prm)
    n = c["points"].shape[0]
    h = C.c_void_p()
    x = np.ascontiguousarray(c["points"])
    assert L.wos_tape_record(sc._h, C.byref(prm), x.ctypes.data, n, 0, 1, 0, C.byref(h), None, None, 0) == 0
    for skip in (None, "pv", "gv", "n", "steps", "all"):
        bufs = {"p": np.empty(n, np.float32), "g": np.empty((n, 2), np.float32), "pv": np.full(n, np.nan, np.float32),
                "gv": np.full((n, 2), np.nan, np.float32), "n": np.full(n, -1, np.int32), "steps": np.full(n, -1, np.int32)}
        gone = {"pv", "gv", "n", "steps"} if skip == "all" else {skip}
        ptr = {k: (None if k in gone else a.ctypes.data) for k, a in bufs.items()}
        assert L.wos_tape_solve(h, sc._h, 1, ptr["p"], ptr["g"], ptr["pv"], ptr["gv"], ptr["n"], ptr["steps"], None, None,
                                0) == 0, L.wos_last_error()
        for k, a in bufs.items():
            if k in gone:
                assert np.all(np.isnan(a)) if a.dtype == np.float32 else np.all(a == -1)
            elif a.dtype == np.float32:
                assert_bits_equal(a.ravel(), ref[k].ravel())
            else:
                np.testing.assert_array_equal(a, ref[k])
    assert L.wos_tape_solve(h, sc._h, 1, None, None, None, None, None, None, None, None, 0) == -1
    # WOS_ASYNC with device pointers: a ticket now, the statistics later
    p = torch.empty(n, dtype=torch.float32, device="cuda")
    g = torch.empty((n, 2), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    st = _lib.Stats()
    side = torch.cuda.Stream()
    assert L.wos_tape_solve(h, sc._h, 1, p.data_ptr(), g.data_ptr(), None, None, None, None, C.byref(st),
                            side.cuda_stream, _lib.WOS_PTRS_DEVICE | _lib.WOS_ASYNC) == 0
    assert st.ticket > 0 and st.walks_recorded == 0
    full = sc.solve_stats(st.ticket)
    assert full["walks_recorded"] == ref["st"]["walks_recorded"] and full["kernel_ms"] > 0
    assert_bits_equal(p.cpu().numpy(), ref["p"])
    assert_bits_equal(g.cpu().numpy().ravel(), ref["g"].ravel())
    info = _lib.TapeInfo()
    assert L.wos_tape_get_info(h, C.byref(info)) == 0 and info.n_points == n
    assert L.wos_tape_destroy(h) == 0
    sc.close()


# ---- 11. projector --------------------------------------------------------------------------------------------
def test_projector_reuse_walks(gpu):
    import torch
    from wos_amd import projection as pj
    from wos_amd import workloads
    cfg = workloads.karman_config(n_walks=32, n_points=600)
    scene_cfg = dict(workloads.SCENE_BASE, boundary=workloads.KARMAN_OBJ)
    samples = torch.from_numpy(cfg["points"]).cuda()
    src = cc.channels(cfg["source"], 4)
    divs = [torch.from_numpy(src[0]).cuda(), torch.from_numpy(src[1]).cuda(), torch.from_numpy(src[3] * 0.5).cuda()]
    plain = pj.PressureProjector(scene_cfg, cfg["solver"], cfg["output"], samples)
    reuse = pj.PressureProjector(scene_cfg, cfg["solver"], cfg["output"], samples, reuse_walks=True)
    vel = pj.Siren(2, 2, 1, 16).cuda()
    prev = pj.Siren(2, 2, 1, 16).cuda()
    for k, div in enumerate(divs):
        a = plain.solve(div, variance=True)
        b = reuse.solve(div, variance=True)
        assert len(a) == len(b) == 4
        for x, y in zip(a, b):
            assert y.is_cuda and x.shape == y.shape
            assert_bits_equal(x.cpu().numpy().ravel(), y.cpu().numpy().ravel())
        for key in COUNTERS:
            assert plain.last_stats[key] == reuse.last_stats[key]
        la = plain.projection_loss(vel, prev, a[1], 256, generator=torch.Generator(device="cuda").manual_seed(k))
        lb = reuse.projection_loss(vel, prev, b[1], 256, generator=torch.Generator(device="cuda").manual_seed(k))
        assert la.item() == lb.item()
    assert reuse._tape is not None and plain._tape is None
    # several channels through the same tape
    a, b = plain.solve(torch.from_numpy(src[:3]).cuda()), reuse.solve(torch.from_numpy(src[:3]).cuda())
    assert b[0].shape == (3, samples.shape[0])
    assert_bits_equal(a[1].cpu().numpy().ravel(), b[1].cpu().numpy().ravel())


def test_projector_reuse_walks_rccl_world1(gpu, tmp_path):
    """reuse_walks over a world-1 RCCL group with force_gather in a fresh process: the shard is
    recorded at global indices and three divs equal the unsharded plain projector's."""
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "tape_projector_worker.py")
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, worker, str(port), str(tmp_path)], env=env, capture_output=True, text=True,
                       timeout=150)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0, r.stderr[-4000:]
    assert "PressureProjector reuse_walks over RCCL" in r.stdout
    d = np.load(tmp_path / "tapeproj.npz")
    assert d["p0"].shape[0] > 900 and int(d["records"]) == 1
    for k in range(3):
        for key in ("p", "g"):
            assert_bits_equal(d[f"{key}{k}"].ravel(), d[f"{key}{k}_ref"].ravel())
        assert d[f"loss{k}"] == d[f"loss{k}_ref"]
    assert not np.array_equal(d["p0"], d["p1"])
