"""Several source fields on one set of walks (wos_solve_channels) on the GPU.

Contract: channel c of a multi-channel solve equals, bit for bit, the single solve of the same
scene with source c and Dirichlet constant g_c -- so the CPU oracle and the unchanged
WosScene.solve are both yardsticks, with no tolerance anywhere.

1. Channel by channel against the live oracle on the cases of tests/variance_cases.py, C = 2, 3, 4.
2. Against the engine's own single solve (1500 karman points x 128 walks), walk counters not
   multiplied by C, one batch and three.
3. Independent of both: negated and scaled channels, a non-finite texel in one channel.
4. Every walk-kernel variant: the schedule bits and robust float semantics.
5. Plumbing: CUDA tensors on a side stream, the raw C ABI with each optional pointer NULL,
   back to one channel, the WOS_E_INVALID cases, PressureProjector (unsharded and through the
   world-1 RCCL gather) and zombie_bindings.wost.
"""
import ctypes as C
import functools
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import channel_cases as cc
import variance_cases as vc
from channel_cases import eq_bits

pytestmark = pytest.mark.gpu

ORACLE_CASES = ("karman_w128", "karman_w40", "karman_w2", "karman_noanti_w40", "karman_nocv_w40", "dirichlet_w40",
                "cube3d_w24", "karman_idx_w40")


# ---------------------------------------------------------------------------------------------
# 1. the live oracle
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _oracle_case(name, own_g):
    """The oracle's solve of each of the case's four channel sources (own_g: with the channel's own
    Dirichlet constant), computed once and shared by the C = 2, 3, 4 runs."""
    import oracle_lib
    c = vc.case(name)
    prm = oracle_lib.make_params(c["solver"], c["output"])
    out = []
    for k, src in enumerate(cc.channels(c["source"], 4)):
        kw = dict(c["kw"])
        if own_g:
            kw["dirichlet_value"] = cc.DIRICHLET_VALUES[k]
        sc = oracle_lib.OracleScene(c["vertices"], c["prims"], src, c["absorption"], watertight=True, **kw)
        p, g, n, steps, _, m2 = oracle_lib.solve(sc, prm, c["points"], index_base=c["index_base"],
                                                 index_stride=c["index_stride"], m2=True)
        pv = np.where(p != 0, vc.expected_variance(m2, n), np.float32(0)).astype(np.float32)
        for a in (p, g, n, steps, pv):
            a.setflags(write=False)
        out.append({"p": p, "g": g, "n": n, "steps": steps, "pv": pv})
    return out


def _check_vs_oracle(name, nch, own_g):
    from wos_amd import WosScene, solver_params
    c = vc.case(name)
    ref = _oracle_case(name, own_g)
    gvals = cc.DIRICHLET_VALUES[:nch] if own_g else None
    sc = WosScene(c["vertices"], c["prims"], cc.channels(c["source"], nch), c["absorption"], watertight=True,
                  dirichlet_values=gvals, **c["kw"])
    assert sc.channels == nch
    p, g, pv, gv, st, n_est, steps = sc.solve(c["points"], solver_params(c["solver"], c["output"]), variance=True,
                                              counts=True, index_base=c["index_base"], index_stride=c["index_stride"])
    sc.close()
    n = c["points"].shape[0]
    assert p.shape == (nch, n) and g.shape == (nch, n, c["dim"]) and pv.shape == p.shape and gv.shape == g.shape
    assert n_est.shape == (n,) and steps.shape == (n,)
    np.testing.assert_array_equal(n_est, ref[0]["n"])
    np.testing.assert_array_equal(steps, ref[0]["steps"])
    assert st["walks_recorded"] == int(ref[0]["n"].sum())
    assert np.count_nonzero(ref[0]["p"]) > n // 2 and np.count_nonzero(ref[0]["pv"]) > n // 2
    for k in range(nch):
        np.testing.assert_array_equal(ref[k]["n"], ref[0]["n"])  # the premise (tests/test_channels_cpu.py)
        eq_bits(p[k], ref[k]["p"], f"{name} C={nch} channel {k}: p")
        eq_bits(g[k], ref[k]["g"], f"{name} C={nch} channel {k}: grad")
        eq_bits(pv[k], ref[k]["pv"], f"{name} C={nch} channel {k}: p_var")


@pytest.mark.parametrize("nch", [2, 3, 4])
@pytest.mark.parametrize("name", ORACLE_CASES)
def test_channels_bit_exact_vs_oracle(gpu, oracle, name, nch):
    _check_vs_oracle(name, nch, own_g=False)


@pytest.mark.parametrize("nch", [2, 3, 4])
def test_channels_own_dirichlet_values_vs_oracle(gpu, oracle, nch):
    _check_vs_oracle("dirichlet_w40", nch, own_g=True)


# ---------------------------------------------------------------------------------------------
# 2. the engine's own single solve
# ---------------------------------------------------------------------------------------------
N_LIVE = 1500
COUNTERS = ("walk_steps", "wasted_steps", "walks_recorded", "walks_escaped", "walks_max_length", "walks_rr",
            "walks_dirichlet", "points_estimated", "rejection_iters")


@pytest.fixture(scope="module")
def karman():
    import objparse
    from wos_amd import solver_params, workloads
    cfg = workloads.karman_config(n_walks=128)
    v, ix = objparse.load(cfg["obj"], 2)
    return {"cfg": cfg, "v": v, "ix": ix, "pts": np.ascontiguousarray(cfg["points"][:N_LIVE]),
            "prm": solver_params(cfg["solver"], cfg["output"]), "src": cc.channels(cfg["source"], 4)}


@pytest.fixture(scope="module")
def karman_single(gpu, karman):
    """WosScene.solve of every channel source alone (one-channel scenes), shared and left unchanged."""
    from wos_amd import WosScene
    sc = WosScene(karman["v"], karman["ix"], karman["src"][0], 350.0, watertight=True)
    out = []
    for k in range(4):
        sc.set_source(karman["src"][k])
        assert sc.channels == 1
        p, g, pv, gv, st, n, steps = sc.solve(karman["pts"], karman["prm"], variance=True, counts=True)
        assert p.shape == (N_LIVE,)
        for a in (p, g, pv, gv, n, steps):
            a.setflags(write=False)
        out.append({"p": p, "g": g, "pv": pv, "gv": gv, "n": n, "steps": steps, "st": st})
    sc.close()
    return out


def _solve_karman(karman, nch, **kw):
    from wos_amd import WosScene
    sc = WosScene(karman["v"], karman["ix"], karman["src"][:nch], 350.0, watertight=True)
    try:
        return sc.solve(karman["pts"], karman["prm"], variance=True, counts=True, **kw)
    finally:
        sc.close()


def _check_vs_single(out, single, nch):
    p, g, pv, gv, st, n, steps = out
    for k in range(nch):
        eq_bits(p[k], single[k]["p"], f"channel {k}: p")
        eq_bits(g[k], single[k]["g"], f"channel {k}: grad")
        eq_bits(pv[k], single[k]["pv"], f"channel {k}: p_var")
        eq_bits(gv[k], single[k]["gv"], f"channel {k}: grad_var")
    np.testing.assert_array_equal(n, single[0]["n"])
    np.testing.assert_array_equal(steps, single[0]["steps"])
    for key in COUNTERS:  # the walks are counted once, not once per channel
        assert st[key] == single[0]["st"][key], key


def test_channels_equal_single_solves(gpu, karman, karman_single):
    out = _solve_karman(karman, 3)
    assert out[4]["walk_launches"] == 1
    assert np.count_nonzero(out[0][0]) > 0.9 * N_LIVE and np.count_nonzero(out[3][1]) > 0.9 * 2 * N_LIVE
    _check_vs_single(out, karman_single, 3)


def test_channels_equal_single_solves_across_batches(gpu, karman, karman_single):
    """A batch is sized in walk tasks whatever their size in bytes (60 + 12 (C - 1) per task), so
    1500 points x 128 walks at 2^16 tasks per batch are three batches of 512 points, as for one
    channel (solve_locked: chunk = max_batch_tasks / walks per point)."""
    from wos_amd.engine import set_max_batch_tasks
    prev = set_max_batch_tasks(2 ** 16)
    try:
        out = _solve_karman(karman, 3)
    finally:
        set_max_batch_tasks(prev)
    assert out[4]["walk_launches"] == 3
    _check_vs_single(out, karman_single, 3)


# ---------------------------------------------------------------------------------------------
# 3. independent of the oracle and of the single solve
# ---------------------------------------------------------------------------------------------
def _small(name, src, **kw):
    from wos_amd import WosScene, solver_params
    c = vc.case(name)
    sc = WosScene(c["vertices"], c["prims"], src, c["absorption"], watertight=True, **c["kw"])
    try:
        return sc.solve(c["points"], solver_params(c["solver"], c["output"], **kw), variance=True, counts=True)
    finally:
        sc.close()


@pytest.mark.parametrize("name", ["karman_w40", "cube3d_w24"])
def test_negated_and_scaled_channels(gpu, name):
    f = vc.case(name)["source"]
    src = cc.channels(f, 4)
    src[1] = f * np.float32(2.0 ** -3)  # exact: a power of two
    p, g, pv, gv, _, _, _ = _small(name, src)
    assert np.count_nonzero(p[0]) > p.shape[1] // 2 and np.count_nonzero(pv[0]) > p.shape[1] // 2
    # value comparisons: -0 == +0
    np.testing.assert_array_equal(p[3], -p[0])
    np.testing.assert_array_equal(g[3], -g[0])
    eq_bits(pv[3], pv[0], "variance of the negated channel")
    eq_bits(gv[3], gv[0], "gradient variance of the negated channel")
    np.testing.assert_array_equal(p[1], p[0] * np.float32(2.0 ** -3))
    np.testing.assert_array_equal(g[1], g[0] * np.float32(2.0 ** -3))
    np.testing.assert_array_equal(pv[1], pv[0] * np.float32(2.0 ** -6))
    np.testing.assert_array_equal(gv[1], gv[0] * np.float32(2.0 ** -6))
    assert not np.any(p[2]) and not np.any(g[2]) and not np.any(pv[2]) and not np.any(gv[2])


def test_nonfinite_texel_stays_in_its_channel(gpu):
    f = vc.case("karman_w40")["source"]
    src = cc.channels(f, 3)
    clean = _small("karman_w40", src)
    bad = src.copy()
    # a texel that walks of point 20 read (found with one-hot sources on the oracle: p[20] != 0)
    assert f.shape == (401, 1002)
    bad[1, 19, 482] = np.inf
    dirty = _small("karman_w40", bad)
    for k in (0, 2):
        for a, b in zip(clean[:4], dirty[:4]):
            eq_bits(a[k], b[k], f"channel {k} beside a non-finite texel in channel 1")
    np.testing.assert_array_equal(clean[5], dirty[5])
    np.testing.assert_array_equal(clean[6], dirty[6])
    assert not np.isfinite(dirty[0][1][20]), "the texel is read by a walk of point 20"


# ---------------------------------------------------------------------------------------------
# 4. every kernel variant
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=["karman_w40", "cube3d_w24"])
def default_schedule(request, gpu):
    name = request.param
    src = cc.channels(vc.case(name)["source"], 3)
    out = _small(name, src)
    for a in out[:4] + out[5:]:
        a.setflags(write=False)
    return name, src, out


@pytest.mark.parametrize("bits", range(1, 8))
def test_schedule_variants(gpu, default_schedule, bits):
    from wos_amd import _lib
    name, src, want = default_schedule
    sched = ((_lib.SCHED_GEOM_GLOBAL if bits & 1 else 0) | (_lib.SCHED_FULL_NEUMANN if bits & 2 else 0) |
             (_lib.SCHED_NO_TAIL_SPREAD if bits & 4 else 0))
    out = _small(name, src, schedule=sched)
    assert out[4]["geom_global"] == (bits & 1)
    for k, (a, b) in enumerate(zip(out[:4], want[:4])):
        eq_bits(a, b, f"{name} schedule {sched:#x}: output {k}")
    np.testing.assert_array_equal(out[5], want[5])
    np.testing.assert_array_equal(out[6], want[6])
    assert out[4]["walk_steps"] == want[4]["walk_steps"] and out[4]["walks_recorded"] == want[4]["walks_recorded"]


@pytest.mark.parametrize("name", ["karman_w40", "cube3d_w24"])
def test_robust_float_channels(gpu, name):
    from wos_amd import WosScene, solver_params
    c = vc.case(name)
    src = cc.channels(c["source"], 3)
    prm = solver_params(dict(c["solver"], robustFloatSemantics=True), c["output"])
    assert prm.robust_float == 1
    sc = WosScene(c["vertices"], c["prims"], src, c["absorption"], watertight=True, **c["kw"])
    p, g, pv, gv, st, n, steps = sc.solve(c["points"], prm, variance=True, counts=True)
    assert sc.channels == 3 and np.count_nonzero(p[0]) > p.shape[1] // 2
    for k in range(3):
        sc.set_source(src[k])
        p1, g1, pv1, gv1, st1, n1, steps1 = sc.solve(c["points"], prm, variance=True, counts=True)
        eq_bits(p[k], p1, f"robust channel {k}: p")
        eq_bits(g[k], g1, f"robust channel {k}: grad")
        eq_bits(pv[k], pv1, f"robust channel {k}: p_var")
        eq_bits(gv[k], gv1, f"robust channel {k}: grad_var")
        np.testing.assert_array_equal(n, n1)
        np.testing.assert_array_equal(steps, steps1)
        assert st["walk_steps"] == st1["walk_steps"] and st["rejection_iters"] == st1["rejection_iters"]
    sc.close()


# ---------------------------------------------------------------------------------------------
# 5. plumbing
# ---------------------------------------------------------------------------------------------
N_PLUMB = 300


def test_channels_cuda_tensors_async(gpu, karman, karman_single):
    import torch
    from wos_amd import WosScene
    x = torch.from_numpy(karman["pts"][:N_PLUMB]).cuda()
    sc = WosScene(karman["v"], karman["ix"], torch.from_numpy(karman["src"][:3]).cuda(), 350.0, watertight=True)
    side = torch.cuda.Stream()
    p, g, pv, gv, st, n, steps = sc.solve(x, karman["prm"], stream=side, sync=False, variance=True, counts=True)
    assert all(t.is_cuda for t in (p, g, pv, gv, n, steps))
    assert p.shape == (3, N_PLUMB) and g.shape == (3, N_PLUMB, 2) and n.shape == (N_PLUMB,)
    assert set(k for k, v in st.items() if v) == {"ticket"}
    full = sc.solve_stats(st["ticket"])  # waits for the enqueued solve
    assert full["walks_recorded"] == int(karman_single[0]["n"][:N_PLUMB].sum())
    for k in range(3):
        eq_bits(p[k].cpu().numpy(), karman_single[k]["p"][:N_PLUMB])
        eq_bits(g[k].cpu().numpy(), karman_single[k]["g"][:N_PLUMB])
        eq_bits(pv[k].cpu().numpy(), karman_single[k]["pv"][:N_PLUMB])
        eq_bits(gv[k].cpu().numpy(), karman_single[k]["gv"][:N_PLUMB])
    np.testing.assert_array_equal(n.cpu().numpy(), karman_single[0]["n"][:N_PLUMB])
    # one channel with the axis keeps the axis
    sc.set_source(torch.from_numpy(karman["src"][1:2]).cuda())
    assert sc.channels == 1
    p1, g1, _ = sc.solve(x, karman["prm"])
    assert p1.shape == (1, N_PLUMB) and g1.shape == (1, N_PLUMB, 2)
    eq_bits(p1[0].cpu().numpy(), karman_single[1]["p"][:N_PLUMB])
    sc.close()


def test_channels_c_abi_optional_pointers_and_errors(gpu, karman, karman_single):
    from wos_amd import WosScene, _lib
    L = _lib.load()
    n, nch = N_PLUMB, 3
    x = np.ascontiguousarray(karman["pts"][:n])
    sc = WosScene(karman["v"], karman["ix"], karman["src"][:nch], 350.0, watertight=True)
    assert L.wos_scene_channels(sc._h) == nch

    def call(skip):
        bufs = {"p": np.empty((nch, n), np.float32), "g": np.empty((nch, n, 2), np.float32),
                "p_var": np.full((nch, n), np.nan, np.float32), "grad_var": np.full((nch, n, 2), np.nan, np.float32),
                "n_est": np.full(n, -1, np.int32), "steps": np.full(n, -1, np.int32)}
        ptr = {k: (None if k == skip else a.ctypes.data) for k, a in bufs.items()}
        st = _lib.Stats()
        rc = L.wos_solve_channels(sc._h, C.byref(karman["prm"]), x.ctypes.data, n, 0, 1, nch, ptr["p"], ptr["g"],
                                  ptr["p_var"], ptr["grad_var"], ptr["n_est"], ptr["steps"], C.byref(st), None, 0)
        assert rc == 0, L.wos_last_error()
        for k in range(nch):
            eq_bits(bufs["p"][k], karman_single[k]["p"][:n])
            eq_bits(bufs["g"][k], karman_single[k]["g"][:n])
            if skip != "p_var":
                eq_bits(bufs["p_var"][k], karman_single[k]["pv"][:n], f"p_var without {skip}")
            if skip != "grad_var":
                eq_bits(bufs["grad_var"][k], karman_single[k]["gv"][:n], f"grad_var without {skip}")
        if skip != "n_est":
            np.testing.assert_array_equal(bufs["n_est"], karman_single[0]["n"][:n])
        if skip != "steps":
            np.testing.assert_array_equal(bufs["steps"], karman_single[0]["steps"][:n])

    for skip in (None, "p_var", "grad_var", "n_est", "steps"):
        call(skip)

    def invalid(rc):
        assert rc == -1, rc  # WOS_E_INVALID
        msg = L.wos_last_error().decode()
        assert msg, "wos_last_error() says why"
        return msg

    p, g = np.empty((4, n), np.float32), np.empty((4, n, 2), np.float32)
    st = _lib.Stats()
    prm = C.byref(karman["prm"])
    # the one-channel entry points refuse a multi-channel scene instead of solving channel 0
    assert "channels" in invalid(L.wos_solve(sc._h, prm, x.ctypes.data, n, 0, 1, p.ctypes.data, g.ctypes.data, None,
                                             None, C.byref(st), None, 0))
    assert "channels" in invalid(L.wos_solve_var(sc._h, prm, x.ctypes.data, n, 0, 1, p.ctypes.data, g.ctypes.data,
                                                 p.ctypes.data, g.ctypes.data, None, None, C.byref(st), None, 0))
    bp = _lib.BvcParams()
    L.wos_default_bvc_params(C.byref(bp))
    bp.grid_res = 4
    sol, grad = np.empty(16, np.float32), np.empty(32, np.float32)
    assert "channels" in invalid(L.wos_bvc(sc._h, prm, C.byref(bp), sol.ctypes.data, grad.ctypes.data, None, 0, None,
                                           C.byref(st)))
    # a channel count that is not the scene's, or out of range
    for bad in (2, 4, 0, 5, -1):
        invalid(L.wos_solve_channels(sc._h, prm, x.ctypes.data, n, 0, 1, bad, p.ctypes.data, g.ctypes.data, None, None,
                                     None, None, C.byref(st), None, 0))
    dims = (C.c_int32 * 3)(*karman["src"].shape[1:], 0)
    big = np.zeros((5,) + karman["src"].shape[1:], np.float32)
    for bad in (0, 5):
        invalid(L.wos_scene_set_source_channels(sc._h, big.ctypes.data, bad, dims, None, 0, None))
    assert L.wos_scene_channels(sc._h) == nch, "a refused call changes nothing"
    # wos_scene_set_source returns the scene to one channel: wos_solve is the parent path again
    src1 = np.ascontiguousarray(karman["src"][1])
    assert L.wos_scene_set_source(sc._h, src1.ctypes.data, dims, 0, None) == 0
    assert L.wos_scene_channels(sc._h) == 1
    rc = L.wos_solve(sc._h, prm, x.ctypes.data, n, 0, 1, p.ctypes.data, g.ctypes.data, None, None, C.byref(st), None, 0)
    assert rc == 0, L.wos_last_error()
    eq_bits(p[0], karman_single[1]["p"][:n], "wos_solve after wos_scene_set_source")
    eq_bits(g[0], karman_single[1]["g"][:n])
    # with one channel wos_solve_channels is wos_solve_var
    rc = L.wos_solve_channels(sc._h, prm, x.ctypes.data, n, 0, 1, 1, p.ctypes.data, g.ctypes.data, p[1].ctypes.data,
                              None, None, None, C.byref(st), None, 0)
    assert rc == 0, L.wos_last_error()
    eq_bits(p[0], karman_single[1]["p"][:n])
    eq_bits(p[1], karman_single[1]["pv"][:n])
    sc.close()


def test_dirichlet_values_refused_with_a_dirichlet_image(gpu):
    from wos_amd import WosError, WosScene
    c = vc.case("dirichlet_w40")
    kw = dict(c["kw"])
    kw.pop("dirichlet_value")
    sc = WosScene(c["vertices"], c["prims"], c["source"], c["absorption"], watertight=True,
                  dirichlet_image=np.ones((4, 4), np.float32), dirichlet_image_box=(0.0, 0.0, 1.0, 1.0), **kw)
    src = cc.channels(c["source"], 2)
    with pytest.raises(WosError, match="Dirichlet image"):
        sc.set_source(src, dirichlet_values=(1.0, 2.0))
    assert sc.channels == 1
    sc.set_source(src)  # the image is shared by the channels
    assert sc.channels == 2
    sc.close()


def test_pressure_projector_channels(gpu, karman, karman_single):
    import torch
    from wos_amd import projection as pj
    from wos_amd import workloads
    cfg = karman["cfg"]
    scene_cfg = dict(workloads.SCENE_BASE, boundary=workloads.KARMAN_OBJ)
    samples = torch.from_numpy(karman["pts"][:N_PLUMB]).cuda()
    proj = pj.PressureProjector(scene_cfg, cfg["solver"], cfg["output"], samples)
    div = torch.from_numpy(karman["src"][:3]).cuda()
    out = proj.solve(div, variance=True)
    assert len(out) == 4 and all(t.is_cuda for t in out) and out[0].shape == (3, N_PLUMB)
    for k in range(3):
        for t, key in zip(out, ("p", "g", "pv", "gv")):
            eq_bits(t[k].cpu().numpy(), karman_single[k][key][:N_PLUMB], f"projector channel {k} {key}")
    two = proj.solve(div)
    assert len(two) == 2 and two[1].shape == (3, N_PLUMB, 2)
    eq_bits(two[1][1].cpu().numpy(), karman_single[1]["g"][:N_PLUMB])
    # and back to a plain source
    one = proj.solve(div[0])
    assert one[0].shape == (N_PLUMB,)
    eq_bits(one[0].cpu().numpy(), karman_single[0]["p"][:N_PLUMB])


def test_pressure_projector_channels_rccl_world1(gpu, tmp_path):
    """force_gather on a world-1 RCCL group in a fresh process: a (3, H, W) div through ONE
    all_gather_into_tensor of 3 (2 + 2 dim) columns equals the unsharded projector's bit for bit."""
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "channels_projector_worker.py")
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, worker, str(port), str(tmp_path)], env=env, capture_output=True, text=True,
                       timeout=150)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0, r.stderr[-4000:]
    assert "PressureProjector channels over RCCL" in r.stdout
    d = np.load(tmp_path / "chproj.npz")
    n = d["p"].shape[1]
    assert n > 900 and d["p"].shape == (3, n) and d["gv"].shape == (3, n, 2) and int(d["collectives"]) == 1
    for k in ("p", "g", "pv", "gv"):
        eq_bits(d[k], d[k + "1"], k)
    eq_bits(d["p2"], d["p"])
    eq_bits(d["g2"], d["g"])
    assert np.count_nonzero(d["pv"][:2]) > 1600 and not np.any(d["p"][2])


def test_wost_channels(gpu, karman, karman_single):
    import torch
    import zombie_bindings
    from wos_amd import workloads
    cfg = karman["cfg"]
    scene_cfg = dict(workloads.SCENE_BASE, boundary=workloads.KARMAN_OBJ)
    scene = zombie_bindings.Scene(scene_cfg, karman["src"][:2])
    assert scene.dim == 2 and scene._scene.channels == 2
    pts = karman["pts"][:N_PLUMB]
    out = zombie_bindings.wost(scene, cfg["solver"], cfg["output"], pts, return_numpy=True, return_variance=True)
    assert len(out) == 5 and out[1].shape == (2, N_PLUMB) and out[2].shape == (2, N_PLUMB, 2)
    for k in range(2):
        eq_bits(out[1][k], karman_single[k]["p"][:N_PLUMB])
        eq_bits(out[2][k], karman_single[k]["g"][:N_PLUMB])
        eq_bits(out[3][k], karman_single[k]["pv"][:N_PLUMB])
        eq_bits(out[4][k], karman_single[k]["gv"][:N_PLUMB])
    # nested lists, like the reference's return, with the channel axis outermost
    out = zombie_bindings.wost(scene, cfg["solver"], cfg["output"], pts.tolist())
    assert len(out) == 3 and isinstance(out[1], list) and len(out[1]) == 2 and len(out[2][0][0]) == 2
    eq_bits(np.asarray(out[1], np.float32), np.stack([karman_single[k]["p"][:N_PLUMB] for k in range(2)]))
    # CUDA tensors
    x = torch.from_numpy(pts).cuda()
    out = zombie_bindings.wost(scene, cfg["solver"], cfg["output"], x)
    assert out[0] is x and out[1].is_cuda and out[1].shape == (2, N_PLUMB)
    eq_bits(out[2][1].cpu().numpy(), karman_single[1]["g"][:N_PLUMB])
    # the reference's own call pattern is untouched
    plain = zombie_bindings.Scene(scene_cfg, karman["src"][0])
    out = zombie_bindings.wost(plain, cfg["solver"], cfg["output"], pts, return_numpy=True)
    assert len(out) == 3 and out[1].shape == (N_PLUMB,)
    eq_bits(out[1], karman_single[0]["p"][:N_PLUMB])
