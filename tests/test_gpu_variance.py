"""Per-point variance of p and grad p out of the solve (wos_solve_var) on the GPU.

The fold kernel keeps the reference's Welford M2 (SampleStatistics::update, walk_on_stars.h:863-868)
beside the means and returns the getters' values (walk_on_stars.h:811-831):
p_var = solM2 / max(1, n - 1), grad_var[k] = gM2[k] / max(1, n - 1), masked like their means.

1. Bit for bit against tests/golden/variance_cases.npz (the CPU oracle's whole statistics, built
   and tied to the oracle by tests/test_variance_oracle.py) on the cases of tests/variance_cases.py.
2. The solution variance against the live oracle (m2=True): across batches, on CUDA tensors
   enqueued on a side stream, and through the C ABI with either variance pointer NULL.
3. Independent of the oracle: on the harmonic Dirichlet engine scene a walk's value is g at its
   exit, so a second scene with g^2 gives E[g^2] - E[g]^2 from the same walks.
4. The callers: zombie_bindings.wost(..., return_variance=True) and
   PressureProjector.solve(div, variance=True), unsharded and through the RCCL gather.
"""
import ctypes as C
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import engine_pin as ep
import variance_cases as vc

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "variance_cases.npz")


def _eq_bits(a, b, msg=""):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (msg, a.dtype, b.dtype, a.shape, b.shape)
    np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32), err_msg=msg)


# ---------------------------------------------------------------------------------------------
# 1. the fixture
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", vc.CASE_NAMES)
def test_variance_bit_exact_vs_fixture(gpu, name):
    from wos_amd import WosScene, solver_params
    c = vc.case(name)
    fx = np.load(FIXTURE)
    r = {k: fx[f"{name}/{k}"] for k in vc.FIELDS}
    _eq_bits(r["pts"], c["points"], "the fixture was generated on other points")
    sc = WosScene(c["vertices"], c["prims"], c["source"], c["absorption"], watertight=True, **c["kw"])
    prm = solver_params(c["solver"], c["output"])
    kw = dict(index_base=c["index_base"], index_stride=c["index_stride"], counts=True)
    p, g, pv, gv, st, n_est, steps = sc.solve(c["points"], prm, variance=True, **kw)
    p0, g0, st0, n0, steps0 = sc.solve(c["points"], prm, **kw)
    sc.close()
    # the means, counts and steps do not know about the variance
    _eq_bits(p, p0, "p")
    _eq_bits(g, g0, "grad")
    np.testing.assert_array_equal(n_est, n0)
    np.testing.assert_array_equal(steps, steps0)
    assert st["walk_steps"] == st0["walk_steps"] and st["walks_recorded"] == st0["walks_recorded"]
    # ... and are the oracle's
    _eq_bits(p, r["p"], "p vs fixture")
    _eq_bits(g, r["grad"], "grad vs fixture")
    np.testing.assert_array_equal(n_est, r["n_sol"])
    # "oracle output 0 with n_est > 0" is "masked" (test_variance_oracle.py: no unmasked mean is 0)
    live_p = (r["n_sol"] > 0) & (r["p"] != 0)
    live_g = (r["n_sol"] > 0)[:, None] & (r["grad"] != 0)
    assert live_p.sum() > 50 and live_g.sum() > 100
    want_pv = np.where(live_p, vc.expected_variance(r["sol_m2"], r["n_sol"]), np.float32(0)).astype(np.float32)
    want_gv = np.where(live_g, vc.expected_variance(r["g_m2"], r["n_sol"]), np.float32(0)).astype(np.float32)
    _eq_bits(pv, want_pv, "p_var")
    _eq_bits(gv, want_gv, "grad_var")
    assert np.all(pv[~live_p].view(np.uint32) == 0) and np.all(gv[~live_g].view(np.uint32) == 0)
    assert np.any(~live_p) and np.any(pv > 0) and np.all(gv[live_g & (r["n_sol"] > 1)[:, None]] > 0)


# ---------------------------------------------------------------------------------------------
# 2. the live oracle
# ---------------------------------------------------------------------------------------------
N_LIVE = 1500


@pytest.fixture(scope="module")
def karman():
    import objparse
    from wos_amd import WosScene, solver_params, workloads
    cfg = workloads.karman_config(n_walks=128)
    v, ix = objparse.load(cfg["obj"], 2)
    sc = WosScene(v, ix, cfg["source"], 350.0, watertight=True)
    yield {"cfg": cfg, "v": v, "ix": ix, "scene": sc, "pts": np.ascontiguousarray(cfg["points"][:N_LIVE]),
           "prm": solver_params(cfg["solver"], cfg["output"])}
    sc.close()


@pytest.fixture(scope="module")
def karman_oracle(karman, oracle):
    """One oracle solve (m2=True) of the 1500 points, shared and left unchanged."""
    cfg = karman["cfg"]
    osc = oracle.OracleScene(karman["v"], karman["ix"], cfg["source"], 350.0)
    p, g, n, steps, _, m2 = oracle.solve(osc, oracle.make_params(cfg["solver"], cfg["output"], math_mode=0),
                                         karman["pts"], m2=True)
    pv = np.where(p != 0, vc.expected_variance(m2, n), np.float32(0)).astype(np.float32)
    assert np.count_nonzero(pv) > 0.9 * N_LIVE
    for a in (p, g, n, pv):
        a.setflags(write=False)
    return {"p": p, "g": g, "n": n, "pv": pv}


def test_variance_across_batches(gpu, karman, karman_oracle):
    from wos_amd.engine import set_max_batch_tasks
    prev = set_max_batch_tasks(2 ** 16)  # 512 points x 128 walks per batch: three batches
    try:
        p, g, pv, gv, st, n_est, _ = karman["scene"].solve(karman["pts"], karman["prm"], variance=True, counts=True)
    finally:
        set_max_batch_tasks(prev)
    assert st["walk_launches"] == 3
    _eq_bits(p, karman_oracle["p"])
    _eq_bits(g, karman_oracle["g"])
    np.testing.assert_array_equal(n_est, karman_oracle["n"])
    _eq_bits(pv, karman_oracle["pv"], "p_var across batches")
    # one batch gives the same gradient variance
    _, _, pv1, gv1, st1 = karman["scene"].solve(karman["pts"], karman["prm"], variance=True)
    assert st1["walk_launches"] == 1
    _eq_bits(pv1, pv)
    _eq_bits(gv1, gv, "grad_var across batches")


def test_variance_cuda_tensors_async(gpu, karman, karman_oracle):
    import torch
    n = 300
    x = torch.from_numpy(karman["pts"][:n]).cuda()
    side = torch.cuda.Stream()
    p, g, pv, gv, st, n_est, steps = karman["scene"].solve(x, karman["prm"], stream=side, sync=False, variance=True,
                                                           counts=True)
    assert all(t.is_cuda for t in (p, g, pv, gv)) and pv.shape == (n,) and gv.shape == (n, 2)
    assert set(k for k, v in st.items() if v) == {"ticket"}
    full = karman["scene"].solve_stats(st["ticket"])  # waits for the enqueued solve
    assert full["walks_recorded"] == int(karman_oracle["n"][:n].sum())
    _eq_bits(p.cpu().numpy(), karman_oracle["p"][:n])
    _eq_bits(pv.cpu().numpy(), karman_oracle["pv"][:n], "p_var, device pointers, async")
    np.testing.assert_array_equal(n_est.cpu().numpy(), karman_oracle["n"][:n])
    _, _, _, gv_host, _ = karman["scene"].solve(karman["pts"][:n], karman["prm"], variance=True)
    _eq_bits(gv.cpu().numpy(), gv_host, "grad_var, device vs host pointers")


def test_variance_c_abi_either_pointer_null(gpu, karman, karman_oracle):
    from wos_amd import _lib
    L = _lib.load()
    n = 300
    x = np.ascontiguousarray(karman["pts"][:n])
    _, _, _, gv_ref, _ = karman["scene"].solve(x, karman["prm"], variance=True)

    def call(want_pv, want_gv):
        p, g = np.empty(n, np.float32), np.empty((n, 2), np.float32)
        pv = np.full(n, np.nan, np.float32) if want_pv else None
        gv = np.full((n, 2), np.nan, np.float32) if want_gv else None
        st = _lib.Stats()
        rc = L.wos_solve_var(karman["scene"]._h, C.byref(karman["prm"]), x.ctypes.data, n, 0, 1, p.ctypes.data,
                             g.ctypes.data, pv.ctypes.data if want_pv else None, gv.ctypes.data if want_gv else None,
                             None, None, C.byref(st), None, 0)
        assert rc == 0, L.wos_last_error()
        _eq_bits(p, karman_oracle["p"][:n])
        _eq_bits(g, karman_oracle["g"][:n])
        return pv, gv

    pv, gv = call(True, True)
    _eq_bits(pv, karman_oracle["pv"][:n], "p_var, both pointers")
    _eq_bits(gv, gv_ref)
    pv, gv = call(True, False)
    _eq_bits(pv, karman_oracle["pv"][:n], "p_var only")
    pv, gv = call(False, True)
    _eq_bits(gv, gv_ref, "grad_var only")
    call(False, False)  # wos_solve's path


# ---------------------------------------------------------------------------------------------
# 3. independent of the oracle
# ---------------------------------------------------------------------------------------------
def _engine_scene(U, img):
    from wos_amd import WosScene
    (nv, nix), (dv, dix) = U["neumann"], U["dirichlet"]
    return WosScene(nv, nix, np.zeros((4, 4), np.float32), 0.0, dvertices=dv, dprims=dix, dirichlet_image=img,
                    dirichlet_image_box=U["box"], watertight=True)


def test_solution_variance_equals_second_moment(gpu):
    """Mixed engine scene (harmonic, Dirichlet-terminated: a walk's value is g at its exit), every
    13th pixel, 512 walks: the population form p_var (n - 1) / n against E[g^2] - E[g]^2 from a
    second scene with g^2 on the same walks.  Bound: worst-case float32 accumulation over n Welford
    updates in each of the two means, 8 n 2^-24 max(g)^2."""
    from wos_amd import solver_params
    U = ep.upstream_scene()
    sel = np.arange(0, U["pts"].shape[0], 13)
    pts = U["pts"][sel]
    img = U["dirichlet_image"].astype(np.float32)
    prm = solver_params(dict(ep.WOST_SOLVER, nWalks=512), ep.WOST_OUTPUT)
    sc, sc2 = _engine_scene(U, img), _engine_scene(U, img ** 2)
    p, _, pv, _, st, n_est, _ = sc.solve(pts, prm, variance=True, counts=True, index_base=0, index_stride=13)
    p2, _, _, n2, _ = sc2.solve(pts, prm, counts=True, index_base=0, index_stride=13)
    sc.close()
    sc2.close()
    np.testing.assert_array_equal(n_est, n2)
    assert st["walks_dirichlet"] == st["walks_recorded"] > 0
    ok = (n_est > 1) & (p != 0) & (p2 != 0)
    assert ok.sum() > 1500
    n = n_est[ok].astype(np.float64)
    pop = pv[ok].astype(np.float64) * (n - 1) / n
    ref = p2[ok].astype(np.float64) - p[ok].astype(np.float64) ** 2
    bound = 8.0 * n * 2.0 ** -24 * float(np.abs(img).max()) ** 2
    err = np.abs(pop - ref)
    print(f"variance vs second moment: {ok.sum()} points, max |err| {err.max():.3g}, "
          f"max err/bound {np.max(err / bound):.3g}, max var {pop.max():.3g}, bound {bound.max():.3g}")
    assert pop.max() > 100 * bound.max(), "the comparison resolves the variance"
    assert np.all(err <= bound)
    assert np.all(pv[~((n_est > 0) & (p != 0))] == 0)


# ---------------------------------------------------------------------------------------------
# 4. the callers
# ---------------------------------------------------------------------------------------------
def test_wost_return_variance(gpu, karman, karman_oracle):
    import torch
    import zombie_bindings
    from wos_amd import workloads
    cfg = karman["cfg"]
    scene_cfg = dict(workloads.SCENE_BASE, boundary=workloads.KARMAN_OBJ)
    scene = zombie_bindings.Scene(scene_cfg, cfg["source"])
    n = 300
    pts = karman["pts"][:n]
    _, _, _, gv_ref, _ = karman["scene"].solve(pts, karman["prm"], variance=True)
    # numpy
    out = zombie_bindings.wost(scene, cfg["solver"], cfg["output"], pts, return_numpy=True, return_variance=True)
    assert len(out) == 5 and all(isinstance(a, np.ndarray) for a in out)
    _eq_bits(out[1], karman_oracle["p"][:n])
    _eq_bits(out[3], karman_oracle["pv"][:n], "wost numpy p_var")
    _eq_bits(out[4], gv_ref, "wost numpy grad_var")
    # nested lists, like the reference's return
    out = zombie_bindings.wost(scene, cfg["solver"], cfg["output"], pts.tolist(), return_variance=True)
    assert len(out) == 5 and all(isinstance(a, list) for a in out)
    _eq_bits(np.asarray(out[3], np.float32), karman_oracle["pv"][:n], "wost list p_var")
    _eq_bits(np.asarray(out[4], np.float32), gv_ref, "wost list grad_var")
    assert isinstance(out[4][0], list) and len(out[4][0]) == 2
    # CUDA tensors
    x = torch.from_numpy(pts).cuda()
    out = zombie_bindings.wost(scene, cfg["solver"], cfg["output"], x, return_variance=True)
    assert len(out) == 5 and out[0] is x and all(t.is_cuda for t in out[1:])
    _eq_bits(out[3].cpu().numpy(), karman_oracle["pv"][:n], "wost cuda p_var")
    _eq_bits(out[4].cpu().numpy(), gv_ref, "wost cuda grad_var")
    # the reference's signature and return by default
    out = zombie_bindings.wost(scene, cfg["solver"], cfg["output"], pts, return_numpy=True)
    assert len(out) == 3
    _eq_bits(out[1], karman_oracle["p"][:n])


def test_pressure_projector_variance(gpu, karman, karman_oracle):
    import torch
    from wos_amd import projection as pj
    from wos_amd import workloads
    cfg = karman["cfg"]
    n = 300
    scene_cfg = dict(workloads.SCENE_BASE, boundary=workloads.KARMAN_OBJ)
    samples = torch.from_numpy(karman["pts"][:n]).cuda()
    proj = pj.PressureProjector(scene_cfg, cfg["solver"], cfg["output"], samples)
    div = torch.from_numpy(cfg["source"]).cuda()
    out = proj.solve(div, variance=True)
    assert len(out) == 4 and all(t.is_cuda for t in out)
    assert proj.last_stats["walks_recorded"] == int(karman_oracle["n"][:n].sum())
    _, g_ref, pv_ref, gv_ref, _ = karman["scene"].solve(karman["pts"][:n], karman["prm"], variance=True)
    _eq_bits(out[0].cpu().numpy(), karman_oracle["p"][:n])
    _eq_bits(out[1].cpu().numpy(), g_ref)
    _eq_bits(out[2].cpu().numpy(), karman_oracle["pv"][:n], "projector p_var")
    _eq_bits(out[3].cpu().numpy(), gv_ref, "projector grad_var")
    two = proj.solve(div)
    assert len(two) == 2
    _eq_bits(two[0].cpu().numpy(), karman_oracle["p"][:n])


def test_pressure_projector_variance_rccl_world1(gpu, tmp_path):
    """force_gather on a world-1 RCCL group in a fresh process: the four tensors through ONE
    all_gather_into_tensor of 2 + 2 dim columns equal the unsharded projector's bit for bit."""
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "variance_projector_worker.py")
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, worker, str(port), str(tmp_path)], env=env, capture_output=True, text=True,
                       timeout=150)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0, r.stderr[-4000:]
    assert "PressureProjector variance over RCCL" in r.stdout
    d = np.load(tmp_path / "varproj.npz")
    assert d["p"].shape[0] > 900 and d["gv"].shape == (d["p"].shape[0], 2)
    for k in ("p", "g", "pv", "gv"):
        _eq_bits(d[k], d[k + "1"], k)
    _eq_bits(d["p2"], d["p"])
    _eq_bits(d["g2"], d["g"])
    assert np.count_nonzero(d["pv"]) > 800 and np.count_nonzero(d["gv"]) > 1600
