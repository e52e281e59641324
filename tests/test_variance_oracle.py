"""The oracle side of the variance outputs (CPU, no GPU).

tests/golden/variance_cases.npz holds the CPU oracle's whole per-point statistics (the M2 of the
solution and of every gradient component) on the cases of tests/variance_cases.py; the GPU test
(tests/test_gpu_variance.py) compares wos_solve_var against it bit for bit.  Here the fixture is
regenerated and tied to the oracle's own exports, and the four-tensor form of
wos_amd.dist.sharded_projection is run over gloo with the oracle as every rank's solver.
"""
import os
import socket
import sys

import numpy as np
import pytest
import torch.multiprocessing as mp

import variance_cases as vc

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_variance_golden as gen  # noqa: E402


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


@pytest.fixture(scope="module")
def regenerated(tmp_path_factory, oracle):
    if gen.compiler() is None:
        pytest.skip("no C compiler: the fixture cannot be regenerated here")
    return gen.generate(str(tmp_path_factory.mktemp("variance") / "variance_cases.npz"))


def test_fixture_reproduced_bit_for_bit(regenerated):
    fx = np.load(gen.FIXTURE)
    assert sorted(fx.files) == sorted(regenerated)
    assert sorted(fx.files) == sorted(f"{n}/{k}" for n in vc.CASE_NAMES for k in vc.FIELDS)
    for key, a in regenerated.items():
        b = fx[key]
        assert a.dtype == b.dtype and a.shape == b.shape, key
        np.testing.assert_array_equal(_bits(a), _bits(b), err_msg=key)


@pytest.mark.parametrize("name", vc.CASE_NAMES)
def test_wrapper_equals_oracle_exports(regenerated, oracle, name):
    """The wrapper's masked outputs, counts and solution M2 are oracle_solve_m2's, and wherever
    the oracle leaves a mean unmasked it is the wrapper's unmasked mean -- all bit for bit."""
    c = vc.case(name)
    r = {k: regenerated[f"{name}/{k}"] for k in vc.FIELDS}
    prm = oracle.make_params(c["solver"], c["output"], math_mode=0)
    p, g, n_est, _, _, m2 = oracle.solve(gen.oracle_scene(c), prm, c["points"], index_base=c["index_base"],
                                         index_stride=c["index_stride"], m2=True)
    np.testing.assert_array_equal(r["n_sol"], n_est)
    np.testing.assert_array_equal(_bits(r["sol_m2"]), _bits(m2))
    np.testing.assert_array_equal(_bits(r["p"]), _bits(p))
    np.testing.assert_array_equal(_bits(r["grad"]), _bits(g))
    live_p, live_g = (n_est > 0) & (p != 0), (n_est > 0)[:, None] & (g != 0)
    assert live_p.sum() > 50 and live_g.sum() > 100
    np.testing.assert_array_equal(_bits(r["sol_mean"][live_p]), _bits(p[live_p]))
    np.testing.assert_array_equal(_bits(r["g_mean"][live_g]), _bits(g[live_g]))


@pytest.mark.parametrize("name", vc.CASE_NAMES)
def test_fixture_zero_means_masked(name):
    """The GPU test reads "oracle output 0 with n_est > 0" as "masked": no estimated fixture
    point may have an unmasked mean that is exactly 0.  And the cases keep what they are for."""
    fx = np.load(gen.FIXTURE)
    r = {k: fx[f"{name}/{k}"] for k in vc.FIELDS}
    live = r["n_sol"] > 0
    assert not np.any(r["sol_mean"][live] == 0)
    assert not np.any(r["g_mean"][live] == 0)
    assert np.all(r["n_sol"][r["estimated"] == 0] == 0)
    assert np.any(r["estimated"] == 0), "points outside the domain"
    assert np.any(live & (r["p"] == 0)) or np.any(live[:, None] & (r["grad"] == 0)), "masked estimated points"
    if name.startswith("karman"):
        n_walks = vc.case(name)["solver"]["nWalks"]
        assert np.any((r["n_sol"][:96] > 0) & (r["n_sol"][:96] < n_walks)) or n_walks == 2, "partly dropped walks"
    nz = r["n_sol"] > 1
    assert np.all(r["sol_m2"][nz] > 0) and np.all(r["g_m2"][nz] > 0)
    assert np.all(r["sol_m2"][r["n_sol"] <= 1] == 0)


# ---------------------------------------------------------------------------------------------
# sharded_projection with a four-tensor solve_local (gloo, the oracle as every rank's solver)
# ---------------------------------------------------------------------------------------------
N_PTS, N_WALKS = 203, 16


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _four_tensor_solver():
    """solve_local -> (p, grad, p_var, grad_var) on the oracle: the solution variance from
    m2=True; the oracle exports no gradient M2, so those columns carry a deterministic stand-in
    (a function of the point's own results only, so it is the same under any sharding)."""
    import torch
    import objparse
    import oracle_lib
    from wos_amd import workloads
    cfg = workloads.karman_config(n_walks=N_WALKS)
    v, ix = objparse.load(cfg["obj"], 2)
    sc = oracle_lib.OracleScene(v, ix, cfg["source"], 350.0)
    prm = oracle_lib.make_params(cfg["solver"], cfg["output"], n_threads=2)

    def solve_local(local, base, stride):
        p, g, n, _, _, m2 = oracle_lib.solve(sc, prm, np.asarray(local), index_base=base, index_stride=stride,
                                             m2=True)
        pv = vc.expected_variance(m2, n)
        gv = (g * g + pv[:, None]).astype(np.float32)
        return tuple(torch.from_numpy(a) for a in (p, g, pv, gv))

    return solve_local, cfg["points"][:N_PTS]


def _worker(rank, world, port, out_dir):
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path[:0] = [here, os.path.join(os.path.dirname(here), "neural-monte-carlo-fluid-simulation_amd")]
    import torch.distributed as dist
    from wos_amd import dist as wdist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    solve_local, pts = _four_tensor_solver()
    out = wdist.sharded_projection(solve_local, pts, rank, world, 2)
    assert len(out) == 4
    np.savez(os.path.join(out_dir, f"var{rank}.npz"), **{k: t.numpy() for k, t in zip("pgvw", out)})
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_sharded_projection_four_tensors(tmp_path, oracle, world):
    mp.start_processes(_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True,
                       start_method="spawn")
    solve_local, pts = _four_tensor_solver()
    one = [t.numpy() for t in solve_local(pts, 0, 1)]
    assert one[0].shape == (N_PTS,) and one[3].shape == (N_PTS, 2) and np.any(one[2] > 0)
    for r in range(world):
        d = np.load(tmp_path / f"var{r}.npz")
        for k, a in zip("pgvw", one):
            assert d[k].shape == a.shape, k
            np.testing.assert_array_equal(_bits(d[k]), _bits(a), err_msg=k)


def test_sharded_projection_two_tensors_unchanged():
    """Two tensors in, two tensors out (world 1, no process group needed)."""
    import torch
    from wos_amd import dist as wdist
    pts = torch.arange(14, dtype=torch.float32).reshape(7, 2)
    out = wdist.sharded_projection(lambda x, b, s: (x[:, 0] * 2, x + 1), pts, 0, 1, 2)
    assert len(out) == 2 and torch.equal(out[0], pts[:, 0] * 2) and torch.equal(out[1], pts + 1)
    with pytest.raises(ValueError):
        wdist.sharded_projection(lambda x, b, s: (x[:, 0], x, x[:, 0]), pts, 0, 1, 2)
