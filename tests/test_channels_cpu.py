"""Several source fields on one set of walks (wos_solve_channels): what can be checked without a GPU.

1. The three new entry points are exported by the built library and declared in include/wos.h.
2. WosScene refuses a source of the wrong rank or with more than four channels before it
   touches a device.
3. wos_amd.dist.sharded_projection carries channel-major results, p [C, n] and grad [C, n, dim]
   (and the variances), through its ONE all-gather with C (1 + dim) columns (doubled with
   variance), bit-identical to the one-process field; its two- and four-tensor forms are unchanged.
4. The premise of the feature, pinned on the CPU oracle: a walk never looks at the source, so the
   counts, the steps and every walk counter are the same for two different sources, and negating
   the source negates p and grad exactly.
"""
import ctypes as C
import os
import re
import socket

import numpy as np
import pytest
import torch.multiprocessing as mp

import channel_cases as cc
import variance_cases as vc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("wos_scene_set_source_channels", "wos_scene_channels", "wos_solve_channels")


# ---------------------------------------------------------------------------------------------
# 1. symbols
# ---------------------------------------------------------------------------------------------
def test_new_entry_points_exported_and_declared():
    from wos_amd import _lib
    lib = C.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(REPO, "include", "wos.h")).read()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), f"{name} is not exported by {_lib.LIB_PATH}"
        assert re.search(r"\b%s\s*\(" % name, header), f"{name} is not declared in include/wos.h"
        assert name in _lib.EXPORTS
    m = re.search(r"#define\s+WOS_MAX_CHANNELS\s+(\d+)", header)
    assert m and int(m.group(1)) == 4 == _lib.MAX_CHANNELS
    assert re.search(r"#define\s+WOS_ABI_VERSION\s+10\b", header), "additive: the ABI version stays"
    assert lib.wos_abi_version() == 10


# ---------------------------------------------------------------------------------------------
# 2. shape validation before any device call
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,shape", [(2, (7,)), (2, (2, 2, 4, 4)), (2, (5, 4, 4)), (2, (0, 4, 4)),
                                       (3, (4, 4)), (3, (5, 2, 2, 2)), (3, (2, 2, 2, 2, 2))])
def test_scene_refuses_bad_source_shape(dim, shape):
    from wos_amd import WosError, WosScene
    v = np.zeros((4, dim), np.float32)
    ix = np.zeros((2, dim), np.int32)
    with pytest.raises(WosError, match="source"):
        # device 99 does not exist: reaching wos_scene_create would fail differently
        WosScene(v, ix, np.zeros(shape, np.float32), 0.0, device=99)


def test_scene_refuses_dirichlet_values_without_channel_axis():
    from wos_amd import WosError, WosScene
    v = np.zeros((4, 2), np.float32)
    ix = np.zeros((2, 2), np.int32)
    with pytest.raises(WosError, match="dirichlet_values"):
        WosScene(v, ix, np.zeros((4, 4), np.float32), 0.0, device=99, dirichlet_values=(1.0,))


# ---------------------------------------------------------------------------------------------
# 3. the gather
# ---------------------------------------------------------------------------------------------
N_PTS, N_WALKS, N_CH = 61, 8, 3


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _oracle_channels(oracle_lib, pts, base=0, stride=1, n_threads=None):
    """(p [C, n], grad [C, n, 2], p_var [C, n], g2 [C, n, 2]) of the karman scene, channel by
    channel; g2 = grad * grad stands in for the gradient variance (the oracle has none)."""
    import objparse
    from wos_amd import workloads
    cfg = workloads.karman_config(n_walks=N_WALKS)
    v, ix = objparse.load(cfg["obj"], 2)
    prm = oracle_lib.make_params(cfg["solver"], cfg["output"], n_threads=n_threads)
    out = []
    for src in cc.channels(cfg["source"], N_CH):
        sc = oracle_lib.OracleScene(v, ix, src, 350.0)
        p, g, n, _, _, m2 = oracle_lib.solve(sc, prm, pts, index_base=base, index_stride=stride, m2=True)
        out.append((p, g, vc.expected_variance(m2, n), g * g))
    return tuple(np.stack([o[k] for o in out]) for k in range(4))


def _points():
    from wos_amd import workloads
    return np.ascontiguousarray(workloads.karman_config(n_walks=N_WALKS)["points"][:N_PTS])


def _gather_worker(rank, world, port, out_dir):
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path[:0] = [here, os.path.join(os.path.dirname(here), "neural-monte-carlo-fluid-simulation_amd")]
    import torch
    import torch.distributed as dist
    import oracle_lib
    from wos_amd import dist as wdist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    pts = _points()
    calls = []
    real = dist.all_gather_into_tensor

    def counted(buf, send, **kw):
        calls.append(tuple(send.shape))
        return real(buf, send, **kw)

    dist.all_gather_into_tensor = counted
    local = {}

    def solve_channels(x, base, stride):
        local["res"] = tuple(torch.from_numpy(a) for a in _oracle_channels(oracle_lib, x, base, stride, n_threads=2))
        assert local["res"][0].shape == (N_CH, x.shape[0]) and local["res"][1].shape == (N_CH, x.shape[0], 2)
        return local["res"]

    out = {}
    # channel-major, with the variances: one collective of C (2 + 2 dim) columns
    full = wdist.sharded_projection(solve_channels, pts, rank, world, 2)
    assert len(calls) == 1 and calls[0][1] == N_CH * 6, calls
    for k, t in zip(("p", "g", "pv", "gv"), full):
        out["v_" + k] = t.numpy()
    # ... and without: C (1 + dim) columns, from the shard already solved
    calls.clear()
    full = wdist.sharded_projection(lambda x, b, s: local["res"][:2], pts, rank, world, 2)
    assert len(calls) == 1 and calls[0][1] == N_CH * 3, calls
    out["p"], out["g"] = full[0].numpy(), full[1].numpy()
    # the two- and four-tensor forms (channel 0 alone, no channel axis) as before
    calls.clear()
    full = wdist.sharded_projection(lambda x, b, s: tuple(t[0] for t in local["res"][:2]), pts, rank, world, 2)
    assert len(calls) == 1 and calls[0][1] == 3 and full[0].shape == (N_PTS,) and full[1].shape == (N_PTS, 2)
    out["p0"], out["g0"] = full[0].numpy(), full[1].numpy()
    calls.clear()
    full = wdist.sharded_projection(lambda x, b, s: tuple(t[0] for t in local["res"]), pts, rank, world, 2)
    assert len(calls) == 1 and calls[0][1] == 6 and len(full) == 4 and full[3].shape == (N_PTS, 2)
    out["pv0"], out["gv0"] = full[2].numpy(), full[3].numpy()
    np.savez(os.path.join(out_dir, f"ch{rank}.npz"), **out)
    dist.barrier()
    dist.destroy_process_group()


@pytest.fixture(scope="module")
def one_process(oracle):
    ref = _oracle_channels(oracle, _points())
    for a in ref:
        a.setflags(write=False)
    return ref


@pytest.mark.parametrize("world", [2, 3])
def test_sharded_projection_channel_major(tmp_path, one_process, world):
    mp.start_processes(_gather_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True,
                       start_method="spawn")
    p, g, pv, gv = one_process
    assert p.shape == (N_CH, N_PTS) and g.shape == (N_CH, N_PTS, 2) and np.count_nonzero(p[0]) > N_PTS // 2
    for r in range(world):
        d = np.load(tmp_path / f"ch{r}.npz")
        cc.eq_bits(d["p"], p, "p")
        cc.eq_bits(d["g"], g, "grad")
        for k, want in zip(("v_p", "v_g", "v_pv", "v_gv"), (p, g, pv, gv)):
            cc.eq_bits(d[k], want, k)
        cc.eq_bits(d["p0"], p[0])
        cc.eq_bits(d["g0"], g[0])
        cc.eq_bits(d["pv0"], pv[0])
        cc.eq_bits(d["gv0"], gv[0])


# ---------------------------------------------------------------------------------------------
# 4. the premise, on the unchanged oracle
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["karman_w40", "cube3d_w24"])
def test_walks_do_not_depend_on_the_source(oracle, name):
    c = vc.case(name)
    pts = c["points"]
    assert pts.shape[0] == (150 if c["dim"] == 2 else 100)
    prm = oracle.make_params(c["solver"], c["output"])
    res = []
    for src in cc.channels(c["source"], 4):
        sc = oracle.OracleScene(c["vertices"], c["prims"], src, c["absorption"], watertight=True, **c["kw"])
        res.append(oracle.solve(sc, prm, pts, index_base=c["index_base"], index_stride=c["index_stride"]))
    (p0, g0, n0, s0, st0), (p1, g1, n1, s1, st1), (p2, _, n2, s2, st2), (p3, g3, n3, s3, st3) = res
    assert n0.sum() > 0 and np.count_nonzero(p0) > pts.shape[0] // 2
    assert not np.array_equal(p0, p1), "the second source is a different field"
    for n, s, st in ((n1, s1, st1), (n2, s2, st2), (n3, s3, st3)):
        np.testing.assert_array_equal(n, n0)
        np.testing.assert_array_equal(s, s0)
        assert st == st0
    assert not np.any(p2), "no source, no Dirichlet data: the solution is 0"
    # negating the source negates every walk's contribution, and rounding is symmetric
    np.testing.assert_array_equal(p3, -p0)
    np.testing.assert_array_equal(g3, -g0)
