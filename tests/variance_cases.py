"""Cases of the variance fixture (tests/golden/variance_cases.npz), shared by its generator
(tests/golden/make_variance_golden.py), the CPU test that regenerates it
(tests/test_variance_oracle.py) and the GPU test that reads it (tests/test_gpu_variance.py).

The quad fold handles 64 points per block in chunks of 16 records, so the shapes are the
smallest that reach every branch: more than two blocks with a ragged last one, walk counts of
several full chunks (128), a ragged last chunk (40 = 16 + 16 + 8), less than one chunk (2) and --
without antithetic pairs -- an odd number of records per chunk boundary; points outside the
domain, points with dropped walks, a Dirichlet boundary, the fourth quad lane (3D), and RNG
keys that are not the point's position in the call.
"""
import numpy as np

from wos_amd import workloads

# the arrays stored per case, in the generator's order
FIELDS = ("pts", "p", "grad", "estimated", "sol_mean", "g_mean", "n_sol", "sol_m2", "g_m2")


def karman_points():
    """150 points: the first 140 of config B (n_est < nWalks occurs among the first 96), then
    points inside the cylinder, beyond the open ends, on / next to the walls (masked)."""
    cfg = workloads.karman_config(n_walks=128)
    c, r = workloads.karman_obstacle(workloads.scene_size(workloads.KARMAN_OBJ))
    extra = np.array([[c[0], c[1]], [c[0] + r * 0.5, c[1]], [-1.2, 0.0], [2.0, 0.0], [0.0, 0.5995],
                      [0.0, -0.5980], [-1.1032, 0.1], [1.9067, -0.2], [0.0, 0.0], [c[0], c[1] + 0.9 * r]], np.float32)
    return np.ascontiguousarray(np.concatenate([cfg["points"][:140], extra]), np.float32)


def _karman(name, n_walks, index_base=0, index_stride=1, **flags):
    import objparse
    cfg = workloads.karman_config(n_walks=n_walks)
    v, ix = objparse.load(cfg["obj"], 2)
    return {"name": name, "dim": 2, "vertices": v, "prims": ix, "source": cfg["source"], "absorption": 350.0,
            "kw": {}, "solver": dict(cfg["solver"], **flags), "output": cfg["output"], "points": karman_points(),
            "index_base": index_base, "index_stride": index_stride}


def _dirichlet(name, n_walks):
    """Config C's geometry (Neumann box around a Dirichlet disk, g = 1): 100 points around the disk."""
    cfg = workloads.dirichlet_obstacle_config(n_walks=n_walks, res=8)
    pts = np.random.default_rng(11).uniform([0.3, 0.15], [0.7, 0.55], (100, 2)).astype(np.float32)
    # none inside the disk's epsilon shell: there a walk ends at once, antithetic pairs cancel and the
    # gradient mean is exactly 0 -- which the GPU test would read as "masked"
    d = pts - np.float32([0.5, 0.35])
    r = np.linalg.norm(d, axis=1)
    shell = np.abs(r - 0.1) < 0.004
    pts[shell] = (np.float32([0.5, 0.35]) + d[shell] * (0.106 / r[shell])[:, None]).astype(np.float32)
    pts[-2:] = np.array([[0.5, 0.0005], [0.9996, 0.5]], np.float32)  # within the mask distance of the walls
    return {"name": name, "dim": 2, "vertices": cfg["vertices"], "prims": cfg["prims"], "source": cfg["source"],
            "absorption": cfg["absorption"],
            "kw": {"dvertices": cfg["dvertices"], "dprims": cfg["dprims"], "dirichlet_value": 1.0},
            "solver": cfg["solver"], "output": cfg["output"], "points": pts, "index_base": 0, "index_stride": 1}


def _cube(name, n_walks):
    import kat_cases
    c = kat_cases.cube3d(n_walks=n_walks, npts=100)
    pts = c["points"].copy()
    pts[-3:] = np.array([[1.5, 0.0, 0.0], [0.0, 0.0, 0.9995], [0.2, -1.0004, 0.3]], np.float32)
    return {"name": name, "dim": 3, "vertices": c["vertices"], "prims": c["prims"], "source": c["source"],
            "absorption": c["absorption"], "kw": {}, "solver": c["solver"], "output": c["output"], "points": pts,
            "index_base": 0, "index_stride": 1}


CASE_BUILDERS = {}
for _nw in (128, 40, 2):
    CASE_BUILDERS[f"karman_w{_nw}"] = (_karman, dict(n_walks=_nw))
    CASE_BUILDERS[f"karman_nocv_w{_nw}"] = (_karman, dict(n_walks=_nw, disableGradientControlVariates=True))
    CASE_BUILDERS[f"karman_noanti_w{_nw}"] = (_karman, dict(n_walks=_nw, disableGradientAntitheticVariates=True))
CASE_BUILDERS["dirichlet_w40"] = (_dirichlet, dict(n_walks=40))
CASE_BUILDERS["cube3d_w64"] = (_cube, dict(n_walks=64))
CASE_BUILDERS["cube3d_w24"] = (_cube, dict(n_walks=24))
CASE_BUILDERS["karman_idx_w40"] = (_karman, dict(n_walks=40, index_base=3, index_stride=7))
CASE_NAMES = tuple(CASE_BUILDERS)


def case(name):
    fn, kw = CASE_BUILDERS[name]
    return fn(name, **kw)


def expected_variance(m2, n):
    """The reference's getters (walk_on_stars.h:811-831) in float: M2 / float(max(1, n - 1))."""
    d = np.maximum(1, np.asarray(n, np.int64) - 1).astype(np.float32)
    if np.ndim(m2) == 2:
        d = d[:, None]
    return (np.asarray(m2, np.float32) / d).astype(np.float32)
