"""Geometry queries without a GPU (include/wos.h "Geometry queries"): the entry point is declared,
exported and bound, the ABI version did not move, and wos_amd.projection.MeshSDF's forward sign
and backward formula agree with a float64 numpy model on a stub scene whose `query` is a numpy
brute force over a box's segments."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import wos_amd
from wos_amd import _lib, workloads
from wos_amd.projection import MeshSDF, divergence

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "wos.h")


def test_query_entry_point_declared_exported_and_bound():
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\bint\s+wos_scene_query\s*\(\s*wos_scene\s*\*", txt)
    assert re.search(r"WOS_QUERY_NEUMANN\s*=\s*0\s*,\s*WOS_QUERY_DIRICHLET\s*=\s*1", txt)
    L = wos_amd.load_library()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r"\bT (wos_[a-z0-9_]+)$", out, flags=re.M))
    assert "wos_scene_query" in exported and "wos_scene_query" in _lib.EXPORTS and hasattr(L, "wos_scene_query")
    assert len(L.wos_scene_query.argtypes) == 11
    assert (_lib.QUERY_NEUMANN, _lib.QUERY_DIRICHLET) == (0, 1)
    assert (_lib.STATE_ESTIMATED, _lib.STATE_MASK_P, _lib.STATE_MASK_GRAD, _lib.STATE_INSIDE) == (1, 2, 4, 8)


def test_abi_version_unchanged():
    assert wos_amd.load_library().wos_abi_version() == _lib.ABI_VERSION == 10
    assert re.search(r"#define WOS_ABI_VERSION 10\b", open(HEADER).read())


# ---- MeshSDF against a float64 model ------------------------------------------------------------
def _model(v, ix, x):
    """float64 brute force over segments a -> b with normal (s.y, -s.x): (dist, signed, closest,
    direction); the last segment among exact ties, direction 0 where dist is 0."""
    v, x = np.asarray(v, np.float64), np.asarray(x, np.float64)
    a, b = v[ix[:, 0]], v[ix[:, 1]]
    s = b - a
    t = np.clip(((x[:, None, :] - a[None]) * s[None]).sum(-1) / (s * s).sum(-1)[None], 0.0, 1.0)
    cp = a[None] + t[..., None] * s[None]
    d = np.linalg.norm(x[:, None, :] - cp, axis=-1)
    best = d.shape[1] - 1 - np.argmin(d[:, ::-1], axis=1)
    rows = np.arange(x.shape[0])
    cp, d = cp[rows, best], d[rows, best]
    nrm = np.stack([s[best, 1], -s[best, 0]], -1)
    sgn = np.where(((x - cp) * nrm).sum(-1) > 0, 1.0, -1.0)
    direction = np.where(d[:, None] > 0, (x - cp) / np.where(d > 0, d, 1.0)[:, None], 0.0)
    return d, sgn * d, cp, direction


class StubScene:
    """The part of WosScene MeshSDF uses, on the host: query() answers in numpy like the engine
    does for host input."""
    dim = 2

    def __init__(self):
        self.v, self.ix = workloads.box_2d(1.0)  # counter-clockwise: normals outward, inside negative
        self.calls = 0

    def query(self, pts, *, which="neumann", boundary_distance_mask=0.0, closest=False, stream=None):
        assert which == "neumann" and closest
        x = pts.detach().cpu().numpy() if torch.is_tensor(pts) else np.asarray(pts)
        assert x.ndim == 2 and x.shape[1] == 2 and x.dtype == np.float32
        self.calls += 1
        d, sd, cp, _ = _model(self.v, self.ix, x)
        state = np.where(sd < 0, 9, 4).astype(np.int32)
        return d.astype(np.float32), sd.astype(np.float32), state, cp.astype(np.float32)


# interior and exterior points whose closest point is inside a segment, and one ON a segment
PTS = np.array([[0.25, 0.125], [0.75, 0.625], [0.5, 0.0], [1.25, 0.5], [0.375, -0.5], [0.875, 0.25],
                [-0.125, 0.75]], np.float32)
ON = 2  # PTS[ON] lies on the bottom segment: dist == 0


@pytest.mark.parametrize("positive,sign", [("inside", -1.0), ("outside", 1.0)])
def test_meshsdf_forward_sign_and_backward_formula(positive, sign):
    st = StubScene()
    d64, sd64, cp64, dir64 = _model(st.v, st.ix, PTS)
    assert d64[ON] == 0.0 and (sd64 < 0).sum() == 3 and (sd64 > 0).sum() == 3
    x = torch.from_numpy(PTS.copy()).requires_grad_(True)
    val = MeshSDF(st, positive)(x)
    assert val.shape == (PTS.shape[0],) and val.dtype == torch.float32 and st.calls == 1
    # the distances here are exact in float32 (dyadic coordinates): the sign is all that can differ
    np.testing.assert_array_equal(val.detach().numpy(), (sign * sd64).astype(np.float32))
    w = torch.tensor([1.0, -2.0, 3.0, 0.5, -0.25, 4.0, 1.5])
    (g,) = torch.autograd.grad((val * w).sum(), x)
    # d value / dx = sign * sgn(signed_dist) * (x - closest) / |x - closest|, 0 where dist == 0
    want = w.numpy()[:, None].astype(np.float64) * sign * np.sign(sd64)[:, None] * dir64
    np.testing.assert_allclose(g.numpy(), want, rtol=0, atol=4 * 2.0 ** -24 * np.abs(want).max())
    assert np.array_equal(g.numpy()[ON], [0.0, 0.0])
    # a unit vector wherever the distance is not 0
    unit = np.linalg.norm(g.numpy().astype(np.float64) / w.numpy()[:, None], axis=1)
    np.testing.assert_allclose(np.delete(unit, ON), 1.0, atol=4 * 2.0 ** -24)


def test_meshsdf_grid_input_and_divergence_term():
    """(H, W, 2) in, (H, W) out; divergence(sdf(x)[..., None] * c, x) = c . grad sdf, the term the
    reference's analytic circle SDF contributes to divergence(query_velocity(grid), grid)."""
    st = StubScene()
    H, W = 3, 4
    gx, gy = np.meshgrid((np.arange(W) + 0.5) / 8 + 0.0625, (np.arange(H) + 0.5) / 16, indexing="xy")
    grid = np.stack([gx, gy], -1).astype(np.float32)
    _, sd64, _, dir64 = _model(st.v, st.ix, grid.reshape(-1, 2))
    x = torch.from_numpy(grid).requires_grad_(True)
    sdf = MeshSDF(st, "inside")
    val = sdf(x)
    assert val.shape == (H, W)
    np.testing.assert_array_equal(val.detach().numpy().ravel(), (-sd64).astype(np.float32))
    c = torch.tensor([0.75, -1.25])
    div = divergence(sdf(x)[..., None] * c, x)
    assert div.shape == (H, W, 1)
    want = (-np.sign(sd64)[:, None] * dir64 * c.numpy().astype(np.float64)).sum(-1)
    np.testing.assert_allclose(div.detach().numpy().ravel(), want, rtol=0, atol=8 * 2.0 ** -24)


def test_meshsdf_second_derivative_raises():
    x = torch.from_numpy(PTS.copy()).requires_grad_(True)
    val = MeshSDF(StubScene(), "outside")(x)
    (g,) = torch.autograd.grad((val * val).sum(), x, create_graph=True)
    with pytest.raises(RuntimeError, match="once_differentiable"):
        g.sum().backward()


def test_meshsdf_rejects_bad_arguments():
    with pytest.raises(ValueError, match="positive"):
        MeshSDF(StubScene(), "up")
    with pytest.raises(ValueError, match=r"\[\.\.\., 2\]"):
        MeshSDF(StubScene())(torch.zeros(4, 3))
