"""Fused SIREN fit step without a GPU (include/wos.h "Fused SIREN fit step"): the entry point is
declared, exported and bound within ABI 10; wos_siren_fit names what it refuses before any device
work; the float64 restatement of the fit loss -- the backward's model seeded with
g_u = 2 scale r / (n d_out) -- equals torch float64 autograd; diagonal_wrap reproduces the karman
and Taylor-Green wraps exactly and refuses one that rotates components; projection_fit_loss draws
what projection_loss draws."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import siren_fit_model as fm
import siren_model as sm
import siren_vjp_model as vm
import wos_amd
from wos_amd import _lib, siren
from wos_amd import projection as pj

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "wos.h")


# ---- ABI ---------------------------------------------------------------------------------------------
def test_fit_entry_point_declared_exported_and_bound():
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\bint\s+wos_siren_fit\s*\((.*?)\)\s*;", txt, flags=re.S)
    assert m, "wos_siren_fit is not declared"
    args = [a.strip() for a in m.group(1).split(",")]
    names = [re.search(r"(\w+)$", a).group(1) for a in args]
    assert names == ["net", "pts", "n", "target", "scale", "loss", "grad_weights", "grad_biases", "workspace_bytes",
                     "flags", "device", "stream"]
    L = wos_amd.load_library()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r"\bT (wos_[a-z0-9_]+)$", out, flags=re.M))
    assert "wos_siren_fit" in exported and "wos_siren_fit" in _lib.EXPORTS and hasattr(L, "wos_siren_fit")
    assert len(L.wos_siren_fit.argtypes) == len(args) == 12
    assert L.wos_siren_fit.argtypes[2] is C.c_int64 and L.wos_siren_fit.argtypes[8] is C.c_size_t
    assert L.wos_abi_version() == _lib.ABI_VERSION == 10
    assert re.search(r"#define WOS_ABI_VERSION 10\b", open(HEADER).read())


# ---- refusals that need no device --------------------------------------------------------------------
def _host_call(d=2, H=64, Lh=1, d_out=2, n=5):
    """A complete host-pointer call of wos_siren_fit as keyword arguments a test can break one at a time."""
    net = sm.make_net(d, H, Lh, d_out)
    p = siren.pack(net)
    nl = Lh + 2
    ws, bs = [t.numpy() for t in p.weights], [t.numpy() for t in p.biases]
    keep = {"ws": ws, "bs": bs, "x": sm.points(d, n), "t": np.zeros((n, d_out), np.float32),
            "loss": np.full(1, 7.0, np.float32), "gw": [np.full(a.shape, 7.0, np.float32) for a in ws],
            "gb": [np.full(a.shape, 7.0, np.float32) for a in bs]}
    w = (C.c_void_p * nl)(*[a.ctypes.data for a in ws])
    b = (C.c_void_p * nl)(*[a.ctypes.data for a in bs])
    keep["net"] = _lib.SirenNet(p.d_in, p.d_out, p.hidden, p.n_hidden_layers, p.omega, w, b)
    keep["pw"] = (C.c_void_p * nl)(*[a.ctypes.data for a in keep["gw"]])
    keep["pb"] = (C.c_void_p * nl)(*[a.ctypes.data for a in keep["gb"]])
    keep["arrays"] = (w, b)
    return keep


def _call(k, **over):
    a = dict(net=k["net"], pts=k["x"].ctypes.data, n=k["x"].shape[0], target=k["t"].ctypes.data, scale=None,
             loss=k["loss"].ctypes.data, gw=k["pw"], gb=k["pb"], ws=0)
    a.update(over)
    L = _lib.load()
    rc = L.wos_siren_fit(C.byref(a["net"]), a["pts"], a["n"], a["target"], a["scale"], a["loss"], a["gw"], a["gb"],
                         a["ws"], 0, 0, None)
    return rc, L.wos_last_error()


def test_refusals_name_the_field_before_any_device_work():
    k = _host_call()
    for field, value, word in (("d_in", 4, b"d_in"), ("d_in", 1, b"d_in"), ("d_out", 0, b"d_out"), ("d_out", 4, b"d_out"),
                               ("hidden", 100, b"hidden"), ("hidden", 288, b"hidden"), ("hidden", 0, b"hidden"),
                               ("n_hidden_layers", 9, b"n_hidden_layers"), ("n_hidden_layers", -1, b"n_hidden_layers"),
                               ("omega", float("inf"), b"omega")):
        bad = _host_call()
        setattr(bad["net"], field, value)
        rc, msg = _call(bad)
        assert rc == -1 and msg.startswith(b"wos_siren_fit") and word in msg, (field, value, msg)
        if field != "omega":
            assert str(value).encode() in msg, (field, value, msg)
    for n in (0, -3):
        rc, msg = _call(k, n=n)
        assert rc == -1 and b"n must be positive" in msg and str(n).encode() in msg, msg
    rc, msg = _call(k, loss=None)
    assert rc == -1 and b"null loss" in msg
    rc, msg = _call(k, target=None)
    assert rc == -1 and b"null target" in msg
    rc, msg = _call(k, pts=None)
    assert rc == -1 and b"null point buffer" in msg
    for one in ("gw", "gb"):
        rc, msg = _call(k, **{one: None})
        assert rc == -1 and b"exactly one of grad_weights and grad_biases is null" in msg, msg
    hole = (C.c_void_p * 3)(k["pw"][0], None, k["pw"][2])
    rc, msg = _call(k, gw=hole)
    assert rc == -1 and b"grad_weights" in msg and b"layer 1" in msg
    hole = (C.c_void_p * 3)(k["pb"][0], k["pb"][1], None)
    rc, msg = _call(k, gb=hole)
    assert rc == -1 and b"grad_biases" in msg and b"layer 2" in msg
    tile = (2 * 1 + 1) * 64 * 4 * 32
    rc, msg = _call(k, ws=tile - 1)
    assert rc == _lib.WOS_E_CAPACITY and b"workspace_bytes" in msg and b"cannot hold one tile" in msg
    assert k["loss"][0] == 7.0 and all(np.all(a == 7.0) for a in k["gw"] + k["gb"]), "a refused call wrote nothing"


def test_python_layer_names_what_it_refuses():
    net = sm.make_net(2, 32, 1)
    x = sm.points(2, 5)
    t = np.zeros((5, 2), np.float32)
    with pytest.raises(ValueError, match=r"points must be \[\.\.\., 2\]"):
        siren.fit(net, np.zeros((5, 3), np.float32), t)
    with pytest.raises(ValueError, match=r"target must have shape \(5, 2\)"):
        siren.fit(net, x, t[:4])
    with pytest.raises(ValueError, match=r"scale must have shape \(5, 2\)"):
        siren.fit(net, x, t, t[:, :1])
    with pytest.raises(ValueError, match="no points"):
        siren.fit(net, x[:0], t[:0])
    with pytest.raises(ValueError, match="workspace_bytes must be >= 0"):
        siren.fit(net, x, t, workspace_bytes=-1)
    for name, args in (("x", (torch.from_numpy(x).requires_grad_(True), torch.from_numpy(t), None)),
                       ("target", (torch.from_numpy(x), torch.from_numpy(t).requires_grad_(True), None)),
                       ("scale", (torch.from_numpy(x), torch.from_numpy(t), torch.ones(5, 2).requires_grad_(True)))):
        with pytest.raises(ValueError, match=f"{name}.requires_grad"):
            siren.fit_loss(net, *args)


# ---- the model ---------------------------------------------------------------------------------------
MODEL_SHAPES = [(2, 32, 1, None), (3, 64, 2, None), (2, 64, 0, None), (3, 32, 1, 1),
                (3, 32, 8, 3), (2, 160, 1, 2), (2, 64, 1, 3)]  # the deepest net, H / 32 = 5, and d_out > d_in


@pytest.mark.parametrize("with_scale", [False, True], ids=["plain", "scale"])
@pytest.mark.parametrize("d,H,L,d_out", MODEL_SHAPES, ids=[f"d{d}_H{H}_L{L}_o{o or d}" for d, H, L, o in MODEL_SHAPES])
def test_float64_model_equals_float64_autograd(d, H, L, d_out, with_scale):
    """Float64 identities: 1e-9 of each tensor's largest entry."""
    net = sm.make_net(d, H, L, d_out)
    x = sm.points(d, 37, seed=3)
    target, scale = fm.problem(37, d_out or d, with_scale, seed=5)
    loss, got, ub = fm.model64(net, x, target, scale)
    want_loss, want = fm.autograd(vm.net64(net), torch.from_numpy(x.astype(np.float64)), target, scale)
    assert abs(loss - want_loss) <= 1e-12 * want_loss and loss > 0
    if with_scale:
        assert np.any(scale == 0) and np.any(ub == 0)
    for kind, G, W in (("w", got[0], want[0]), ("b", got[1], want[1])):
        assert len(G) == len(W) == L + 2
        for l, (a, b) in enumerate(zip(G, W)):
            assert a.shape == b.shape, (kind, l)
            top = np.abs(b).max()
            assert top > 0 and np.abs(a - b).max() <= 1e-9 * top, (kind, l, np.abs(a - b).max(), top)


# ---- diagonal_wrap -----------------------------------------------------------------------------------
def taylorgreen_wrap(size, eps=0.1):
    """query_velocity's taylorgreen branch (src/2d/models/base.py:182-189): both components weighted
    by the clamped distance to their two walls over eps."""
    def wrap(x, u):
        w = [torch.min(torch.abs(x[..., k] - size[2 * k]).clamp(min=0, max=eps),
                       torch.abs(x[..., k] - size[2 * k + 1]).clamp(min=0, max=eps)) / eps for k in range(2)]
        return torch.stack(w, dim=-1) * u
    return wrap


def rotating_wrap(x, u):
    return torch.stack([-u[..., 1], u[..., 0]], dim=-1)


def test_diagonal_wrap_reproduces_the_diagonal_wraps_exactly_and_refuses_a_rotation():
    size = [0.0, 2.2, 0.0, 1.0]
    x = torch.from_numpy(sm.points(2, 301, seed=9).astype(np.float64))
    x[:40, 0] = torch.linspace(0.0, 0.125, 40, dtype=torch.float64)  # the inlet strip, both ends included
    x[40:60, 1] = torch.linspace(0.0, 0.125, 20, dtype=torch.float64)  # the wall layer
    N = torch.from_numpy(np.random.default_rng(1).standard_normal((301, 2)))
    for wrap in (sm.karman_wrap(size, eps=0.125), sm.karman_wrap(size, eps=0.125, detach_weight=False),
                 taylorgreen_wrap(size, eps=0.125)):
        scale, offset = siren.diagonal_wrap(wrap, x, 2)
        assert scale.shape == offset.shape == (301, 2) and scale.dtype == torch.float64
        assert not scale.requires_grad and not offset.requires_grad
        assert torch.equal(scale * N + offset, wrap(x, N))
    scale, offset = siren.diagonal_wrap(sm.karman_wrap(size, eps=0.125), x, 2)
    inlet = (x[:, 0] >= 0.0) & (x[:, 0] <= 0.125)
    assert int(inlet.sum()) >= 40 and bool((scale[inlet, 0] == 0).all()) and bool((offset[inlet, 0] == 0.5).all())
    assert bool((scale[~inlet, 0] == 1).all()) and bool((offset[~inlet] == 0).all()) and bool((offset[:, 1] == 0).all())
    with pytest.raises(ValueError, match="rotating_wrap.*not diagonal-affine"):
        siren.diagonal_wrap(rotating_wrap, x, 2)
    scale, offset = siren.diagonal_wrap(rotating_wrap, x, 2, check=False)  # unchecked: the caller's risk
    assert scale.shape == (301, 2)


# ---- projection_fit_loss draws what projection_loss draws --------------------------------------------
@pytest.mark.parametrize("dim", [2, 3])
def test_projection_fit_loss_draws_the_samples_of_projection_loss(monkeypatch, dim):
    n, n_samples = 50, 64
    proj = pj.PressureProjector.__new__(pj.PressureProjector)
    proj.dim, proj.device = dim, torch.device("cpu")
    proj.samples = torch.from_numpy(sm.points(dim, n, seed=4))
    grad_p = torch.from_numpy(np.random.default_rng(2).standard_normal((n, dim)).astype(np.float32))
    seen = {}

    def velocity(tag):
        def f(x):
            seen[tag] = x.clone()
            return torch.zeros_like(x)
        return f
    g1 = torch.Generator().manual_seed(123)
    proj.projection_loss(velocity("u"), velocity("u_prev"), grad_p, n_samples, generator=g1)

    def fake_eval(net, x, **kw):
        seen["eval"] = x.clone()
        return torch.zeros_like(x)

    def fake_fit_loss(module, x, target, scale=None):
        seen["fit"], seen["target"], seen["scale"] = x.clone(), target.clone(), scale
        return torch.zeros(())
    monkeypatch.setattr(siren, "eval", fake_eval)
    monkeypatch.setattr(siren, "fit_loss", fake_fit_loss)
    g2 = torch.Generator().manual_seed(123)
    proj.projection_fit_loss(object(), object(), grad_p, n_samples, generator=g2)
    assert torch.equal(g1.get_state(), g2.get_state()), "the same generator consumption"
    assert torch.equal(seen["u"], seen["fit"]) and torch.equal(seen["u_prev"], seen["eval"]), "the same samples"
    assert seen["scale"] is None
    # the target is u_prev - grad_p at those samples: recover the indices from it (u_prev = 0 here)
    idx = torch.randint(0, n - 1 if dim == 2 else n, (n_samples,), generator=torch.Generator().manual_seed(123))
    assert torch.equal(seen["target"], -grad_p[idx]) and torch.equal(seen["fit"], proj.samples[idx])
    # with a wrap: its scale goes to the kernel and its offset into the target
    wrap = sm.karman_wrap([0.0, 2.2, 0.0, 1.0], eps=0.125)
    g3 = torch.Generator().manual_seed(123)
    proj.projection_fit_loss(object(), object(), grad_p, n_samples, wrap=wrap, generator=g3)
    assert torch.equal(g1.get_state(), g3.get_state())
    x = proj.samples[idx]
    scale, offset = siren.diagonal_wrap(wrap, x, dim)
    assert torch.equal(seen["scale"], scale)
    assert torch.equal(seen["target"], wrap(x, torch.zeros_like(x)) - grad_p[idx] - offset)
