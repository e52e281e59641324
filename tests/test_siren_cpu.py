"""Fused SIREN without a GPU (include/wos.h "Fused SIREN"): the two entry points are declared,
exported and bound and the ABI version did not move; wos_amd.siren.pack accepts the reference's
network and names what it refuses; siren.divergence_with_wrap, which is pure torch, reproduces
the float64 autograd divergence of wrap(x, net(x)) from the network's value and Jacobian."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch
import torch.nn as nn

import siren_model as sm
import wos_amd
from wos_amd import _lib, siren
from wos_amd.projection import Siren, Sine, divergence

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "wos.h")


# ---- ABI ------------------------------------------------------------------------------------------
def test_siren_entry_points_declared_exported_and_bound():
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\bint\s+wos_siren_eval\s*\(\s*const\s+wos_siren_net\s*\*", txt)
    assert re.search(r"\bint\s+wos_selftest_siren_layer\s*\(\s*int32_t\s+hidden", txt)
    assert re.search(r"typedef\s+struct\s+wos_siren_net\s*\{[^}]*\bomega\b[^}]*\bweights\b[^}]*\bbiases\b[^}]*\}", txt)
    L = wos_amd.load_library()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r"\bT (wos_[a-z0-9_]+)$", out, flags=re.M))
    for name in ("wos_siren_eval", "wos_selftest_siren_layer"):
        assert name in exported and name in _lib.EXPORTS and hasattr(L, name), name
    assert len(L.wos_siren_eval.argtypes) == 9 and len(L.wos_selftest_siren_layer.argtypes) == 8
    assert [f[0] for f in _lib.SirenNet._fields_] == ["d_in", "d_out", "hidden", "n_hidden_layers", "omega",
                                                      "weights", "biases"]


def test_abi_version_unchanged():
    assert wos_amd.load_library().wos_abi_version() == _lib.ABI_VERSION == 10
    assert re.search(r"#define WOS_ABI_VERSION 10\b", open(HEADER).read())


# ---- pack -----------------------------------------------------------------------------------------
def test_pack_accepts_the_reference_network_without_copying():
    net = Siren(2, 2, 3, 256)
    p = siren.pack(net.net)
    assert (p.d_in, p.d_out, p.hidden, p.n_hidden_layers, p.omega) == (2, 2, 256, 3, 30.0)
    lin = [m for m in net.net if isinstance(m, nn.Linear)]
    assert len(p.weights) == len(p.biases) == 5
    for m, w, b in zip(lin, p.weights, p.biases):
        assert w.data_ptr() == m.weight.data_ptr() and b.data_ptr() == m.bias.data_ptr()
        assert w.dtype == b.dtype == torch.float32 and w.is_contiguous() and not w.requires_grad
    assert [tuple(w.shape) for w in p.weights] == [(256, 2), (256, 256), (256, 256), (256, 256), (2, 256)]
    # the module itself, and a net with no hidden layer and another output width
    assert siren.pack(net).hidden == 256
    q = siren.pack(Siren(3, 1, 0, 32))
    assert (q.d_in, q.d_out, q.hidden, q.n_hidden_layers) == (3, 1, 32, 0)


def _with_relu():
    net = Siren(2, 2, 2, 64).net
    net[3] = nn.ReLU()
    return net


def _without_bias():
    return nn.Sequential(nn.Linear(2, 64), Sine(), nn.Linear(64, 64, bias=False), Sine(), nn.Linear(64, 2))


@pytest.mark.parametrize("make,match", [
    (lambda: Siren(2, 2, 1, 100), r"hidden must be a multiple of 32 in 32\.\.256, got 100"),
    (lambda: Siren(2, 2, 1, 288), r"hidden must be a multiple of 32 in 32\.\.256, got 288"),
    (lambda: Siren(4, 2, 1, 64), r"d_in must be 2 or 3, got 4"),
    (_with_relu, r"module 3 must be a Sine activation, got ReLU"),
    (lambda: Siren(2, 2, 1, 64).double(), r"must be float32, got torch\.float64"),
    (_without_bias, r"bias=False"),
], ids=["H100", "H288", "d_in4", "relu", "float64", "no_bias"])
def test_pack_names_what_it_refuses(make, match):
    with pytest.raises(ValueError, match=match):
        siren.pack(make())


def test_eval_refuses_divergence_of_a_non_square_net_before_any_device_work():
    with pytest.raises(ValueError, match="divergence needs d_out == d_in"):
        siren.eval(Siren(3, 1, 1, 32), np.zeros((4, 3), np.float32), divergence=True)
    with pytest.raises(ValueError, match="no output requested"):
        siren.eval(Siren(2, 2, 1, 32), np.zeros((4, 2), np.float32), value=False)


# ---- divergence_with_wrap ---------------------------------------------------------------------------
@pytest.mark.parametrize("detach_weight", [True, False], ids=["detached_weight", "live_weight"])
@pytest.mark.parametrize("d", [2, 3])
def test_divergence_with_wrap_matches_float64_autograd(d, detach_weight):
    net = sm.make_net(d, 64, 2)
    x = sm.points(d)
    size = [0.0, 2.2, 0.0, 1.0] if d == 2 else [0.0, 1.0, 0.0, 1.0, 0.0, 1.0]
    wrap = sm.karman_wrap(size, detach_weight=detach_weight)
    inlet = (x[:, 0] <= size[0] + 0.1).sum()
    wall = ((x[:, 1] < 0.1) | (x[:, 1] > 0.9)).sum()
    assert 0 < inlet < x.shape[0] and 0 < wall < x.shape[0], "the points must reach the strip and the walls"
    u64, j64, _ = sm.model64(net, x)
    # ground truth: autograd through wrap AND the network, float64
    import copy
    net64 = copy.deepcopy(net).double()
    xg = torch.from_numpy(x.astype(np.float64)).requires_grad_(True)
    want = divergence(wrap(xg, net64(xg)), xg)[..., 0].detach().numpy()
    got = siren.divergence_with_wrap(torch.from_numpy(x.astype(np.float64)), torch.from_numpy(u64),
                                     torch.from_numpy(j64), wrap)
    assert got.dtype == torch.float64 and tuple(got.shape) == (x.shape[0],) and not got.requires_grad
    assert np.abs(got.numpy() - want).max() <= 1e-12 * np.abs(want).max()
    # the wrap matters: the plain trace differs where the clamp or the weight acts
    trace = sum(j64[:, k, k] for k in range(d))
    assert np.abs(trace - want).max() > 1e-3 * np.abs(want).max()


@pytest.mark.parametrize("d", [2, 3])
def test_divergence_with_identity_wrap_is_the_trace_exactly(d):
    net = sm.make_net(d, 32, 1)
    x = sm.points(d, 50)
    u64, j64, _ = sm.model64(net, x)
    u32, j32 = torch.from_numpy(u64.astype(np.float32)), torch.from_numpy(j64.astype(np.float32))
    got = siren.divergence_with_wrap(torch.from_numpy(x), u32, j32, lambda x, u: u)
    trace = j32[:, 0, 0] + j32[:, 1, 1]
    if d == 3:
        trace = trace + j32[:, 2, 2]
    assert got.dtype == torch.float32
    assert np.array_equal(got.numpy().view(np.uint32), trace.numpy().view(np.uint32))
    # grid-shaped input keeps its leading shape
    g = siren.divergence_with_wrap(torch.from_numpy(x).reshape(5, 10, d), u32.reshape(5, 10, d),
                                   j32.reshape(5, 10, d, d), lambda x, u: u)
    assert tuple(g.shape) == (5, 10) and torch.equal(g.reshape(-1), got)
