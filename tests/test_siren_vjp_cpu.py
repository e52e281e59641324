"""Fused SIREN backward without a GPU (include/wos.h "Fused SIREN backward"): the float64 numpy
restatement of the contract equals torch float64 autograd, the two entry points are declared,
exported and bound within ABI 10, divergence_with_wrap(create_graph=True) carries the gradient to
the weights, and vjp / apply name what they refuse before any device work."""
import copy
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import siren_model as sm
import siren_vjp_model as vm
import wos_amd
from wos_amd import _lib, siren
from wos_amd.projection import divergence

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "wos.h")


# ---- the model ---------------------------------------------------------------------------------------
MODEL_SHAPES = [(2, 32, 1, None), (3, 64, 2, None), (2, 64, 0, None), (3, 32, 1, 1),
                (3, 32, 8, 3), (2, 160, 1, 2), (2, 64, 1, 3)]  # the deepest net, H / 32 = 5, and d_out > d_in


@pytest.mark.parametrize("which", ["u", "J", "div", "all"])
@pytest.mark.parametrize("d,H,L,d_out", MODEL_SHAPES, ids=[f"d{d}_H{H}_L{L}_o{o or d}" for d, H, L, o in MODEL_SHAPES])
def test_float64_model_equals_float64_autograd(d, H, L, d_out, which):
    """Float64 identities: 1e-9 of each tensor's largest entry (observed ~1e-13)."""
    if which in ("div", "all") and d_out is not None and d_out != d:
        which = {"div": "J", "all": "uJ"}[which]  # no divergence of a non-square net: its cotangents without g_div
    net = vm.net64(sm.make_net(d, H, L, d_out))
    x = sm.points(d, 37, seed=3).astype(np.float64)
    g_u, g_J, g_div = vm.cotangents(37, d_out or d, d, seed=5)
    g = {"u": (g_u, None, None), "J": (None, g_J, None), "div": (None, None, g_div), "all": (g_u, g_J, g_div),
         "uJ": (g_u, g_J, None)}[which]
    want = vm.autograd_grads(net, torch.from_numpy(x), *g)
    got = vm.model64(*vm.net_arrays(net), x, *g)
    for kind, G, W in (("w", got[0], want[0]), ("b", got[1], want[1])):
        assert len(G) == len(W) == L + 2
        for l, (a, b) in enumerate(zip(G, W)):
            assert a.shape == b.shape, (kind, l)
            scale = np.abs(b).max()
            assert np.abs(a - b).max() <= 1e-9 * scale, (kind, l, np.abs(a - b).max(), scale)
    assert any(np.any(a) for a in got[0])


# ---- ABI ---------------------------------------------------------------------------------------------
def test_vjp_entry_points_declared_exported_and_bound():
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\bint\s+wos_siren_vjp\s*\(\s*const\s+wos_siren_net\s*\*", txt)
    assert re.search(r"\bint\s+wos_selftest_siren_vjp_layer\s*\(\s*int32_t\s+hidden", txt)
    L = wos_amd.load_library()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r"\bT (wos_[a-z0-9_]+)$", out, flags=re.M))
    for name in ("wos_siren_vjp", "wos_selftest_siren_vjp_layer"):
        assert name in exported and name in _lib.EXPORTS and hasattr(L, name), name
    assert len(L.wos_siren_vjp.argtypes) == 12 and len(L.wos_selftest_siren_vjp_layer.argtypes) == 9
    assert L.wos_abi_version() == _lib.ABI_VERSION == 10
    assert re.search(r"#define WOS_ABI_VERSION 10\b", open(HEADER).read())


# ---- divergence_with_wrap(create_graph=True) -----------------------------------------------------------
@pytest.mark.parametrize("detach_weight", [True, False])
def test_divergence_with_wrap_carries_the_gradient_to_the_weights(detach_weight):
    net = vm.net64(sm.make_net(2, 32, 1)).requires_grad_(True)
    size = [0.0, 2.2, 0.0, 1.0]
    wrap = sm.karman_wrap(size, eps=0.125, detach_weight=detach_weight)
    x = torch.from_numpy(sm.points(2, 61, seed=2).astype(np.float64))
    g = torch.from_numpy(np.random.default_rng(4).standard_normal(61))
    params = list(net.parameters())
    # the autograd divergence of wrap(x, net(x))
    xa = x.clone().requires_grad_(True)
    want_div = divergence(wrap(xa, net(xa)), xa, create_graph=True)[..., 0]
    def grads(loss):  # the output bias does not reach a divergence: its gradient is absent, i.e. zero
        return [torch.zeros_like(t) if a is None else a
                for a, t in zip(torch.autograd.grad(loss, params, allow_unused=True), params)]
    want = grads((g * want_div).sum())
    # u and J of the network alone, attached; the wrap by the chain rule
    xb = x.clone().requires_grad_(True)
    u = net(xb)
    J = torch.stack([torch.autograd.grad(u[..., i], xb, torch.ones_like(u[..., i]), create_graph=True)[0]
                     for i in range(2)], dim=-2)
    div = siren.divergence_with_wrap(x, u, J, wrap, create_graph=True)
    assert div.requires_grad
    assert torch.allclose(div.detach(), want_div.detach(), rtol=0, atol=1e-12 * float(want_div.detach().abs().max()))
    got = grads((g * div).sum())
    for a, b in zip(got, want):
        assert float((a - b).abs().max()) <= 1e-9 * float(b.abs().max())
    assert all(float(b.abs().max()) > 0 for b in want[:-1]), "every weight and every bias but the output's counts"
    assert any(float(b.abs().max()) > 0 for b in want)
    # the default: today's result, detached
    plain = siren.divergence_with_wrap(x, u, J, wrap)
    assert not plain.requires_grad and plain.grad_fn is None
    assert torch.equal(plain, siren.divergence_with_wrap(x, u.detach(), J.detach(), wrap, create_graph=False))
    assert torch.equal(plain, div.detach())


# ---- refusals ------------------------------------------------------------------------------------------
def test_vjp_and_apply_name_what_they_refuse():
    net = sm.make_net(2, 32, 1)
    x = sm.points(2, 5)
    g_u, g_J, g_div = vm.cotangents(5, 2, 2)
    with pytest.raises(ValueError, match="no cotangent"):
        siren.vjp(net, x)
    with pytest.raises(ValueError, match=r"grad_value must have shape \(5, 2\)"):
        siren.vjp(net, x, grad_value=g_u[:4])
    with pytest.raises(ValueError, match=r"grad_jacobian must have shape \(5, 2, 2\)"):
        siren.vjp(net, x, grad_jacobian=g_J.reshape(5, 4))
    with pytest.raises(ValueError, match=r"grad_divergence must have shape \(5,\)"):
        siren.vjp(net, x, grad_divergence=g_div[:, None])
    with pytest.raises(ValueError, match=r"points must be \[\.\.\., 2\]"):
        siren.vjp(net, np.zeros((5, 3), np.float32), grad_value=g_u)
    net31 = sm.make_net(3, 32, 1, 1)
    with pytest.raises(ValueError, match="grad_divergence needs d_out == d_in"):
        siren.vjp(net31, sm.points(3, 5), grad_divergence=g_div)
    with pytest.raises(ValueError, match="divergence needs d_out == d_in"):
        siren.apply(net31, torch.from_numpy(sm.points(3, 5)), divergence=True)
    with pytest.raises(ValueError, match="no output requested"):
        siren.apply(net, torch.from_numpy(x), value=False)
    with pytest.raises(ValueError, match="x.requires_grad"):
        siren.apply(copy.deepcopy(net), torch.from_numpy(x).requires_grad_(True))
