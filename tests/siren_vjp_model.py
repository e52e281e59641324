"""Shared models for the fused-SIREN backward tests (tests/test_siren_vjp_cpu.py,
tests/test_gpu_siren_vjp.py): a plain numpy float64 restatement of the backward's formulas
(include/wos.h "Fused SIREN backward"), the same gradients by torch autograd of
l = sum g_u . u + sum g_J . J + sum g_div div in any dtype on any device, fixed random
cotangents, and the per-tensor accuracy rule."""
import copy

import numpy as np
import torch

import siren_model as sm
from wos_amd import siren


def net_arrays(net):
    """(weights, biases, omega) of a Siren as float64 numpy arrays, pack() order."""
    import torch.nn as nn
    lin = [m for m in net.net if isinstance(m, nn.Linear)]
    return ([m.weight.detach().cpu().numpy().astype(np.float64) for m in lin],
            [m.bias.detach().cpu().numpy().astype(np.float64) for m in lin], 30.0)


def cotangents(n, d_out, d_in, seed=0):
    """(g_u [n, d_out], g_J [n, d_out, d_in], g_div [n]) standard normal, float32, from a fixed seed."""
    rng = np.random.default_rng(1000 + seed)
    return (rng.standard_normal((n, d_out)).astype(np.float32),
            rng.standard_normal((n, d_out, d_in)).astype(np.float32),
            rng.standard_normal(n).astype(np.float32))


def model64(weights, biases, omega, x, g_u=None, g_J=None, g_div=None):
    """(grad_weights, grad_biases), float64: the formulas of the contract, written out.
    a [n, H], t [n, d_in, H] per sine layer; absent cotangents count as zero."""
    x = np.asarray(x, np.float64)
    n, d_in = x.shape
    L, d_out = len(weights) - 2, weights[-1].shape[0]
    # forward, keeping every sine layer's pre-activations
    zs, Zs, As, Ts = [], [], [], []
    z = x @ weights[0].T + biases[0]
    Z = np.broadcast_to(weights[0].T[None], (n, d_in, weights[0].shape[0]))
    for l in range(L + 1):
        if l > 0:
            z = As[-1] @ weights[l].T + biases[l]
            Z = Ts[-1] @ weights[l].T
        s, c = np.sin(omega * z), np.cos(omega * z)
        zs.append(z), Zs.append(Z), As.append(s), Ts.append(omega * c[:, None, :] * Z)
    # seeds
    ub = np.zeros((n, d_out)) if g_u is None else np.asarray(g_u, np.float64)
    Jb = np.zeros((n, d_out, d_in)) if g_J is None else np.asarray(g_J, np.float64).copy()
    if g_div is not None:
        assert d_out == d_in
        Jb = Jb + np.asarray(g_div, np.float64)[:, None, None] * np.eye(d_in)[None]
    gw, gb = [None] * (L + 2), [None] * (L + 2)
    # output layer
    Wo = weights[L + 1]
    gw[L + 1] = ub.T @ As[L] + np.einsum("pik,pkh->ih", Jb, Ts[L])
    gb[L + 1] = ub.sum(0)
    da = ub @ Wo                                   # [n, H]
    dt = np.einsum("pik,ih->pkh", Jb, Wo)          # [n, d_in, H]
    for l in range(L, -1, -1):
        s, c = np.sin(omega * zs[l]), np.cos(omega * zs[l])
        dZ = omega * c[:, None, :] * dt
        dz = omega * c * da - omega ** 2 * s * (dt * Zs[l]).sum(1)
        gb[l] = dz.sum(0)
        if l == 0:
            gw[0] = dz.T @ x + dZ.sum(0).T         # [H, d_in]
            break
        gw[l] = dz.T @ As[l - 1] + np.einsum("pkr,pkh->rh", dZ, Ts[l - 1])
        da = dz @ weights[l]
        dt = dZ @ weights[l]
    return gw, gb


def autograd_grads(net, x, g_u=None, g_J=None, g_div=None):
    """The same gradients by autograd, in x's dtype on x's device (net must match): first
    derivatives with create_graph, then the gradient of l with respect to every Linear layer's
    weight and bias.  Returns numpy (grad_weights, grad_biases) in pack() order."""
    import torch.nn as nn
    lin = [m for m in net.net if isinstance(m, nn.Linear)]
    params = [m.weight for m in lin] + [m.bias for m in lin]
    was = [t.requires_grad for t in params]
    for t in params:
        t.requires_grad_(True)
    try:
        x = x.detach().clone().requires_grad_(True)
        u = net(x)
        loss = 0.0
        if g_u is not None:
            loss = loss + (torch.as_tensor(g_u, dtype=x.dtype, device=x.device) * u).sum()
        if g_J is not None or g_div is not None:
            rows = [torch.autograd.grad(u[..., i], x, torch.ones_like(u[..., i]), create_graph=True)[0]
                    for i in range(u.shape[-1])]
            jac = torch.stack(rows, dim=-2)
            if g_J is not None:
                loss = loss + (torch.as_tensor(g_J, dtype=x.dtype, device=x.device) * jac).sum()
            if g_div is not None:
                div = sum(jac[..., i, i] for i in range(x.shape[-1]))
                loss = loss + (torch.as_tensor(g_div, dtype=x.dtype, device=x.device) * div).sum()
        grads = torch.autograd.grad(loss, params, allow_unused=True)
    finally:
        for t, r in zip(params, was):
            t.requires_grad_(r)
    out = [np.zeros(tuple(t.shape)) if g is None else g.detach().cpu().numpy() for g, t in zip(grads, params)]
    return out[:len(lin)], out[len(lin):]


def net64(net):
    return copy.deepcopy(net).double().cpu()


def assert_grads_as_accurate(got, torch32, ref64, g_u, what, record=None):
    """Rule 2 per parameter tensor: sm.assert_as_accurate_as_torch for every weight and bias, except
    the output bias, dbo = sum_p g_u, where torch may be exact: there the bound is the error bound
    of any f32 summation of n terms, (n - 1) 2^-24 sum |g_u|.  A tensor whose float64 gradient is
    identically zero (no cotangent reaches it) must be zero."""
    (gw, gb), (tw, tb), (rw, rb) = got, torch32, ref64
    nl = len(gw)
    for kind, G, T, R in (("w", gw, tw, rw), ("b", gb, tb, rb)):
        for l in range(nl):
            name = f"{what} d{kind}[{l}]"
            g, r = np.asarray(G[l], np.float64), np.asarray(R[l], np.float64)
            assert g.shape == r.shape, name
            if not np.any(r):
                assert not np.any(g), f"{name}: must be exactly zero"
                continue
            if kind == "b" and l == nl - 1:
                gu = np.asarray(g_u, np.float64)
                bound = (gu.shape[0] - 1) * 2.0 ** -24 * np.abs(gu).sum(0)
                print(f"{name}: error {np.abs(g - r).max():.3e}, bound {bound.min():.3e}")
                assert np.all(np.abs(g - r) <= bound), f"{name}: {np.abs(g - r)} over {bound}"
                continue
            ratios = sm.error_ratios(g, T[l], r)
            if record is not None:
                record[f"d{kind}{l}"] = {"rms_ratio": ratios[0], "max_ratio": ratios[1], "torch_rms": ratios[2],
                                         "torch_max": ratios[3]}
    # assert after every figure is on record
    for kind, G, T, R in (("w", gw, tw, rw), ("b", gb, tb, rb)):
        for l in range(nl):
            if not np.any(R[l]) or (kind == "b" and l == nl - 1):
                continue
            sm.assert_as_accurate_as_torch(np.asarray(G[l], np.float64), T[l], np.asarray(R[l], np.float64),
                                           f"{what} d{kind}[{l}]")
