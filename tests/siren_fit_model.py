"""Shared models for the fused-SIREN fit-step tests (tests/test_siren_fit_cpu.py,
tests/test_gpu_siren_fit.py): fixed targets and scales, the float64 fit loss and its gradients
through siren_vjp_model.model64 seeded with g_u = 2 scale r / (n d_out), and the same by torch
autograd of mean((scale net(x) - target)^2) in any dtype on any device."""
import numpy as np
import torch

import siren_vjp_model as vm


def problem(n, d_out, with_scale, seed=0):
    """(target [n, d_out], scale [n, d_out] or None), float32 from a fixed seed.  The scale has exact
    zeros in it: every fifth point's first component (the inlet mask) and a few whole points."""
    rng = np.random.default_rng(2000 + seed)
    target = (0.5 * rng.standard_normal((n, d_out))).astype(np.float32)
    if not with_scale:
        return target, None
    scale = rng.random((n, d_out)).astype(np.float32) * 1.5
    scale[::5, 0] = 0.0
    scale[3::17, :] = 0.0
    return target, scale


def seeds64(u, target, scale):
    """(r, ub, loss) in float64 from the network's value u [n, d_out]."""
    u = np.asarray(u, np.float64)
    s = np.ones_like(u) if scale is None else np.asarray(scale, np.float64)
    r = s * u - np.asarray(target, np.float64)
    return r, 2.0 * s * r / r.size, float(np.mean(r * r))


def model64(net, x, target, scale):
    """(loss, (grad_weights, grad_biases), ub), float64: the contract's formulas through the
    backward's own float64 model seeded with g_u = 2 scale r / (n d_out)."""
    net64 = vm.net64(net)
    x64 = np.asarray(x, np.float64)
    with torch.no_grad():
        u = net64(torch.from_numpy(x64)).numpy()
    _, ub, loss = seeds64(u, target, scale)
    return loss, vm.model64(*vm.net_arrays(net64), x64, ub), ub


def autograd(net, x, target, scale):
    """(loss, (grad_weights, grad_biases)) by torch autograd of mean((scale net(x) - target)^2), in
    x's dtype on x's device (net must match); numpy out, pack() order."""
    import torch.nn as nn
    lin = [m for m in net.net if isinstance(m, nn.Linear)]
    params = [m.weight for m in lin] + [m.bias for m in lin]
    was = [t.requires_grad for t in params]
    for t in params:
        t.requires_grad_(True)
    try:
        u = net(x.detach())
        t = torch.as_tensor(target, dtype=x.dtype, device=x.device)
        if scale is not None:
            u = torch.as_tensor(scale, dtype=x.dtype, device=x.device) * u
        loss = torch.mean((u - t) ** 2)
        grads = torch.autograd.grad(loss, params)
    finally:
        for t, r in zip(params, was):
            t.requires_grad_(r)
    out = [g.detach().cpu().numpy() for g in grads]
    return float(loss.detach()), (out[:len(lin)], out[len(lin):])


def loss_bound(count, loss64):
    """|loss - L64| for f32 squares of once-rounded residuals summed in any order and scaled once."""
    return (count + 8) * 2.0 ** -24 * loss64
