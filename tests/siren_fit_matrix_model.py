"""Shared models for the matrix-wrap fit-step tests (tests/test_siren_fit_matrix_cpu.py,
tests/test_gpu_siren_fit_matrix.py): fixed targets and per-point matrices S, the float64 fit loss
mean((S net(x) - target)^2) and its gradients through siren_vjp_model.model64 seeded with
g_u = S^T (2 r) / (n d_out), the same by torch autograd in any dtype on any device, the kernel's
f32 residual chain restated, and the derived bound of the loss."""
import numpy as np
import torch

import siren_vjp_model as vm


def problem(n, d_out, seed=0):
    """(target [n, d_out], S [n, d_out, d_out]), float32 from a fixed seed.  S is dense, in [-1, 1.5),
    with exact zeros in it -- every fifth point's entry [0][d_out - 1], every seventh point's first row
    -- and a few all-zero matrices (an inlet: the wrapped value does not depend on the network there)."""
    rng = np.random.default_rng(4000 + seed)
    target = (0.5 * rng.standard_normal((n, d_out))).astype(np.float32)
    S = (rng.random((n, d_out, d_out)) * 2.5 - 1.0).astype(np.float32)
    S[::5, 0, d_out - 1] = 0.0
    S[2::7, 0, :] = 0.0
    S[3::17] = 0.0
    return target, S


def diagonal(scale):
    """[n, d_out] factors as [n, d_out, d_out] diagonal matrices, the off-diagonal entries exact zeros."""
    scale = np.asarray(scale, np.float32)
    S = np.zeros(scale.shape + (scale.shape[-1],), np.float32)
    for i in range(scale.shape[-1]):
        S[..., i, i] = scale[..., i]
    return S


def seeds64(u, target, S):
    """(r, ub, loss) in float64 from the network's value u [n, d_out]: r = S u - target,
    ub = S^T (2 r) / (n d_out)."""
    u, S = np.asarray(u, np.float64), np.asarray(S, np.float64)
    r = np.einsum("pim,pm->pi", S, u) - np.asarray(target, np.float64)
    return r, np.einsum("pim,pi->pm", S, 2.0 * r) / r.size, float(np.mean(r * r))


def model64(net, x, target, S):
    """(loss, (grad_weights, grad_biases), ub), float64: the contract's formulas through the
    backward's own float64 model seeded with g_u = S^T (2 r) / (n d_out)."""
    net64 = vm.net64(net)
    x64 = np.asarray(x, np.float64)
    with torch.no_grad():
        u = net64(torch.from_numpy(x64)).numpy()
    _, ub, loss = seeds64(u, target, S)
    return loss, vm.model64(*vm.net_arrays(net64), x64, ub), ub


def autograd(net, x, target, S):
    """(loss, (grad_weights, grad_biases)) by torch autograd of mean((S @ net(x) - target)^2), in x's
    dtype on x's device (net must match); numpy out, pack() order."""
    import torch.nn as nn
    lin = [m for m in net.net if isinstance(m, nn.Linear)]
    params = [m.weight for m in lin] + [m.bias for m in lin]
    was = [t.requires_grad for t in params]
    for t in params:
        t.requires_grad_(True)
    try:
        u = net(x.detach())
        t = torch.as_tensor(target, dtype=x.dtype, device=x.device)
        Sm = torch.as_tensor(S, dtype=x.dtype, device=x.device)
        loss = torch.mean(((Sm @ u.unsqueeze(-1)).squeeze(-1) - t) ** 2)
        grads = torch.autograd.grad(loss, params)
    finally:
        for t, r in zip(params, was):
            t.requires_grad_(r)
    out = [g.detach().cpu().numpy() for g in grads]
    return float(loss.detach()), (out[:len(lin)], out[len(lin):])


def _fma32(a, b, c):
    """fmaf on float32 arrays: the product of two float32 is exact in float64, the sum is rounded to
    float64 and then to float32 (a double rounding differs from fmaf in the last bit on rare ties only)."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def residual32(u, target, S):
    """The kernel's residual chain on float32 u: r_i = -target_i, then r_i = fmaf(S[i][m], u_m, r_i) for
    m = 0 .. d_out - 1 in order."""
    u, S = np.asarray(u, np.float32), np.asarray(S, np.float32)
    r = -np.asarray(target, np.float32)
    for m in range(u.shape[-1]):
        r = _fma32(S[..., :, m], u[..., None, m], r)
    return r


def seed32(r, S, count):
    """The kernel's seed chain on the float32 residuals r: g_i = r_i + r_i, acc = S[0][m] g_0 (rounded),
    acc = fmaf(S[i][m], g_i, acc) for i = 1 .. d_out - 1, ub_m = acc (1 / count) with 1 / count rounded once."""
    r, S = np.asarray(r, np.float32), np.asarray(S, np.float32)
    g = r + r
    acc = S[..., 0, :] * g[..., 0, None]
    for i in range(1, r.shape[-1]):
        acc = _fma32(S[..., i, :], g[..., i, None], acc)
    return acc * (np.float32(1.0) / np.float32(count))


def loss_bound(u, target, S):
    """|loss - L64| for the kernel's loss against float64 of the same float32 u (DESIGN.md "Fused SIREN
    fits through a mixing wrap", *Accuracy*).  With N = n d_out, e = 2^-24:
      * the residual is a chain of d_out fused multiply-adds from -t_i, so the computed rh_i differs from
        r_i = (S u - t)_i by at most g A_i, g = d_out e / (1 - d_out e), A_i = |t_i| + sum_m |S_im u_m|
        (Higham, Accuracy and Stability of Numerical Algorithms, section 3.1, for d_out roundings);
      * f32 squares of rh summed in any order and scaled once are within (N + 8) e sum rh^2 of sum rh^2
        (the plain fit step's bound, siren_fit_model.loss_bound);
      * |sum rh^2 - sum r^2| <= sum (2 |r_i| g A_i + (g A_i)^2).
    All divided by N.  Returns (bound, L64)."""
    u64, S64, t64 = np.asarray(u, np.float64), np.asarray(S, np.float64), np.asarray(target, np.float64)
    d_out, N = u64.shape[-1], t64.size
    r = np.einsum("pim,pm->pi", S64, u64) - t64
    e = 2.0 ** -24
    g = d_out * e / (1.0 - d_out * e)
    A = np.abs(t64) + np.einsum("pim,pm->pi", np.abs(S64), np.abs(u64))
    rh = residual32(u, target, S).astype(np.float64)
    bound = ((N + 8) * e * np.sum(rh * rh) + np.sum(2.0 * np.abs(r) * g * A + (g * A) ** 2)) / N
    return float(bound), float(np.mean(r * r))
