"""Shared models for the fused-SIREN tests (tests/test_siren_cpu.py, tests/test_gpu_siren.py):
Siren-initialised nets from a fixed torch seed, a float64 torch-autograd evaluation of
(u, J, div), the existing float32 autograd path (wos_amd.projection.divergence plus a Jacobian
by the same loop), the karman-like wrap of the time-stepper's query_velocity, and the error rule
that compares the fused kernel with the float32 autograd path against the float64 model."""
import copy
import functools

import numpy as np
import torch

from wos_amd.projection import Siren, divergence


@functools.lru_cache(maxsize=None)
def make_net(d_in, hidden, n_hidden, d_out=None, seed=0):
    """A Siren(d_in, d_out, n_hidden, hidden) on the CPU, float32; the same weights for the same
    arguments (do not modify the returned module)."""
    gen_state = torch.random.get_rng_state()
    torch.manual_seed(7919 * seed + 1000 * d_in + 10 * hidden + n_hidden + 100000 * (d_out or d_in))
    net = Siren(d_in, d_out or d_in, n_hidden, hidden)
    torch.random.set_rng_state(gen_state)
    return net.requires_grad_(False)


def points(d_in, n=193, seed=0):
    """n uniform points in [0, 2.2] x [0, 1] (2D) or the unit cube (3D), float32."""
    x = np.random.default_rng(seed).random((n, d_in))
    if d_in == 2:
        x = x * np.array([2.2, 1.0])
    return x.astype(np.float32)


def autograd_eval(net, x):
    """(u [n, d_out], J [n, d_out, d_in], div [n] or None) of net at the tensor x by the reference's
    autograd loop (diff_ops.py:45-51), in x's dtype on x's device; div through
    wos_amd.projection.divergence itself when d_out == d_in."""
    x = x.detach().clone().requires_grad_(True)
    u = net(x)
    rows = [torch.autograd.grad(u[..., i], x, torch.ones_like(u[..., i]), retain_graph=True)[0]
            for i in range(u.shape[-1])]
    jac = torch.stack(rows, dim=-2)
    div = divergence(u, x)[..., 0] if u.shape[-1] == x.shape[-1] else None
    return u.detach(), jac.detach(), None if div is None else div.detach()


def model64(net, x):
    """autograd_eval in float64 on the CPU, numpy out: the tests' ground truth."""
    net64 = copy.deepcopy(net).double().cpu()
    u, jac, div = autograd_eval(net64, torch.from_numpy(np.asarray(x, np.float64)))
    return u.numpy(), jac.numpy(), None if div is None else div.numpy()


def karman_wrap(size, eps=0.1, inlet_vel=0.5, detach_weight=True):
    """query_velocity's karman branch (src/2d/models/base.py:169-180) restated out of place:
    u_x clamped to the inlet velocity on the strip x0 <= x <= x0 + eps, then u_y weighted by the
    clamped distance to the two walls y = size[2], size[3] over eps (detached in the reference;
    detach_weight=False keeps its x-derivative so that term of the chain rule is exercised too).
    A third component passes through."""
    def wrap(x, u):
        inlet = (x[..., 0] >= size[0]) & (x[..., 0] <= size[0] + eps)
        ux = torch.where(inlet, torch.full_like(u[..., 0], inlet_vel), u[..., 0])
        w = torch.min(torch.abs(x[..., 1] - size[2]).clamp(min=0, max=eps),
                      torch.abs(x[..., 1] - size[3]).clamp(min=0, max=eps)) / eps
        if detach_weight:
            w = w.detach()
        return torch.stack([ux, w * u[..., 1]] + [u[..., k] for k in range(2, u.shape[-1])], dim=-1)
    return wrap


def error_ratios(fused, torch32, ref64):
    """(RMS(e_fused) / RMS(e_torch), max|e_fused| / max|e_torch|, RMS(e_torch), max|e_torch|) with
    e = value - float64 reference."""
    ef = np.asarray(fused, np.float64) - ref64
    et = np.asarray(torch32, np.float64) - ref64
    rms_f, rms_t = np.sqrt(np.mean(ef ** 2)), np.sqrt(np.mean(et ** 2))
    max_f, max_t = np.abs(ef).max(), np.abs(et).max()
    return float(rms_f / rms_t), float(max_f / max_t), float(rms_t), float(max_t)


def assert_as_accurate_as_torch(fused, torch32, ref64, what):
    """The accuracy rule: the fused result's error against float64 is at most 2.5 x (RMS) and
    4 x (max) the existing float32 autograd path's own error.  Returns the two ratios."""
    r_rms, r_max, rms_t, max_t = error_ratios(fused, torch32, ref64)
    print(f"{what}: rms ratio {r_rms:.3f} max ratio {r_max:.3f} (torch f32 rms {rms_t:.3e} max {max_t:.3e})")
    assert rms_t > 0 and max_t > 0, f"{what}: the float32 yardstick has no error at all"
    assert r_rms <= 2.5, f"{what}: RMS error {r_rms:.3f} x the float32 autograd path's"
    assert r_max <= 4.0, f"{what}: max error {r_max:.3f} x the float32 autograd path's"
    return r_rms, r_max
