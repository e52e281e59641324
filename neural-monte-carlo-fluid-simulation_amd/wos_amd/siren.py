"""Fused SIREN value, input Jacobian and divergence (wos_siren_eval, csrc/wos_siren.hip).

The reference's projection step differentiates its velocity network by autograd
(get_divergence, src/2d/models/model_split.py:230-236; divergence, diff_ops.py:45-51): one
forward and `dim` backward passes with every activation in HBM.  eval() runs the same MLP
(networks.py:25-68) in forward mode in one kernel: per point the value and its d_in tangents
go through the layers together and only u, J or div come back.  Not differentiable: training
through the projection keeps PressureProjector.source_from_velocity(create_graph=True).
"""
import collections
import ctypes as C
import math

import numpy as np

from . import _lib
from ._lib import check

MAX_HIDDEN = 256          # csrc/wos_siren.h kSirenMaxHidden
MAX_HIDDEN_LAYERS = 8     # csrc/wos_siren.h kSirenMaxHiddenLayers

PackedSiren = collections.namedtuple("PackedSiren", "d_in d_out hidden n_hidden_layers omega weights biases")


def _is_torch(x):
    return type(x).__module__.startswith("torch")


def pack(net, omega=30.0):
    """Validate an nn.Sequential of the reference's structure -- Linear, Sine, L x [Linear, Sine],
    Linear; wos_amd.projection.Siren(...).net or the reference's MLP(...).net, a Sine being any
    module whose class is named `Sine` (both compute sin(30 x): `omega`) -- and return
    PackedSiren(d_in, d_out, hidden, n_hidden_layers, omega, weights, biases): the Linear layers'
    own weight [out, in] and bias tensors, detached and not copied.  ValueError names what does
    not fit wos_siren_eval's envelope."""
    import torch.nn as nn
    net = getattr(net, "net", net) if not isinstance(net, nn.Sequential) else net
    if not isinstance(net, nn.Sequential):
        raise ValueError(f"siren.pack: expected an nn.Sequential (Siren.net / MLP.net), got {type(net).__name__}")
    mods = list(net)
    if len(mods) < 3 or len(mods) % 2 == 0:
        raise ValueError(f"siren.pack: expected Linear, Sine, ..., Linear (an odd count >= 3), got {len(mods)} modules")
    lin = []
    for i, m in enumerate(mods):
        if i % 2 == 0:
            if not isinstance(m, nn.Linear):
                raise ValueError(f"siren.pack: module {i} must be a Linear layer, got {type(m).__name__}")
            if m.bias is None:
                raise ValueError(f"siren.pack: module {i} (Linear) has bias=False; every layer needs a bias")
            lin.append(m)
        elif type(m).__name__ != "Sine":
            raise ValueError(f"siren.pack: module {i} must be a Sine activation, got {type(m).__name__}")
    d_in, hidden, d_out, n_hidden = lin[0].in_features, lin[0].out_features, lin[-1].out_features, len(lin) - 2
    if d_in not in (2, 3):
        raise ValueError(f"siren.pack: d_in must be 2 or 3, got {d_in}")
    if not 1 <= d_out <= 3:
        raise ValueError(f"siren.pack: d_out must be 1..3, got {d_out}")
    if hidden % 32 != 0 or not 32 <= hidden <= MAX_HIDDEN:
        raise ValueError(f"siren.pack: hidden must be a multiple of 32 in 32..{MAX_HIDDEN}, got {hidden}")
    if n_hidden > MAX_HIDDEN_LAYERS:
        raise ValueError(f"siren.pack: at most {MAX_HIDDEN_LAYERS} hidden layers, got {n_hidden}")
    for i, m in enumerate(lin[1:], 1):
        if m.in_features != hidden or (i <= n_hidden and m.out_features != hidden):
            raise ValueError(f"siren.pack: Linear {i} is {m.in_features} -> {m.out_features}; every hidden layer "
                             f"must be {hidden} wide")
    if not math.isfinite(float(omega)):
        raise ValueError(f"siren.pack: omega must be finite, got {omega}")
    import torch
    weights, biases = [], []
    dev = lin[0].weight.device
    for i, m in enumerate(lin):
        for name, t, out in (("weight", m.weight, weights), ("bias", m.bias, biases)):
            if t.dtype != torch.float32:
                raise ValueError(f"siren.pack: Linear {i} {name} must be float32, got {t.dtype}")
            if t.device != dev:
                raise ValueError(f"siren.pack: Linear {i} {name} is on {t.device}, the first layer on {dev}")
            t = t.detach()
            if not t.is_contiguous():
                raise ValueError(f"siren.pack: Linear {i} {name} is not contiguous")
            out.append(t)
    return PackedSiren(d_in, d_out, hidden, n_hidden, float(omega), weights, biases)


def _net_struct(p, ptrs_w, ptrs_b):
    n = p.n_hidden_layers + 2
    w = (C.c_void_p * n)(*ptrs_w)
    b = (C.c_void_p * n)(*ptrs_b)
    return _lib.SirenNet(p.d_in, p.d_out, p.hidden, p.n_hidden_layers, p.omega, w, b), (w, b)


def eval(net, x, *, value=True, jacobian=False, divergence=False, stream=None):  # noqa: A001 (the module's verb)
    """u = net(x), J[n, i, k] = d u_i / d x_k and div = trace J of an [..., d_in] batch of points,
    in one fused kernel.  `net`: what pack() takes, or a PackedSiren.  Returns the requested of
    (u [..., d_out], J [..., d_out, d_in], div [...]) in that order -- one of them bare, several
    as a tuple.  A torch CUDA tensor in (the net on the same device): torch tensors out, enqueued
    on `stream` (a torch.cuda.Stream or a raw hipStream_t; default torch's current stream) without
    a host synchronisation.  numpy (or a CPU tensor) in: numpy out, blocking, the net's tensors
    staged from wherever they live.  Outputs are detached float32; a point's outputs are the same
    bits in any batch and for any choice of outputs."""
    p = net if isinstance(net, PackedSiren) else pack(net)
    if not (value or jacobian or divergence):
        raise ValueError("siren.eval: no output requested")
    if divergence and p.d_out != p.d_in:
        raise ValueError(f"siren.eval: divergence needs d_out == d_in, got d_out {p.d_out}, d_in {p.d_in}")
    L = _lib.load()
    want = (bool(value), bool(jacobian), bool(divergence))
    tails = ((p.d_out,), (p.d_out, p.d_in), ())
    if _is_torch(x) and x.is_cuda:
        import torch
        if any(t.device != x.device for t in p.weights + p.biases):
            raise ValueError(f"siren.eval: the points are on {x.device}, the network on {p.weights[0].device}")
        xs = x.detach().to(torch.float32).contiguous()
        if xs.shape[-1] != p.d_in:
            raise ValueError(f"siren.eval: points must be [..., {p.d_in}], got shape {tuple(x.shape)}")
        lead = tuple(xs.shape[:-1])
        xs = xs.reshape(-1, p.d_in)
        n = xs.shape[0]
        out = [torch.empty((n,) + tails[k], dtype=torch.float32, device=xs.device) if want[k] else None
               for k in range(3)]
        if n > 0:
            cur = torch.cuda.current_stream(xs.device)
            held = [xs] + [t for t in out if t is not None] + p.weights + p.biases
            if stream is None:
                s = cur.cuda_stream
            else:
                ts = stream if isinstance(stream, torch.cuda.Stream) else torch.cuda.ExternalStream(int(stream),
                                                                                                    device=xs.device)
                s = ts.cuda_stream
                ts.wait_stream(cur)  # points, weights and fresh outputs belong to torch's current stream
                for t in held:
                    t.record_stream(ts)  # ... and are used on `stream`: the allocator must wait for it
            st, keep = _net_struct(p, [t.data_ptr() for t in p.weights], [t.data_ptr() for t in p.biases])
            ptr = [t.data_ptr() if t is not None else None for t in out]
            check(L.wos_siren_eval(C.byref(st), xs.data_ptr(), n, *ptr, _lib.WOS_PTRS_DEVICE | _lib.WOS_ASYNC,
                                   xs.device.index or 0, s), "wos_siren_eval")
            del keep
        res = [t.reshape(lead + tails[k]) for k, t in enumerate(out) if t is not None]
    else:
        if _is_torch(x):
            x = x.detach().cpu().numpy()
        xs = np.ascontiguousarray(x, dtype=np.float32)
        if xs.ndim < 1 or xs.shape[-1] != p.d_in:
            raise ValueError(f"siren.eval: points must be [..., {p.d_in}], got shape {tuple(xs.shape)}")
        lead = tuple(xs.shape[:-1])
        xs = xs.reshape(-1, p.d_in)
        n = xs.shape[0]
        out = [np.empty((n,) + tails[k], np.float32) if want[k] else None for k in range(3)]
        if n > 0:
            host = [np.ascontiguousarray(t.cpu().numpy()) for t in p.weights + p.biases]
            nl = p.n_hidden_layers + 2
            st, keep = _net_struct(p, [a.ctypes.data for a in host[:nl]], [a.ctypes.data for a in host[nl:]])
            ptr = [a.ctypes.data if a is not None else None for a in out]
            dev = p.weights[0].device.index or 0 if p.weights[0].is_cuda else 0
            s = stream.cuda_stream if hasattr(stream, "cuda_stream") else stream
            check(L.wos_siren_eval(C.byref(st), xs.ctypes.data, n, *ptr, 0, dev, s), "wos_siren_eval")
            del keep, host
        res = [a.reshape(lead + tails[k]) for k, a in enumerate(out) if a is not None]
    return res[0] if len(res) == 1 else tuple(res)


def selftest_layer(W, b, X, device=0):
    """wos_selftest_siren_layer: the kernel's hidden-layer product alone.  W [H, H], b [H],
    X [n, 1 + d_in, H] (numpy) -> the pre-activations Z [n, 1 + d_in, H]: Z[:, 0] = X[:, 0] W^T + b,
    Z[:, s] = X[:, s] W^T for s > 0."""
    W = np.ascontiguousarray(W, np.float32)
    b = np.ascontiguousarray(b, np.float32)
    X = np.ascontiguousarray(X, np.float32)
    if W.ndim != 2 or W.shape[0] != W.shape[1] or b.shape != (W.shape[0],) or X.ndim != 3 or X.shape[2] != W.shape[0]:
        raise ValueError("siren.selftest_layer: W [H, H], b [H], X [n, 1 + d_in, H]")
    Z = np.empty_like(X)
    check(_lib.load().wos_selftest_siren_layer(W.shape[0], X.shape[1] - 1, X.shape[0], W.ctypes.data, b.ctypes.data,
                                               X.ctypes.data, Z.ctypes.data, device), "wos_selftest_siren_layer")
    return Z


def divergence_with_wrap(x, u_net, J, wrap):
    """div of u = wrap(x, N(x)) from the network's value u_net = N(x) [..., d_out] and Jacobian
    J [..., d_out, d_in] (eval(..., jacobian=True)), for a pointwise `wrap` -- the time-stepper's
    query_velocity (src/2d/models/base.py:158-180), which clamps and weights the network's output
    with position-dependent masks.  Chain rule, with autograd through `wrap` alone (an elementwise
    graph: no network in it): div = sum_i [ d wrap_i / d x_i + sum_m d wrap_i / d N_m * J[m, i] ].
    `wrap` must not modify its arguments in place.  Pure torch: runs wherever x lives; returns a
    detached tensor [...] of x's dtype.  wrap = lambda x, u: u gives trace J exactly."""
    import torch
    xl = x.detach().requires_grad_(True)
    ul = u_net.detach().to(xl.dtype).requires_grad_(True)
    Jd = J.detach().to(xl.dtype)
    u = wrap(xl, ul)
    if u.shape[-1] != xl.shape[-1]:
        raise ValueError(f"divergence_with_wrap: wrap returned {u.shape[-1]} components for {xl.shape[-1]} coordinates")
    div = None
    for i in range(u.shape[-1]):
        ui = u[..., i]
        if not ui.requires_grad:  # a component that depends on neither x nor the network: a constant
            term = torch.zeros_like(xl[..., 0])
        else:
            gx, gn = torch.autograd.grad(ui, (xl, ul), torch.ones_like(ui), retain_graph=True, allow_unused=True)
            term = (gn * Jd[..., :, i]).sum(-1) if gn is not None else None
            if gx is not None:
                term = gx[..., i] if term is None else gx[..., i] + term
            if term is None:
                term = torch.zeros_like(xl[..., 0])
        div = term if div is None else div + term
    return div.detach()
