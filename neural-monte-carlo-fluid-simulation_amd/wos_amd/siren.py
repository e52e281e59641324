"""Fused SIREN value, input Jacobian and divergence (wos_siren_eval, csrc/wos_siren.hip).

The reference's projection step differentiates its velocity network by autograd
(get_divergence, src/2d/models/model_split.py:230-236; divergence, diff_ops.py:45-51): one
forward and `dim` backward passes with every activation in HBM.  eval() runs the same MLP
(networks.py:25-68) in forward mode in one kernel: per point the value and its d_in tangents
go through the layers together and only u, J or div come back.  vjp() is its backward with
respect to the weights (wos_siren_vjp, csrc/wos_siren_vjp.hip), apply() the two as one autograd
function over a module's own parameters: PressureProjector.source_from_network(differentiable=True)
trains through the projection without an autograd graph over the network.  fit() is one iteration
of the time-stepper's velocity fits -- the regression loss of the value and its weight gradients in
one value-only pass (wos_siren_fit, csrc/wos_siren_fit.hip) -- fit_loss() the same as an autograd
scalar, diagonal_wrap() the (scale, offset) form of query_velocity's masks that fit() takes and
affine_wrap() the same for a wrap that mixes the velocity's components (a matrix per point).
adam_step() is the loop's optimiser -- clip_grad_norm_ and torch.optim.Adam.step() in one call on an
AdamState (wos_adam_step, csrc/wos_siren_train.hip) -- and fit_run() K iterations of gather, fit()
and adam_step() on a fixed pool from one call (wos_siren_fit_run); fit_run_batches() K iterations of
fit() and adam_step() on fresh rows of another count every iteration, read in place
(wos_siren_fit_run_batches).
"""
import collections
import ctypes as C
import math

import numpy as np

from . import _lib
from ._lib import check

MAX_HIDDEN = 256          # csrc/wos_siren.h kSirenMaxHidden
MAX_HIDDEN_LAYERS = 8     # csrc/wos_siren.h kSirenMaxHiddenLayers
MAX_MEMBERS = 4           # csrc/wos_siren.h kSirenMaxMembers: the members of an ensemble fit loop

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


def _ptr_array(arrays):
    """The addresses of torch tensors or numpy arrays as a C array of pointers."""
    return (C.c_void_p * len(arrays))(*[a.data_ptr() if _is_torch(a) else a.ctypes.data for a in arrays])


def _net_struct(p, host=None):
    """(wos_siren_net, what keeps its pointers alive) over the network's own tensors, or over `host`,
    numpy arrays in their place."""
    n = p.n_hidden_layers + 2
    arrays = p.weights + p.biases if host is None else host
    w, b = _ptr_array(arrays[:n]), _ptr_array(arrays[n:])
    return _lib.SirenNet(p.d_in, p.d_out, p.hidden, p.n_hidden_layers, p.omega, w, b), (w, b, host)


def _host_call(p, stream):
    """What a host-pointer call takes: (host, device, stream), the network's tensors staged as numpy
    arrays from wherever they live, the device ordinal to run on and the raw stream."""
    host = [np.ascontiguousarray(t.cpu().numpy()) for t in p.weights + p.biases]
    dev = p.weights[0].device.index or 0 if p.weights[0].is_cuda else 0
    return host, dev, stream.cuda_stream if hasattr(stream, "cuda_stream") else stream


def _operand(who, name, a, shape, on_gpu, device, like="the points"):
    """One array operand of `who` as a contiguous float32 array of `shape` and of the points' kind: a
    tensor on `device` (on_gpu), else numpy."""
    if tuple(np.shape(a)) != shape:
        raise ValueError(f"siren.{who}: {name} must have shape {shape}, got {tuple(np.shape(a))}")
    if on_gpu:
        import torch
        if not _is_torch(a) or a.device != device:
            raise ValueError(f"siren.{who}: {name} must be a tensor on {device}, like {like}")
        return a.detach().to(torch.float32).contiguous()
    if _is_torch(a):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(a, dtype=np.float32)


def _scale_operand(who, name, a, lead, d_out, on_gpu, device, like="the points"):
    """A fit's scale as _operand() takes it, in either of its two forms: (array, matrix) with matrix
    False for lead + (d_out,), a factor per component, and True for lead + (d_out, d_out), a matrix per
    point (WOS_FIT_SCALE_MATRIX).  None stays (None, False)."""
    if a is None:
        return None, False
    shape = tuple(np.shape(a))
    diagonal, full = tuple(lead) + (d_out,), tuple(lead) + (d_out, d_out)
    if shape not in (diagonal, full):
        raise ValueError(f"siren.{who}: {name} must have shape {diagonal} (a factor per component) or {full} (a matrix "
                         f"per point), got {shape}")
    return _operand(who, name, a, shape, on_gpu, device, like), shape == full


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
            s = _stream_of(stream, [xs] + [t for t in out if t is not None] + p.weights + p.biases, xs.device)
            st, keep = _net_struct(p)
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
            host, dev, s = _host_call(p, stream)
            st, keep = _net_struct(p, host)
            ptr = [a.ctypes.data if a is not None else None for a in out]
            check(L.wos_siren_eval(C.byref(st), xs.ctypes.data, n, *ptr, 0, dev, s), "wos_siren_eval")
            del keep
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


def vjp(net, x, *, grad_value=None, grad_jacobian=None, grad_divergence=None, stream=None, workspace_bytes=None):
    """The backward of eval() with respect to the network: for the cotangents grad_value [..., d_out],
    grad_jacobian [..., d_out, d_in] and grad_divergence [...] of eval's three outputs at the points
    x [..., d_in] (any subset, at least one), (grad_weights, grad_biases) -- two lists in pack()
    order, the gradient of sum(grad_value * u) + sum(grad_jacobian * J) + sum(grad_divergence * div)
    summed over the points, float32.  A torch CUDA tensor in: torch tensors out, enqueued on
    `stream` as in eval() without a host synchronisation; numpy (or a CPU tensor) in: numpy out,
    blocking.  workspace_bytes caps the per-chunk stash (None: the library's 256 MiB).  The same
    call gives the same bits every time; there is no gradient with respect to x or omega."""
    p = net if isinstance(net, PackedSiren) else pack(net)
    if grad_value is None and grad_jacobian is None and grad_divergence is None:
        raise ValueError("siren.vjp: no cotangent given (grad_value, grad_jacobian and grad_divergence are all None)")
    if grad_divergence is not None and p.d_out != p.d_in:
        raise ValueError(f"siren.vjp: grad_divergence needs d_out == d_in, got d_out {p.d_out}, d_in {p.d_in}")
    if len(x.shape) < 1 or x.shape[-1] != p.d_in:
        raise ValueError(f"siren.vjp: points must be [..., {p.d_in}], got shape {tuple(x.shape)}")
    lead = tuple(x.shape[:-1])
    tails = ((p.d_out,), (p.d_out, p.d_in), ())
    names = ("grad_value", "grad_jacobian", "grad_divergence")
    on_gpu = _is_torch(x) and x.is_cuda
    g = [None if c is None else _operand("vjp", names[k], c, lead + tails[k], on_gpu, x.device if on_gpu else None)
         for k, c in enumerate((grad_value, grad_jacobian, grad_divergence))]
    ws = 0 if workspace_bytes is None else int(workspace_bytes)
    if ws < 0:
        raise ValueError(f"siren.vjp: workspace_bytes must be >= 0, got {workspace_bytes}")
    nl = p.n_hidden_layers + 2
    L = _lib.load()
    if on_gpu:
        import torch
        if any(t.device != x.device for t in p.weights + p.biases):
            raise ValueError(f"siren.vjp: the points are on {x.device}, the network on {p.weights[0].device}")
        xs = x.detach().to(torch.float32).contiguous().reshape(-1, p.d_in)
        gw = [torch.empty_like(t) for t in p.weights]
        gb = [torch.empty_like(t) for t in p.biases]
        s = _stream_of(stream, [xs] + [t for t in g if t is not None] + gw + gb + p.weights + p.biases, xs.device)
        st, keep = _net_struct(p)
        check(L.wos_siren_vjp(C.byref(st), xs.data_ptr(), xs.shape[0], *[None if t is None else t.data_ptr() for t in g],
                              _ptr_array(gw), _ptr_array(gb), ws, _lib.WOS_PTRS_DEVICE | _lib.WOS_ASYNC,
                              xs.device.index or 0, s), "wos_siren_vjp")
        del keep
        return gw, gb
    if _is_torch(x):
        x = x.detach().cpu().numpy()
    xs = np.ascontiguousarray(x, dtype=np.float32).reshape(-1, p.d_in)
    host, dev, s = _host_call(p, stream)
    st, keep = _net_struct(p, host)
    gw = [np.empty(a.shape, np.float32) for a in host[:nl]]
    gb = [np.empty(a.shape, np.float32) for a in host[nl:]]
    check(L.wos_siren_vjp(C.byref(st), xs.ctypes.data, xs.shape[0], *[None if a is None else a.ctypes.data for a in g],
                          _ptr_array(gw), _ptr_array(gb), ws, 0, dev, s), "wos_siren_vjp")
    del keep
    return gw, gb


def selftest_vjp_layer(W, dZ, X, device=0):
    """wos_selftest_siren_vjp_layer: the backward's two hidden-layer products alone.  W [H, H],
    dZ and X [n, 1 + d_in, H] (numpy) -> (dX [n, 1 + d_in, H] = dZ W, dW [H, H] = sum_{p,s} dZ[p,s] X[p,s]^T)."""
    W = np.ascontiguousarray(W, np.float32)
    dZ = np.ascontiguousarray(dZ, np.float32)
    X = np.ascontiguousarray(X, np.float32)
    if W.ndim != 2 or W.shape[0] != W.shape[1] or X.ndim != 3 or X.shape[2] != W.shape[0] or dZ.shape != X.shape:
        raise ValueError("siren.selftest_vjp_layer: W [H, H], dZ and X [n, 1 + d_in, H]")
    dX, dW = np.empty_like(X), np.empty_like(W)
    check(_lib.load().wos_selftest_siren_vjp_layer(W.shape[0], X.shape[1] - 1, X.shape[0], W.ctypes.data, dZ.ctypes.data,
                                                   X.ctypes.data, dX.ctypes.data, dW.ctypes.data, device),
          "wos_selftest_siren_vjp_layer")
    return dX, dW


_apply_function = None


def _apply_fn():
    """The autograd function behind apply(), defined at first use (this module imports without torch)."""
    global _apply_function
    if _apply_function is not None:
        return _apply_function
    import torch

    class _SirenApply(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x, shape, want, *params):
            nl = len(params) // 2
            p = PackedSiren(*shape, [t.detach() for t in params[:nl]], [t.detach() for t in params[nl:]])
            out = eval(p, x, value=want[0], jacobian=want[1], divergence=want[2])
            out = out if isinstance(out, tuple) else (out,)
            ctx.shape, ctx.want = shape, want
            ctx.set_materialize_grads(False)
            ctx.save_for_backward(x.detach(), *params)
            return tuple(torch.as_tensor(o) for o in out)

        @staticmethod
        @torch.autograd.function.once_differentiable
        def backward(ctx, *grads):
            x, *params = ctx.saved_tensors
            nl = len(params) // 2
            p = PackedSiren(*ctx.shape, [t.detach() for t in params[:nl]], [t.detach() for t in params[nl:]])
            g, it = [None, None, None], iter(grads)
            for k in range(3):
                if ctx.want[k]:
                    g[k] = next(it)
            gw, gb = vjp(p, x, grad_value=g[0], grad_jacobian=g[1], grad_divergence=g[2])
            return (None, None, None) + tuple(torch.as_tensor(t) for t in gw + gb)

    _apply_function = _SirenApply
    return _apply_function


def apply(module, x, *, value=True, jacobian=False, divergence=False):
    """eval() as a differentiable function of the module's own parameters: the same outputs with the
    same bits, attached to module.parameters() through one autograd node whose backward is vjp()
    with whichever cotangents arrive (once differentiable: a second-order request raises).
    `module`: what pack() takes, as a module (its Linear layers' weight and bias tensors are the
    inputs).  x is a constant: there is no gradient with respect to the points, and an x that
    requires grad is refused."""
    import torch.nn as nn
    p = pack(module)
    if not (value or jacobian or divergence):
        raise ValueError("siren.apply: no output requested")
    if divergence and p.d_out != p.d_in:
        raise ValueError(f"siren.apply: divergence needs d_out == d_in, got d_out {p.d_out}, d_in {p.d_in}")
    if getattr(x, "requires_grad", False):
        raise ValueError("siren.apply: x.requires_grad is set, and there is no gradient with respect to the points; "
                         "pass x.detach()")
    seq = module if isinstance(module, nn.Sequential) else module.net
    lin = [m for m in seq if isinstance(m, nn.Linear)]
    params = [m.weight for m in lin] + [m.bias for m in lin]
    out = _apply_fn().apply(x, tuple(p[:5]), (bool(value), bool(jacobian), bool(divergence)), *params)
    return out[0] if len(out) == 1 else out


def divergence_with_wrap(x, u_net, J, wrap, create_graph=False):
    """div of u = wrap(x, N(x)) from the network's value u_net = N(x) [..., d_out] and Jacobian
    J [..., d_out, d_in] (eval(..., jacobian=True)), for a pointwise `wrap` -- the time-stepper's
    query_velocity (src/2d/models/base.py:158-180), which clamps and weights the network's output
    with position-dependent masks.  Chain rule, with autograd through `wrap` alone (an elementwise
    graph: no network in it): div = sum_i [ d wrap_i / d x_i + sum_m d wrap_i / d N_m * J[m, i] ].
    `wrap` must not modify its arguments in place.  Pure torch: runs wherever x lives; returns a
    detached tensor [...] of x's dtype.  wrap = lambda x, u: u gives trace J exactly.
    create_graph=True: u_net and J are used as they come (apply(..., value=True, jacobian=True)),
    the derivatives of `wrap` keep their graph and the result stays attached, so its gradient
    reaches whatever produced u_net and J through the elementwise graph of `wrap` only."""
    import torch
    xl = x.detach().requires_grad_(True)
    if create_graph:
        ul = u_net.to(xl.dtype)
        if not ul.requires_grad:
            ul = ul.detach().requires_grad_(True)
        Jd = J.to(xl.dtype)
    else:
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
            gx, gn = torch.autograd.grad(ui, (xl, ul), torch.ones_like(ui), retain_graph=True, allow_unused=True,
                                         create_graph=create_graph)
            term = (gn * Jd[..., :, i]).sum(-1) if gn is not None else None
            if gx is not None:
                term = gx[..., i] if term is None else gx[..., i] + term
            if term is None:
                term = torch.zeros_like(xl[..., 0])
        div = term if div is None else div + term
    return div if create_graph else div.detach()


fit_calls = collections.Counter()  # "loss_only" / "grads": how many times fit() went down either path


def fit(net, x, target, scale=None, *, grads=True, stream=None, workspace_bytes=None):
    """One step of the time-stepper's velocity fits without its optimiser (wos_siren_fit,
    csrc/wos_siren_fit.hip): loss = mean((scale * net(x) - target)^2) over the points x [..., d_in]
    and the outputs, target and scale [..., d_out] (scale=None: 1), and its gradient with respect to
    every weight and bias.  scale [..., d_out, d_out], a matrix S per point, makes it
    mean((S @ net(x) - target)^2): the form of a wrap that mixes the network's components
    (affine_wrap()); a matrix that is diagonal gives the bits of its diagonal as a [..., d_out] scale.  Returns (loss, grad_weights, grad_biases), the two lists in pack() order,
    or the loss alone with grads=False: no backward sweep, no stash, no gradient buffer, the same
    bits in the loss.  A torch CUDA tensor in: torch tensors out (loss a 0-d device tensor), enqueued
    on `stream` as in eval() without a host synchronisation; numpy (or a CPU tensor) in: numpy out
    (loss a numpy float32 scalar), blocking.  workspace_bytes caps the per-chunk stash (None: the
    library's 256 MiB).  net(x) is eval()'s value bit for bit; the same call gives the same bits
    every time.  There is no gradient with respect to x, target, scale or omega."""
    p = net if isinstance(net, PackedSiren) else pack(net)
    if len(x.shape) < 1 or x.shape[-1] != p.d_in:
        raise ValueError(f"siren.fit: points must be [..., {p.d_in}], got shape {tuple(x.shape)}")
    lead = tuple(x.shape[:-1])
    on_gpu = _is_torch(x) and x.is_cuda
    dev = x.device if on_gpu else None
    if target is None:
        raise ValueError("siren.fit: target is None")
    t = _operand("fit", "target", target, lead + (p.d_out,), on_gpu, dev)
    sc, matrix = _scale_operand("fit", "scale", scale, lead, p.d_out, on_gpu, dev)
    form = _lib.WOS_FIT_SCALE_MATRIX if matrix else 0
    n = 1
    for k in lead:
        n *= int(k)
    if n <= 0:
        raise ValueError("siren.fit: no points (n must be positive: the loss is a mean)")
    ws = 0 if workspace_bytes is None else int(workspace_bytes)
    if ws < 0:
        raise ValueError(f"siren.fit: workspace_bytes must be >= 0, got {workspace_bytes}")
    nl = p.n_hidden_layers + 2
    L = _lib.load()
    fit_calls["grads" if grads else "loss_only"] += 1
    if on_gpu:
        import torch
        if any(w.device != x.device for w in p.weights + p.biases):
            raise ValueError(f"siren.fit: the points are on {x.device}, the network on {p.weights[0].device}")
        xs = x.detach().to(torch.float32).contiguous().reshape(-1, p.d_in)
        loss = torch.empty((), dtype=torch.float32, device=xs.device)
        gw, gb, flat = [], [], None
        if grads:  # one buffer, the tensors views of it in pack() order: fit_loss scales it in one launch
            flat = torch.empty(sum(a.numel() for a in p.weights + p.biases), dtype=torch.float32, device=xs.device)
            views, at = [], 0
            for a in p.weights + p.biases:
                views.append(flat[at:at + a.numel()].view(a.shape))
                at += a.numel()
            gw, gb = views[:nl], views[nl:]
        held = [xs, t, loss] + ([] if sc is None else [sc]) + ([] if flat is None else [flat]) + p.weights + p.biases
        s = _stream_of(stream, held, xs.device)
        st, keep = _net_struct(p)
        check(L.wos_siren_fit(C.byref(st), xs.data_ptr(), n, t.data_ptr(), None if sc is None else sc.data_ptr(),
                              loss.data_ptr(), _ptr_array(gw) if grads else None, _ptr_array(gb) if grads else None, ws,
                              _lib.WOS_PTRS_DEVICE | _lib.WOS_ASYNC | form, xs.device.index or 0, s), "wos_siren_fit")
        del keep
        return (loss, gw, gb) if grads else loss
    if _is_torch(x):
        x = x.detach().cpu().numpy()
    xs = np.ascontiguousarray(x, dtype=np.float32).reshape(-1, p.d_in)
    host, dev, s = _host_call(p, stream)
    st, keep = _net_struct(p, host)
    loss = np.empty((), np.float32)
    gw = [np.empty(a.shape, np.float32) for a in host[:nl]] if grads else []
    gb = [np.empty(a.shape, np.float32) for a in host[nl:]] if grads else []
    check(L.wos_siren_fit(C.byref(st), xs.ctypes.data, n, t.ctypes.data, None if sc is None else sc.ctypes.data,
                          loss.ctypes.data, _ptr_array(gw) if grads else None, _ptr_array(gb) if grads else None, ws, form,
                          dev, s), "wos_siren_fit")
    del keep
    return (loss[()], gw, gb) if grads else loss[()]


_fit_function = None


def _fit_fn():
    """The autograd function behind fit_loss(), defined at first use (this module imports without torch)."""
    global _fit_function
    if _fit_function is not None:
        return _fit_function
    import torch

    class _SirenFitLoss(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x, target, scale, shape, *params):
            nl = len(params) // 2
            p = PackedSiren(*shape, [t.detach() for t in params[:nl]], [t.detach() for t in params[nl:]])
            # under no_grad, or with no parameter that requires grad, nothing will ask for a backward
            if not any(ctx.needs_input_grad[4:]):
                return torch.as_tensor(fit(p, x, target, scale, grads=False))
            loss, gw, gb = fit(p, x, target, scale)
            kept = [torch.as_tensor(t) for t in gw + gb]
            ctx.shapes = [tuple(t.shape) for t in kept]
            # the device path hands out views of one buffer: keep that; otherwise gather one
            base = kept[0]._base if all(t._base is not None and t._base is kept[0]._base for t in kept) else None
            ctx.save_for_backward(base if base is not None else torch.cat([t.reshape(-1) for t in kept]))
            return torch.as_tensor(loss)

        @staticmethod
        @torch.autograd.function.once_differentiable
        def backward(ctx, g):
            scaled, out, at = g * ctx.saved_tensors[0], [], 0
            for shape, need in zip(ctx.shapes, ctx.needs_input_grad[4:]):
                count = math.prod(shape)
                out.append(scaled[at:at + count].view(shape) if need else None)
                at += count
            return (None, None, None, None) + tuple(out)

    _fit_function = _SirenFitLoss
    return _fit_function


def fit_loss(module, x, target, scale=None):
    """mean((scale * module(x) - target)^2) -- scale [..., d_out], or [..., d_out, d_out] and then
    mean((scale @ module(x) - target)^2), as in fit() -- as a differentiable scalar of the module's own
    parameters, through one autograd node over fit(): the forward computes the loss and every
    parameter gradient in the fused step and keeps the gradients, the backward multiplies them by
    the incoming scalar (once differentiable: a second-order request raises; retain_graph=True works,
    nothing is recomputed).  Under torch.no_grad(), or when no parameter requires grad, only the
    loss-only path runs and no gradient buffer is allocated.  `module`: what pack() takes, as a
    module.  x, target and scale are constants: one that requires grad is refused."""
    import torch
    import torch.nn as nn
    p = pack(module)
    for name, a in (("x", x), ("target", target), ("scale", scale)):
        if getattr(a, "requires_grad", False):
            raise ValueError(f"siren.fit_loss: {name}.requires_grad is set, and there is no gradient with respect to "
                             f"{name}; pass {name}.detach()")
    seq = module if isinstance(module, nn.Sequential) else module.net
    lin = [m for m in seq if isinstance(m, nn.Linear)]
    params = [m.weight for m in lin] + [m.bias for m in lin]
    if not torch.is_grad_enabled():
        params = [t.detach() for t in params]
    return _fit_fn().apply(x, target, scale, tuple(p[:5]), *params)


class AdamState:
    """torch.optim.Adam's state for one network, as wos_adam_step and wos_siren_fit_run take it:
    exp_avg and exp_avg_sq, flat float32 buffers of zeros on the network's device over
    weights + biases in pack() order (the order of fit()'s flat gradient buffer), and `step`, the
    number of steps taken (a Python int).  lr, betas and eps stay Python floats: the library derives
    the step's scalars from the doubles, as torch does.  max_grad_norm=None (or <= 0): no clipping --
    the reference's default, grad_clip = -1."""

    def __init__(self, net, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, max_grad_norm=None):
        import torch
        p = net if isinstance(net, PackedSiren) else pack(net)
        self.lr, self.betas, self.eps = float(lr), (float(betas[0]), float(betas[1])), float(eps)
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.counts = [int(t.numel()) for t in p.weights + p.biases]
        total = sum(self.counts)
        self.exp_avg = torch.zeros(total, dtype=torch.float32, device=p.weights[0].device)
        self.exp_avg_sq = torch.zeros_like(self.exp_avg)
        self.step = 0

    @property
    def clips(self):
        return self.max_grad_norm is not None and self.max_grad_norm > 0

    def params(self):
        """The wos_adam_params of this state."""
        return _lib.AdamParams(self.lr, self.betas[0], self.betas[1], self.eps,
                               self.max_grad_norm if self.clips else -1.0)


def _stream_of(stream, held, device):
    """eval()'s stream discipline: the raw stream to enqueue on, after making `stream` wait for
    torch's current stream and recording the held tensors on it."""
    import torch
    cur = torch.cuda.current_stream(device)
    if stream is None:
        return cur.cuda_stream
    ts = stream if isinstance(stream, torch.cuda.Stream) else torch.cuda.ExternalStream(int(stream), device=device)
    ts.wait_stream(cur)  # the tensors belong to torch's current stream
    for t in held:
        t.record_stream(ts)  # ... and are used on `stream`: the allocator must wait for it
    return ts.cuda_stream


def adam_step(net, grads, state, *, stream=None):
    """clip_grad_norm_ (when state.max_grad_norm is set) and torch.optim.Adam.step() in one call
    (wos_adam_step, csrc/wos_siren_train.hip) on the network's weights and biases, with the gradients
    grads = (grad_weights, grad_biases) as fit() returns them; they are read, never scaled in place.
    Torch CUDA gradients (the network on the same device): the network's own tensors and the state's
    moments are updated in place through their data_ptr(), enqueued on `stream` as in eval() without
    a host synchronisation; returns the unclipped gradient norm (a 0-d device tensor) when clipping
    is on, else None.  numpy gradients: the host-pointer path, blocking -- the network itself is left
    alone and (weights, biases, norm or None) come back as numpy, the updated copies in pack() order;
    the state's moments are updated.  Either way state.step is incremented: the step taken is
    state.step + 1."""
    p = net if isinstance(net, PackedSiren) else pack(net)
    gw, gb = grads
    nl = p.n_hidden_layers + 2
    if len(gw) != nl or len(gb) != nl:
        raise ValueError(f"siren.adam_step: grads must be ({nl} weight gradients, {nl} bias gradients), got "
                         f"({len(gw)}, {len(gb)})")
    tensors, g = p.weights + p.biases, list(gw) + list(gb)
    for k, (t, a) in enumerate(zip(tensors, g)):
        if tuple(a.shape) != tuple(t.shape):
            raise ValueError(f"siren.adam_step: gradient {k} has shape {tuple(a.shape)}, its tensor {tuple(t.shape)}")
    if state.counts != [int(t.numel()) for t in tensors]:
        raise ValueError("siren.adam_step: state was made for a network of another shape")
    n = len(tensors)
    counts = (C.c_int64 * n)(*state.counts)
    opt = state.params()
    L = _lib.load()
    if _is_torch(g[0]) and g[0].is_cuda:
        import torch
        dev = g[0].device
        if any(not _is_torch(a) or a.device != dev or a.dtype != torch.float32 for a in g):
            raise ValueError(f"siren.adam_step: every gradient must be a float32 tensor on {dev}")
        if any(t.device != dev for t in tensors) or state.exp_avg.device != dev:
            raise ValueError(f"siren.adam_step: the gradients are on {dev}, the network on {tensors[0].device}, "
                             f"the state on {state.exp_avg.device}")
        g = [a.detach().contiguous() for a in g]
        norm = torch.empty((), dtype=torch.float32, device=dev) if state.clips else None
        held = g + tensors + [state.exp_avg, state.exp_avg_sq] + ([] if norm is None else [norm])
        s = _stream_of(stream, held, dev)
        check(L.wos_adam_step(n, counts, _ptr_array(tensors), _ptr_array(g), state.exp_avg.data_ptr(),
                              state.exp_avg_sq.data_ptr(), state.step + 1, C.byref(opt),
                              None if norm is None else norm.data_ptr(), _lib.WOS_PTRS_DEVICE | _lib.WOS_ASYNC,
                              dev.index or 0, s), "wos_adam_step")
        state.step += 1
        return norm
    g = [np.ascontiguousarray(a.detach().cpu().numpy() if _is_torch(a) else a, dtype=np.float32) for a in g]
    host = [np.array(t.cpu().numpy(), dtype=np.float32, order="C") for t in tensors]  # copies: the net is left alone
    m, v = state.exp_avg.cpu().numpy().copy(), state.exp_avg_sq.cpu().numpy().copy()
    norm = np.empty((), np.float32) if state.clips else None
    dev = tensors[0].device.index or 0 if tensors[0].is_cuda else 0
    s = stream.cuda_stream if hasattr(stream, "cuda_stream") else stream
    check(L.wos_adam_step(n, counts, _ptr_array(host), _ptr_array(g), m.ctypes.data, v.ctypes.data, state.step + 1,
                          C.byref(opt), None if norm is None else norm.ctypes.data, 0, dev, s), "wos_adam_step")
    import torch
    state.exp_avg.copy_(torch.from_numpy(m))
    state.exp_avg_sq.copy_(torch.from_numpy(v))
    state.step += 1
    return host[:nl], host[nl:], None if norm is None else norm[()]


def fit_run(net, state, pool_x, pool_target, pool_scale, idx, *, stop_loss=None, check_every=0, stream=None,
            workspace_bytes=None):
    """K iterations of gather -> fit() -> adam_step() in one call (wos_siren_fit_run,
    csrc/wos_siren_train.hip), for a fit whose samples, target and scale are fixed for the whole loop
    (the projection fit): iteration i takes the rows idx[i] of pool_x [n_pool, d_in], pool_target and
    pool_scale [n_pool, d_out] or [n_pool, d_out, d_out] (fit()'s two forms; it may be None), and equals, bit for bit in the loss, every
    parameter and both moments, x = pool_x[idx[i]], fit(net, x, ...), adam_step(net, grads, state).
    THE NETWORK'S OWN TENSORS ARE UPDATED IN PLACE, as are the state's moments.  CUDA tensors only;
    idx [K, batch] int64, contiguous.  Returns (losses [K] float32, status [2] int64) as device
    tensors: status[0] the iterations applied, status[1] the indices outside [0, n_pool) (clamped).
    stop_loss=None: never stop, nothing is read on the host, state.step advances by K.
    stop_loss >= 0: the reference's early stop -- the first iteration whose loss is <= stop_loss is
    still applied, every later one is a no-op and its loss stays NaN; state.step then advances by
    status[0], READ ON THE HOST: one synchronisation per call.  check_every=c > 0 synchronises after
    every c iterations and stops enqueuing once stopped (the same bits; the call blocks, and a
    clamped index raises WosError after the run: the iterations are applied, with the row clamped, and
    state.step has advanced by status[0], so network and state still agree); check_every=0 enqueues
    everything on `stream` as in eval().  With check_every=0 a stop does not shorten the call: every
    remaining iteration still runs its gather, packs, fit step and norm kernel, and only the Adam
    update and the loss write are switched off -- set check_every where early stops are expected."""
    import torch
    p = net if isinstance(net, PackedSiren) else pack(net)
    if not (_is_torch(pool_x) and pool_x.is_cuda):
        raise ValueError("siren.fit_run: pool_x must be a CUDA tensor (device pointers only)")
    dev = pool_x.device
    if pool_x.dim() != 2 or pool_x.shape[1] != p.d_in or pool_x.shape[0] < 1:
        raise ValueError(f"siren.fit_run: pool_x must be [n_pool, {p.d_in}], got shape {tuple(pool_x.shape)}")
    n_pool = int(pool_x.shape[0])
    xs = pool_x.detach().to(torch.float32).contiguous()
    t = _operand("fit_run", "pool_target", pool_target, (n_pool, p.d_out), True, dev, "pool_x")
    sc, matrix = _scale_operand("fit_run", "pool_scale", pool_scale, (n_pool,), p.d_out, True, dev, "pool_x")
    if not _is_torch(idx) or idx.device != dev or idx.dtype != torch.int64 or idx.dim() != 2 or not idx.is_contiguous() \
            or idx.shape[0] < 1 or idx.shape[1] < 1:
        raise ValueError(f"siren.fit_run: idx must be a contiguous int64 tensor [K, batch] on {dev}")
    K, batch = int(idx.shape[0]), int(idx.shape[1])

    def call(L, head, *rest):
        return L.wos_siren_fit_run(*head, xs.data_ptr(), t.data_ptr(), None if sc is None else sc.data_ptr(), n_pool,
                                   idx.data_ptr(), K, batch, *rest)
    return _run_loop("fit_run", "pool is", p, state, dev, [xs, t, idx] + ([] if sc is None else [sc]), K, call, stop_loss,
                     check_every, stream, workspace_bytes, clamps=True, matrix=matrix)


def _run_loop(who, what, p, state, dev, inputs, K, call, stop_loss, check_every, stream, workspace_bytes, clamps=False,
              ensemble=False, matrix=False):
    """What fit_run(), fit_run_batches() and their ensemble forms share once their inputs are device
    tensors on `dev`: the checks of the network, the state and the loop's settings, the outputs, the
    stream discipline, the call -- call(library, head, *the arguments from exp_avg on), head being the
    entry point's leading arguments, (net,) or (n_members, nets) -- and the state's step after it.
    ensemble: p and state are the members' lists, the moments go over as arrays of pointers, losses
    and status gain a leading member axis, and each state's step advances by its own status[e][0].
    matrix: the scales are matrices per point (WOS_FIT_SCALE_MATRIX)."""
    import torch
    ps, states = (list(p), list(state)) if ensemble else ([p], [state])
    tensors = []
    for e, (q, sta) in enumerate(zip(ps, states)):
        of = f" of member {e}" if ensemble else ""
        mine = q.weights + q.biases
        if any(w.device != dev for w in mine) or sta.exp_avg.device != dev:
            raise ValueError(f"siren.{who}: the {what} on {dev}, the network{of} on {mine[0].device}, the state on "
                             f"{sta.exp_avg.device}")
        if sta.counts != [int(w.numel()) for w in mine]:
            raise ValueError(f"siren.{who}: state{of} was made for a network of another shape")
        tensors += mine
    first = states[0]
    for e, sta in enumerate(states[1:], 1):
        if (sta.lr, sta.betas, sta.eps, sta.max_grad_norm if sta.clips else None, sta.step) != \
                (first.lr, first.betas, first.eps, first.max_grad_norm if first.clips else None, first.step):
            raise ValueError(f"siren.{who}: the members share the optimiser's parameters and its step: the state of member "
                             f"{e} differs from member 0's in lr, betas, eps, max_grad_norm or step")
    ws = 0 if workspace_bytes is None else int(workspace_bytes)
    if ws < 0:
        raise ValueError(f"siren.{who}: workspace_bytes must be >= 0, got {workspace_bytes}")
    check_every = int(check_every)
    if check_every < 0:
        raise ValueError(f"siren.{who}: check_every must be >= 0, got {check_every}")
    if stop_loss is not None and not float(stop_loss) >= 0.0:
        raise ValueError(f"siren.{who}: stop_loss must be None or >= 0, got {stop_loss}")
    E = len(ps)
    losses = torch.empty((E, K) if ensemble else K, dtype=torch.float32, device=dev)
    # zeros: a call refused before any device work applied nothing
    status = torch.zeros((E, 2) if ensemble else 2, dtype=torch.int64, device=dev)
    moments = [sta.exp_avg for sta in states] + [sta.exp_avg_sq for sta in states]
    s = _stream_of(stream, inputs + [losses, status] + moments + tensors, dev)
    structs = [_net_struct(q) for q in ps]
    if ensemble:
        head = (E, (_lib.SirenNet * E)(*[st for st, _ in structs]))
        m, v = _ptr_array(moments[:E]), _ptr_array(moments[E:])
    else:
        head = (C.byref(structs[0][0]),)
        m, v = moments[0].data_ptr(), moments[1].data_ptr()
    opt = first.params()
    flags = _lib.WOS_PTRS_DEVICE | (0 if check_every > 0 else _lib.WOS_ASYNC) | (_lib.WOS_FIT_SCALE_MATRIX if matrix else 0)
    rc = call(_lib.load(), head, m, v, first.step, C.byref(opt), -1.0 if stop_loss is None else float(stop_loss), check_every,
              losses.data_ptr(), status.data_ptr(), ws, flags, dev.index or 0, s)
    del structs

    def advance():  # each state by the iterations applied to its own network
        applied = status.reshape(E, 2)[:, 0].tolist()
        for sta, k in zip(states, applied):
            sta.step += int(k)
    if clamps and rc == -1 and check_every > 0:
        # The blocking call refuses a clamped index only after the run: its iterations are applied to the
        # network and the moments, so the state's step follows them before the error is raised.
        torch.cuda.synchronize(dev)
        advance()
    check(rc, f"wos_siren_{who}")
    if stop_loss is None:
        for sta in states:
            sta.step += K
    else:
        _current_waits_for(stream, dev)
        advance()
    return losses, status


def _current_waits_for(stream, device):
    """Torch's current stream waits for `stream`, on which the loop's status was written (None: it is the current one)."""
    import torch
    if stream is not None:
        ts = stream if isinstance(stream, torch.cuda.Stream) else torch.cuda.ExternalStream(int(stream), device=device)
        torch.cuda.current_stream(device).wait_stream(ts)


def fit_run_batches(net, state, x, target, scale, counts, *, stop_loss=None, check_every=0, stream=None,
                    workspace_bytes=None):
    """K iterations of fit() -> adam_step() in one call (wos_siren_fit_run_batches) for a fit whose
    points are new every iteration and of another count every iteration (the advection fit, with the
    samples inside an obstacle dropped): x [total, d_in], target and scale [total, d_out] (scale may be
    None, or [total, d_out, d_out]: fit()'s two forms) hold the rows of all iterations one after the other, counts the K positive row counts, which
    sum to total.  Iteration i reads its counts[i] rows in place, as the slice x[o:o + counts[i]] with
    o = sum(counts[:i]), and equals, bit for bit in the loss, every parameter and both moments,
    fit(net, x[o:o + n], target[o:o + n], scale[o:o + n]) and adam_step(net, grads, state): the loss is
    the mean over that iteration's own rows.  THE NETWORK'S OWN TENSORS ARE UPDATED IN PLACE, as are
    the state's moments.  CUDA tensors only; the offsets are built on the host.  Returns
    (losses [K] float32, status [2] int64) as device tensors: status[0] the iterations applied,
    status[1] always 0.  stop_loss, check_every, `stream`, workspace_bytes and state.step as in
    fit_run()."""
    import torch
    p = net if isinstance(net, PackedSiren) else pack(net)
    if len(x.shape) != 2 or x.shape[1] != p.d_in or x.shape[0] < 1:
        raise ValueError(f"siren.fit_run_batches: x must be [total, {p.d_in}], got shape {tuple(x.shape)}")
    total = int(x.shape[0])
    offsets = _batch_offsets("siren.fit_run_batches", counts, total)
    if not (_is_torch(x) and x.is_cuda):
        raise ValueError("siren.fit_run_batches: x must be a CUDA tensor (device pointers only)")
    dev = x.device
    xs = x.detach().to(torch.float32).contiguous()
    t = _operand("fit_run_batches", "target", target, (total, p.d_out), True, dev, "x")
    sc, matrix = _scale_operand("fit_run_batches", "scale", scale, (total,), p.d_out, True, dev, "x")
    K = len(offsets) - 1

    def call(L, head, *rest):
        return L.wos_siren_fit_run_batches(*head, xs.data_ptr(), t.data_ptr(), None if sc is None else sc.data_ptr(),
                                           (C.c_int64 * (K + 1))(*offsets), K, *rest)
    return _run_loop("fit_run_batches", "points are", p, state, dev, [xs, t] + ([] if sc is None else [sc]), K, call,
                     stop_loss, check_every, stream, workspace_bytes, matrix=matrix)


def _batch_offsets(who, counts, total):
    """The K + 1 row offsets of K positive counts that sum to `total`, as Python ints."""
    offsets = [0]
    for i, c in enumerate(counts):
        if int(c) != c or int(c) <= 0:
            raise ValueError(f"{who}: counts[{i}] must be a positive int (a mean over nothing), got {c!r}")
        offsets.append(offsets[-1] + int(c))
    if len(offsets) < 2:
        raise ValueError(f"{who}: counts is empty (at least one iteration)")
    if offsets[-1] != total:
        raise ValueError(f"{who}: counts sum to {offsets[-1]}, the tensors hold {total} rows")
    return offsets


def _members(who, nets, states):
    """The packed members of an ensemble call and their shared shape."""
    ps = [net if isinstance(net, PackedSiren) else pack(net) for net in nets]
    states = list(states)
    if not 1 <= len(ps) <= MAX_MEMBERS:
        raise ValueError(f"siren.{who}: an ensemble has 1..{MAX_MEMBERS} members, got {len(ps)}")
    if len(states) != len(ps):
        raise ValueError(f"siren.{who}: {len(ps)} networks, but {len(states)} states")
    for e, q in enumerate(ps[1:], 1):
        if tuple(q[:5]) != tuple(ps[0][:5]):
            raise ValueError(f"siren.{who}: member {e} is {tuple(q[:5])}, member 0 {tuple(ps[0][:5])} (d_in, d_out, hidden, "
                             f"n_hidden_layers, omega): the members of an ensemble have one shape")
    return ps, states


def _member_operands(who, name, arrays, E, shape, dev, like, optional=False):
    """One operand per member, each as _operand() takes it; optional: the list, or an entry, may be None."""
    if arrays is None and optional:
        return [None] * E
    arrays = list(arrays)
    if len(arrays) != E:
        raise ValueError(f"siren.{who}: {name} must hold one array per member ({E}), got {len(arrays)}")
    return [None if a is None and optional else _operand(who, f"{name}[{e}]", a, shape, True, dev, like)
            for e, a in enumerate(arrays)]


def _member_scales(who, name, arrays, E, lead, d_out, dev, like):
    """One scale per member (the list, or an entry, may be None), each in either of fit()'s two forms:
    (scales, matrix).  One call has one form: when any member's is a matrix per point, a member's
    factors per component become diagonal matrices, which give the same values."""
    if arrays is None:
        return [None] * E, False
    arrays = list(arrays)
    if len(arrays) != E:
        raise ValueError(f"siren.{who}: {name} must hold one array per member ({E}), got {len(arrays)}")
    pairs = [_scale_operand(who, f"{name}[{e}]", a, lead, d_out, True, dev, like) for e, a in enumerate(arrays)]
    matrix = any(m for _, m in pairs)
    if not matrix:
        return [sc for sc, _ in pairs], False
    import torch
    return [sc if sc is None or m else torch.diag_embed(sc).contiguous() for sc, m in pairs], True


def fit_run_ensemble(nets, states, pool_x, pool_targets, pool_scales, idx, *, stop_loss=None, check_every=0, stream=None,
                     workspace_bytes=None):
    """fit_run() for the E <= 4 members of an ensemble in one device loop (wos_siren_fit_run_ensemble):
    nets and states are lists of E networks of one shape and their AdamStates (the same lr, betas, eps,
    max_grad_norm and step), pool_targets a list of E tensors [n_pool, d_out], pool_scales None or a
    list whose entries may be None, [n_pool, d_out] or [n_pool, d_out, d_out] (with both forms in one
    list, the factors per component go over as diagonal matrices).  The members share pool_x and the index draw idx -- common random
    numbers, as the walks of a multi-channel solve -- and every launch of an iteration covers all of
    them.  Member e's losses, parameters and moments are, bit for bit, fit_run()'s on member e alone.
    EVERY NETWORK IS UPDATED IN PLACE.  Returns (losses [E, K], status [E, 2]) on the device.  The stop
    is per member: a stopped member's updates and loss writes are no-ops while the others go on, each
    state's step advances by its own status[e][0], and check_every=c stops enqueuing once every member
    has stopped.  Everything else as in fit_run()."""
    import torch
    ps, states = _members("fit_run_ensemble", nets, states)
    p, E = ps[0], len(ps)
    if not (_is_torch(pool_x) and pool_x.is_cuda):
        raise ValueError("siren.fit_run_ensemble: pool_x must be a CUDA tensor (device pointers only)")
    dev = pool_x.device
    if pool_x.dim() != 2 or pool_x.shape[1] != p.d_in or pool_x.shape[0] < 1:
        raise ValueError(f"siren.fit_run_ensemble: pool_x must be [n_pool, {p.d_in}], got shape {tuple(pool_x.shape)}")
    n_pool = int(pool_x.shape[0])
    xs = pool_x.detach().to(torch.float32).contiguous()
    ts = _member_operands("fit_run_ensemble", "pool_targets", pool_targets, E, (n_pool, p.d_out), dev, "pool_x")
    scs, matrix = _member_scales("fit_run_ensemble", "pool_scales", pool_scales, E, (n_pool,), p.d_out, dev, "pool_x")
    if not _is_torch(idx) or idx.device != dev or idx.dtype != torch.int64 or idx.dim() != 2 or not idx.is_contiguous() \
            or idx.shape[0] < 1 or idx.shape[1] < 1:
        raise ValueError(f"siren.fit_run_ensemble: idx must be a contiguous int64 tensor [K, batch] on {dev}")
    K, batch = int(idx.shape[0]), int(idx.shape[1])
    t_ptrs, s_ptrs = _ptr_array(ts), _opt_ptr_array(scs)

    def call(L, head, *rest):
        return L.wos_siren_fit_run_ensemble(*head, xs.data_ptr(), t_ptrs, s_ptrs, n_pool, idx.data_ptr(), K, batch, *rest)
    return _run_loop("fit_run_ensemble", "pool is", ps, states, dev, [xs, idx] + ts + [sc for sc in scs if sc is not None], K,
                     call, stop_loss, check_every, stream, workspace_bytes, clamps=True, ensemble=True, matrix=matrix)


def fit_run_batches_ensemble(nets, states, x, targets, scales, counts, *, stop_loss=None, check_every=0, stream=None,
                             workspace_bytes=None):
    """fit_run_batches() for the E <= 4 members of an ensemble in one device loop
    (wos_siren_fit_run_batches_ensemble): the members share the points x [total, d_in] and the row
    counts; targets is a list of E tensors [total, d_out], scales None or a list whose entries may be
    None, [total, d_out] or [total, d_out, d_out] as in fit_run_ensemble().  Member e's losses, parameters and moments are, bit for bit, fit_run_batches()'s on member e
    alone.  nets, states, the returned (losses [E, K], status [E, 2]) and the per-member stop as in
    fit_run_ensemble()."""
    import torch
    ps, states = _members("fit_run_batches_ensemble", nets, states)
    p, E = ps[0], len(ps)
    if len(x.shape) != 2 or x.shape[1] != p.d_in or x.shape[0] < 1:
        raise ValueError(f"siren.fit_run_batches_ensemble: x must be [total, {p.d_in}], got shape {tuple(x.shape)}")
    total = int(x.shape[0])
    offsets = _batch_offsets("siren.fit_run_batches_ensemble", counts, total)
    if not (_is_torch(x) and x.is_cuda):
        raise ValueError("siren.fit_run_batches_ensemble: x must be a CUDA tensor (device pointers only)")
    dev = x.device
    xs = x.detach().to(torch.float32).contiguous()
    ts = _member_operands("fit_run_batches_ensemble", "targets", targets, E, (total, p.d_out), dev, "x")
    scs, matrix = _member_scales("fit_run_batches_ensemble", "scales", scales, E, (total,), p.d_out, dev, "x")
    K = len(offsets) - 1
    t_ptrs, s_ptrs = _ptr_array(ts), _opt_ptr_array(scs)

    def call(L, head, *rest):
        return L.wos_siren_fit_run_batches_ensemble(*head, xs.data_ptr(), t_ptrs, s_ptrs, (C.c_int64 * (K + 1))(*offsets), K,
                                                    *rest)
    return _run_loop("fit_run_batches_ensemble", "points are", ps, states, dev, [xs] + ts + [sc for sc in scs if sc is not None],
                     K, call, stop_loss, check_every, stream, workspace_bytes, ensemble=True, matrix=matrix)


def _opt_ptr_array(arrays):
    """_ptr_array over entries that may be None (a NULL entry); None when every entry is."""
    if all(a is None for a in arrays):
        return None
    return (C.c_void_p * len(arrays))(*[None if a is None else a.data_ptr() for a in arrays])


_probes = {}  # diagonal_wrap's probe of the last (shape, dtype, device)


def diagonal_wrap(wrap, x, d_out, check=True):
    """(scale, offset) [..., d_out] of a pointwise wrap that is diagonal-affine in the network's
    output, wrap(x, N) = scale * N + offset -- the time-stepper's query_velocity for karman (inlet
    clamp, wall and obstacle weights) and taylorgreen (src/2d/models/base.py:169-189):
    offset = wrap(x, 0), scale = wrap(x, 1) - offset.  check=True probes one random N and raises
    ValueError unless wrap(x, N) equals scale * N + offset to float rounding: a wrap that mixes the
    output's components (the jpipe branch) has no diagonal form -- affine_wrap() returns its matrix,
    which fit() takes as well.  Pure torch, detached, of x's dtype on x's device."""
    import torch
    with torch.no_grad():
        xd = x.detach()
        shape = tuple(xd.shape[:-1]) + (int(d_out),)
        zero = torch.zeros(shape, dtype=xd.dtype, device=xd.device)
        offset = wrap(xd, zero.clone())
        if tuple(offset.shape) != shape:
            raise ValueError(f"siren.diagonal_wrap: wrap returned shape {tuple(offset.shape)} for an output of {shape}")
        scale = wrap(xd, torch.ones_like(zero)) - offset
        if check:
            key = (shape, xd.dtype, xd.device)
            probe = _probes.get(key)
            if probe is None:  # one random N per shape, dtype and device, in [0.5, 2.5): no entry is 0 or 1
                gen = torch.Generator(device="cpu").manual_seed(20240229)
                probe = (torch.rand(shape, generator=gen, dtype=torch.float64) * 2.0 + 0.5).to(xd.dtype).to(xd.device)
                _probes.clear()
                _probes[key] = probe
            got = wrap(xd, probe.clone())
            want = scale * probe + offset
            eps = torch.finfo(xd.dtype).eps
            tol = 8 * eps * (scale.abs() * probe.abs() + offset.abs() + got.abs())
            bad = (got - want).abs() > tol
            if bool(bad.any()):
                name = getattr(wrap, "__name__", type(wrap).__name__)
                raise ValueError(f"siren.diagonal_wrap: wrap '{name}' is not diagonal-affine in the network's output "
                                 f"(it mixes components or is nonlinear: {int(bad.sum())} of {bad.numel()} entries "
                                 f"differ from scale * N + offset); siren.affine_wrap covers a wrap that mixes components")
    return scale, offset


def _affine_columns(wrap, xd, d_out):
    """(S [..., d_out, d_out], offset [..., d_out]) of a wrap that is affine in the network's output:
    offset = wrap(x, 0), column m of S = wrap(x, e_m) - offset.  d_out + 1 calls of wrap, nothing read
    on the host."""
    import torch
    shape = tuple(xd.shape[:-1]) + (int(d_out),)
    zero = torch.zeros(shape, dtype=xd.dtype, device=xd.device)
    offset = wrap(xd, zero.clone())
    if tuple(offset.shape) != shape:
        raise ValueError(f"siren.affine_wrap: wrap returned shape {tuple(offset.shape)} for an output of {shape}")
    cols = []
    for m in range(int(d_out)):
        e = zero.clone()
        e[..., m] = 1
        cols.append(wrap(xd, e) - offset)
    return torch.stack(cols, dim=-1), offset


def affine_wrap(wrap, x, d_out, check=True):
    """(scale, offset, mixes) of a pointwise wrap that is affine in the network's output,
    wrap(x, N) = S(x) N + offset(x): offset = wrap(x, 0) [..., d_out] and column m of S is
    wrap(x, e_m) - offset.  mixes is False when every off-diagonal entry of S is exactly zero; scale is
    then the [..., d_out] diagonal, bit for bit what diagonal_wrap() returns (query_velocity's karman
    and taylorgreen branches).  Otherwise mixes is True and scale is S [..., d_out, d_out] -- the jpipe
    branch's free-slip form u = (I - (1 - w) n n^T) N (src/2d/models/base.py:191-222;
    wos_amd.projection.slip_wrap) -- which fit() and the fit loops take as it is.  check=True probes one
    random N, diagonal_wrap()'s, and raises ValueError unless wrap(x, N) equals S N + offset to float
    rounding (diagonal_wrap()'s tolerance, taken per point, not per component: the entries of a
    projector cancel): a wrap that is nonlinear in N is refused by name.  mixes is read on the host: one
    synchronisation.  Pure torch, detached, of x's dtype on x's device."""
    import torch
    with torch.no_grad():
        xd = x.detach()
        S, offset = _affine_columns(wrap, xd, d_out)
        shape = tuple(offset.shape)
        if check:
            key = (shape, xd.dtype, xd.device)
            probe = _probes.get(key)
            if probe is None:  # diagonal_wrap's probe, made the same way
                gen = torch.Generator(device="cpu").manual_seed(20240229)
                probe = (torch.rand(shape, generator=gen, dtype=torch.float64) * 2.0 + 0.5).to(xd.dtype).to(xd.device)
                _probes.clear()
                _probes[key] = probe
            got = wrap(xd, probe.clone())
            want = (S * probe.unsqueeze(-2)).sum(-1) + offset
            eps = torch.finfo(xd.dtype).eps
            # diagonal_wrap's rule, 8 eps (|S| |N| + |offset| + |wrap(x, N)|), with the three terms summed
            # over the point's components: an entry such as 1 - n_i^2 of a projector is formed with an
            # absolute error of eps of the matrix's size, which its own size does not show
            tol = 8 * eps * (S.abs().sum((-2, -1)) * probe.abs().sum(-1) + offset.abs().sum(-1) + got.abs().sum(-1))
            bad = (got - want).abs() > tol.unsqueeze(-1)
            if bool(bad.any()):
                name = getattr(wrap, "__name__", type(wrap).__name__)
                raise ValueError(f"siren.affine_wrap: wrap '{name}' is not affine in the network's output (it is "
                                 f"nonlinear: {int(bad.sum())} of {bad.numel()} entries differ from S N + offset); keep "
                                 f"the siren.apply route for it")
        off_diagonal = S * (1 - torch.eye(int(d_out), dtype=S.dtype, device=S.device))
        mixes = bool((off_diagonal != 0).any())
        if not mixes:
            return diagonal_wrap(wrap, xd, d_out, check=False)[0], offset, False
    return S, offset, True
