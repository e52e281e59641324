"""Fused SIREN backward on the GPU (wos_siren_vjp, csrc/wos_siren_vjp.hip): the two hidden-layer
products' lane maps against exact integer data, accuracy of every parameter gradient against the
float64 model with float32 autograd as the yardstick, tail tiles and chunks, determinism, the
C ABI's pointer and refusal rules, siren.apply, and training through PressureProjector.

Measured on the MI355X (ratios of the fused backward's error to float32 autograd's, RMS / max,
against float64; the caps are 2.5 / 4): see profiles/siren_vjp_accuracy.json."""
import copy
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest
import torch

import siren_model as sm
import siren_vjp_model as vm
from wos_amd import _lib, siren, workloads
from wos_amd import projection as pj

pytestmark = pytest.mark.gpu


def bits(a):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def host(grads):
    return [t.cpu().numpy() for t in grads[0]], [t.cpu().numpy() for t in grads[1]]


def same_bits(a, b):
    return all(np.array_equal(bits(s), bits(t)) for s, t in zip(a[0] + a[1], b[0] + b[1]))


def _cuda_net(d, H, L, d_out=None):
    return copy.deepcopy(sm.make_net(d, H, L, d_out)).cuda()


# ---- 1. lane maps, exact -----------------------------------------------------------------------------
@pytest.mark.parametrize("n_points", [1, 31, 32, 33, 65])
@pytest.mark.parametrize("d_in", [2, 3])
@pytest.mark.parametrize("H", [32, 64, 96, 128, 160, 192, 224, 256])
def test_backward_layer_lane_maps_exact(gpu, H, d_in, n_points):
    """Integers of magnitude <= 3: dX sums at most 256 * 9, dW at most 65 * 4 * 9 terms' worth, all exact
    in f32, so a dropped or doubled k, an untransposed W, a tangent in the wrong column or a padding
    column that counts all show."""
    i, k = np.meshgrid(np.arange(H), np.arange(H), indexing="ij")
    W = ((3 * i + 5 * k) % 7 - 3).astype(np.int64)
    p, s, h = np.meshgrid(np.arange(n_points), np.arange(1 + d_in), np.arange(H), indexing="ij")
    dZ = ((5 * p + 11 * s + 7 * h + (p * h) % 3 + (s * h) % 5) % 7 - 3).astype(np.int64)
    X = ((3 * p + 2 * s + 5 * h + (p * s) % 4 + (p * h) % 5) % 7 - 3).astype(np.int64)
    want_dX = np.einsum("ki,psk->psi", W, dZ)
    want_dW = np.einsum("psr,psc->rc", dZ, X)
    assert max(np.abs(want_dX).max(), np.abs(want_dW).max()) < 2 ** 24 and not np.array_equal(W, W.T)
    assert not np.array_equal(want_dW, want_dW.T)
    dX, dW = siren.selftest_vjp_layer(W, dZ, X, device=gpu)
    assert dX.shape == dZ.shape and dW.shape == (H, H) and dX.dtype == dW.dtype == np.float32
    assert np.array_equal(dX.astype(np.int64), want_dX) and np.array_equal(dX, want_dX.astype(np.float32))
    assert np.array_equal(dW.astype(np.int64), want_dW) and np.array_equal(dW, want_dW.astype(np.float32))


# ---- 2. accuracy against float64 -----------------------------------------------------------------------
SHAPES = [(2, 32, 1, None), (2, 128, 2, None), (2, 256, 3, None), (3, 256, 3, None), (3, 96, 2, None), (2, 64, 0, None),
          (3, 64, 1, 1),
          # H / 32 = 5, 6, 7: two row tiles per wave with a dropped duplicate, and a partial second 128-tile of dW
          (2, 160, 1, None), (3, 192, 2, None), (2, 224, 3, None),
          # the reference's depth, and L = 8 (12 reduce segments) at the smallest and the largest width
          (2, 256, 5, None), (3, 32, 8, None), (3, 256, 8, None),
          # d_out != d_in
          (2, 64, 1, 3), (3, 64, 1, 2), (2, 64, 1, 1)]


@functools.lru_cache(maxsize=None)
def _reference(d, H, L, d_out, which, n=193):
    """(x, cotangents, float64 model, float32 autograd on the GPU) of one case, computed once."""
    net, x = sm.make_net(d, H, L, d_out), sm.points(d, n, seed=0)
    g_u, g_J, g_div = vm.cotangents(n, d_out or d, d)
    g = (g_u, g_J, g_div if (d_out or d) == d else None) if which == "all" else (None, None, g_div)
    ref = vm.model64(*vm.net_arrays(net), x, *g)
    t32 = vm.autograd_grads(_cuda_net(d, H, L, d_out), torch.from_numpy(x).cuda(), *g)
    return x, g, ref, t32


def _vjp(net, x, g, **kw):
    dev = [None if a is None else torch.from_numpy(a).cuda() for a in g]
    return host(siren.vjp(net, torch.from_numpy(x).cuda(), grad_value=dev[0], grad_jacobian=dev[1],
                          grad_divergence=dev[2], **kw))


CASES = [(s, w) for s in SHAPES for w in ("all", "div") if not (w == "div" and s[3] is not None)]


@pytest.mark.parametrize("shape,which", CASES, ids=[f"d{s[0]}_H{s[1]}_L{s[2]}_o{s[3] or s[0]}_{w}" for s, w in CASES])
def test_gradients_as_accurate_as_float32_autograd(gpu, shape, which):
    d, H, L, d_out = shape
    x, g, ref, t32 = _reference(d, H, L, d_out, which)
    got = _vjp(_cuda_net(d, H, L, d_out), x, g)
    rec = {}
    try:
        vm.assert_grads_as_accurate(got, t32, ref, g[0], f"({d},{H},{L},{d_out or d}) {which}", record=rec)
    finally:
        out = os.environ.get("WOS_SIREN_VJP_ACCURACY_OUT")  # a measuring run keeps the figures; the suite writes nothing
        if out:
            with open(out, "a") as f:
                f.write(json.dumps({"d": d, "hidden": H, "hidden_layers": L, "d_out": d_out or d, "points": 193,
                                    "cotangents": which, **rec}) + "\n")


# ---- 3. tail tiles and chunks ----------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 31, 33, 65])
def test_tail_tiles(gpu, n):
    x, g, ref, t32 = _reference(2, 64, 1, None, "all", n)
    got = _vjp(_cuda_net(2, 64, 1), x, g)
    vm.assert_grads_as_accurate(got, t32, ref, g[0], f"n = {n}")


def _tile_bytes(d, H, L):
    return (2 * L + 1) * H * (1 + d) * 4 * 32


@pytest.mark.parametrize("tiles", [1, 2])
def test_chunks_of_one_and_two_tiles(gpu, tiles):
    d, H, L = 2, 64, 1
    x, g, ref, t32 = _reference(d, H, L, None, "all")
    ws = tiles * _tile_bytes(d, H, L) + 100  # 7 tiles in chunks of `tiles`; the slack must not buy another tile
    got = _vjp(_cuda_net(d, H, L), x, g, workspace_bytes=ws)
    vm.assert_grads_as_accurate(got, t32, ref, g[0], f"chunks of {tiles}")
    again = _vjp(_cuda_net(d, H, L), x, g, workspace_bytes=ws)
    assert same_bits(got, again)


def test_workspace_below_one_tile_is_refused(gpu):
    x, g, _, _ = _reference(2, 64, 1, None, "all")
    with pytest.raises(_lib.WosError, match="workspace_bytes"):
        _vjp(_cuda_net(2, 64, 1), x, g, workspace_bytes=_tile_bytes(2, 64, 1) - 1)
    assert b"cannot hold one tile" in _lib.load().wos_last_error()


def test_no_hidden_layer_host_pointers_equal_device_pointers(gpu):
    """L = 0: no packed copies, the temporary is the H zeros and the plan's work (accuracy at L = 0: SHAPES above)."""
    net, n = _cuda_net(2, 32, 0), 33  # one full tile and one point
    x, g = sm.points(2, n), vm.cotangents(n, 2, 2)
    dev = siren.vjp(net, torch.from_numpy(x).cuda(), grad_value=torch.from_numpy(g[0]).cuda(),
                    grad_jacobian=torch.from_numpy(g[1]).cuda(), grad_divergence=torch.from_numpy(g[2]).cuda())
    host = siren.vjp(net, x, grad_value=g[0], grad_jacobian=g[1], grad_divergence=g[2])
    for kind in (0, 1):
        assert len(host[kind]) == 2
        for l, (a, b) in enumerate(zip(host[kind], dev[kind])):
            assert isinstance(a, np.ndarray) and np.array_equal(bits(a), bits(b)), (kind, l)
            assert np.isfinite(a).all() and np.abs(a).max() > 0, (kind, l)


# ---- 4. determinism and zeros ----------------------------------------------------------------------------
@pytest.mark.parametrize("side", [False, True], ids=["current_stream", "side_stream"])
def test_determinism_zeros_and_written_not_accumulated(gpu, side):
    d, H, L = 3, 256, 3
    net = _cuda_net(d, H, L)
    x = torch.from_numpy(sm.points(d, 193)).cuda()
    g = [torch.from_numpy(a).cuda() for a in vm.cotangents(193, d, d)]
    stream = torch.cuda.Stream() if side else None

    def run(gs):
        out = siren.vjp(net, x, grad_value=gs[0], grad_jacobian=gs[1], grad_divergence=gs[2], stream=stream)
        if side:
            stream.synchronize()
        return host(out)
    first = run(g)
    assert same_bits(first, run(g)), "two calls, the same bits"
    assert all(np.isfinite(a).all() and np.any(a) for a in first[0] + first[1])
    zeros = run([torch.zeros_like(t) for t in g])
    assert all(not np.any(bits(a)) for a in zeros[0] + zeros[1]), "zero cotangents, zero gradients"
    # the C ABI on buffers full of NaN: written, not accumulated
    p = siren.pack(net)
    nl = L + 2
    gw = [torch.full_like(t, float("nan")) for t in p.weights]
    gb = [torch.full_like(t, float("nan")) for t in p.biases]
    w = (C.c_void_p * nl)(*[t.data_ptr() for t in p.weights])
    b = (C.c_void_p * nl)(*[t.data_ptr() for t in p.biases])
    st = _lib.SirenNet(p.d_in, p.d_out, p.hidden, p.n_hidden_layers, p.omega, w, b)
    pw = (C.c_void_p * nl)(*[t.data_ptr() for t in gw])
    pb = (C.c_void_p * nl)(*[t.data_ptr() for t in gb])
    torch.cuda.synchronize()
    s = stream.cuda_stream if side else None
    rc = _lib.load().wos_siren_vjp(C.byref(st), x.data_ptr(), 193, g[0].data_ptr(), g[1].data_ptr(), g[2].data_ptr(),
                                   pw, pb, 0, _lib.WOS_PTRS_DEVICE | _lib.WOS_ASYNC, gpu, s)
    assert rc == 0, _lib.load().wos_last_error()
    torch.cuda.synchronize()
    assert same_bits(first, host((gw, gb))), "NaN-filled buffers come back as the first call's bits"


# ---- 5. C ABI ------------------------------------------------------------------------------------------
def _c_net(p, ws, bs, ptr):
    n = p.n_hidden_layers + 2
    w = (C.c_void_p * n)(*[ptr(t) for t in ws])
    b = (C.c_void_p * n)(*[ptr(t) for t in bs])
    return _lib.SirenNet(p.d_in, p.d_out, p.hidden, p.n_hidden_layers, p.omega, w, b)


def test_c_abi_pointers_and_refusals(gpu):
    L = _lib.load()
    net = _cuda_net(2, 64, 1)
    p = siren.pack(net)
    n, nl = 45, 3
    x = sm.points(2, n)
    g = vm.cotangents(n, 2, 2)
    xd = torch.from_numpy(x).cuda()
    gd = [torch.from_numpy(a).cuda() for a in g]
    want = host(siren.vjp(net, xd, grad_value=gd[0], grad_jacobian=gd[1], grad_divergence=gd[2]))
    # host pointers, blocking: weights, points, cotangents and gradients all on the host
    hw, hb = [t.cpu().numpy() for t in p.weights], [t.cpu().numpy() for t in p.biases]
    hnet = _c_net(p, hw, hb, lambda a: a.ctypes.data)
    ow, ob = [np.full(a.shape, np.nan, np.float32) for a in hw], [np.full(a.shape, np.nan, np.float32) for a in hb]
    pw = (C.c_void_p * nl)(*[a.ctypes.data for a in ow])
    pb = (C.c_void_p * nl)(*[a.ctypes.data for a in ob])
    rc = L.wos_siren_vjp(C.byref(hnet), x.ctypes.data, n, *[a.ctypes.data for a in g], pw, pb, 0, 0, gpu, None)
    assert rc == 0, L.wos_last_error()
    assert same_bits((ow, ob), want), "host pointers equal device pointers"
    # each cotangent alone through host pointers equals the python layer on the device
    for k in range(3):
        only = [a.ctypes.data if m == k else None for m, a in enumerate(g)]
        assert L.wos_siren_vjp(C.byref(hnet), x.ctypes.data, n, *only, pw, pb, 0, 0, gpu, None) == 0, L.wos_last_error()
        kw = dict(zip(("grad_value", "grad_jacobian", "grad_divergence"), [t if m == k else None for m, t in enumerate(gd)]))
        assert same_bits((ow, ob), host(siren.vjp(net, xd, **kw))), f"cotangent {k} alone"
    # n = 0 writes zeros, host and device
    for a in ow + ob:
        a.fill(np.nan)
    assert L.wos_siren_vjp(C.byref(hnet), None, 0, *[a.ctypes.data for a in g], pw, pb, 0, 0, gpu, None) == 0
    assert all(not np.any(bits(a)) for a in ow + ob)
    dnet = _c_net(p, p.weights, p.biases, lambda t: t.data_ptr())
    dw, db = [torch.full_like(t, float("nan")) for t in p.weights], [torch.full_like(t, float("nan")) for t in p.biases]
    qw = (C.c_void_p * nl)(*[t.data_ptr() for t in dw])
    qb = (C.c_void_p * nl)(*[t.data_ptr() for t in db])
    flags = _lib.WOS_PTRS_DEVICE
    torch.cuda.synchronize()
    assert L.wos_siren_vjp(C.byref(dnet), xd.data_ptr(), 0, *[t.data_ptr() for t in gd], qw, qb, 0, flags, gpu, None) == 0
    assert all(not np.any(bits(t)) for t in dw + db)
    # refusals
    for t in dw + db:
        t.fill_(7.0)
    torch.cuda.synchronize()
    gp = [t.data_ptr() for t in gd]

    def call(net_=dnet, n_=n, g_=gp, w_=qw, b_=qb, ws=0):
        return L.wos_siren_vjp(C.byref(net_), xd.data_ptr(), n_, *g_, w_, b_, ws, flags, gpu, None)
    assert call(g_=[None, None, None]) == -1 and b"no cotangent" in L.wos_last_error()
    assert call(n_=-1) == -1 and b"n is negative" in L.wos_last_error()
    assert call(w_=None) == -1 and b"grad_weights" in L.wos_last_error()
    assert call(b_=None) == -1 and b"grad_biases" in L.wos_last_error()
    hole = (C.c_void_p * nl)(qw[0], None, qw[2])
    assert call(w_=hole) == -1 and b"grad_weights" in L.wos_last_error() and b"layer 1" in L.wos_last_error()
    assert call(ws=100) == _lib.WOS_E_CAPACITY and b"workspace_bytes" in L.wos_last_error()
    bad = _c_net(p, p.weights, p.biases, lambda t: t.data_ptr())
    bad.hidden = 100
    assert call(net_=bad) == -1 and b"hidden" in L.wos_last_error() and b"100" in L.wos_last_error()
    bad.hidden, bad.d_out = 64, 1
    assert call(net_=bad, g_=[None, None, gp[2]]) == -1 and b"g_div needs d_out == d_in" in L.wos_last_error()
    for field, value in (("d_in", 4), ("d_out", 0), ("n_hidden_layers", 9), ("omega", float("inf"))):
        bad = _c_net(p, p.weights, p.biases, lambda t: t.data_ptr())
        setattr(bad, field, value)
        assert call(net_=bad) == -1 and field.encode() in L.wos_last_error(), field
    torch.cuda.synchronize()
    assert all(bool((t == 7.0).all()) for t in dw + db), "a refused call wrote nothing"


# ---- 6. siren.apply --------------------------------------------------------------------------------------
def test_apply_is_eval_forward_and_vjp_backward(gpu):
    net = _cuda_net(2, 128, 2).requires_grad_(True)
    x = torch.from_numpy(sm.points(2, 130)).cuda()
    g = [torch.from_numpy(a).cuda() for a in vm.cotangents(130, 2, 2)]
    outs = siren.apply(net, x, value=True, jacobian=True, divergence=True)
    for a, b in zip(outs, siren.eval(net, x, value=True, jacobian=True, divergence=True)):
        assert a.requires_grad and np.array_equal(bits(a), bits(b))
    lin = [m for m in net.net if isinstance(m, torch.nn.Linear)]
    params = [m.weight for m in lin] + [m.bias for m in lin]
    loss = (g[0] * outs[0]).sum() + (g[1] * outs[1]).sum() + (g[2] * outs[2]).sum()
    got = torch.autograd.grad(loss, params, retain_graph=True)
    want = siren.vjp(net, x, grad_value=g[0], grad_jacobian=g[1], grad_divergence=g[2])
    assert same_bits(host((list(got[:4]), list(got[4:]))), host(want))
    # one output of three used: the others' cotangents are absent
    got = torch.autograd.grad((g[2] * outs[2]).sum(), params, retain_graph=True)
    assert same_bits(host((list(got[:4]), list(got[4:]))), host(siren.vjp(net, x, grad_divergence=g[2])))
    # a bare output, and a second-order request
    div = siren.apply(net, x, value=False, divergence=True)
    assert torch.is_tensor(div) and np.array_equal(bits(div), bits(outs[2]))
    first = torch.autograd.grad((g[2] * div).sum(), params, create_graph=True)
    with pytest.raises(RuntimeError, match="once_differentiable|differentiated twice|does not require grad"):
        torch.autograd.grad(sum((t * t).sum() for t in first), params)


# ---- 7. end to end -----------------------------------------------------------------------------------------
def _params(net):
    lin = [m for m in net.net if isinstance(m, torch.nn.Linear)]
    return [m.weight for m in lin] + [m.bias for m in lin]


@pytest.mark.parametrize("wrapped", [False, True], ids=["plain", "karman_wrap"])
def test_training_through_the_projection(gpu, wrapped):
    cfg = workloads.karman_config(n_walks=16, n_points=200)
    scene_cfg = dict(workloads.SCENE_BASE, boundary=workloads.KARMAN_OBJ)
    size = workloads.scene_size(workloads.KARMAN_OBJ)
    samples = torch.from_numpy(cfg["points"]).cuda()
    proj = pj.PressureProjector(scene_cfg, cfg["solver"], cfg["output"], samples, reuse_walks=True,
                                deterministic_backward=True)
    net = _cuda_net(2, 128, 2).requires_grad_(True)
    params = _params(net)
    grid = pj.sample_uniform_2d(24, size, with_boundary=True, device=samples.device)
    box = [grid[..., 0].min().item(), grid[..., 0].max().item(), grid[..., 1].min().item(), grid[..., 1].max().item()]
    wrap = sm.karman_wrap(box, eps=0.125, detach_weight=False) if wrapped else None
    rng = np.random.default_rng(11)
    cp = torch.from_numpy(rng.standard_normal(200).astype(np.float32)).cuda()
    cg = torch.from_numpy(rng.standard_normal((200, 2)).astype(np.float32)).cuda()

    def leg(source):
        for t in params:
            t.grad = None
        div = source()
        div.retain_grad()
        p, grad_p = proj.solve(div, differentiable=True)
        ((cp * p).sum() + (cg * grad_p).sum()).backward()
        # autograd leaves a parameter the loss does not reach (the output bias under a plain divergence) without a grad
        return div.detach(), div.grad.detach().clone(), [np.zeros(tuple(t.shape), np.float32) if t.grad is None
                                                         else t.grad.detach().cpu().numpy().copy() for t in params]

    fused = lambda: proj.source_from_network(net, 24, size, wrap=wrap, differentiable=True)  # noqa: E731
    velocity = (lambda x: wrap(x, net(x))) if wrapped else net
    div_a, gdiv_a, grads_a = leg(fused)
    div_b, gdiv_b, grads_b = leg(lambda: proj.source_from_velocity(velocity, 24, size, create_graph=True))
    assert np.array_equal(bits(div_a), bits(proj.source_from_network(net, 24, size, wrap=wrap))), "the same bits as today"
    assert div_a.shape == div_b.shape
    # the loss is linear in p and grad_p: the tape hands both legs the same cotangent of div
    assert np.array_equal(bits(gdiv_a), bits(gdiv_b))
    # float64: the autograd divergence of the (wrapped) network on the grid, seeded with that cotangent
    net64 = vm.net64(net).requires_grad_(True)
    g64 = grid.detach().cpu().double().requires_grad_(True)
    u64 = net64(g64)
    src64 = -pj.divergence(wrap(g64, u64) if wrapped else u64, g64, create_graph=True)[..., 0]
    ref = torch.autograd.grad((gdiv_a.cpu().double() * src64).sum(), _params(net64), allow_unused=True)
    ref = [np.zeros(tuple(t.shape)) if r is None else r.numpy() for r, t in zip(ref, _params(net64))]
    nl = len(params) // 2
    for k, (a, b, r) in enumerate(zip(grads_a, grads_b, ref)):
        name = f"d{'w' if k < nl else 'b'}[{k % nl}]"
        if not np.any(r):
            assert not np.any(a), f"{name}: must be exactly zero"
            continue
        sm.assert_as_accurate_as_torch(a, b, r, f"end to end ({'wrap' if wrapped else 'plain'}) {name}")
    # a second backward: the same bits
    _, _, again = leg(fused)
    for a, b in zip(grads_a, again):
        assert np.array_equal(bits(a), bits(b))
