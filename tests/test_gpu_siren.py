"""Fused SIREN on the GPU (wos_siren_eval, csrc/wos_siren.hip): the hidden-layer product's lane
maps against exact integer data, bitwise invariance of a point's outputs, accuracy against a
float64 model with the existing float32 autograd path as the yardstick, the C ABI's pointer
and refusal rules, and PressureProjector.source_from_network on karman.

Measured on the MI355X (ratios of the fused kernel's error to the float32 autograd path's, RMS /
max, against float64; the caps are 2.5 / 4): see profiles/siren_accuracy.json."""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest
import torch

import siren_model as sm
from wos_amd import _lib, siren, workloads
from wos_amd import projection as pj

pytestmark = pytest.mark.gpu


def bits(a):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- 1. lane maps, exact -----------------------------------------------------------------------------
@pytest.mark.parametrize("n_points", [1, 31, 32, 33, 65])
@pytest.mark.parametrize("d_in", [2, 3])
@pytest.mark.parametrize("H", [32, 64, 96, 128, 160, 192, 224, 256])
def test_hidden_layer_lane_maps_exact(gpu, H, d_in, n_points):
    """Integers in [-4, 4]: every sum is at most 256 * 16 + 4 = 4100 in magnitude, exact in f32, so
    a dropped or doubled k, a swapped row and column or a tangent in the wrong column all show."""
    i, k = np.meshgrid(np.arange(H), np.arange(H), indexing="ij")
    W = ((3 * i + 5 * k) % 9 - 4).astype(np.int64)
    b = ((7 * np.arange(H) + 2) % 9 - 4).astype(np.int64)
    p, s, h = np.meshgrid(np.arange(n_points), np.arange(1 + d_in), np.arange(H), indexing="ij")
    X = ((5 * p + 11 * s + 7 * h + (p * h) % 3 + (s * h) % 5) % 9 - 4).astype(np.int64)
    want = np.einsum("ik,psk->psi", W, X)
    want[:, 0, :] += b
    assert np.abs(want).max() <= 4100 and not np.array_equal(W, W.T)
    Z = siren.selftest_layer(W, b, X, device=gpu)
    assert Z.shape == X.shape and Z.dtype == np.float32
    assert np.array_equal(Z.astype(np.int64), want) and np.array_equal(Z, want.astype(np.float32))


# ---- 2. invariance, bitwise --------------------------------------------------------------------------
def _cuda_net(d, H, L, d_out=None):
    import copy
    return copy.deepcopy(sm.make_net(d, H, L, d_out)).cuda()


def test_outputs_are_bitwise_invariant(gpu):
    net = _cuda_net(2, 128, 2)
    x = torch.from_numpy(sm.points(2, 130)).cuda()
    u, jac, div = siren.eval(net, x, value=True, jacobian=True, divergence=True)
    assert tuple(u.shape) == (130, 2) and tuple(jac.shape) == (130, 2, 2) and tuple(div.shape) == (130,)
    assert all(t.is_cuda and t.dtype == torch.float32 and not t.requires_grad for t in (u, jac, div))
    full = [bits(t) for t in (u, jac, div)]
    for m in (1, 63, 64, 65):
        part = siren.eval(net, x[:m], value=True, jacobian=True, divergence=True)
        for a, b in zip(part, full):
            assert np.array_equal(bits(a), b[:m]), f"rows [0:{m}]"
    rev = siren.eval(net, x.flip(0), value=True, jacobian=True, divergence=True)
    for a, b in zip(rev, full):
        assert np.array_equal(bits(a), b[::-1]), "reversed order"
    again = siren.eval(net, x, value=True, jacobian=True, divergence=True)
    for a, b in zip(again, full):
        assert np.array_equal(bits(a), b), "second run"
    assert np.array_equal(bits(siren.eval(net, x)), full[0]), "u alone"
    assert np.array_equal(bits(siren.eval(net, x, value=False, jacobian=True)), full[1]), "jac alone"
    assert np.array_equal(bits(siren.eval(net, x, value=False, divergence=True)), full[2]), "div alone"
    assert np.array_equal(bits(jac[:, 0, 0] + jac[:, 1, 1]), full[2]), "div = J00 + J11 in f32"
    # numpy in, numpy out: the staged path computes the same bits
    host = siren.eval(net, x.cpu().numpy(), value=True, jacobian=True, divergence=True)
    for a, b in zip(host, full):
        assert isinstance(a, np.ndarray) and np.array_equal(bits(a), b), "host pointers"


def test_divergence_is_the_ordered_trace_in_3d(gpu):
    net = _cuda_net(3, 64, 1)
    x = torch.from_numpy(sm.points(3, 70)).cuda()
    jac, div = siren.eval(net, x, value=False, jacobian=True, divergence=True)
    assert np.array_equal(bits((jac[:, 0, 0] + jac[:, 1, 1]) + jac[:, 2, 2]), bits(div))
    # a grid-shaped batch keeps its leading shape
    u = siren.eval(net, x[:60].reshape(3, 4, 5, 3))
    assert tuple(u.shape) == (3, 4, 5, 3) and np.array_equal(bits(u).reshape(60, 3), bits(siren.eval(net, x[:60])))


# ---- 3. accuracy -------------------------------------------------------------------------------------
SHAPES = [(2, 32, 1, None), (2, 128, 2, None), (2, 256, 3, None), (3, 256, 3, None), (3, 96, 2, None), (2, 64, 0, None),
          # H / 32 = 5, 6, 7: two row tiles per wave, some waves' second one a dropped duplicate
          (2, 160, 1, None), (3, 192, 2, None), (2, 224, 3, None),
          # the reference's depth, and L = 8 at the smallest and the largest width
          (2, 256, 5, None), (3, 32, 8, None), (3, 256, 8, None),
          # d_out != d_in: value and Jacobian only
          (2, 64, 1, 3), (3, 64, 1, 2), (2, 64, 1, 1)]


def _id(d, H, L, d_out):
    return f"d{d}_H{H}_L{L}" + ("" if d_out is None else f"_o{d_out}")


@functools.lru_cache(maxsize=None)
def _reference(d, H, L, d_out=None):
    """(x, float64 model, float32 autograd path on the GPU) of one shape, computed once; div is None
    where d_out != d_in."""
    net, x = sm.make_net(d, H, L, d_out), sm.points(d, 193, seed=0)
    ref = sm.model64(net, x)
    t32 = tuple(None if t is None else t.cpu().numpy()
                for t in sm.autograd_eval(_cuda_net(d, H, L, d_out), torch.from_numpy(x).cuda()))
    return x, ref, t32


@pytest.mark.parametrize("d,H,L,d_out", SHAPES, ids=[_id(*s) for s in SHAPES])
def test_as_accurate_as_the_float32_autograd_path(gpu, d, H, L, d_out):
    x, ref, t32 = _reference(d, H, L, d_out)
    square = d_out is None
    got = siren.eval(_cuda_net(d, H, L, d_out), torch.from_numpy(x).cuda(), value=True, jacobian=True, divergence=square)
    names = ("u", "J", "div") if square else ("u", "J")
    assert len(got) == len(names) and tuple(got[0].shape) == (193, d_out or d) and tuple(got[1].shape) == (193, d_out or d, d)
    what = f"({d},{H},{L})" if square else f"({d},{H},{L},{d_out})"
    rec = {}
    for name, g, t, r in zip(names, got, t32, ref):
        rec[name] = sm.error_ratios(g.cpu().numpy(), t, r)
    out = os.environ.get("WOS_SIREN_ACCURACY_OUT")  # a measuring run keeps the figures; the suite writes nothing
    if out:
        with open(out, "a") as f:
            f.write(json.dumps({"d": d, "hidden": H, "hidden_layers": L, **({} if square else {"d_out": d_out}), "points": 193,
                                **{k: {"rms_ratio": v[0], "max_ratio": v[1], "torch_rms": v[2], "torch_max": v[3]}
                                   for k, v in rec.items()}}) + "\n")
    for name, g, t, r in zip(names, got, t32, ref):
        sm.assert_as_accurate_as_torch(g.cpu().numpy(), t, r, f"{what} {name}")


@pytest.mark.parametrize("d,H,L", [(2, 160, 1), (3, 224, 1)], ids=["d2_H160_L1", "d3_H224_L1"])
def test_value_only_call_equals_the_full_call_bit_for_bit(gpu, d, H, L):
    """The value-only kernel (one column per point) with two row tiles per wave and a dropped
    duplicate: H / 32 = 5 and 7.  The same chains as the full call, so the same bits."""
    net = _cuda_net(d, H, L)
    x = torch.from_numpy(sm.points(d, 193, seed=0)).cuda()
    full = siren.eval(net, x, value=True, jacobian=True, divergence=True)[0]
    only = siren.eval(net, x, value=True, jacobian=False, divergence=False)
    assert torch.is_tensor(only) and tuple(only.shape) == (193, d)
    assert bool(torch.isfinite(only).all()) and bool(only.any())
    assert np.array_equal(bits(only), bits(full))
    # and that value is the network's: against float64, with torch's float32 forward as the yardstick
    u64 = sm.model64(sm.make_net(d, H, L), x.cpu().numpy())[0]
    with torch.no_grad():
        u32 = net(x).cpu().numpy()
    sm.assert_as_accurate_as_torch(only.cpu().numpy(), u32, u64, f"({d},{H},{L}) value only")


# ---- 4. C ABI ------------------------------------------------------------------------------------------
def _c_net(p, tensors_or_arrays_w, tensors_or_arrays_b, ptr):
    n = p.n_hidden_layers + 2
    w = (C.c_void_p * n)(*[ptr(t) for t in tensors_or_arrays_w])
    b = (C.c_void_p * n)(*[ptr(t) for t in tensors_or_arrays_b])
    return _lib.SirenNet(p.d_in, p.d_out, p.hidden, p.n_hidden_layers, p.omega, w, b)


def test_c_abi_pointers_and_refusals(gpu):
    L = _lib.load()
    net = _cuda_net(2, 64, 1)
    p = siren.pack(net)
    n = 45
    x = sm.points(2, n)
    xd = torch.from_numpy(x).cuda()
    want = [bits(t) for t in siren.eval(net, xd, value=True, jacobian=True, divergence=True)]
    shapes = [(n, 2), (n, 2, 2), (n,)]
    # host pointers, blocking: weights, points and outputs all on the host
    hw, hb = [t.cpu().numpy() for t in p.weights], [t.cpu().numpy() for t in p.biases]
    hnet = _c_net(p, hw, hb, lambda a: a.ctypes.data)
    for drop in (None, 0, 1, 2):  # all three, then each output NULL in turn
        outs = [None if k == drop else np.full(s, np.nan, np.float32) for k, s in enumerate(shapes)]
        rc = L.wos_siren_eval(C.byref(hnet), x.ctypes.data, n, *[None if a is None else a.ctypes.data for a in outs],
                              0, gpu, None)
        assert rc == 0, L.wos_last_error()
        for a, b in zip(outs, want):
            assert a is None or np.array_equal(bits(a), b), f"host pointers, output {drop} null"
    # device pointers, WOS_ASYNC on a side stream
    dnet = _c_net(p, p.weights, p.biases, lambda t: t.data_ptr())
    side = torch.cuda.Stream()
    outs = [torch.full(s, float("nan"), device="cuda") for s in shapes]
    torch.cuda.synchronize()
    rc = L.wos_siren_eval(C.byref(dnet), xd.data_ptr(), n, *[t.data_ptr() for t in outs],
                          _lib.WOS_PTRS_DEVICE | _lib.WOS_ASYNC, gpu, side.cuda_stream)
    assert rc == 0, L.wos_last_error()
    side.synchronize()
    for a, b in zip(outs, want):
        assert np.array_equal(bits(a), b), "device pointers, async"
    # refusals
    o = outs[0].data_ptr()
    flags = _lib.WOS_PTRS_DEVICE
    assert L.wos_siren_eval(C.byref(dnet), xd.data_ptr(), n, None, None, None, flags, gpu, None) == -1
    assert b"no output requested" in L.wos_last_error()
    assert L.wos_siren_eval(C.byref(dnet), xd.data_ptr(), 0, o, None, None, flags, gpu, None) == 0  # n = 0
    assert L.wos_siren_eval(C.byref(dnet), None, 0, o, None, None, flags, gpu, None) == 0
    assert L.wos_siren_eval(C.byref(dnet), xd.data_ptr(), -1, o, None, None, flags, gpu, None) == -1
    bad = _c_net(p, p.weights, p.biases, lambda t: t.data_ptr())
    bad.hidden = 100
    assert L.wos_siren_eval(C.byref(bad), xd.data_ptr(), n, o, None, None, flags, gpu, None) == -1
    assert b"hidden" in L.wos_last_error() and b"100" in L.wos_last_error()
    bad.hidden, bad.d_out = 64, 1
    assert L.wos_siren_eval(C.byref(bad), xd.data_ptr(), n, None, None, outs[2].data_ptr(), flags, gpu, None) == -1
    assert b"div needs d_out == d_in" in L.wos_last_error()
    for field, value in (("d_in", 4), ("d_out", 0), ("n_hidden_layers", 9), ("omega", float("inf"))):
        bad = _c_net(p, p.weights, p.biases, lambda t: t.data_ptr())
        setattr(bad, field, value)
        assert L.wos_siren_eval(C.byref(bad), xd.data_ptr(), n, o, None, None, flags, gpu, None) == -1
        assert field.encode() in L.wos_last_error(), field
    torch.cuda.synchronize()
    for a, b in zip(outs, want):  # a refused call wrote nothing
        assert np.array_equal(bits(a), b)
    # the python layer: a non-square net gives u and J, and refuses div
    net31 = _cuda_net(3, 32, 1, d_out=1)
    x3 = torch.from_numpy(sm.points(3, 40)).cuda()
    u, jac = siren.eval(net31, x3, jacobian=True)
    ref = sm.model64(sm.make_net(3, 32, 1, d_out=1), x3.cpu().numpy())
    assert tuple(u.shape) == (40, 1) and tuple(jac.shape) == (40, 1, 3)
    assert np.abs(u.cpu().numpy() - ref[0]).max() < 1e-5 and np.abs(jac.cpu().numpy() - ref[1]).max() < 1e-4


def test_no_hidden_layer_host_pointers_equal_device_pointers(gpu):
    """L = 0: no packed weights, so the device-pointer call allocates nothing and the host-pointer call only its staging."""
    net = _cuda_net(2, 32, 0)
    x = sm.points(2, 33)  # one full tile and one point
    dev = siren.eval(net, torch.from_numpy(x).cuda(), value=True, jacobian=True, divergence=True)
    host = siren.eval(net, x, value=True, jacobian=True, divergence=True)
    for what, a, b in zip(("u", "J", "div"), host, dev):  # (accuracy at L = 0: SHAPES above)
        assert isinstance(a, np.ndarray) and np.array_equal(bits(a), bits(b)), what
        assert np.isfinite(a).all() and np.abs(a).max() > 0, what


# ---- 5. projector --------------------------------------------------------------------------------------
def test_projector_source_from_network(gpu):
    cfg = workloads.karman_config(n_walks=16, n_points=200)
    scene_cfg = dict(workloads.SCENE_BASE, boundary=workloads.KARMAN_OBJ)
    size = workloads.scene_size(workloads.KARMAN_OBJ)
    samples = torch.from_numpy(cfg["points"]).cuda()
    proj = pj.PressureProjector(scene_cfg, cfg["solver"], cfg["output"], samples)
    net = _cuda_net(2, 128, 2)
    old = proj.source_from_velocity(net, 24, size)
    new = proj.source_from_network(net, 24, size)
    assert new.shape == old.shape and new.dtype == old.dtype == torch.float32 and new.device == old.device
    assert new.is_contiguous() and not new.requires_grad
    grid = pj.sample_uniform_2d(24, size, with_boundary=True, device=samples.device)
    assert tuple(new.shape) == tuple(grid.shape[:-1])
    assert np.array_equal(bits(new), bits(-siren.eval(net, grid, value=False, divergence=True)))
    # against float64, with the old path as the yardstick -- plain, and through the karman-like wrap
    net64 = __import__("copy").deepcopy(sm.make_net(2, 128, 2)).double()
    g64 = grid.detach().cpu().double().requires_grad_(True)
    ref = -pj.divergence(net64(g64), g64)[..., 0].detach().numpy()
    sm.assert_as_accurate_as_torch(new.cpu().numpy(), old.cpu().numpy(), ref, "source_from_network")
    # the wrap's box is the grid's own extent: float32 numbers, so the float32 and float64 evaluations
    # of its masks and of |y - wall| agree on the boundary rows and the strip's first column
    box = [grid[..., 0].min().item(), grid[..., 0].max().item(), grid[..., 1].min().item(), grid[..., 1].max().item()]
    for detach in (True, False):
        wrap = sm.karman_wrap(box, eps=0.125, detach_weight=detach)
        old_w = proj.source_from_velocity(lambda x: wrap(x, net(x)), 24, size)
        new_w = proj.source_from_network(net, 24, size, wrap=wrap)
        assert new_w.shape == old_w.shape and new_w.dtype == old_w.dtype and new_w.is_contiguous()
        g64 = grid.detach().cpu().double().requires_grad_(True)
        ref_w = -pj.divergence(wrap(g64, net64(g64)), g64)[..., 0].detach().numpy()
        assert np.abs(ref_w - ref).max() > 1e-3 * np.abs(ref).max(), "the wrap must act on this grid"
        sm.assert_as_accurate_as_torch(new_w.cpu().numpy(), old_w.cpu().numpy(), ref_w,
                                       f"source_from_network, wrap (detach_weight={detach})")
    p, grad_p = proj.solve(new)
    assert tuple(p.shape) == (200,) and tuple(grad_p.shape) == (200, 2)
    assert torch.isfinite(p).all() and torch.isfinite(grad_p).all()
