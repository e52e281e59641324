"""The device-resident advection fit without a GPU (include/wos.h "Device-resident fit loop over
ragged batches"; wos_amd.siren.fit_run_batches, wos_amd.projection.fit_advection):
wos_siren_fit_run_batches is declared, exported and bound within ABI 10; it names what it refuses
before any device work and writes nothing; the two Python functions name what they refuse; and
fit_advection hands siren.fit_run_batches, per iteration, exactly the points, targets, scales and
counts that calls of advection_fit_loss on a generator seeded alike hand siren.fit_loss."""
import ctypes as C
import os
import re
import subprocess
import types

import numpy as np
import pytest
import torch

import siren_model as sm
import wos_amd
from wos_amd import _lib, siren
from wos_amd import projection as pj

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "wos.h")

ARGS = ["net", "pts", "target", "scale", "offsets", "n_iters", "exp_avg", "exp_avg_sq", "step0", "opt", "stop_loss",
        "check_every", "losses", "status", "workspace_bytes", "flags", "device", "stream"]


# ---- ABI ---------------------------------------------------------------------------------------------
def test_entry_point_declared_exported_and_bound():
    name = "wos_siren_fit_run_batches"
    raw = open(HEADER).read()
    txt = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", txt, flags=re.S)
    assert m, f"{name} is not declared"
    args = [a.strip() for a in m.group(1).split(",")]
    assert [re.search(r"(\w+)$", a).group(1) for a in args] == ARGS
    assert re.search(r"const\s+int64_t\s*\*\s*offsets", m.group(1)), "offsets is an array of int64_t"
    L = wos_amd.load_library()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r"\bT (wos_[a-z0-9_]+)$", out, flags=re.M))
    assert name in exported and name in _lib.EXPORTS and hasattr(L, name)
    assert len(getattr(L, name).argtypes) == len(ARGS)
    assert L.wos_abi_version() == _lib.ABI_VERSION == 10, "an addition within ABI 10"
    assert re.search(r"#define WOS_ABI_VERSION 10\b", raw)
    assert "offsets is a HOST array of n_iters + 1 row offsets" in re.sub(r"\s*\n \*\s*", " ", raw), "the header says so"


# ---- refusals that need no device --------------------------------------------------------------------
def _opt(**over):
    f = dict(lr=1e-4, beta1=0.9, beta2=0.999, eps=1e-8, max_grad_norm=-1.0)
    f.update(over)
    return _lib.AdamParams(f["lr"], f["beta1"], f["beta2"], f["eps"], f["max_grad_norm"])


def _call(**over):
    """wos_siren_fit_run_batches on host memory passed as device pointers: every refusal comes before
    any device work.  Returns (rc, message, nothing was written)."""
    net = sm.make_net(2, 64, 1)
    p = siren.pack(net)
    ws, bs = [t.numpy() for t in p.weights], [t.numpy() for t in p.biases]
    total = sum(a.size for a in ws + bs)
    k = {"x": sm.points(2, 9), "t": np.zeros((9, 2), np.float32), "m": np.zeros(total, np.float32),
         "v": np.zeros(total, np.float32), "losses": np.full(2, 7.0, np.float32), "status": np.full(2, 7, np.int64)}
    w = (C.c_void_p * 3)(*[a.ctypes.data for a in ws])
    b = (C.c_void_p * 3)(*[a.ctypes.data for a in bs])
    net_c = _lib.SirenNet(p.d_in, p.d_out, p.hidden, p.n_hidden_layers, p.omega, w, b)
    for field, value in over.pop("net_fields", {}).items():
        setattr(net_c, field, value)
    a = dict(pts=k["x"].ctypes.data, target=k["t"].ctypes.data, scale=None, offsets=(0, 4, 9), n_iters=2,
             m=k["m"].ctypes.data, v=k["v"].ctypes.data, step0=0, opt=_opt(), stop_loss=-1.0, check_every=0,
             losses=k["losses"].ctypes.data, status=k["status"].ctypes.data, ws=0, flags=_lib.WOS_PTRS_DEVICE)
    a.update(over)
    offsets = None if a["offsets"] is None else (C.c_int64 * len(a["offsets"]))(*a["offsets"])
    before = [x.copy() for x in ws + bs]
    L = _lib.load()
    rc = L.wos_siren_fit_run_batches(C.byref(net_c), a["pts"], a["target"], a["scale"], offsets, a["n_iters"], a["m"], a["v"],
                                     a["step0"], None if a["opt"] is None else C.byref(a["opt"]), a["stop_loss"],
                                     a["check_every"], a["losses"], a["status"], a["ws"], a["flags"], 0, None)
    unchanged = (np.all(k["losses"] == 7.0) and np.all(k["status"] == 7) and not k["m"].any() and not k["v"].any()
                 and all(np.array_equal(x, y) for x, y in zip(before, ws + bs)))
    return rc, L.wos_last_error(), unchanged


def test_refusals_name_the_field_before_any_device_work():
    cases = [({"pts": None}, b"null pts"), ({"target": None}, b"null target"), ({"offsets": None}, b"null offsets"),
             ({"losses": None}, b"null losses"), ({"status": None}, b"null status"), ({"m": None}, b"null exp_avg"),
             ({"v": None}, b"null exp_avg_sq"), ({"opt": None}, b"null opt"),
             ({"n_iters": 0}, b"n_iters"), ({"n_iters": -2}, b"n_iters"),
             ({"offsets": (-1, 4, 9)}, b"offsets[0]"),
             ({"offsets": (0, 0, 9)}, b"iteration 0"), ({"offsets": (3, 9, 9)}, b"iteration 1"),
             ({"offsets": (0, 5, 4)}, b"iteration 1"), ({"offsets": (5, 4, 9)}, b"iteration 0"),
             ({"flags": 0}, b"WOS_PTRS_DEVICE"), ({"flags": _lib.WOS_ASYNC}, b"WOS_PTRS_DEVICE"),
             ({"flags": _lib.WOS_PTRS_DEVICE | _lib.WOS_ASYNC, "check_every": 1}, b"check_every"),
             ({"check_every": -1}, b"check_every"),
             ({"stop_loss": float("nan")}, b"stop_loss"), ({"step0": -1}, b"step0"),
             ({"opt": _opt(lr=float("nan"))}, b"lr"), ({"opt": _opt(beta1=1.0)}, b"beta1"),
             ({"net_fields": {"d_in": 4}}, b"d_in"), ({"net_fields": {"hidden": 100}}, b"hidden")]
    for over, word in cases:
        rc, msg, unchanged = _call(**over)
        assert rc == -1 and msg.startswith(b"wos_siren_fit_run_batches") and word in msg, (over, msg)
        assert unchanged, "a refused call wrote nothing"
    for over in ({"offsets": (0, 0, 9)}, {"offsets": (0, 5, 4)}):
        assert b"offsets" in _call(**over)[1]


def test_a_workspace_below_one_tile_is_a_capacity_error():
    tile = (2 * 1 + 1) * 64 * 4 * 32
    rc, msg, unchanged = _call(ws=tile - 1)
    assert rc == _lib.WOS_E_CAPACITY and msg.startswith(b"wos_siren_fit_run_batches")
    assert b"workspace_bytes" in msg and b"cannot hold one tile" in msg and unchanged


def test_python_layer_names_what_it_refuses():
    net = sm.make_net(2, 32, 1)
    state = siren.AdamState(net)
    x = torch.from_numpy(sm.points(2, 9))
    t = torch.zeros((9, 2))
    with pytest.raises(ValueError, match=r"counts sum to 8, the tensors hold 9 rows"):
        siren.fit_run_batches(net, state, x, t, None, [3, 5])
    with pytest.raises(ValueError, match=r"counts sum to 10"):
        siren.fit_run_batches(net, state, x, t, None, [4, 6])
    with pytest.raises(ValueError, match=r"counts\[1\] must be a positive int"):
        siren.fit_run_batches(net, state, x, t, None, [9, 0])
    with pytest.raises(ValueError, match=r"counts\[0\] must be a positive int"):
        siren.fit_run_batches(net, state, x, t, None, [-1, 10])
    with pytest.raises(ValueError, match="counts is empty"):
        siren.fit_run_batches(net, state, x, t, None, [])
    with pytest.raises(ValueError, match=r"x must be \[total, 2\]"):
        siren.fit_run_batches(net, state, x.reshape(-1), t, None, [9])
    with pytest.raises(ValueError, match="x must be a CUDA tensor"):
        siren.fit_run_batches(net, state, x, t, None, [4, 5])
    assert state.step == 0
    size = [0.0, 2.2, 0.0, 1.0]
    with pytest.raises(ValueError, match="exactly one of n_samples"):
        pj.fit_advection(net, net, 0.05, size, 3)
    with pytest.raises(ValueError, match="exactly one of n_samples"):
        pj.fit_advection(net, net, 0.05, size, 3, n_samples=8, samples=lambda k: torch.zeros(k, 8, 2))
    for bad in (dict(n_iters=0), dict(n_iters=-1), dict(n_iters=3, iters_per_call=0), dict(n_iters=3, iters_per_call=-4)):
        with pytest.raises(ValueError, match="n_iters and iters_per_call must be positive"):
            pj.fit_advection(net, net, 0.05, size, bad.pop("n_iters"), n_samples=8, **bad)
    with pytest.raises(ValueError, match="n_samples must be positive"):
        pj.fit_advection(net, net, 0.05, size, 3, n_samples=0)
    with pytest.raises(ValueError, match="size must hold 4 bounds"):
        pj.fit_advection(net, net, 0.05, size + [0.0, 1.0], 3, n_samples=8)


# ---- fit_advection hands over what advection_fit_loss hands over -------------------------------------
SIZES = {2: [0.0, 2.2, 0.0, 1.0], 3: [0.0, 1.0, -0.5, 0.5, 0.25, 1.5]}


def _fake_eval(net, x, **kw):
    """A pointwise stand-in for siren.eval, computed in float64: large enough that backtracking leaves the box."""
    xd = x.to(torch.float64)
    return (net.gain * torch.sin(3.0 * xd + net.phase) + 0.25 * net.gain).to(x.dtype)


def _draw(n, d, size, gen):
    """sample_random_2D (src/2d/utils/model_utils.py:22-31; 3D: src/3d/utils/model_utils.py:31-40)."""
    x = torch.rand(n, d, generator=gen)
    for c in range(d):
        x[..., c] = x[..., c] * (size[2 * c + 1] - size[2 * c]) + size[2 * c]
    return x


@pytest.mark.parametrize("with_keep", [False, True], ids=["all", "keep"])
@pytest.mark.parametrize("wrapped", [False, True], ids=["plain", "karman_wrap"])
@pytest.mark.parametrize("tilde", [False, True], ids=["prev", "prev_tilde"])
@pytest.mark.parametrize("dim", [2, 3])
def test_fit_advection_hands_over_what_advection_fit_loss_does(monkeypatch, dim, tilde, wrapped, with_keep):
    n, K, dt, size = 37, 5, 0.3, SIZES[dim]
    net = sm.make_net(dim, 32, 1)
    prev = types.SimpleNamespace(gain=1.5, phase=0.3)
    til = types.SimpleNamespace(gain=-0.75, phase=1.1) if tilde else None
    wrap = sm.karman_wrap(size, eps=0.125) if wrapped else None
    centre = torch.tensor([0.5 * (size[2 * c] + size[2 * c + 1]) for c in range(dim)])
    keep = (lambda x: ((x - centre) ** 2).sum(-1) > 0.3 ** 2) if with_keep else None
    want, got = [], []

    def fake_fit_loss(module, x, target, scale=None):
        want.append((x.clone(), target.clone(), None if scale is None else scale.clone()))
        return torch.zeros(())

    def fake_fit_run_batches(net_, state, x, target, scale, counts, *, stop_loss=None, **kw):
        assert net_ is net and stop_loss is None and sum(counts) == x.shape[0] == target.shape[0]
        got.append({"step": state.step, "counts": list(counts)})
        at = 0
        for c in counts:
            got[-1].setdefault("rows", []).append((x[at:at + c].clone(), target[at:at + c].clone(),
                                                   None if scale is None else scale[at:at + c].clone()))
            at += c
        state.step += len(counts)
        return torch.arange(len(counts), dtype=torch.float32), torch.tensor([len(counts), 0])
    monkeypatch.setattr(siren, "eval", _fake_eval)
    monkeypatch.setattr(siren, "fit_loss", fake_fit_loss)
    monkeypatch.setattr(siren, "fit_run_batches", fake_fit_run_batches)
    g1 = torch.Generator().manual_seed(321)
    clamped = free = 0
    for _ in range(K):
        x = _draw(n, dim, size, g1)
        if keep is not None:
            x = x[keep(x)]
        pj.advection_fit_loss(net, prev, x, dt, size, network_tilde=til, wrap=wrap)
        u = _fake_eval(prev, x)
        back = x - (u if wrap is None else wrap(x, u)) * dt
        lo, hi = torch.tensor(size[0::2]), torch.tensor(size[1::2])
        out = (back < lo) | (back > hi)
        clamped, free = clamped + int(out.sum()), free + int((~out).sum())
    assert clamped > 0 and free > 0, "the case: some backtracked coordinates are clamped, some are not"
    counts = [w[0].shape[0] for w in want]
    assert len(want) == K and (len(set(counts)) > 1) == with_keep and all(c > 0 for c in counts)
    assert all((w[2] is None) == (wrap is None) for w in want)
    for per_call in (1, 2, 8):  # one at a time, not dividing, larger than n_iters
        got.clear()
        g2 = torch.Generator().manual_seed(321)
        losses, state = pj.fit_advection(net, prev, dt, size, K, n_samples=n, network_tilde=til, wrap=wrap, keep=keep,
                                         generator=g2, iters_per_call=per_call)
        assert torch.equal(g1.get_state(), g2.get_state()), "the same generator consumption"
        assert len(got) == -(-K // per_call) and [c["step"] for c in got] == list(range(0, K, per_call))
        assert losses.shape == (K,) and state.step == K and isinstance(state, siren.AdamState)
        assert [c for call in got for c in call["counts"]] == counts
        rows = [r for call in got for r in call["rows"]]
        for i, (w, r) in enumerate(zip(want, rows)):
            for what, a, b in zip(("points", "target", "scale"), w, r):
                assert (a is None) == (b is None), f"iteration {i}: {what}"
                assert a is None or (a.dtype == b.dtype and torch.equal(a, b)), f"iteration {i}: {what} differs"
    # samples= : the callable's block is used as it comes
    fixed = torch.stack([_draw(n, dim, size, torch.Generator().manual_seed(9 + i)) for i in range(K)])
    served = []

    def samples(k):
        served.append(k)
        first = sum(served[:-1])
        return fixed[first:first + k]
    got.clear()
    pj.fit_advection(net, prev, dt, size, K, samples=samples, network_tilde=til, wrap=wrap, iters_per_call=2)
    assert served == [2, 2, 1] and [c for call in got for c in call["counts"]] == [n] * K
    assert torch.equal(torch.cat([r[0] for call in got for r in call["rows"]]), fixed.reshape(-1, dim))


def test_fit_advection_refuses_an_iteration_without_points_before_its_block(monkeypatch):
    n, size = 16, SIZES[2]
    net = sm.make_net(2, 32, 1)
    prev = types.SimpleNamespace(gain=0.5, phase=0.0)
    blocks = []

    def fake_fit_run_batches(net_, state, x, target, scale, counts, **kw):
        blocks.append(list(counts))
        state.step += len(counts)
        return torch.zeros(len(counts)), torch.tensor([len(counts), 0])
    monkeypatch.setattr(siren, "eval", _fake_eval)
    monkeypatch.setattr(siren, "fit_run_batches", fake_fit_run_batches)
    seen = []

    def keep(x):  # the second block's second iteration, iteration 3, loses every point
        seen.append(x.shape[0])
        mask = torch.ones(x.shape[0], dtype=torch.bool)
        if len(seen) == 2:
            mask[n:] = False
        return mask
    state = siren.AdamState(net)
    with pytest.raises(ValueError, match=r"iteration 3 without a point"):
        pj.fit_advection(net, prev, 0.1, size, 6, n_samples=n, keep=keep, state=state, iters_per_call=2,
                         generator=torch.Generator().manual_seed(1))
    assert blocks == [[n, n]] and state.step == 2 and seen == [2 * n, 2 * n]
