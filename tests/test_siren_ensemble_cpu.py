"""The ensemble fit loops without a GPU (include/wos.h "Ensemble fit loops"; wos_amd.siren
fit_run_ensemble / fit_run_batches_ensemble, wos_amd.projection fit_projection_ensemble /
fit_advection_ensemble): the two entry points are declared, exported and bound within ABI 10; they
name the field and the member of what they refuse, before any device work, and write nothing; and
the two projection functions hand each member exactly the points, targets, scales, indices and counts
that the single-network functions hand over for that member with a generator seeded alike."""
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

TAIL = ["exp_avg", "exp_avg_sq", "step0", "opt", "stop_loss", "check_every", "losses", "status", "workspace_bytes", "flags",
        "device", "stream"]
ARGS = {"wos_siren_fit_run_ensemble": ["n_members", "nets", "pool_pts", "pool_target", "pool_scale", "n_pool", "idx",
                                       "n_iters", "batch"] + TAIL,
        "wos_siren_fit_run_batches_ensemble": ["n_members", "nets", "pts", "target", "scale", "offsets", "n_iters"] + TAIL}


# ---- ABI ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(ARGS))
def test_entry_points_declared_exported_and_bound(name):
    raw = open(HEADER).read()
    txt = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", txt, flags=re.S)
    assert m, f"{name} is not declared"
    args = [a.strip() for a in m.group(1).split(",")]
    assert [re.search(r"(\w+)$", a).group(1) for a in args] == ARGS[name]
    target = "pool_target" if "pool_target" in ARGS[name] else "target"
    assert re.search(r"const\s+float\s*\*\s*const\s*\*\s*" + target + r"\b", m.group(1)), "an array of pointers per member"
    assert re.search(r"float\s*\*\s*const\s*\*\s*exp_avg\b", m.group(1))
    L = wos_amd.load_library()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r"\bT (wos_[a-z0-9_]+)$", out, flags=re.M))
    assert name in exported and name in _lib.EXPORTS and hasattr(L, name)
    assert len(getattr(L, name).argtypes) == len(ARGS[name])
    assert L.wos_abi_version() == _lib.ABI_VERSION == 10, "an addition within ABI 10"
    assert re.search(r"#define WOS_ABI_VERSION 10\b", raw)
    assert siren.MAX_MEMBERS == 4 and re.search(r"#define WOS_MAX_CHANNELS 4\b", raw)


# ---- refusals that need no device --------------------------------------------------------------------
def _opt(**over):
    f = dict(lr=1e-4, beta1=0.9, beta2=0.999, eps=1e-8, max_grad_norm=-1.0)
    f.update(over)
    return _lib.AdamParams(f["lr"], f["beta1"], f["beta2"], f["eps"], f["max_grad_norm"])


def _ptrs(values):
    return None if values is None else (C.c_void_p * max(1, len(values)))(*values)


def _call(form, E=3, edit=None, **over):
    """One of the two entry points on host memory passed as device pointers: every refusal comes before
    any device work.  edit(members) changes the members' structs and pointer lists in place.  Returns
    (rc, message, nothing was written)."""
    nets = [sm.make_net(2, 64, 1, seed=e) for e in range(E)]
    packed = [siren.pack(n) for n in nets]
    arrays = [[t.numpy() for t in p.weights + p.biases] for p in packed]
    total = sum(a.size for a in arrays[0]) if E else 0
    held = {"x": sm.points(2, 9), "idx": np.zeros((2, 4), np.int64), "losses": np.full((max(E, 1), 2), 7.0, np.float32),
            "status": np.full((max(E, 1), 2), 7, np.int64),
            "t": [np.zeros((9, 2), np.float32) for _ in range(E)], "s": [np.ones((9, 2), np.float32) for _ in range(E)],
            "m": [np.zeros(total, np.float32) for _ in range(E)], "v": [np.zeros(total, np.float32) for _ in range(E)]}
    mem = {"w": [[a.ctypes.data for a in arr[:3]] for arr in arrays], "b": [[a.ctypes.data for a in arr[3:]] for arr in arrays],
           "fields": [dict(d_in=p.d_in, d_out=p.d_out, hidden=p.hidden, n_hidden_layers=p.n_hidden_layers, omega=p.omega)
                      for p in packed],
           "target": [a.ctypes.data for a in held["t"]], "scale": [None, *[a.ctypes.data for a in held["s"][1:]]][:E],
           "m": [a.ctypes.data for a in held["m"]], "v": [a.ctypes.data for a in held["v"]]}
    a = dict(n_members=E, nets=True, pts=held["x"].ctypes.data, target=True, scale=True, offsets=(0, 4, 9), n_pool=9,
             idx=held["idx"].ctypes.data, n_iters=2, batch=4, m=True, v=True, step0=0, opt=_opt(), stop_loss=-1.0,
             check_every=0, losses=held["losses"].ctypes.data, status=held["status"].ctypes.data, ws=0,
             flags=_lib.WOS_PTRS_DEVICE)
    a.update(over)
    if edit:
        edit(mem)
    keep = [(_ptrs(w), _ptrs(b)) for w, b in zip(mem["w"], mem["b"])]
    structs = (_lib.SirenNet * max(E, 1))(*[
        _lib.SirenNet(f["d_in"], f["d_out"], f["hidden"], f["n_hidden_layers"], f["omega"], w, b)
        for f, (w, b) in zip(mem["fields"], keep)])
    arr = lambda key, name: _ptrs(mem[name]) if a[key] is True else a[key]  # noqa: E731
    offsets = None if a["offsets"] is None else (C.c_int64 * len(a["offsets"]))(*a["offsets"])
    tail = (arr("m", "m"), arr("v", "v"), a["step0"], None if a["opt"] is None else C.byref(a["opt"]), a["stop_loss"],
            a["check_every"], a["losses"], a["status"], a["ws"], a["flags"], 0, None)
    before = [[x.copy() for x in arr_] for arr_ in arrays]
    L = _lib.load()
    nets_arg = structs if a["nets"] is True else a["nets"]
    if form == "pool":
        rc = L.wos_siren_fit_run_ensemble(a["n_members"], nets_arg, a["pts"], arr("target", "target"), arr("scale", "scale"),
                                          a["n_pool"], a["idx"], a["n_iters"], a["batch"], *tail)
    else:
        rc = L.wos_siren_fit_run_batches_ensemble(a["n_members"], nets_arg, a["pts"], arr("target", "target"),
                                                  arr("scale", "scale"), offsets, a["n_iters"], *tail)
    unchanged = (np.all(held["losses"] == 7.0) and np.all(held["status"] == 7)
                 and not any(x.any() for x in held["m"] + held["v"])
                 and all(np.array_equal(x, y) for xs, ys in zip(before, arrays) for x, y in zip(xs, ys)))
    return rc, L.wos_last_error(), unchanged


FN = {"pool": b"wos_siren_fit_run_ensemble", "batches": b"wos_siren_fit_run_batches_ensemble"}


def _refused(form, words, **kw):
    rc, msg, unchanged = _call(form, **kw)
    assert rc == -1 and msg.startswith(FN[form] + b":"), (kw, rc, msg)
    for word in words:
        assert word in msg, (kw, msg)
    assert unchanged, "a refused call wrote nothing"


def _set(key, e, value, layer=None):
    def edit(mem):
        if layer is None:
            mem[key][e] = value(mem) if callable(value) else value
        else:
            mem[key][e][layer] = value(mem) if callable(value) else value
    return edit


def _field(e, name, value):
    def edit(mem):
        mem["fields"][e][name] = value
    return edit


@pytest.mark.parametrize("form", ["pool", "batches"])
def test_an_accepted_shape_reaches_the_device_checks_only(form):
    """The fixture itself is refused by nothing below: with a workspace under one tile it gets as far as
    the last refusal before the device, WOS_E_CAPACITY."""
    tile = (2 * 1 + 1) * 64 * 4 * 32
    for E in (1, 2, 3, 4):
        rc, msg, unchanged = _call(form, E=E, ws=tile - 1)
        assert rc == _lib.WOS_E_CAPACITY and msg.startswith(FN[form]) and b"cannot hold one tile" in msg and unchanged


@pytest.mark.parametrize("form", ["pool", "batches"])
def test_the_ensemble_refusals_name_the_field_and_the_member(form):
    for n in (0, -1, 5):
        _refused(form, [b"n_members must be 1..4"], n_members=n)
    _refused(form, [b"null nets"], nets=None)
    for name, value in (("d_in", 3), ("d_out", 1), ("hidden", 96), ("n_hidden_layers", 2), ("omega", 20.0)):
        grow = (lambda mem: [mem[k][2].append(mem[k][2][1]) for k in ("w", "b")]) if name == "n_hidden_layers" else None
        def edit(mem, name=name, value=value, grow=grow):
            mem["fields"][2][name] = value
            if grow:
                grow(mem)
        _refused(form, [b"member 2", name.encode(), b"member 0"], edit=edit)
    # each member's own envelope, by member
    _refused(form, [b"member 1", b"hidden must be a multiple of 32"], edit=_field(1, "hidden", 100))
    _refused(form, [b"member 2", b"omega must be finite"], edit=_field(2, "omega", float("inf")))
    _refused(form, [b"member 1", b"null weights or biases pointer of layer 2"], edit=_set("w", 1, None, layer=2))
    # two members training the same tensor, or keeping their moments in the same buffer
    _refused(form, [b"members 0 and 2 share", b"weights pointer"], edit=_set("w", 2, lambda mem: mem["w"][0][1], layer=1))
    _refused(form, [b"members 1 and 2 share", b"biases pointer"], edit=_set("b", 2, lambda mem: mem["b"][1][0], layer=0))
    _refused(form, [b"members 0 and 1 share", b"exp_avg buffer"], edit=_set("m", 1, lambda mem: mem["m"][0]))
    _refused(form, [b"members 1 and 2 share", b"exp_avg_sq buffer"], edit=_set("v", 2, lambda mem: mem["v"][1]))
    _refused(form, [b"members 0 and 2 share", b"moment buffer"], edit=_set("m", 2, lambda mem: mem["v"][0]))
    # NULL entries and NULL arrays
    target = b"pool_target" if form == "pool" else b"target"
    _refused(form, [b"null " + target + b" of member 1"], edit=_set("target", 1, None))
    _refused(form, [b"null " + target], target=None)
    _refused(form, [b"null exp_avg of member 2"], edit=_set("m", 2, None))
    _refused(form, [b"null exp_avg_sq of member 0"], edit=_set("v", 0, None))
    _refused(form, [b"null exp_avg"], m=None)
    _refused(form, [b"null exp_avg_sq"], v=None)


@pytest.mark.parametrize("form", ["pool", "batches"])
def test_every_refusal_of_the_single_network_entry_point(form):
    shared = [({"pts": None}, b"null p"), ({"losses": None}, b"null losses"), ({"status": None}, b"null status"),
              ({"opt": None}, b"null opt"), ({"n_iters": 0}, b"n_iters"), ({"n_iters": -2}, b"n_iters"),
              ({"flags": 0}, b"WOS_PTRS_DEVICE"), ({"flags": _lib.WOS_ASYNC}, b"WOS_PTRS_DEVICE"),
              ({"flags": _lib.WOS_PTRS_DEVICE | _lib.WOS_ASYNC, "check_every": 1}, b"check_every"),
              ({"check_every": -1}, b"check_every"), ({"stop_loss": float("nan")}, b"stop_loss"), ({"step0": -1}, b"step0"),
              ({"opt": _opt(lr=float("nan"))}, b"lr"), ({"opt": _opt(beta1=1.0)}, b"beta1"), ({"opt": _opt(beta2=-0.1)}, b"beta2"),
              ({"opt": _opt(eps=-1.0)}, b"eps")]
    own = {"pool": [({"idx": None}, b"null idx"), ({"batch": 0}, b"batch"), ({"n_pool": 0}, b"n_pool")],
           "batches": [({"offsets": None}, b"null offsets"), ({"offsets": (-1, 4, 9)}, b"offsets[0]"),
                       ({"offsets": (0, 0, 9)}, b"iteration 0"), ({"offsets": (3, 9, 9)}, b"iteration 1"),
                       ({"offsets": (0, 5, 4)}, b"iteration 1")]}
    for over, word in shared + own[form]:
        _refused(form, [word], **over)
    for E in (1, 4):
        _refused(form, [b"d_in must be 2 or 3"], E=E, edit=lambda mem: [f.update(d_in=4) for f in mem["fields"]])


def test_python_layer_names_what_it_refuses():
    nets = [sm.make_net(2, 32, 1, seed=e) for e in range(3)]
    states = [siren.AdamState(n) for n in nets]
    x, t = torch.from_numpy(sm.points(2, 9)), [torch.zeros((9, 2))] * 3
    idx = torch.zeros((2, 4), dtype=torch.int64)
    with pytest.raises(ValueError, match=r"1\.\.4 members, got 5"):
        siren.fit_run_ensemble(nets + nets[:2], states + states[:2], x, t, None, idx)
    with pytest.raises(ValueError, match="1..4 members, got 0"):
        siren.fit_run_batches_ensemble([], [], x, [], None, [9])
    with pytest.raises(ValueError, match="3 networks, but 2 states"):
        siren.fit_run_ensemble(nets, states[:2], x, t, None, idx)
    with pytest.raises(ValueError, match="member 2 is .* one shape"):
        siren.fit_run_batches_ensemble(nets[:2] + [sm.make_net(2, 64, 1)], states, x, t, None, [9])
    with pytest.raises(ValueError, match="counts sum to 8, the tensors hold 9 rows"):
        siren.fit_run_batches_ensemble(nets, states, x, t, None, [3, 5])
    with pytest.raises(ValueError, match="CUDA tensor"):
        siren.fit_run_ensemble(nets, states, x, t, None, idx)
    with pytest.raises(ValueError, match="CUDA tensor"):
        siren.fit_run_batches_ensemble(nets, states, x, t, None, [4, 5])
    assert all(s.step == 0 for s in states)
    size = [0.0, 2.2, 0.0, 1.0]
    with pytest.raises(ValueError, match="exactly one of n_samples"):
        pj.fit_advection_ensemble(nets, nets, 0.05, size, 3)
    with pytest.raises(ValueError, match="n_iters and iters_per_call must be positive"):
        pj.fit_advection_ensemble(nets, nets, 0.05, size, 0, n_samples=8)
    with pytest.raises(ValueError, match="networks_prev must hold one entry per member"):
        pj.fit_advection_ensemble(nets, nets[:2], 0.05, size, 3, n_samples=8)
    with pytest.raises(ValueError, match="wraps must hold one entry per member"):
        pj.fit_advection_ensemble(nets, nets, 0.05, size, 3, n_samples=8, wraps=[None])
    with pytest.raises(ValueError, match=r"1\.\.4 members, got 5"):
        pj.fit_advection_ensemble(nets + nets[:2], nets + nets[:2], 0.05, size, 3, n_samples=8)
    proj = pj.PressureProjector.__new__(pj.PressureProjector)
    proj.dim, proj.device, proj.samples = 2, torch.device("cpu"), x
    with pytest.raises(ValueError, match=r"grad_p must be \(3, 9, 2\)"):
        proj.fit_projection_ensemble(nets, nets, torch.zeros((9, 2)), 4, 3)


# ---- the ensemble functions hand each member what the single-network functions hand it ------------------------
SIZES = {2: [0.0, 2.2, 0.0, 1.0], 3: [0.0, 1.0, -0.5, 0.5, 0.25, 1.5]}


def _fake_eval(net, x, **kw):
    """A pointwise stand-in for siren.eval, computed in float64: large enough that backtracking leaves the box."""
    xd = x.to(torch.float64)
    return (net.gain * torch.sin(3.0 * xd + net.phase) + 0.25 * net.gain).to(x.dtype)


def _clone(a):
    return None if a is None else a.clone()


def _equal(a, b, what):
    assert (a is None) == (b is None), what
    assert a is None or (a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b)), f"{what} differs"


@pytest.mark.parametrize("tilde", [False, True], ids=["prev", "prev_tilde"])
@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("E", [1, 2, 3, 4])
def test_fit_advection_ensemble_hands_each_member_what_fit_advection_does(monkeypatch, E, dim, tilde):
    """A wrap on the even members only (the karman wrap is 2D: in 3D a sign flip of one component), a
    second frozen network on the odd ones when `tilde`, and a `keep` that drops a ball."""
    n, K, dt, size = 37, 5, 0.3, SIZES[dim]
    nets = [sm.make_net(dim, 32, 1, seed=e) for e in range(E)]
    prevs = [types.SimpleNamespace(gain=1.5 + 0.25 * e, phase=0.3 * (e + 1)) for e in range(E)]
    tildes = [types.SimpleNamespace(gain=-0.75, phase=1.1 + e) if tilde and e % 2 else None for e in range(E)]
    flip = torch.tensor([1.0, -2.0, 0.5][:dim])
    a_wrap = sm.karman_wrap(size, eps=0.125) if dim == 2 else (lambda x, u: u * flip + 0.125 * x)
    wraps = [a_wrap if e % 2 == 0 else None for e in range(E)]
    centre = torch.tensor([0.5 * (size[2 * c] + size[2 * c + 1]) for c in range(dim)])
    keep = lambda x: ((x - centre) ** 2).sum(-1) > 0.3 ** 2  # noqa: E731
    single, members = [], []

    def fake_fit_run_batches(net_, state, x, target, scale, counts, *, stop_loss=None, **kw):
        assert stop_loss is None and sum(counts) == x.shape[0] == target.shape[0]
        single.append(dict(net=net_, step=state.step, counts=list(counts), x=x.clone(), target=target.clone(), scale=_clone(scale)))
        state.step += len(counts)
        return torch.arange(len(counts), dtype=torch.float32), torch.tensor([len(counts), 0])

    def fake_ensemble(nets_, states, x, targets, scales, counts, *, stop_loss=None, **kw):
        assert stop_loss is None and len(nets_) == len(states) == len(targets) == len(scales) == E
        members.append(dict(nets=list(nets_), steps=[s.step for s in states], counts=list(counts), x=x.clone(),
                            targets=[t.clone() for t in targets], scales=[_clone(s) for s in scales]))
        for s in states:
            s.step += len(counts)
        return (torch.arange(len(counts), dtype=torch.float32).repeat(E, 1) + 10.0 * torch.arange(E)[:, None],
                torch.tensor([[len(counts), 0]] * E))
    monkeypatch.setattr(siren, "eval", _fake_eval)
    monkeypatch.setattr(siren, "fit_run_batches", fake_fit_run_batches)
    monkeypatch.setattr(siren, "fit_run_batches_ensemble", fake_ensemble)
    for per_call in (1, 2, 8):  # one at a time, not dividing, larger than n_iters
        single.clear()
        members.clear()
        gens = [torch.Generator().manual_seed(321) for _ in range(E + 1)]
        for e in range(E):
            pj.fit_advection(nets[e], prevs[e], dt, size, K, n_samples=n, network_tilde=tildes[e], wrap=wraps[e], keep=keep,
                             generator=gens[e], iters_per_call=per_call)
        losses, states = pj.fit_advection_ensemble(nets, prevs, dt, size, K, n_samples=n, networks_tilde=tildes, wraps=wraps,
                                                   keep=keep, generator=gens[E], iters_per_call=per_call)
        assert torch.equal(gens[0].get_state(), gens[E].get_state()), "one draw per iteration serves all members"
        blocks = -(-K // per_call)
        assert len(members) == blocks and len(single) == E * blocks
        assert losses.shape == (E, K) and [s.step for s in states] == [K] * E
        assert torch.equal(losses[:, 0], 10.0 * torch.arange(E)), "member e's row is member e's"
        for b, call in enumerate(members):
            assert call["nets"] == nets and call["steps"] == [b * per_call] * E
            for e in range(E):
                want = single[e * blocks + b]
                assert want["net"] is nets[e] and want["step"] == b * per_call and want["counts"] == call["counts"]
                _equal(want["x"], call["x"], f"block {b}: the shared points, against member {e}'s")
                _equal(want["target"], call["targets"][e], f"block {b} member {e}: target")
                _equal(want["scale"], call["scales"][e], f"block {b} member {e}: scale")
                assert (call["scales"][e] is None) == (wraps[e] is None)
        counts = [c for call in members for c in call["counts"]]
        assert len(counts) == K and len(set(counts)) > 1, "the case: keep leaves ragged counts"


@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("E", [1, 2, 3, 4])
def test_fit_projection_ensemble_hands_each_member_what_fit_projection_does(monkeypatch, E, dim):
    n, n_samples, K = 50, 16, 5
    proj = pj.PressureProjector.__new__(pj.PressureProjector)
    proj.dim, proj.device = dim, torch.device("cpu")
    proj.samples = torch.from_numpy(sm.points(dim, n, seed=4))
    grad_p = torch.from_numpy(np.random.default_rng(2).standard_normal((E, n, dim)).astype(np.float32))
    nets = [sm.make_net(dim, 32, 1, seed=e) for e in range(E)]
    prevs = [types.SimpleNamespace(gain=1.5 + 0.25 * e, phase=0.3 * (e + 1)) for e in range(E)]
    flip = torch.tensor([1.0, -2.0, 0.5][:dim])
    a_wrap = sm.karman_wrap(SIZES[2], eps=0.125) if dim == 2 else (lambda x, u: u * flip + 0.125 * x)
    wraps = [None if e % 2 == 0 else a_wrap for e in range(E)]
    single, members = [], []

    def fake_fit_run(net_, state, pool_x, pool_target, pool_scale, idx, *, stop_loss=None, **kw):
        assert pool_x is proj.samples and stop_loss is None
        single.append(dict(net=net_, step=state.step, idx=idx.clone(), target=pool_target.clone(), scale=_clone(pool_scale)))
        state.step += idx.shape[0]
        return torch.zeros(idx.shape[0]), torch.tensor([idx.shape[0], 0])

    def fake_ensemble(nets_, states, pool_x, pool_targets, pool_scales, idx, *, stop_loss=None, **kw):
        assert pool_x is proj.samples and stop_loss is None and len(nets_) == len(pool_targets) == len(pool_scales) == E
        members.append(dict(nets=list(nets_), steps=[s.step for s in states], idx=idx.clone(),
                            targets=[t.clone() for t in pool_targets], scales=[_clone(s) for s in pool_scales]))
        for s in states:
            s.step += idx.shape[0]
        return torch.zeros((E, idx.shape[0])), torch.tensor([[idx.shape[0], 0]] * E)
    monkeypatch.setattr(siren, "eval", _fake_eval)
    monkeypatch.setattr(siren, "fit_run", fake_fit_run)
    monkeypatch.setattr(siren, "fit_run_ensemble", fake_ensemble)
    for per_call in (1, 2, 8):
        single.clear()
        members.clear()
        gens = [torch.Generator().manual_seed(99) for _ in range(E + 1)]
        for e in range(E):
            proj.fit_projection(nets[e], prevs[e], grad_p[e], n_samples, K, wrap=wraps[e], generator=gens[e],
                                iters_per_call=per_call)
        losses, states = proj.fit_projection_ensemble(nets, prevs, grad_p, n_samples, K, wraps=wraps, generator=gens[E],
                                                      iters_per_call=per_call)
        assert torch.equal(gens[0].get_state(), gens[E].get_state()), "one draw per iteration serves all members"
        blocks = -(-K // per_call)
        assert len(members) == blocks and len(single) == E * blocks
        assert losses.shape == (E, K) and [s.step for s in states] == [K] * E
        for b, call in enumerate(members):
            assert call["nets"] == nets and call["steps"] == [b * per_call] * E
            assert call["idx"].shape == (min(per_call, K - b * per_call), n_samples)
            for e in range(E):
                want = single[e * blocks + b]
                assert want["net"] is nets[e]
                _equal(want["idx"], call["idx"], f"block {b}: the shared indices, against member {e}'s")
                _equal(want["target"], call["targets"][e], f"block {b} member {e}: target")
                _equal(want["scale"], call["scales"][e], f"block {b} member {e}: scale")
                assert (call["scales"][e] is None) == (wraps[e] is None)


def test_a_stopped_member_leaves_the_later_blocks_and_no_block_follows_the_last_stop(monkeypatch):
    """The fake behaves as wos_siren_fit_run_ensemble does: member e's losses are 1 - i / 10 + 0.3 e by the
    global iteration i until the first one at or below stop_loss, NaN after it."""
    n, n_samples, K, E, stop = 50, 8, 9, 3, np.float32(0.95)
    proj = pj.PressureProjector.__new__(pj.PressureProjector)
    proj.dim, proj.device = 2, torch.device("cpu")
    proj.samples = torch.from_numpy(sm.points(2, n, seed=4))
    nets = [sm.make_net(2, 32, 1, seed=e) for e in range(E)]
    prevs = [types.SimpleNamespace(gain=1.0, phase=0.1 * e) for e in range(E)]
    offset = {id(net): 0.3 * e for e, net in enumerate(nets)}
    calls = []

    def fake_ensemble(nets_, states, pool_x, pool_targets, pool_scales, idx, *, stop_loss=None, **kw):
        k = idx.shape[0]
        calls.append(([nets.index(m) for m in nets_], k))
        losses, status = torch.full((len(nets_), k), float("nan")), torch.zeros((len(nets_), 2), dtype=torch.int64)
        for row, (m, s) in enumerate(zip(nets_, states)):
            for i in range(k):
                losses[row, i] = 1.0 - (s.step + i) / 10 + offset[id(m)]
                status[row, 0] = i + 1
                if losses[row, i] <= np.float32(stop_loss):
                    break
            s.step += int(status[row, 0])
        return losses, status
    monkeypatch.setattr(siren, "eval", _fake_eval)
    monkeypatch.setattr(siren, "fit_run_ensemble", fake_ensemble)
    gen = torch.Generator().manual_seed(5)
    losses, states = proj.fit_projection_ensemble(nets, prevs, torch.zeros((E, n, 2)), n_samples, K, generator=gen,
                                                  early_stop=float(stop), iters_per_call=2)
    # members 0 and 2 stop at iterations 1 and 7, the last of their blocks (status[e][0] equals the block's
    # length, and the last applied loss tells); member 1 at iteration 4, the first of the third block
    assert [s.step for s in states] == [2, 5, 8]
    assert calls == [([0, 1, 2], 2), ([1, 2], 2), ([1, 2], 2), ([2], 2)], "a stopped member leaves; nothing after the last stop"
    for e, applied in enumerate([2, 5, 8]):
        assert bool(torch.isfinite(losses[e, :applied]).all()) and bool(torch.isnan(losses[e, applied:]).all())
    want = torch.Generator().manual_seed(5)
    for _ in range(8):
        torch.randint(0, n - 1, (n_samples,), generator=want)
    assert torch.equal(gen.get_state(), want.get_state()), "four blocks of two draws, none after every member stopped"
