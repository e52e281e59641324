"""The ensemble fit loops on the GPU (wos_siren_fit_run_ensemble, wos_siren_fit_run_batches_ensemble,
csrc/wos_capi_siren.cpp; wos_amd.siren.fit_run_ensemble / fit_run_batches_ensemble,
wos_amd.projection.fit_projection_ensemble / fit_advection_ensemble): every member of an ensemble
call ends, bit for bit in every loss, parameter and moment, where the single-network entry point
called on that member alone ends -- so no tolerance appears below.  E = 1 .. 4 over the shapes at
which the kernels take another path, pool batches and ragged row counts, clipping, a continued run,
a one-tile workspace; permuted and twin members; a NaN in one member; a stop in one member."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

import siren_fit_model as fm
import siren_model as sm
from wos_amd import _lib, siren, workloads
from wos_amd import projection as pj

pytestmark = pytest.mark.gpu

KW = dict(lr=1e-4, betas=(0.9, 0.999), eps=1e-8)
K = 6
# (d_in, H, L, d_out): one row tile; idle waves (H / 32 = 2 of 4 own a row tile); two row tiles per wave, of
# which the last wave drops its second; 12 reduce segments and 20 Adam tensors per member
SHAPES = [(2, 32, 1, 2), (3, 64, 2, 3), (2, 160, 1, 2), (3, 32, 8, 1)]
SHAPE_IDS = [f"d{s[0]}_H{s[1]}_L{s[2]}_o{s[3]}" for s in SHAPES]
BATCHES = [1, 33, 65]
COUNTS = [1, 32, 33, 65, 31, 64]  # the advection fit's ragged five and a sixth iteration of two exact tiles
N_POOL = 97


def bits(a):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def _cuda_net(shape, seed=0, gain=None):
    d, H, L, d_out = shape
    net = copy.deepcopy(sm.make_net(d, H, L, d_out, seed=seed)).cuda()
    if gain is not None:
        with torch.no_grad():
            net.net[-1].weight.mul_(gain)
    return net


def _tensors(net):
    p = siren.pack(net)
    return p.weights + p.biases


def _same_run(net_a, state_a, net_b, state_b, what):
    for k, (a, b) in enumerate(zip(_tensors(net_a), _tensors(net_b))):
        assert same(a, b), f"{what}: parameter tensor {k}, {np.sum(bits(a) != bits(b))} of {a.numel()} differ"
    assert same(state_a.exp_avg, state_b.exp_avg), f"{what}: exp_avg"
    assert same(state_a.exp_avg_sq, state_b.exp_avg_sq), f"{what}: exp_avg_sq"
    assert state_a.step == state_b.step, what


def _members(shape, E, clip=None, seeds=None):
    """Two copies of E different networks with fresh states: one for the single runs, one for the ensemble."""
    seeds = list(range(E)) if seeds is None else seeds
    a, b = [_cuda_net(shape, seed=s) for s in seeds], [_cuda_net(shape, seed=s) for s in seeds]
    return (a, [siren.AdamState(n, max_grad_norm=clip, **KW) for n in a],
            b, [siren.AdamState(n, max_grad_norm=clip, **KW) for n in b])


def _data(shape, E, n, first=0):
    """Shared points [first + n, d_in] and per member a target and a scale; the odd members have no scale."""
    d, _, _, d_out = shape
    x = torch.from_numpy(sm.points(d, first + n, seed=6)).cuda()
    targets, scales = [], []
    for e in range(E):
        t, sc = fm.problem(first + n, d_out, e % 2 == 0, seed=3 + e)
        targets.append(torch.from_numpy(t).cuda())
        scales.append(None if sc is None else torch.from_numpy(sc).cuda())
    return x, targets, scales


def _idx(batch, seed=11, k=K):
    return torch.randint(0, N_POOL, (k, batch), generator=torch.Generator().manual_seed(seed)).cuda()


def _check(E, want, losses, status, nets_a, states_a, nets_b, states_b, what, k=K):
    assert losses.is_cuda and losses.shape == (E, k) and status.dtype == torch.int64 and status.tolist() == [[k, 0]] * E, what
    for e in range(E):
        assert same(losses[e], want[e]), f"{what}: member {e} losses {losses[e].tolist()} single run {want[e].tolist()}"
        assert bool(torch.isfinite(losses[e]).all())
        _same_run(nets_a[e], states_a[e], nets_b[e], states_b[e], f"{what}: member {e}")


# ---- 1. the ensemble call = E single calls, bit for bit ------------------------------------------------------
@pytest.mark.parametrize("E", [1, 2, 3, 4])
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_fit_run_ensemble_equals_the_single_runs(gpu, shape, E):
    x, targets, scales = _data(shape, E, N_POOL)
    for batch in BATCHES:
        for clip in (None, 0.1):
            idx = _idx(batch)
            nets_a, states_a, nets_b, states_b = _members(shape, E, clip)
            want = [siren.fit_run(nets_a[e], states_a[e], x, targets[e], scales[e], idx)[0] for e in range(E)]
            losses, status = siren.fit_run_ensemble(nets_b, states_b, x, targets, scales, idx)
            _check(E, want, losses, status, nets_a, states_a, nets_b, states_b, f"batch {batch}, clip {clip}")
            fresh = _cuda_net(shape, seed=E - 1)
            assert any(not same(a, b) for a, b in zip(_tensors(nets_b[-1]), _tensors(fresh))), "the run moved the network"


@pytest.mark.parametrize("E", [1, 2, 3, 4])
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_fit_run_batches_ensemble_equals_the_single_runs(gpu, shape, E):
    x, targets, scales = _data(shape, E, sum(COUNTS))
    for clip in (None, 0.1):
        nets_a, states_a, nets_b, states_b = _members(shape, E, clip)
        want = [siren.fit_run_batches(nets_a[e], states_a[e], x, targets[e], scales[e], COUNTS)[0] for e in range(E)]
        losses, status = siren.fit_run_batches_ensemble(nets_b, states_b, x, targets, scales, COUNTS)
        _check(E, want, losses, status, nets_a, states_a, nets_b, states_b, f"ragged, clip {clip}")


@pytest.mark.parametrize("E", [1, 2, 3, 4])
def test_a_first_offset_of_three_rows_through_the_c_abi(gpu, E):
    """offsets[0] = 3 at d_in = 3: the first batch starts 36 bytes into the shared and the members'
    arrays.  The single runs go through wos_siren_fit_run_batches with the same offsets."""
    shape, first = (3, 64, 2, 3), 3
    x, targets, scales = _data(shape, E, sum(COUNTS), first=first)
    offsets = (C.c_int64 * (K + 1))(*np.concatenate([[first], first + np.cumsum(COUNTS)]).tolist())
    nets_a, states_a, nets_b, states_b = _members(shape, E, 0.1)
    lib = _lib.load()
    opt = states_a[0].params()
    ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731

    def net_struct(net):
        p = siren.pack(net)
        w = (C.c_void_p * 4)(*[t.data_ptr() for t in p.weights])
        b = (C.c_void_p * 4)(*[t.data_ptr() for t in p.biases])
        return _lib.SirenNet(p.d_in, p.d_out, p.hidden, p.n_hidden_layers, p.omega, w, b), (w, b)
    torch.cuda.synchronize()
    want = []
    for e in range(E):
        losses, status = torch.zeros(K, device="cuda"), torch.full((2,), 9, dtype=torch.int64, device="cuda")
        st, keep = net_struct(nets_a[e])
        rc = lib.wos_siren_fit_run_batches(C.byref(st), x.data_ptr(), targets[e].data_ptr(), ptr(scales[e]), offsets, K,
                                           states_a[e].exp_avg.data_ptr(), states_a[e].exp_avg_sq.data_ptr(), 0,
                                           C.byref(opt), -1.0, 0, losses.data_ptr(), status.data_ptr(), 0,
                                           _lib.WOS_PTRS_DEVICE, 0, None)
        assert rc == 0, lib.wos_last_error()
        states_a[e].step = K
        want.append(losses)
    structs = [net_struct(n) for n in nets_b]
    arr = lambda ts: (C.c_void_p * E)(*[ptr(t) for t in ts])  # noqa: E731
    losses = torch.zeros((E, K), device="cuda")
    status = torch.full((E, 2), 9, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    rc = lib.wos_siren_fit_run_batches_ensemble(E, (_lib.SirenNet * E)(*[s for s, _ in structs]), x.data_ptr(), arr(targets),
                                                arr(scales), offsets, K, arr([s.exp_avg for s in states_b]),
                                                arr([s.exp_avg_sq for s in states_b]), 0, C.byref(opt), -1.0, 2,
                                                losses.data_ptr(), status.data_ptr(), 0, _lib.WOS_PTRS_DEVICE, 0, None)
    assert rc == 0, lib.wos_last_error()
    for s in states_b:
        s.step = K
    _check(E, want, losses, status, nets_a, states_a, nets_b, states_b, "first offset 3, blocking, check_every 2")


# ---- 2. a continued run and a one-tile workspace -------------------------------------------------------------
@pytest.mark.parametrize("E", [2, 4])
def test_chunked_and_continued_from_step_five(gpu, E):
    shape = (2, 64, 1, 2)
    ws = (2 * 1 + 1) * 64 * 4 * 32  # one tile per member: a 65-row batch goes in three chunks, a 33-row one in two
    x, targets, scales = _data(shape, E, sum(COUNTS))
    nets_a, states_a, nets_b, states_b = _members(shape, E, 0.1)
    five = COUNTS[:5]
    rows5 = sum(five)
    cut = lambda ts: [None if t is None else t[:rows5] for t in ts]  # noqa: E731
    want = [siren.fit_run_batches(nets_a[e], states_a[e], x[:rows5], targets[e][:rows5], cut(scales)[e], five,
                                  workspace_bytes=ws)[0] for e in range(E)]
    losses, status = siren.fit_run_batches_ensemble(nets_b, states_b, x[:rows5], cut(targets), cut(scales), five,
                                                    workspace_bytes=ws)
    _check(E, want, losses, status, nets_a, states_a, nets_b, states_b, "one-tile workspace, ragged", k=5)
    # step0 = 5 with non-zero moments: the pool form continues, chunked as well
    assert all(s.step == 5 and bool(s.exp_avg.any()) and bool(s.exp_avg_sq.any()) for s in states_b)
    px, pt, ps = _data(shape, E, N_POOL)
    idx = _idx(65, seed=12)
    want = [siren.fit_run(nets_a[e], states_a[e], px, pt[e], ps[e], idx, workspace_bytes=ws)[0] for e in range(E)]
    losses, status = siren.fit_run_ensemble(nets_b, states_b, px, pt, ps, idx, workspace_bytes=ws)
    assert all(s.step == 5 + K for s in states_b)
    _check(E, want, losses, status, nets_a, states_a, nets_b, states_b, "continued from step 5, one-tile workspace")


# ---- 3. the members do not see each other -------------------------------------------------------------------
@pytest.mark.parametrize("form", ["pool", "batches"])
def test_permuting_the_members_permutes_the_results(gpu, form):
    shape, E, perm = (3, 64, 2, 3), 4, [2, 0, 3, 1]
    n = N_POOL if form == "pool" else sum(COUNTS)
    x, targets, scales = _data(shape, E, n)
    last = _idx(33) if form == "pool" else COUNTS
    run = siren.fit_run_ensemble if form == "pool" else siren.fit_run_batches_ensemble
    nets_a, states_a, nets_b, states_b = _members(shape, E, 0.1)
    pick = lambda xs: [xs[e] for e in perm]  # noqa: E731
    la, sa = run(nets_a, states_a, x, targets, scales, last)
    lb, sb = run(pick(nets_b), pick(states_b), x, pick(targets), pick(scales), last)
    assert sa.tolist() == sb.tolist() == [[K, 0]] * E
    for at, e in enumerate(perm):
        assert same(lb[at], la[e]), f"member {e} at place {at}"
        _same_run(nets_a[e], states_a[e], nets_b[e], states_b[e], f"member {e} at place {at}")
    assert not same(la[0], la[1]), "the members differ"


@pytest.mark.parametrize("form", ["pool", "batches"])
def test_twin_members_end_with_equal_bits(gpu, form):
    """Members 0 and 2 have equal weights and equal data in separate buffers."""
    shape, E = (2, 160, 1, 2), 3
    n = N_POOL if form == "pool" else sum(COUNTS)
    x, targets, scales = _data(shape, E, n)
    targets[2], scales[2] = targets[0].clone(), scales[0].clone()
    nets, states, _, _ = _members(shape, E, 0.1, seeds=[0, 1, 0])
    assert all(a.data_ptr() != b.data_ptr() for a, b in zip(_tensors(nets[0]), _tensors(nets[2])))
    if form == "pool":
        losses, _ = siren.fit_run_ensemble(nets, states, x, targets, scales, _idx(65))
    else:
        losses, _ = siren.fit_run_batches_ensemble(nets, states, x, targets, scales, COUNTS)
    assert same(losses[0], losses[2]) and not same(losses[0], losses[1])
    _same_run(nets[0], states[0], nets[2], states[2], "twins")


@pytest.mark.parametrize("form", ["pool", "batches"])
def test_a_nan_in_one_member_stays_there(gpu, form):
    shape, E = (3, 64, 2, 3), 3
    n = N_POOL if form == "pool" else sum(COUNTS)
    x, targets, scales = _data(shape, E, n)
    targets[1] = targets[1].clone()
    targets[1][5, 1] = float("nan")  # row 5: in iteration 2 of the ragged form, and drawn below for the pool form
    nets_a, states_a, nets_b, states_b = _members(shape, E, 0.1)
    if form == "pool":
        idx = _idx(33)
        idx[1, 7] = 5
        want = {e: siren.fit_run(nets_a[e], states_a[e], x, targets[e], scales[e], idx)[0] for e in (0, 2)}
        losses, status = siren.fit_run_ensemble(nets_b, states_b, x, targets, scales, idx)
    else:
        want = {e: siren.fit_run_batches(nets_a[e], states_a[e], x, targets[e], scales[e], COUNTS)[0] for e in (0, 2)}
        losses, status = siren.fit_run_batches_ensemble(nets_b, states_b, x, targets, scales, COUNTS)
    assert status.tolist() == [[K, 0]] * E
    assert bool(torch.isnan(losses[1]).any()) and bool(torch.isnan(_tensors(nets_b[1])[0]).any()), "the NaN reached member 1"
    for e in (0, 2):
        assert same(losses[e], want[e]) and bool(torch.isfinite(losses[e]).all())
        _same_run(nets_a[e], states_a[e], nets_b[e], states_b[e], f"member {e} beside a NaN member")


# ---- 4. a stop in one member ----------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["pool", "batches"])
def test_a_stop_in_member_zero_leaves_member_one_running(gpu, form):
    """The same rows every iteration, so member 0's loss falls; the threshold lies between its second
    and its third loss, and far below member 1's, whose target is twenty times as large."""
    shape, n = (2, 64, 1, 2), 33
    x1, t1, s1 = _data(shape, 2, n)
    t1[1] = 20.0 * t1[1] + 3.0
    if form == "pool":
        x, targets, scales = x1, t1, s1
        last = torch.arange(n).repeat(K, 1).cuda()
        single, run = siren.fit_run, siren.fit_run_ensemble
    else:
        rep = lambda a: None if a is None else a.repeat(K, 1)  # noqa: E731
        x, targets, scales = rep(x1), [rep(t) for t in t1], [rep(s) for s in s1]
        last = [n] * K
        single, run = siren.fit_run_batches, siren.fit_run_batches_ensemble
    free_nets, free_states, _, _ = _members(shape, 2)
    free = [single(free_nets[e], free_states[e], x, targets[e], scales[e], last)[0].cpu().numpy() for e in range(2)]
    f = free[0]
    assert f[0] > f[1] > f[2], f"the test's premise, a falling loss: {f.tolist()}"
    stop = float(np.float32(0.5 * (float(f[1]) + float(f[2]))))
    assert f[2] <= np.float32(stop) < f[1] and free[1].min() > 10 * stop, (f.tolist(), free[1].tolist())
    stopped_net, _, _, _ = _members(shape, 1)
    stopped_state = siren.AdamState(stopped_net[0], **KW)
    single(stopped_net[0], stopped_state, x, targets[0], scales[0], last, stop_loss=stop)
    assert stopped_state.step == 3
    results = []
    for check_every in (0, 1):
        _, _, nets, states = _members(shape, 2)
        losses, status = run(nets, states, x, targets, scales, last, stop_loss=stop, check_every=check_every)
        assert status.tolist() == [[3, 0], [K, 0]], (check_every, status.tolist())
        assert [s.step for s in states] == [3, K]
        assert same(losses[0, :3], free[0][:3]) and bool(torch.isnan(losses[0, 3:]).all()), losses.tolist()
        assert same(losses[1], free[1]), "member 1 never stops"
        _same_run(stopped_net[0], stopped_state, nets[0], states[0], f"member 0 frozen where its single run stopped ({check_every})")
        _same_run(free_nets[1], free_states[1], nets[1], states[1], f"member 1 as its unstopped single run ({check_every})")
        results.append(losses)
    assert same(results[0], results[1])


# ---- 5. the two projection functions ------------------------------------------------------------------------
SIZE = [0.0, 2.2, 0.0, 1.0]
DT, GAIN, N_SAMPLES = 0.5, 20.0, 65


def outside_disk(x):
    return (x[..., 0] - 0.6) ** 2 + (x[..., 1] - 0.5) ** 2 > 0.25 ** 2


def _gen(seed=77):
    return torch.Generator(device="cuda").manual_seed(seed)


@pytest.mark.parametrize("E", [2, 4])
def test_fit_advection_ensemble_equals_fit_advection(gpu, E):
    """Blocks of 2, 2 and 1; a disk `keep`, so the counts differ and are no multiple of 32; a wrap on the
    even members and a second frozen network on the odd ones."""
    shape, n_iters = (2, 64, 1, 2), 5
    prevs = [_cuda_net(shape, seed=10 + e, gain=GAIN) for e in range(E)]
    tildes = [_cuda_net(shape, seed=20 + e, gain=GAIN) if e % 2 else None for e in range(E)]
    wraps = [None if e % 2 else sm.karman_wrap(SIZE, eps=0.125) for e in range(E)]
    counts = []

    def keep(x):
        mask = outside_disk(x)
        counts.append(mask.reshape(-1, N_SAMPLES).sum(1).tolist())
        return mask
    nets_a, _, nets_b, _ = _members(shape, E)
    want, states_a = [], []
    for e in range(E):
        g = _gen()
        losses, state = pj.fit_advection(nets_a[e], prevs[e], DT, SIZE, n_iters, n_samples=N_SAMPLES, network_tilde=tildes[e],
                                         wrap=wraps[e], keep=keep, generator=g, iters_per_call=2)
        want.append(losses)
        states_a.append(state)
    flat = [c for block in counts[:3] for c in block]
    assert len(set(flat)) >= 2 and any(c % 32 for c in flat), f"the case: ragged counts, got {flat}"
    g2 = _gen()
    losses, states_b = pj.fit_advection_ensemble(nets_b, prevs, DT, SIZE, n_iters, n_samples=N_SAMPLES, networks_tilde=tildes,
                                                 wraps=wraps, keep=keep, generator=g2, iters_per_call=2)
    assert torch.equal(g.get_state(), g2.get_state()), "the generator consumption of the single loop"
    assert losses.shape == (E, n_iters) and [s.step for s in states_b] == [n_iters] * E
    for e in range(E):
        assert same(losses[e], want[e]), f"member {e}: {losses[e].tolist()} fit_advection {want[e].tolist()}"
        _same_run(nets_a[e], states_a[e], nets_b[e], states_b[e], f"fit_advection_ensemble, member {e}")


@pytest.mark.parametrize("E", [2, 4])
def test_fit_projection_ensemble_equals_fit_projection(gpu, E):
    """A tiny karman scene: one (E, H, W) solve on one set of walks, then one loop over the members."""
    shape, n_iters = (2, 64, 1, 2), 5
    cfg = workloads.karman_config(n_walks=32, n_points=300)
    scene_cfg = dict(workloads.SCENE_BASE, boundary=workloads.KARMAN_OBJ)
    samples = torch.from_numpy(cfg["points"]).cuda()
    proj = pj.PressureProjector(scene_cfg, cfg["solver"], cfg["output"], samples)
    src = torch.from_numpy(cfg["source"]).cuda()
    _, grad_p = proj.solve(torch.stack([src * (1.0 + 0.5 * e) for e in range(E)]))
    assert tuple(grad_p.shape) == (E, samples.shape[0], 2) and not same(grad_p[0], grad_p[1])
    prevs = [_cuda_net(shape, seed=10 + e) for e in range(E)]
    wraps = [None if e % 2 else sm.karman_wrap(SIZE, eps=0.125) for e in range(E)]
    nets_a, _, nets_b, _ = _members(shape, E)
    want, states_a = [], []
    for e in range(E):
        g = _gen()
        losses, state = proj.fit_projection(nets_a[e], prevs[e], grad_p[e].contiguous(), N_SAMPLES, n_iters, wrap=wraps[e],
                                            generator=g, iters_per_call=2)
        want.append(losses)
        states_a.append(state)
    g2 = _gen()
    losses, states_b = proj.fit_projection_ensemble(nets_b, prevs, grad_p, N_SAMPLES, n_iters, wraps=wraps, generator=g2,
                                                    iters_per_call=2)
    assert torch.equal(g.get_state(), g2.get_state()), "the generator consumption of the single loop"
    assert losses.shape == (E, n_iters) and [s.step for s in states_b] == [n_iters] * E
    for e in range(E):
        assert same(losses[e], want[e]) and bool(torch.isfinite(losses[e]).all()), f"member {e}"
        _same_run(nets_a[e], states_a[e], nets_b[e], states_b[e], f"fit_projection_ensemble, member {e}")
    proj.scene.close() if hasattr(proj.scene, "close") else None
