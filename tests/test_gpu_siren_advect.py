"""The device-resident advection fit on the GPU (wos_siren_fit_run_batches,
csrc/wos_capi_siren.cpp; wos_amd.siren.fit_run_batches, wos_amd.projection.fit_advection):
fit_run_batches bit for bit against siren.fit and siren.adam_step on the row slices -- ragged counts,
chunked, continued, from a first offset that is not zero, stopped early -- and fit_advection bit for
bit against the reference's loop restated here in plain torch (src/2d/models/model_split.py:88-110),
with a wrap, a second frozen network and samples dropped inside an obstacle."""
import copy
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import siren_fit_model as fm
import siren_model as sm
from wos_amd import _lib, siren
from wos_amd import projection as pj

pytestmark = pytest.mark.gpu

KW = dict(lr=1e-4, betas=(0.9, 0.999), eps=1e-8)
COUNTS = [1, 32, 33, 65, 31]  # a lone point, an exact tile, one past, three tiles with a partial last one, a short tile
TOTAL = sum(COUNTS)


def bits(a):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def _cuda_net(d, H, L, d_out=None, seed=0, gain=None):
    """A fresh copy of sm.make_net on the GPU; gain multiplies the output layer (a velocity of order one)."""
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


# ---- 1. fit_run_batches = the separate calls, bit for bit ------------------------------------------------
def _rows(d, d_out, with_scale, n=TOTAL, seed=6):
    x = torch.from_numpy(sm.points(d, n, seed=seed)).cuda()
    target, scale = fm.problem(n, d_out, with_scale, seed=3)
    return x, torch.from_numpy(target).cuda(), None if scale is None else torch.from_numpy(scale).cuda()


def _loop(net, state, rows, counts, first=0, n=None, ws=None):
    """siren.fit and siren.adam_step made separately on copies of the row slices, n iterations."""
    x, target, scale = rows
    losses, at = [], first
    for c in counts[:n]:
        cut = lambda a: None if a is None else a[at:at + c].clone()  # noqa: E731
        loss, gw, gb = siren.fit(net, cut(x), cut(target), cut(scale), workspace_bytes=ws)
        siren.adam_step(net, (gw, gb), state)
        losses.append(loss)
        at += c
    return torch.stack(losses)


SHAPES = [(2, 32, 1, 2), (3, 64, 2, 3), (2, 160, 1, 2)]  # the last: two row tiles per wave


@pytest.mark.parametrize("clip", [None, 0.1], ids=["noclip", "clip"])
@pytest.mark.parametrize("with_scale", [False, True], ids=["plain", "scale"])
@pytest.mark.parametrize("shape", SHAPES, ids=[f"d{s[0]}_H{s[1]}_L{s[2]}" for s in SHAPES])
def test_fit_run_batches_equals_the_separate_calls(gpu, shape, with_scale, clip):
    rows = _rows(shape[0], shape[3], with_scale)
    net_a, net_b = _cuda_net(*shape), _cuda_net(*shape)
    state_a, state_b = siren.AdamState(net_a, max_grad_norm=clip, **KW), siren.AdamState(net_b, max_grad_norm=clip, **KW)
    want = _loop(net_a, state_a, rows, COUNTS)
    losses, status = siren.fit_run_batches(net_b, state_b, *rows, COUNTS)
    K = len(COUNTS)
    assert losses.is_cuda and losses.shape == (K,) and status.dtype == torch.int64 and status.tolist() == [K, 0]
    assert same(losses, want), f"losses {losses.tolist()} separate calls {want.tolist()}"
    assert bool(torch.isfinite(losses).all()) and state_b.step == K
    _same_run(net_a, state_a, net_b, state_b, "fit_run_batches")
    assert any(not same(a, b) for a, b in zip(_tensors(net_b), _tensors(_cuda_net(*shape)))), "the run moved the network"


def test_fit_run_batches_without_a_hidden_layer_equals_the_separate_calls(gpu):
    """L = 0: no packed copies in the run's temporary, which starts with the H zeros."""
    shape, counts = (2, 32, 0, 2), [33, 33]  # one full tile and one point, twice
    rows = _rows(2, 2, True, n=sum(counts))
    net_a, net_b = _cuda_net(*shape), _cuda_net(*shape)
    state_a, state_b = siren.AdamState(net_a, max_grad_norm=0.1, **KW), siren.AdamState(net_b, max_grad_norm=0.1, **KW)
    want = _loop(net_a, state_a, rows, counts)
    losses, status = siren.fit_run_batches(net_b, state_b, *rows, counts)
    assert status.tolist() == [2, 0] and same(losses, want), f"losses {losses.tolist()} separate calls {want.tolist()}"
    assert bool(torch.isfinite(losses).all()) and state_b.step == 2
    _same_run(net_a, state_a, net_b, state_b, "fit_run_batches, L = 0")
    assert any(not same(a, b) for a, b in zip(_tensors(net_b), _tensors(_cuda_net(*shape)))), "the run moved the network"


def test_fit_run_batches_chunked_and_continued(gpu):
    shape = (2, 64, 1, 2)
    rows = _rows(2, 2, True)
    ws = (2 * 1 + 1) * 64 * 4 * 32  # one tile: the 65-row batch goes in three chunks, the 33-row one in two
    net_a, net_b = _cuda_net(*shape), _cuda_net(*shape)
    state_a, state_b = siren.AdamState(net_a, **KW), siren.AdamState(net_b, **KW)
    want = _loop(net_a, state_a, rows, COUNTS, ws=ws)
    losses, _ = siren.fit_run_batches(net_b, state_b, *rows, COUNTS, workspace_bytes=ws)
    assert same(losses, want)
    _same_run(net_a, state_a, net_b, state_b, "one-tile workspace")
    # step0 = 5 with a non-zero state: the run continues the separate calls, and they continue it
    assert state_b.step == 5 and bool(state_b.exp_avg.any()) and bool(state_b.exp_avg_sq.any())
    again = _rows(2, 2, True, seed=8)
    want = _loop(net_a, state_a, again, COUNTS)
    losses, status = siren.fit_run_batches(net_b, state_b, *again, COUNTS)
    assert status.tolist() == [5, 0] and state_b.step == 10 and same(losses, want)
    _same_run(net_a, state_a, net_b, state_b, "continued from step 5")


def test_a_first_offset_that_is_not_zero_through_the_c_abi(gpu):
    """offsets[0] = 3 at d_in = 3: the first batch starts 36 bytes into the caller's arrays, and no
    batch after it on a 16-byte boundary either."""
    shape, first = (3, 64, 2, 3), 3
    rows = _rows(3, 3, True, n=first + TOTAL)
    offsets = np.concatenate([[first], first + np.cumsum(COUNTS)]).astype(np.int64)
    assert rows[0].data_ptr() % 256 == 0 and [int(o) * 12 % 16 for o in offsets[:3]] == [4, 0, 0] and offsets[3] * 12 % 16
    K = len(COUNTS)
    net_a, net_b = _cuda_net(*shape), _cuda_net(*shape)
    state_a, state_b = siren.AdamState(net_a, **KW), siren.AdamState(net_b, **KW)
    want = _loop(net_a, state_a, rows, COUNTS, first=first)
    p = siren.pack(net_b)
    w = (C.c_void_p * 4)(*[t.data_ptr() for t in p.weights])
    b = (C.c_void_p * 4)(*[t.data_ptr() for t in p.biases])
    st = _lib.SirenNet(p.d_in, p.d_out, p.hidden, p.n_hidden_layers, p.omega, w, b)
    losses, status = torch.zeros(K, device="cuda"), torch.full((2,), 9, dtype=torch.int64, device="cuda")
    opt = state_b.params()
    torch.cuda.synchronize()
    lib = _lib.load()
    rc = lib.wos_siren_fit_run_batches(C.byref(st), rows[0].data_ptr(), rows[1].data_ptr(), rows[2].data_ptr(),
                                       (C.c_int64 * (K + 1))(*offsets.tolist()), K, state_b.exp_avg.data_ptr(),
                                       state_b.exp_avg_sq.data_ptr(), 0, C.byref(opt), -1.0, 2, losses.data_ptr(),
                                       status.data_ptr(), 0, _lib.WOS_PTRS_DEVICE, 0, None)
    assert rc == 0, lib.wos_last_error()
    state_b.step = K
    assert status.tolist() == [K, 0] and same(losses, want), f"losses {losses.tolist()} separate calls {want.tolist()}"
    _same_run(net_a, state_a, net_b, state_b, "first offset 3, blocking, check_every 2")


# ---- 2. early stop ---------------------------------------------------------------------------------------------
def test_fit_run_batches_early_stop(gpu):
    shape, n, K = (2, 64, 1, 2), 33, 5
    one = _rows(2, 2, True, n=n)
    rows = tuple(a.repeat(K, 1) for a in one)  # the same rows every iteration: the loss goes down
    counts = [n] * K
    free_net, free_state = _cuda_net(*shape), siren.AdamState(_cuda_net(*shape), **KW)
    free, status = siren.fit_run_batches(free_net, free_state, *rows, counts)
    assert status.tolist() == [K, 0] and bool(torch.isfinite(free).all())
    f = free.cpu().numpy()
    assert f[0] > f[1] > f[2], f"the test's premise, a falling loss: {f.tolist()}"
    stop = float(np.float32(0.5 * (float(f[1]) + float(f[2]))))
    assert f[2] <= np.float32(stop) < f[1], "between the second and the third loss"
    three_net, three_state = _cuda_net(*shape), siren.AdamState(_cuda_net(*shape), **KW)
    _loop(three_net, three_state, rows, counts, n=3)
    results = []
    for check_every in (0, 1):
        net, state = _cuda_net(*shape), siren.AdamState(_cuda_net(*shape), **KW)
        losses, status = siren.fit_run_batches(net, state, *rows, counts, stop_loss=stop, check_every=check_every)
        assert status.tolist() == [3, 0] and state.step == 3, (check_every, status.tolist())
        assert same(losses[:3], free[:3]) and bool(torch.isnan(losses[3:]).all()), losses.tolist()
        _same_run(three_net, three_state, net, state, f"stopped after three steps (check_every {check_every})")
        results.append(losses)
    assert same(results[0], results[1])


# ---- 3. fit_advection end to end -----------------------------------------------------------------------------
SIZE = {2: [0.0, 2.2, 0.0, 1.0], 3: [0.0, 1.0, 0.0, 1.0, 0.0, 1.0]}
DT, GAIN, N_SAMPLES = 0.5, 20.0, 65


def outside_disk(x):
    """The fluid side of an obstacle: outside the disk (in 3D the cylinder) of radius 0.25 at (0.6, 0.5)."""
    return (x[..., 0] - 0.6) ** 2 + (x[..., 1] - 0.5) ** 2 > 0.25 ** 2


def _own_loop(net, state, prev, tilde, wrap, keep, dim, n_iters, gen, n_samples=N_SAMPLES):
    """_advect_velocity in _training_loop (src/2d/models/model_split.py:88-110, base.py:130-152) restated:
    sample_random_2D, the obstacle filter, query_velocity as wrap(x, N(x)) with the networks through
    siren.eval, the backtrack and the in-place clamp per axis, then siren.fit on (curr_u - advected_u)
    in its (scale, offset) form and siren.adam_step.  Returns (losses, counts, clamped, unclamped)."""
    size = SIZE[dim]
    losses, counts, clamped, unclamped = [], [], 0, 0

    def query(n_, pts):
        u = siren.eval(n_, pts)
        return u if wrap is None else wrap(pts, u)
    for _ in range(n_iters):
        samples = torch.rand(n_samples, dim, device="cuda", generator=gen)
        for c in range(dim):
            samples[..., c] = samples[..., c] * (size[2 * c + 1] - size[2 * c]) + size[2 * c]
        if keep is not None:
            samples = samples[keep(samples)]
        prev_u = query(prev, samples)
        back = samples - prev_u * DT
        for c in range(dim):
            out = (back[..., c] < size[2 * c]) | (back[..., c] > size[2 * c + 1])
            clamped, unclamped = clamped + int(out.sum()), unclamped + int((~out).sum())
            back[..., c] = torch.clamp(torch.clone(back[..., c]), min=size[2 * c], max=size[2 * c + 1])
        if tilde is None:
            advected_u = query(prev, back)
        else:
            advected_u = 2 * query(prev, back) - query(tilde, back)
        scale = None
        if wrap is not None:
            scale, offset = siren.diagonal_wrap(wrap, samples, dim)
            advected_u = advected_u - offset
        loss, gw, gb = siren.fit(net, samples, advected_u, scale)
        siren.adam_step(net, (gw, gb), state)
        losses.append(loss)
        counts.append(int(samples.shape[0]))
    return torch.stack(losses), counts, clamped, unclamped


def _frozen(dim, with_tilde):
    return _cuda_net(dim, 64, 1, seed=1, gain=GAIN), _cuda_net(dim, 64, 1, seed=2, gain=GAIN) if with_tilde else None


def _gen(seed=77):
    return torch.Generator(device="cuda").manual_seed(seed)


CASES = [(2, False, False), (2, False, True), (2, True, True), (3, False, True)]


@pytest.mark.parametrize("with_tilde", [False, True], ids=["prev", "prev_tilde"])
@pytest.mark.parametrize("dim,wrapped,with_keep", CASES,
                         ids=[f"{d}d_{'karman_wrap' if w else 'plain'}{'_keep' if k else ''}" for d, w, k in CASES])
def test_fit_advection_end_to_end(gpu, dim, wrapped, with_keep, with_tilde):
    n_iters = 5
    wrap = sm.karman_wrap(SIZE[2], eps=0.125) if wrapped else None
    keep = outside_disk if with_keep else None
    prev, tilde = _frozen(dim, with_tilde)
    net_a, net_b = _cuda_net(dim, 64, 1), _cuda_net(dim, 64, 1)
    state_a = siren.AdamState(net_a, lr=1e-4)
    g1, g2 = _gen(), _gen()
    want, counts, clamped, unclamped = _own_loop(net_a, state_a, prev, tilde, wrap, keep, dim, n_iters, g1)
    print(f"counts {counts}; backtracked coordinates clamped {clamped}, not clamped {unclamped}")
    assert clamped > 0 and unclamped > 0, "the case: some backtracked coordinates are clamped and some are not"
    if with_keep:
        assert len(set(counts)) >= 2 and any(c % 32 for c in counts), f"the case: ragged counts, got {counts}"
    else:
        assert counts == [N_SAMPLES] * n_iters
    losses, state_b = pj.fit_advection(net_b, prev, DT, SIZE[dim], n_iters, n_samples=N_SAMPLES, network_tilde=tilde,
                                       wrap=wrap, keep=keep, generator=g2, iters_per_call=2)
    assert losses.shape == (n_iters,) and bool(torch.isfinite(losses).all()) and state_b.step == n_iters
    assert torch.equal(g1.get_state(), g2.get_state()), "the generator consumption of the loop"
    assert same(losses, want), f"losses {losses.tolist()} the loop's {want.tolist()}"
    _same_run(net_a, state_a, net_b, state_b, "fit_advection against the loop")
    # iteration 0 is advection_fit_loss's loss on the same points
    g3 = _gen()
    x = torch.rand(N_SAMPLES, dim, device="cuda", generator=g3)
    for c in range(dim):
        x[..., c] = x[..., c] * (SIZE[dim][2 * c + 1] - SIZE[dim][2 * c]) + SIZE[dim][2 * c]
    x = x if keep is None else x[keep(x)]
    with torch.no_grad():
        first = pj.advection_fit_loss(_cuda_net(dim, 64, 1), prev, x, DT, SIZE[dim], network_tilde=tilde, wrap=wrap)
    assert same(first, losses[0])


# ---- 4. an iteration left without a point ---------------------------------------------------------------------
def test_an_iteration_without_points_is_refused_before_its_block(gpu):
    dim, n = 2, N_SAMPLES
    prev, _ = _frozen(dim, False)
    calls = []

    def keep(x):  # the second block holds iterations 2 and 3: iteration 3 loses every point
        calls.append(int(x.shape[0]))
        mask = outside_disk(x)
        if len(calls) == 2:
            mask[n:] = False
        return mask
    net, state = _cuda_net(dim, 64, 1), siren.AdamState(_cuda_net(dim, 64, 1), lr=1e-4)
    with pytest.raises(ValueError, match=r"iteration 3 without a point"):
        pj.fit_advection(net, prev, DT, SIZE[dim], 5, n_samples=n, keep=keep, state=state, generator=_gen(), iters_per_call=2)
    assert calls == [2 * n, 2 * n] and state.step == 2
    want, want_state = _cuda_net(dim, 64, 1), siren.AdamState(_cuda_net(dim, 64, 1), lr=1e-4)
    pj.fit_advection(want, prev, DT, SIZE[dim], 2, n_samples=n, keep=outside_disk, state=want_state, generator=_gen(),
                     iters_per_call=2)
    _same_run(want, want_state, net, state, "as the first block left them")


# ---- 5. early stop ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _free_run(n_iters=5):
    prev, _ = _frozen(2, False)
    losses, _ = pj.fit_advection(_cuda_net(2, 64, 1), prev, DT, SIZE[2], n_iters, n_samples=N_SAMPLES, keep=outside_disk,
                                 generator=_gen(31), iters_per_call=n_iters)
    return losses.cpu().numpy()


@pytest.mark.parametrize("where", ["last_of_a_block", "middle_of_a_block"])
def test_fit_advection_early_stop(gpu, where):
    """The threshold is the least of the free run's first four losses, at iteration `at`: the run is
    deterministic, so it stops there.  iters_per_call = at + 1 makes that the last iteration of the
    first block (status[0] equals the block's length), at + 2 one inside it."""
    n_iters = 5
    free = _free_run(n_iters)
    at = int(np.argmin(free[:4]))
    thr = float(free[at])
    assert int(np.flatnonzero(free <= np.float32(thr))[0]) == at
    per_call = at + 1 if where == "last_of_a_block" else at + 2
    prev, _ = _frozen(2, False)
    net, g1 = _cuda_net(2, 64, 1), _gen(31)
    losses, state = pj.fit_advection(net, prev, DT, SIZE[2], n_iters, n_samples=N_SAMPLES, keep=outside_disk, generator=g1,
                                     early_stop=thr, iters_per_call=per_call)
    assert state.step == at + 1, f"stopped after {state.step} steps, the free run's losses {free.tolist()} say {at + 1}"
    assert losses.shape == (n_iters,) and same(losses[:at + 1], free[:at + 1]), losses.tolist()
    assert bool(torch.isnan(losses[at + 1:]).all()), losses.tolist()
    # the first block was drawn whole, before its run, and nothing after the stop
    g2 = _gen(31)
    for _ in range(per_call):
        torch.rand(N_SAMPLES, 2, device="cuda", generator=g2)
    assert torch.equal(g1.get_state(), g2.get_state())
    want, want_state = _cuda_net(2, 64, 1), siren.AdamState(_cuda_net(2, 64, 1), lr=1e-4)
    pj.fit_advection(want, prev, DT, SIZE[2], at + 1, n_samples=N_SAMPLES, keep=outside_disk, state=want_state,
                     generator=_gen(31), iters_per_call=per_call)
    _same_run(want, want_state, net, state, f"a run of exactly {at + 1} iterations")


# ---- 6. sanity ---------------------------------------------------------------------------------------------------
def test_two_hundred_iterations_lower_the_loss_on_held_out_points(gpu):
    """Smoke level only: the correctness claims rest on the tests above."""
    dim = 2
    prev, _ = _frozen(dim, False)
    net = _cuda_net(dim, 64, 1)
    x = torch.from_numpy(sm.points(dim, 193, seed=12)).cuda()
    back = x - siren.eval(prev, x) * DT
    back = torch.stack([back[..., c].clamp(min=SIZE[dim][2 * c], max=SIZE[dim][2 * c + 1]) for c in range(dim)], dim=-1)
    target = siren.eval(prev, back)
    before = float(siren.fit(net, x, target, grads=False))
    losses, state = pj.fit_advection(net, prev, DT, SIZE[dim], 200, n_samples=193, generator=_gen(5))
    after = float(siren.fit(net, x, target, grads=False))
    print(f"loss on the held-out points before {before:.6e} after 200 iterations {after:.6e}")
    assert state.step == 200 and bool(torch.isfinite(losses).all()) and after < before
