"""Multi-GPU pressure projection: one process per GPU, query points sharded by
stride, one all-gather of [p, grad] per projection (RCCL over xGMI when the
process group uses the "nccl" backend; gloo on CPU for tests).

The walk-on-stars solve has no cross-point state (walk_on_stars.h:76-105 runs
every point independently), so ranks exchange nothing while solving.  The RNG of
a point is keyed by its GLOBAL index, so the gathered field is bit-identical for
any world size.  Stride sharding (rank r owns points r, r+W, ...) balances the
spatially varying per-point cost (near-wall points take more steps).
"""
import numpy as np


def shard(n, rank, world):
    """Global indices owned by `rank` (stride sharding) and the padded shard length."""
    idx = np.arange(rank, n, world)
    n_pad = (n + world - 1) // world
    return idx, n_pad


def sharded_projection(solve_local, pts, rank, world, dim, group=None, device=None, force_gather=False):
    """Solve all `pts` ([N, dim], identical on every rank) across `world` ranks.

    solve_local(local_pts, index_base, index_stride) -> (p [n_local], grad [n_local, dim])
    as torch tensors on `device` (any device the process group's backend accepts).
    Returns full (p [N], grad [N, dim]) torch tensors on every rank.  A solve_local that
    returns four tensors (p, grad, p_var [n_local], grad_var [n_local, dim]) -- a solve
    with variance=True -- gets four full tensors back, through the same single collective
    with 2 + 2 * dim columns.  A solve_local that returns channel-major tensors -- p [C, n_local],
    grad [C, n_local, dim] (and the variances alike): several source channels on one set of
    walks -- gets channel-major full tensors back, p [C, N], grad [C, N, dim], still through
    the one collective, whose rows are then C * (1 + dim) columns wide (doubled with variance).

    One code path for every backend: the shard, padded to n_pad rows, goes through ONE
    `all_gather_into_tensor` into a (world * n_pad, 1 + dim) buffer (RCCL over xGMI with
    "nccl", gloo in the CPU tests), and the field is reassembled by a view: global point
    i = j * world + r is row j of rank r's block.  `force_gather` runs the collective even
    at world 1 (exercises the RCCL call on a one-GPU lease).
    """
    import torch
    import torch.distributed as dist

    n = pts.shape[0]
    idx, n_pad = shard(n, rank, world)
    local = pts[rank::world]
    res = tuple(solve_local(local, rank, world))
    if len(res) not in (2, 4):
        raise ValueError(f"solve_local must return (p, grad) or (p, grad, p_var, grad_var), got {len(res)} values")
    res = tuple(torch.as_tensor(t, device=device) for t in res)
    # channel-major results (grad [C, n_local, dim]): point-major rows with the channels side by side
    nch = res[1].shape[0] if res[1].ndim == 3 else 0
    if nch:
        res = tuple(t.reshape(nch, idx.size, -1).permute(1, 0, 2) for t in res)
    # columns: p | grad[dim] (| p_var | grad_var[dim]); with channels p[C] | grad[C][dim] (| ...)
    widths = tuple(w * max(nch, 1) for w in (1, dim) * (len(res) // 2))
    cols = [t.reshape(-1, w) for t, w in zip(res, widths)]
    p = cols[0]
    ncol = sum(widths)
    gathered = world > 1 or force_gather
    # gloo has no device collectives: a gloo group (CPU rehearsal of the N-rank path,
    # ranks sharing one GPU) stages the shard through host memory
    staged = gathered and p.device.type != "cpu" and dist.get_backend(group) == "gloo"
    bdev = torch.device("cpu") if staged else p.device
    send = torch.zeros(n_pad, ncol, dtype=torch.float32, device=bdev)
    c0 = 0
    for t, w in zip(cols, widths):
        send[: idx.size, c0:c0 + w] = t.to(bdev)
        c0 += w
    if gathered:
        buf = torch.empty(world * n_pad, ncol, dtype=torch.float32, device=bdev)
        dist.all_gather_into_tensor(buf, send, group=group)
        if staged:
            buf = buf.to(p.device)
    else:
        buf = send
    # (world, n_pad) blocks -> point order r + world * j; the padded rows (j >= count of
    # rank r) are exactly the indices >= n
    full = buf.view(world, n_pad, ncol).transpose(0, 1).reshape(world * n_pad, ncol)[:n]
    out, c0 = [], 0
    for k, w in enumerate(widths):
        if nch:  # back to channel-major: p [C, N], grad [C, N, dim]
            t = full[:, c0:c0 + w].reshape(n, nch, w // nch).permute(1, 0, 2)
            out.append(t[..., 0].contiguous() if k % 2 == 0 else t.contiguous())
        else:
            out.append(full[:, c0].contiguous() if w == 1 else full[:, c0:c0 + w].contiguous())
        c0 += w
    return tuple(out)


def make_gather(world, dist, n_local, n_pad, dim, dev, torch):
    """bench.py's per-projection gather, on the same collective as sharded_projection:
    every rank sends its shard padded to n_pad rows into a (world * n_pad, 1 + dim)
    buffer with ONE all_gather_into_tensor.  With the gloo backend (CPU-only rehearsal
    of the N-rank path, tests/test_bench_dist.py) the payload is staged through host
    memory; with nccl (RCCL) it stays in HBM.  None at world 1 (nothing to exchange)."""
    if world == 1:
        return None
    staged = dist.get_backend() == "gloo" and dev.type != "cpu"
    bdev = torch.device("cpu") if staged else dev
    send = torch.zeros(n_pad, 1 + dim, dtype=torch.float32, device=bdev)
    buf = torch.empty(world * n_pad, 1 + dim, dtype=torch.float32, device=bdev)

    def gather(p, g):
        send[:n_local, 0] = p.to(bdev)
        send[:n_local, 1:] = g.to(bdev)
        dist.all_gather_into_tensor(buf, send)

    gather.buf = buf
    return gather
