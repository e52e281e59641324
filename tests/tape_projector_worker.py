"""PressureProjector(reuse_walks=True) over a world-1 RCCL group with force_gather, in a fresh
child process (launched by tests/test_gpu_tape.py, as tests/channels_projector_worker.py is for
the channels): the shard is recorded once at global indices, three divs are replayed through the
shard + all_gather_into_tensor path, against the plain unsharded projector.

    python tests/tape_projector_worker.py PORT OUT_DIR
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.join(os.path.dirname(HERE), "neural-monte-carlo-fluid-simulation_amd")]


def main():
    port, out_dir = int(sys.argv[1]), sys.argv[2]
    import numpy as np
    import torch
    import torch.distributed as dist
    import channel_cases as cc
    from wos_amd import engine
    from wos_amd import projection as pj
    from wos_amd import workloads
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    cfg = workloads.karman_config(n_walks=32, n_points=1024)
    scene_cfg = dict(cfg["scene"], boundary=cfg["obj"])
    samples = torch.from_numpy(cfg["points"]).to(dev)
    src = cc.channels(cfg["source"], 4)
    divs = [torch.from_numpy(np.ascontiguousarray(s)).to(dev) for s in (src[0], src[1], src[3])]
    records = []
    real = engine.WosScene.record

    def counted(self, *a, **kw):
        records.append(kw)
        return real(self, *a, **kw)

    engine.WosScene.record = counted
    reuse = pj.PressureProjector(scene_cfg, cfg["solver"], cfg["output"], samples, group=dist.group.WORLD,
                                 force_gather=True, reuse_walks=True)
    plain = pj.PressureProjector(scene_cfg, cfg["solver"], cfg["output"], samples)
    vel, prev = pj.Siren(2, 2, 1, 16).to(dev), pj.Siren(2, 2, 1, 16).to(dev)
    arrays = {}
    for k, div in enumerate(divs):
        got, ref = reuse.solve(div), plain.solve(div)
        assert len(got) == 2 and all(t.is_cuda for t in got) and dist.get_backend() == "nccl"
        for key, a, b in zip(("p", "g"), got, ref):
            arrays[f"{key}{k}"], arrays[f"{key}{k}_ref"] = a.cpu().numpy(), b.cpu().numpy()
        gen = lambda: torch.Generator(device=dev).manual_seed(k)
        arrays[f"loss{k}"] = np.float64(reuse.projection_loss(vel, prev, got[1], 256, generator=gen()).item())
        arrays[f"loss{k}_ref"] = np.float64(plain.projection_loss(vel, prev, ref[1], 256, generator=gen()).item())
    engine.WosScene.record = real
    assert records == [{"index_base": 0, "index_stride": 1}], records
    print(f"PressureProjector reuse_walks over RCCL, world 1, {samples.shape[0]} samples, {len(divs)} divs", flush=True)
    arrays["records"] = np.int64(len(records))
    np.savez(os.path.join(out_dir, "tapeproj.npz"), **arrays)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
