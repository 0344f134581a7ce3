"""Multi-process CPU tests (gloo, world_size 2) of the view-sharded data-parallel path:
replicas stay bit-identical and equal a single-process run that averages both views' gradients each step."""
import os
import socket

import pytest

import torch
import torch.distributed as dist
import torch.multiprocessing as mp


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


class TinyGaussians:
    """Duck-types the part of the reference's GaussianModel the DP hooks touch: parameter groups, Adam with
    eps=1e-15, step() = optimizer.step(); optimizer.zero_grad() (gaussian_model.py:465-497)."""

    def __init__(self, seed=0, P=257):
        g = torch.Generator().manual_seed(seed)
        self.xyz = torch.nn.Parameter(torch.randn(P, 3, generator=g))
        self.sh = torch.nn.Parameter(torch.randn(P, 16, 3, generator=g))
        self.opacity = torch.nn.Parameter(torch.randn(P, 1, generator=g))
        self.unused = torch.nn.Parameter(torch.randn(P, 2, generator=g))     # gets no gradient: must not deadlock
        self.optimizer = torch.optim.Adam([{"params": [self.xyz], "lr": 1e-2}, {"params": [self.sh], "lr": 2e-3},
                                           {"params": [self.opacity], "lr": 5e-2}, {"params": [self.unused], "lr": 1e-2}],
                                          lr=0.0, eps=1e-15)

    def parameters(self):
        return [self.xyz, self.sh, self.opacity, self.unused]

    def step(self):
        self.optimizer.step()
        self.optimizer.zero_grad()


def _loss(model, view):
    g = torch.Generator().manual_seed(1000 + view)
    w = torch.randn(257, 3, generator=g)
    return ((model.xyz * w).sum(-1).tanh() * torch.sigmoid(model.opacity[:, 0])).sum() + \
        (model.sh.mean(1) * w).square().sum() * 0.1


def _worker(rank, world, port, steps, out_dir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from relightable3dgaussian_amd import dp
    model = TinyGaussians()
    red = dp.GradAllReducer(model.parameters(), bucket_bytes=20_000)      # several buckets
    assert len(red.buckets) >= 2
    dp.patch_model_step(model, red)
    views = dp.shard_views(list(range(2 * steps)), rank, world)
    for i in range(steps):
        _loss(model, views[i]).backward()
        model.step()
    stats = [torch.full((5,), float(rank + 1)) for _ in range(4)] + [torch.tensor([rank * 3.0, 7.0 - rank])]
    dp.reduce_densification_stats(*stats)
    assert torch.equal(stats[0], torch.full((5,), 3.0)) and torch.equal(stats[4], torch.tensor([3.0, 7.0]))
    # the fused path's statistics object: sum of the four accumulators, max of the radii
    from relightable3dgaussian_amd.densify import DensificationStats
    st = DensificationStats(7, torch.device("cpu"))
    st._slab[:4] = float(rank + 1)
    st.max_radii2D.copy_(torch.arange(7.0) * (1 if rank == 0 else -1) + 3 * rank)
    st.all_reduce()
    assert torch.equal(st._slab[:4], torch.full((4, 7), 3.0))
    assert torch.equal(st.max_radii2D, torch.maximum(torch.arange(7.0), 3 - torch.arange(7.0)))
    torch.save([p.detach().clone() for p in model.parameters()], os.path.join(out_dir, "rank%d.pt" % rank))
    dist.destroy_process_group()


def test_two_rank_replicas_identical_and_match_averaged_single_process(tmp_path):
    steps, world = 6, 2
    mp.spawn(_worker, args=(world, _free_port(), steps, str(tmp_path)), nprocs=world, join=True)
    r0 = torch.load(os.path.join(tmp_path, "rank0.pt"))
    r1 = torch.load(os.path.join(tmp_path, "rank1.pt"))
    for a, b in zip(r0, r1):
        assert torch.equal(a, b), "replicas diverged"
    # single process: average the two views' gradients by hand
    model = TinyGaussians()
    for i in range(steps):
        (0.5 * (_loss(model, 2 * i) + _loss(model, 2 * i + 1))).backward()
        model.step()
    for a, b in zip(r0, model.parameters()):
        assert torch.allclose(a, b.detach(), rtol=1e-5, atol=1e-6)


def test_shard_views_partition():
    from relightable3dgaussian_amd import dp
    views = list(range(10))
    parts = [dp.shard_views(views, r, 4) for r in range(4)]
    assert sorted(sum(parts, [])) == views and all(len(p) in (2, 3) for p in parts)


class _FakeTracer:
    """Stands in for bvh.RayTracer on CPU: visibility is a deterministic function of the ray alone, so the sharded
    result can be compared with the single-process one exactly."""

    def __init__(self, means3D, scales, rotations):
        self.calls = 0

    def trace_visibility(self, rays_o, rays_d, means3D, symm_inv, opacity, normals):
        self.calls += rays_o.shape[0]
        v = torch.sin(7.0 * (rays_o * rays_d).sum(-1) + 3.0 * rays_d[..., 0])
        return {"visibility": torch.where(v > 0, 0.9 + 0.1 * v, torch.zeros_like(v)).unsqueeze(-1)}


def _visibility_inputs(P):
    g = torch.Generator().manual_seed(5)
    xyz = torch.randn(P, 3, generator=g)
    scales = torch.rand(P, 3, generator=g) * 0.05 + 0.01
    rot = torch.nn.functional.normalize(torch.randn(P, 4, generator=g), dim=-1)
    opacity = torch.rand(P, 1, generator=g)
    normal = torch.nn.functional.normalize(torch.randn(P, 3, generator=g), dim=-1)
    return xyz, scales, rot, opacity, normal


def _visibility_worker(rank, world, port, P, K, out_dir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from relightable3dgaussian_amd.train_step import update_visibility
    vis, dirs, areas, tracer = update_visibility(*_visibility_inputs(P), K, tracer_cls=_FakeTracer)
    torch.save(dict(vis=vis, dirs=dirs, areas=areas, traced=tracer.calls), os.path.join(out_dir, "vis%d.pt" % rank))
    dist.destroy_process_group()


def test_sharded_update_visibility_equals_single_process(tmp_path):
    """ray bundles sharded over ranks against a replicated BVH + one all-gather.  Ragged split (P not a
    multiple of the world size, chunk boundaries inside a rank's block), world 2 and 3."""
    from relightable3dgaussian_amd.train_step import update_visibility
    P, K = 103, 30                       # K=30 -> 2 chunks of 51 rows (+1)
    want = update_visibility(*_visibility_inputs(P), K, tracer_cls=_FakeTracer)
    assert want[3].calls == P
    for world in (2, 3):
        d = tmp_path / ("w%d" % world)
        d.mkdir()
        mp.spawn(_visibility_worker, args=(world, _free_port(), P, K, str(d)), nprocs=world, join=True)
        traced = 0
        for r in range(world):
            got = torch.load(os.path.join(d, "vis%d.pt" % r))
            assert torch.equal(got["vis"], want[0]) and got["vis"].shape == (P, K, 1)
            assert torch.equal(got["dirs"], want[1]) and torch.equal(got["areas"], want[2])
            traced += got["traced"]
        assert traced == P               # every bundle traced exactly once across the ranks


# --- bench.py --gpus N launches N ranks itself (the flag used to be parsed and ignored) -------------------
def _run_bench(extra, env=None, timeout=240):
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    e = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        e.pop(k, None)
    e.update(env or {})
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py")] + extra, capture_output=True, text=True,
                       timeout=timeout, env=e, stdin=subprocess.DEVNULL, cwd="/tmp")
    lines = [x for x in r.stdout.splitlines() if x.startswith("{")]
    return r, (json.loads(lines[-1]) if lines else None)


def test_bench_gpus_flag_starts_that_many_ranks():
    """`python bench.py --gpus 2` (the driver's literal command shape, no launcher around it) must start 2 ranks,
    rendezvous on 127.0.0.1, reduce over ranks and print ONE line with n_gpus 2.  No GPU here: the kernels are skipped
    (--plumbing-only); tests/test_fused_dp_gpu.py runs the same command with the kernels on the GPU box."""
    r, doc = _run_bench(["--gpus", "2", "--steps", "3", "--warmup", "1", "--plumbing-only"],
                        env={"R3DG_DIST_BACKEND": "gloo"})
    assert r.returncode == 0, r.stderr[-2000:]
    assert doc is not None and doc["n_gpus"] == 2 and doc["steps"] == 3
    assert sum(1 for x in r.stdout.splitlines() if x.startswith("{")) == 1


def test_bench_gpus_flag_fails_loudly_without_enough_devices():
    import torch
    if torch.cuda.device_count() >= 2:
        pytest.skip("this box has the devices")
    r, doc = _run_bench(["--gpus", "2", "--steps", "1", "--warmup", "0"], env={"R3DG_DIST_BACKEND": "nccl"})
    assert r.returncode != 0 and doc is None
    assert "--gpus 2 requested" in (r.stderr + r.stdout)


def test_bench_rejects_world_size_mismatch():
    r, doc = _run_bench(["--gpus", "4", "--plumbing-only"], env={"WORLD_SIZE": "1", "RANK": "0"})
    assert r.returncode != 0 and "WORLD_SIZE" in (r.stderr + r.stdout)


def test_bench_config_presets_fill_in_what_the_command_line_left_open(monkeypatch):
    """`--config teaser8` = BASELINE configs[4] (2M Gaussians, 1800x700, relight at sample_num 384); `--config dtu4` = configs[3]
    (1600x1200, run_dtu.sh objective, sample_num 32).  A flag given on the command line wins over the preset, in either order
    and in both spellings."""
    import importlib.util
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(root, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "8", "--config", "teaser8"])
    a = bench.parse()
    assert (a.points, a.width, a.height, a.relight_samples, a.gpus, a.sample_num) == (2_000_000, 1800, 700, 384, 8, 64)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--points=500000", "--config", "teaser8", "--relight-samples", "128"])
    a = bench.parse()
    assert (a.points, a.width, a.relight_samples) == (500_000, 1800, 128)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--config", "dtu4", "--gpus", "4"])
    a = bench.parse()
    assert (a.width, a.height, a.objective, a.sample_num, a.points, a.gpus) == (1600, 1200, "syn4", 32, 300_000, 4)
    monkeypatch.setattr(sys, "argv", ["bench.py"])
    a = bench.parse()
    assert a.config is None and (a.points, a.res, a.sample_num, a.stage) == (300_000, 800, 64, 2)


def test_bench_full_and_dump_outputs_flags(monkeypatch):
    """A plain run leaves the side measurements out (`--full` is off by default); `--dump-outputs DIR` names the directory."""
    import importlib.util
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(root, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench.parse()
    assert a.full is False and a.dump_outputs is None and (a.steps, a.warmup) == (7, 2)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "out/dir"])
    a = bench.parse()
    assert a.full is True and a.dump_outputs == "out/dir"


def test_bench_dump_outputs_writes_fixed_samples(tmp_path):
    """bench_core.dump_outputs: float32 / float64 files; per-Gaussian rows and image pixels of a large step reduced to the same
    seeded samples on every call (their indices are written too); small arrays whole; never more than DUMP_LIMIT bytes."""
    import numpy as np
    from relightable3dgaussian_amd import bench_core as bc
    P, H, W = bc.DUMP_ROWS + 1000, 600, 500                 # 300 000 pixels: more than DUMP_PIXELS
    g = torch.Generator().manual_seed(0)
    pairs = [("num_rendered", 1234), ("n_contrib", torch.randint(0, 9, (H, W), dtype=torch.int32, generator=g)),
             ("image", torch.rand(3, H, W, generator=g)), ("radii", torch.randint(0, 5, (P,), dtype=torch.int32, generator=g)),
             ("loss", torch.tensor(0.25, dtype=torch.float64)), ("grad_xyz", torch.rand(P, 3, generator=g)),
             ("grad_env", torch.rand(4, 8, 3, generator=g))]
    for d in ("a", "b"):
        bc.dump_outputs(str(tmp_path / d), pairs, P, H, W)
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted([n + ".npy" for n, _ in pairs] + ["gaussian_index.npy", "pixel_index.npy"])
    z = {n[:-4]: np.load(os.path.join(tmp_path, "a", n)) for n in names}
    for n in names:
        assert np.array_equal(z[n[:-4]], np.load(os.path.join(tmp_path, "b", n)))
    rows, pix = z["gaussian_index"].astype(np.int64), z["pixel_index"].astype(np.int64)
    assert len(rows) == bc.DUMP_ROWS and len(set(rows)) == bc.DUMP_ROWS and rows.max() < P
    assert len(pix) == bc.DUMP_PIXELS and len(set(pix)) == bc.DUMP_PIXELS and pix.max() < H * W
    assert z["image"].dtype == np.float32 and z["image"].shape == (3, bc.DUMP_PIXELS)
    assert np.array_equal(z["image"], pairs[2][1].reshape(3, -1).numpy()[:, pix])
    assert z["n_contrib"].dtype == np.float64 and np.array_equal(z["n_contrib"], pairs[1][1].reshape(-1).numpy()[pix])
    assert z["grad_xyz"].dtype == np.float32 and np.array_equal(z["grad_xyz"], pairs[5][1].numpy()[rows])
    assert np.array_equal(z["radii"], pairs[3][1].numpy()[rows].astype(np.float64))
    assert z["grad_env"].shape == (4, 8, 3) and z["loss"].dtype == np.float64 and float(z["loss"]) == 0.25
    assert float(z["num_rendered"]) == 1234
    with pytest.raises(RuntimeError):
        bc.dump_outputs(str(tmp_path / "c"), [("big", torch.zeros(bc.DUMP_LIMIT // 4 + 1))], P, H, W)
