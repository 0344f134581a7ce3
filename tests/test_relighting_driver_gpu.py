"""python -m relightable3dgaussian_amd.relighting on a config directory made of the reference-written PLY fixtures: the PNG files
it writes against RelightRenderer.frame called directly on compose.assemble of the same config, byte for byte (both sides run
the same kernels on the same composite; the forward is bit-repeatable), the --bake run, and the refusals."""
import json
import math
import os
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
W, H, K = 64, 48, 16
CAPTURES = ("pbr_env", "normal", "base_color")


def _w2c(eye):
    from relightable3dgaussian_amd import synthetic
    return synthetic.look_at_camera(eye, width=W, height=H).world_view_transform.t().contiguous().numpy()


def _rot_z(a):
    return [[math.cos(a), -math.sin(a), 0.0], [math.sin(a), math.cos(a), 0.0], [0.0, 0.0, 1.0]]


@pytest.fixture(scope="module")
def config(tmp_path_factory):
    root = tmp_path_factory.mktemp("relighting")
    cfg = root / "config"
    cfg.mkdir()
    stage2, stage1 = (os.path.join(GOLDEN, "ply_reference_%s.ply" % t) for t in ("stage2", "stage1"))
    a, b, c = np.eye(4), np.eye(4), np.eye(4)
    a[:3, 3] = [-0.6, 0.0, 0.0]
    b[:3, :3] = 0.7 * np.array(_rot_z(0.8))
    b[:3, 3] = [0.9, 0.4, 0.1]
    c[:3, :3] *= 1.5
    c[:3, 3] = [0.0, 0.0, -1.2]
    (cfg / "transform.json").write_text(json.dumps({
        "first": {"path": stage2, "transform": a.tolist()},
        "ground": {"path": stage1, "transform": c.reshape(-1).tolist()},
        "second": {"path": stage2, "transform": b.tolist()}}))
    eyes = [(4.0, 0.5, 1.5), (3.0, 2.5, 1.0), (0.5, 4.0, 2.0)]
    keys = ["0", "1", "2"]
    (cfg / "trajectory.json").write_text(json.dumps({
        "camera": {"height": H, "width": W, "fov": 39.6},
        "trajectory": {k: _w2c(e).reshape(-1).tolist() for k, e in zip(keys, eyes)}}))
    (cfg / "light_transform.json").write_text(json.dumps({"transform": {k: _rot_z(0.4 * i) for i, k in enumerate(keys)}}))
    g = torch.Generator().manual_seed(17)
    env = (torch.rand(16, 32, 3, generator=g) * 2.0).numpy()
    np.save(str(root / "env.npy"), env)
    return types.SimpleNamespace(root=root, cfg=str(cfg), env=str(root / "env.npy"), keys=keys)


def _decode(path):
    from PIL import Image
    return np.asarray(Image.open(path))


def test_main_writes_the_frames_a_direct_render_gives(config):
    from relightable3dgaussian_amd import compose, relight, relighting
    out = str(config.root / "out")
    assert relighting.main(["-co", config.cfg, "-e", config.env, "--output", out, "--capture_list", ", ".join(CAPTURES),
                            "--sample_num", str(K), "-bg", "0.25"]) == 0
    cfg = compose.load_scene_config(config.cfg)
    composite = compose.assemble([p for _, p, _ in cfg.objects], [t for _, _, t in cfg.objects], device=DEV)
    assert composite["xyz"].shape[0] == 97 + 33 + 97
    envmap = relighting.load_envmap(config.env, device=DEV)
    renderer = relight.RelightRenderer(types.SimpleNamespace(**composite), envmap, K, device_visibility=True)
    bg = torch.full((3,), 0.25, device=DEV)
    differing, contrast = {}, {c: 0.0 for c in CAPTURES}
    for key, w2c in cfg.trajectory:
        cam = relighting.camera_of(w2c, W, H).to(DEV)
        res = renderer.frame(cam, bg, env_transform=cfg.light_transforms[key], outputs=CAPTURES)
        want = dict(pbr_env=res["pbr_env"], normal=res["normal"] * 0.5 + 0.5 + (1 - res["opacity"]) * 0.25,
                    base_color=res["base_color"] + (1 - res["opacity"]) * 0.25)
        for c in CAPTURES:
            got = _decode(os.path.join(out, c, "frame_%s.png" % key))
            q = want[c].mul(255).add(0.5).clamp(0, 255).permute(1, 2, 0).to(torch.uint8).cpu().numpy()
            assert got.shape == (H, W, 3) and got.dtype == np.uint8
            n = int((got != q).sum())
            if n:
                differing[(c, key)] = (n, int(np.abs(got.astype(int) - q.astype(int)).max()))
            contrast[c] = max(contrast[c], float(q.std()))
    print("frames that differ from the direct render (bytes, largest step):", differing or "none")
    assert not differing, differing
    # (every capture shows something in some frame; the fixtures' Gaussians are large and overlap, so the traced visibility leaves
    # a view of the far side all but black)
    assert min(contrast.values()) > 1.0, contrast
    assert sorted(os.listdir(out)) == sorted(CAPTURES)
    assert all(sorted(os.listdir(os.path.join(out, c))) == ["frame_%s.png" % k for k in config.keys] for c in CAPTURES)


def test_bake_run_completes_and_writes_frames(config):
    from relightable3dgaussian_amd import relighting
    out = str(config.root / "out_bake")
    assert relighting.main(["-co", config.cfg, "-e", config.env, "--output", out, "--capture_list", "pbr_env,roughness",
                            "--sample_num", str(K), "--bake", "--bake_iterations", "64", "--rotate-sh", "--white_background"]) == 0
    for k in config.keys:
        assert _decode(os.path.join(out, "pbr_env", "frame_%s.png" % k)).shape == (H, W, 3)
        assert _decode(os.path.join(out, "roughness", "frame_%s.png" % k)).shape == (H, W)


def test_render_trajectory_yields_device_frames(config):
    from relightable3dgaussian_amd import compose, relighting
    cfg = compose.load_scene_config(config.cfg)
    composite = compose.assemble([p for _, p, _ in cfg.objects], [t for _, _, t in cfg.objects], device=DEV)
    cams = [relighting.camera_of(w2c, W, H) for _, w2c in cfg.trajectory]
    frames = list(relighting.render_trajectory(composite, relighting.load_envmap(config.env, device=DEV), cams, None,
                                               ("render", "pbr"), sample_num=K))
    assert [i for i, _ in frames] == [0, 1, 2]
    for _, f in frames:
        assert set(f) == {"render", "pbr"} and all(t.is_cuda and tuple(t.shape) == (3, H, W) for t in f.values())


def test_refusals_name_their_reason(config, tmp_path):
    from relightable3dgaussian_amd import relighting
    with pytest.raises(RuntimeError, match=r"\.npy.*\.hdr"):
        relighting.main(["-co", config.cfg, "-e", str(tmp_path / "env.exr"), "--output", str(tmp_path / "o")])
    with pytest.raises(RuntimeError, match="points"):
        relighting.main(["-co", config.cfg, "-e", config.env, "--output", str(tmp_path / "o"), "--capture_list", "points"])
    with pytest.raises(RuntimeError, match="transform.json"):
        relighting.main(["-co", str(tmp_path), "-e", config.env, "--output", str(tmp_path / "o")])
