"""The Blender-format dataset reader and the training driver without a GPU: the C ABI declaration and argument checks of
r3dg_view_unpack, dataset.read_transforms / cameras_of / unpack_reference / initial_points against what the reference's own reader
produced (tests/golden/dataset_reference.npz, written by tests/golden/make_dataset_golden.py), the view pick of train.py:115-119,
the stage-2 position rate, the environment-light checkpoint, the driver's refusal of lambdas it cannot honour, and the unpack
kernels' code objects."""
import ctypes as C
import json
import os
import random

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
PROTOTYPE = """\
int r3dg_view_unpack(void* stream, int width, int height, int channels, const uint8_t* d_pixels, const float* d_background,
                     float* d_image, float* d_mask);
"""
SPLITS = (("rgba", 3, 7, 5, 4), ("rgb", 2, 6, 6, 3))          # name, views, width, height, channels


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "dataset_reference.npz"))


def write_split(root, name, pixels, c2w, fovx):
    from PIL import Image
    os.makedirs(os.path.join(root, name), exist_ok=True)
    frames = []
    for i in range(pixels.shape[0]):
        Image.fromarray(pixels[i]).save(os.path.join(root, name, "r_%d.png" % i))
        frames.append({"file_path": "./%s/r_%d" % (name, i), "transform_matrix": c2w[i].tolist()})
    with open(os.path.join(root, "transforms_%s.json" % name), "w") as fh:
        json.dump({"camera_angle_x": fovx, "frames": frames}, fh)


# ---- 1. the C ABI ---------------------------------------------------------------------------------------------------------------
def test_header_declares_view_unpack_and_the_library_checks_its_arguments():
    from relightable3dgaussian_amd import _abi, _lib
    with open(os.path.join(ROOT, "include", "r3dg_hip.h")) as fh:
        assert PROTOTYPE in fh.read()
    p, i = C.c_void_p, C.c_int
    assert _abi.prototypes["r3dg_view_unpack"] == (i, [p, i, i, i, p, p, p, p])
    L = _lib.lib()
    f = L.r3dg_view_unpack
    # (nothing is launched: every call is refused or empty)
    for channels in (0, 1, 2, 5, -3):
        assert f(None, 8, 8, channels, 1, 1, 1, 1) != 0
    assert b"view_unpack" in L.r3dg_last_error()
    assert f(None, -1, 8, 4, 1, 1, 1, 1) != 0 and f(None, 8, -1, 3, 1, 1, 1, 1) != 0
    assert f(None, 8, 8, 4, None, 1, 1, 1) != 0 and f(None, 8, 8, 4, 1, None, 1, 1) != 0 and f(None, 8, 8, 3, 1, 1, None, 1) != 0
    assert f(None, 1 << 16, 1 << 15, 4, 1, 1, 1, 1) != 0                      # 2^31 pixels: r3dg_relight_quantize's limit
    assert f(None, 0, 8, 4, None, None, None, None) == 0 and f(None, 8, 0, 3, None, None, None, None) == 0
    assert f(None, 0, 8, 2, None, None, None, None) != 0                      # (the channel count is checked first)


# ---- 2. cameras -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,V,W,H,Cn", SPLITS)
def test_read_transforms_and_cameras_follow_the_reference_reader(golden, tmp_path, name, V, W, H, Cn):
    from relightable3dgaussian_amd import dataset, synthetic
    z = golden
    write_split(str(tmp_path), name, z[name + "_pixels"], z[name + "_transform_matrix"], float(z["camera_angle_x"]))
    records = dataset.read_transforms(str(tmp_path), name)
    assert [r["name"] for r in records] == list(z[name + "_names"]) and len(records) == V
    for j, r in enumerate(records):
        assert (r["width"], r["height"]) == (W, H) and os.path.exists(r["path"])
        np.testing.assert_allclose(r["R"], z[name + "_R"][j], rtol=0, atol=1e-12)
        np.testing.assert_allclose(r["T"], z[name + "_T"][j], rtol=0, atol=1e-12)
        assert abs(r["FovX"] - z[name + "_fov"][j, 0]) < 1e-12 and abs(r["FovY"] - z[name + "_fov"][j, 1]) < 1e-9
    cams = dataset.cameras_of(records, [(H, W)] * V, None)
    for j, cam in enumerate(cams):
        assert isinstance(cam, synthetic.SynthCamera) and (cam.image_height, cam.image_width) == (H, W)
        np.testing.assert_allclose(cam.world_view_transform.numpy(), z[name + "_world_view_transform"][j], rtol=0, atol=2e-6)
        np.testing.assert_allclose(cam.full_proj_transform.numpy(), z[name + "_full_proj_transform"][j], rtol=2e-6, atol=2e-6)
        np.testing.assert_allclose(cam.camera_center.numpy(), z[name + "_camera_center"][j], rtol=0, atol=5e-6)
        assert abs(cam.tanfovx - np.tan(0.5 * cam.FoVx)) < 1e-12 and abs(cam.tanfovy - np.tan(0.5 * cam.FoVy)) < 1e-12
        assert cam.cx == W / 2.0 and cam.cy == H / 2.0
    assert dataset.cameras_of(records)[0].image_width == W                      # (sizes default to the records' own)
    extent, translate = synthetic.cameras_extent(cams)
    assert abs(extent - float(z[name + "_extent"])) <= 1e-5 * float(z[name + "_extent"])


def test_fovy_is_the_readers_for_images_that_are_not_square(golden):
    """dataset_readers.py:264 takes the focal length from the HEIGHT and the angle back from the WIDTH: for the 7 x 5 split FovY is
    larger than FovX, and that is what the reference trains with."""
    fovx, fovy = golden["rgba_fov"][0]
    assert fovy > fovx and abs(fovy - 2 * np.arctan(7 / (2 * (5 / (2 * np.tan(fovx / 2)))))) < 1e-12


# ---- 3. pixels ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,V,W,H,Cn", SPLITS)
@pytest.mark.parametrize("bg_name,bg", [("white", (1, 1, 1)), ("black", (0, 0, 0))])
def test_unpack_reference_is_the_readers_image_bit_for_bit(golden, name, V, W, H, Cn, bg_name, bg):
    from relightable3dgaussian_amd import dataset
    z = golden
    pixels = z[name + "_pixels"]
    assert pixels.shape == (V, H, W, Cn) and pixels.dtype == np.uint8
    if Cn == 4:
        alpha = pixels[..., 3]
        assert (alpha == 0).any() and (alpha == 255).any() and ((alpha > 0) & (alpha < 255)).any()
    for j in range(V):
        image, mask = dataset.unpack_reference(pixels[j], bg)
        assert image.dtype == torch.float32 and mask.dtype == torch.float32
        assert tuple(image.shape) == (3, H, W) and tuple(mask.shape) == (1, H, W)
        want_i, want_m = z["%s_image_%s" % (name, bg_name)][j], z["%s_mask_%s" % (name, bg_name)][j]
        assert np.array_equal(image.numpy().view(np.uint32), want_i.view(np.uint32))
        assert np.array_equal(mask.numpy().view(np.uint32), want_m.view(np.uint32))
    # a tensor background is read like a sequence
    a = dataset.unpack_reference(pixels[0], torch.tensor([0.25, 0.5, 0.75]))[0]
    b = dataset.unpack_reference(pixels[0], (0.25, 0.5, 0.75))[0]
    assert torch.equal(a, b)
    with pytest.raises(RuntimeError):
        dataset.unpack_reference(pixels[0][..., :2], bg)


# ---- 4. view order and the stage-2 position rate -----------------------------------------------------------------------------------
@pytest.mark.parametrize("V,seed", [(1, 0), (5, 3), (100, 12345)])
def test_reference_view_order_is_the_stack_of_train_py(V, seed):
    from relightable3dgaussian_amd import dataset
    order = dataset.reference_view_order(V, seed)
    got = [order(it) for it in range(1, 3 * V + 3)]
    rng, stack, want = random.Random(seed), [], []
    for _ in range(3 * V + 2):
        if not stack:
            stack = list(range(V))
        want.append(stack.pop(rng.randint(0, len(stack) - 1)))
    assert got == want
    for b in range(3):
        assert sorted(got[b * V:(b + 1) * V]) == list(range(V))                 # every block of V picks is a permutation
    again = dataset.reference_view_order(V, seed)
    assert [again(it) for it in range(1, V + 1)] == got[:V]


def test_stage2_position_rate_continues_from_the_first_iteration():
    from relightable3dgaussian_amd import train_loop as tl
    sch, extent = tl.Schedule(), 4.7
    a = (sch.position_lr_init * extent, sch.position_lr_final * extent, sch.position_lr_delay_mult, sch.position_lr_max_steps)
    for it in (1, 2, 500, 10_000):
        assert tl.stage2_position_lr(sch, extent, it, 30_000) == tl.position_lr(30_000 + it, *a)
        assert tl.stage2_position_lr(sch, extent, it, 30_000) == pytest.approx(sch.position_lr_final * extent, rel=1e-12)
        assert tl.stage2_position_lr(sch, extent, it) == tl.position_lr(it, *a)                  # the default: today's restart
        assert tl.stage2_position_lr(sch, extent, it, 1000, 0.5) == 0.5 * tl.position_lr(1000 + it, *a)
    assert tl.stage2_position_lr(sch, extent, 1) > 50 * tl.stage2_position_lr(sch, extent, 1, 30_000)
    import inspect
    for fn in (tl.train_stage1, tl.train_stage2):
        assert inspect.signature(fn).parameters["view_order"].default is None
    assert inspect.signature(tl.train_stage2).parameters["first_iteration"].default == 0


# ---- 5. initial points ------------------------------------------------------------------------------------------------------------
def test_initial_points_reads_the_readers_ply_and_draws_the_random_cloud(golden, tmp_path):
    from relightable3dgaussian_amd import dataset
    z = golden
    root = tmp_path / "with_ply"
    root.mkdir()
    (root / "points3d.ply").write_bytes(z["ply_bytes"].tobytes())
    points, colors, normals = dataset.initial_points(str(root), seed=0)
    for got, want in ((points, z["ply_points"]), (colors, z["ply_colors"]), (normals, z["ply_normals"])):
        assert got.shape == (50, 3) and got.dtype == want.dtype and np.array_equal(got, want)
    # what this module writes for the same values is the file storePly wrote, byte for byte
    rgb = np.round(z["ply_colors"] * 255.0)
    dataset.write_points_ply(str(tmp_path / "again.ply"), z["ply_points"], rgb, z["ply_normals"])
    assert (tmp_path / "again.ply").read_bytes() == z["ply_bytes"].tobytes()
    # all-zero normals are replaced by random ones (fetchPly)
    dataset.write_points_ply(str(root / "points3d.ply"), z["ply_points"], rgb, np.zeros((50, 3)))
    n0 = dataset.initial_points(str(root), seed=5)[2]
    assert n0.shape == (50, 3) and (n0 >= 0).all() and (n0 < 1).all() and not np.all(n0 == 0)
    assert np.array_equal(n0, dataset.initial_points(str(root), seed=5)[2])
    # a missing file: the 100 000 random points of dataset_readers.py:288-299, written once, the same for the same seed
    roots = []
    for k, seed in enumerate((7, 7, 8)):
        r = tmp_path / ("empty%d" % k)
        r.mkdir()
        roots.append(dataset.initial_points(str(r), seed=seed))
        assert (r / "points3d.ply").exists()
        again = dataset.initial_points(str(r), seed=seed + 100)                  # (now read from the file)
        assert np.array_equal(again[0], roots[-1][0]) and np.array_equal(again[2], roots[-1][2])
    p = roots[0][0]
    assert p.shape == (100_000, 3) and p.dtype == np.float32 and p.min() >= -1.3 and p.max() <= 1.3
    assert p.min() < -1.29 and p.max() > 1.29
    assert np.array_equal(roots[0][0], roots[1][0]) and np.array_equal(roots[0][1], roots[1][1])
    assert not np.array_equal(roots[0][0], roots[2][0])
    assert np.allclose(np.linalg.norm(roots[0][2], axis=-1), 1.0, atol=1e-5)
    assert np.all(roots[0][1] == np.float32(127.0 / 255.0))                     # SH2RGB(random / 255) * 255 truncates to 127


# ---- 6. the environment-light checkpoint -------------------------------------------------------------------------------------------
def test_env_checkpoint_has_the_layout_of_direct_light_map_capture(tmp_path):
    from relightable3dgaussian_amd import training
    g = torch.Generator().manual_seed(3)
    env = 3.0 * torch.rand(1, 16, 32, 3, generator=g)
    m, v = 0.1 * torch.randn(16 * 32 * 3, generator=g), torch.rand(16 * 32 * 3, generator=g)
    obj = training.env_checkpoint(env, m, v, steps=7, lr=0.1, iteration=32)
    path = str(tmp_path / "env_light_chkpnt32.pth")
    torch.save(obj, path)
    captured, iteration = torch.load(path, map_location="cpu", weights_only=True)
    assert iteration == 32 and isinstance(captured, list) and len(captured) == 2
    assert isinstance(captured[0], torch.nn.Parameter) and torch.equal(captured[0].detach(), env)
    sd = captured[1]
    assert len(sd["param_groups"]) == 1 and sd["param_groups"][0]["name"] == "env" and sd["param_groups"][0]["lr"] == 0.1
    assert sd["param_groups"][0]["eps"] == 1e-15
    # DirectLightMap.training_setup's optimizer accepts it (scene/direct_light_map.py:18-23, create_from_ckpt :41-52)
    fresh = torch.nn.Parameter(torch.zeros(1, 16, 32, 3))
    opt = torch.optim.Adam([{"params": [fresh], "lr": 0.05, "name": "env"}], lr=0.0, eps=1e-15)
    opt.load_state_dict(sd)
    st = opt.state[fresh]
    assert float(st["step"]) == 7.0 and torch.equal(st["exp_avg"].reshape(-1), m) and torch.equal(st["exp_avg_sq"].reshape(-1), v)
    assert opt.param_groups[0]["lr"] == 0.1
    assert torch.equal(training.read_env_checkpoint(path, 16), env)
    with pytest.raises(RuntimeError, match="env_resolution"):
        training.read_env_checkpoint(path, 32)
    # no optimizer state yet
    empty = training.env_checkpoint(env, m, v, steps=0, lr=0.1, iteration=0)
    assert empty[0][1]["state"] == {} and empty[1] == 0


# ---- 7. what the driver refuses ----------------------------------------------------------------------------------------------------
def _args(*extra):
    from relightable3dgaussian_amd import training
    return training.build_parser().parse_args(["-s", "/nonexistent/data", "-m", "/nonexistent/out"] + list(extra))


def test_arguments_carry_the_reference_names_and_defaults():
    from relightable3dgaussian_amd import training, train_loop
    a = _args()
    assert (a.type, a.iterations, a.sample_num, a.env_resolution, a.light_init) == ("render", 30_000, 64, 16, 3.0)
    assert (a.save_interval, a.checkpoint_interval, a.eval, a.white_background, a.checkpoint) == (5000, 5000, False, False, None)
    assert (a.lambda_dssim, a.lambda_pbr, a.lambda_light, a.lambda_env_smooth, a.lambda_depth) == (0.2, 1.0, 0.0, 0.0, 0.0)
    sch = training.schedule_of(_args("--densify_from_iter", "8", "--densification_interval", "4", "--position_lr_init", "0.001",
                                     "--iterations", "24"))
    assert (sch.densify_from_iter, sch.densification_interval, sch.position_lr_init, sch.iterations) == (8, 4, 0.001, 24)
    assert sch.opacity_lr == train_loop.Schedule().opacity_lr
    w = training.loss_weights_of(_args("--lambda_normal_render_depth", "0.01", "--lambda_mask_entropy", "0.1",
                                       "--lambda_depth_var", "0.01", "--lambda_normal_smooth", "0.01"))
    assert (w["normal_render_depth"], w["mask_entropy"], w["depth_var"], w["normal_smooth"]) == (0.01, 0.1, 0.01, 0.01)
    w2 = training.loss_weights_of(_args("-t", "neilf", "--lambda_light", "0.01", "--lambda_env_smooth", "0.01",
                                        "--lambda_normal_render_depth", "0.02", "--lambda_base_color_smooth", "1"))
    assert (w2["pbr"], w2["light"], w2["env_smooth"], w2["normal"], w2["base_color_smooth"]) == (1.0, 0.01, 0.01, 0.02, 1.0)


UNSUPPORTED = [("render", f) for f in ("surface", "opacity", "base_color", "visibility", "visibility_smooth", "depth",
                                       "normal_mvs_depth")] + \
              [("neilf", f) for f in ("surface", "opacity", "base_color", "visibility", "visibility_smooth", "depth",
                                      "normal_mvs_depth", "mask_entropy", "normal_smooth")]


@pytest.mark.parametrize("kind,flag", UNSUPPORTED)
def test_unsupported_lambdas_raise_and_name_the_flag(kind, flag):
    """Before anything is loaded: the dataset directory of these arguments does not exist."""
    from relightable3dgaussian_amd import training
    with pytest.raises(RuntimeError, match=r"--lambda_%s\b" % flag):
        training.train(_args("-t", kind, "--lambda_" + flag, "0.5"))


def test_lambda_dssim_other_than_the_built_in_one_raises():
    from relightable3dgaussian_amd import training
    for kind in ("render", "neilf"):
        with pytest.raises(RuntimeError, match="--lambda_dssim"):
            training.train(_args("-t", kind, "--lambda_dssim", "0.3"))


@pytest.mark.parametrize("mode", ["P", "L", "LA", "I;16"])
def test_an_image_that_is_not_rgb_or_rgba_raises_and_names_the_file(tmp_path, mode):
    from PIL import Image
    from relightable3dgaussian_amd import dataset
    good = str(tmp_path / "good.png")
    Image.fromarray(np.zeros((4, 4, 4), np.uint8)).save(good)
    bad = str(tmp_path / ("bad_%s.png" % mode.replace(";", "")))
    if mode == "I;16":
        Image.fromarray(np.arange(16, dtype=np.uint16).reshape(4, 4)).save(bad)
    else:
        Image.new(mode, (4, 4)).save(bad)
    assert dataset.probe(good) == (4, 4, 4)
    with pytest.raises(RuntimeError, match=os.path.basename(bad)):
        dataset.ViewStore([good, bad], device="cuda")


# ---- 8. kernel resources -----------------------------------------------------------------------------------------------------------
def test_the_unpack_kernels_use_no_scratch_memory(tmp_path):
    """hipcc's metadata for gfx950, read as tests/test_kernel_resources_cpu.py reads it: both instances keep their four pixels in
    registers."""
    from relightable3dgaussian_amd import build as B
    from tests.test_kernel_resources_cpu import _metadata
    if not os.path.exists(B.HIPCC):
        pytest.skip("no hipcc")
    assert B.EXTRA["view_store.hip"] == ["-ffp-contract=off"]
    _, kernels = _metadata("view_store.hip", str(tmp_path))
    found = {k: v for k, v in kernels.items() if "view_unpack_kernel" in k}
    assert len(found) == 2, kernels
    assert all(scratch == 0 for scratch, _ in found.values()), found
    assert all(0 < vgprs <= 128 for _, vgprs in found.values()), found
