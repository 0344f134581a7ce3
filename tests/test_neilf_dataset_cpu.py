"""The NeILF-format reader, the resolution rule and the two new yardsticks without a GPU: dataset.read_neilf_scene / cameras_of /
initial_points_neilf / unpack_masked_reference / resize_reference against what the reference's own readNeILFInfo, loadCam and Camera
produced on CPU (tests/golden/neilf_dataset_reference.npz, written by tests/golden/make_neilf_golden.py), the scale / target-size
table of `--resolution`, what the reader and the store refuse, layout detection, the driver's flags, the C ABI declarations and
argument checks of r3dg_view_unpack_masked / r3dg_view_resize, and the new kernels' code objects."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "neilf_dataset_reference.npz")
RESOLUTIONS = (1, 2, 5)                       # loadCam's `resolution`: 5 is a target WIDTH (scales 9 / 5 and 7 / 5)
PROTOTYPES = ("""\
int r3dg_view_unpack_masked(void* stream, int width, int height, const uint8_t* d_pixels, const uint8_t* d_mask_bytes,
                            float* d_image, float* d_mask);
""", """\
int r3dg_view_resize(void* stream, int width, int height, int channels, const uint8_t* d_pixels, const uint8_t* d_mask_bytes,
                     const float* d_background, int out_width, int out_height, float* d_image, float* d_mask);
""")


def write_neilf_scene(root, indexes, flags, file_names, pixels, masks, extrinsics, focal, ppt, bbox, ply_bytes=None):
    """A NeILF-format directory: <root>/inputs/{sfm_scene.json, images/*, pmasks/*, model/sparse.ply}.  pixels[i]: [H,W,3] uint8 (or
    None: no file, for a camera that is not valid); masks[i]: [H,W] uint8 or None (no mask file)."""
    from PIL import Image
    inputs = os.path.join(root, "inputs")
    for sub in ("images", "pmasks", "model"):
        os.makedirs(os.path.join(inputs, sub), exist_ok=True)
    images, paths = {}, {}
    for i, index in enumerate(indexes):
        paths[str(index)] = "images/" + file_names[i]
        images[str(index)] = {"flg": int(flags[i]), "camera": {
            "intrinsic": {"focal": [float(focal[i][0]), float(focal[i][1])], "ppt": [float(ppt[i][0]), float(ppt[i][1])]},
            "extrinsic": [float(x) for x in np.asarray(extrinsics[i], np.float64).reshape(-1)]}}
        if pixels[i] is not None:
            Image.fromarray(np.asarray(pixels[i])).save(os.path.join(inputs, "images", file_names[i]))
        if masks[i] is not None:
            Image.fromarray(np.asarray(masks[i]), mode="L").save(
                os.path.join(inputs, "pmasks", os.path.splitext(file_names[i])[0] + ".png"))
    scene = {"bbox": {"transform": [float(x) for x in np.asarray(bbox, np.float64).reshape(-1)]},
             "image_path": {"file_paths": paths}, "camera_track_map": {"images": images}}
    with open(os.path.join(inputs, "sfm_scene.json"), "w") as fh:
        json.dump(scene, fh)
    if ply_bytes is not None:
        with open(os.path.join(inputs, "model", "sparse.ply"), "wb") as fh:
            fh.write(bytes(ply_bytes))
    return root


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def scene_from_golden(z, root):
    """The directory the golden file was made from."""
    n = len(z["indexes"])
    pixels = [z["pixels_%02d" % i] if ("pixels_%02d" % i) in z.files else None for i in range(n)]
    masks = [z["maskbytes_%02d" % i] if ("maskbytes_%02d" % i) in z.files else None for i in range(n)]
    return write_neilf_scene(str(root), [str(s) for s in z["indexes"]], z["flags"], [str(s) for s in z["file_names"]], pixels, masks,
                             z["extrinsics"], z["focal"], z["ppt"], z["bbox"], z["sparse_ply_bytes"].tobytes())


def _bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- 1. the reader ----------------------------------------------------------------------------------------------------------------
def test_reader_follows_load_cams_from_scene(golden, tmp_path):
    from relightable3dgaussian_amd import dataset, synthetic
    z = golden
    root = scene_from_golden(z, tmp_path)
    train, test = dataset.read_neilf_scene(root, eval=True)
    names = lambda rs: [r["name"] for r in rs]
    assert names(train) == list(z["train_names"]) and names(test) == list(z["test_names"])
    assert [r["uid"] for r in test] == ["2", "12"] and len(train) == 12
    assert "14" not in [r["uid"] for r in train + test] and int(z["flags"][14]) != 2              # the camera with flg != 2
    everything, nothing = dataset.read_neilf_scene(root, eval=False)
    assert names(everything) == list(z["all_names"]) and nothing == [] and len(everything) == 14
    for split, records in (("train", train), ("test", test)):
        for j, r in enumerate(records):
            key = "%s_%02d_" % (split, j)
            assert r["R"].dtype == np.float64 and r["T"].dtype == np.float64
            np.testing.assert_allclose(r["R"], z[key + "R"], rtol=0, atol=1e-12)
            np.testing.assert_allclose(r["T"], z[key + "T"], rtol=0, atol=1e-12)
            assert (r["FovX"], r["FovY"]) == tuple(z[key + "fov"])
            assert (r["fx"], r["fy"], r["cx"], r["cy"]) == tuple(z[key + "intrinsics"])
            assert (r["height"], r["width"]) == tuple(z[key + "size"]) and os.path.exists(r["path"])
            # the mask-path rule: inputs/pmasks/<basename>.png, only when that file exists
            has = bool(z[key + "has_mask"])
            assert (r["mask_path"] is not None) == has
            if has:
                assert r["mask_path"] == os.path.join(root, "inputs", "pmasks", r["name"] + ".png") and os.path.exists(r["mask_path"])
    assert any(r["mask_path"] is None for r in train) and any(r["mask_path"] is not None for r in train)
    assert {(r["height"], r["width"]) for r in train} == {(6, 9), (5, 7)}
    assert all(r["fx"] != r["fy"] and r["cx"] != r["width"] / 2 for r in train)
    cams = dataset.cameras_of(train)
    extent, _ = synthetic.cameras_extent(cams)
    assert abs(extent - float(z["extent"])) <= 1e-5 * float(z["extent"])


@pytest.mark.parametrize("resolution", RESOLUTIONS)
def test_cameras_carry_the_matrices_of_the_reference_camera_bit_for_bit(golden, tmp_path, resolution):
    from relightable3dgaussian_amd import dataset
    z = golden
    root = scene_from_golden(z, tmp_path)
    for split, records in zip(("train", "test"), dataset.read_neilf_scene(root, eval=True)):
        scales = [dataset.view_scale(resolution, r["width"]) for r in records]
        sizes = [dataset.target_size(r["height"], r["width"], s) for r, s in zip(records, scales)]
        cams = dataset.cameras_of(records, sizes, None, scales)
        for j, (cam, r) in enumerate(zip(cams, records)):
            key = "%s_%02d_r%d_" % (split, j, resolution)
            assert (cam.image_height, cam.image_width) == tuple(z[key + "size"])
            fx, fy, cx, cy = z[key + "intrinsics"]
            assert (cam.cx, cam.cy) == (cx, cy)
            assert (r["fx"] / scales[j], r["fy"] / scales[j]) == (fx, fy)
            proj = dataset._projection_center_shift(0.01, 100.0, cx, cy, fx, fy, cam.image_width, cam.image_height).transpose(0, 1)
            assert np.array_equal(_bits(proj), _bits(z[key + "projection_matrix"]))
            assert np.array_equal(_bits(cam.world_view_transform), _bits(z[key + "world_view_transform"]))
            assert np.array_equal(_bits(cam.full_proj_transform), _bits(z[key + "full_proj_transform"]))
            # the centre is a row of a float32 LU inverse (torch.inverse): which way its last bit rounds depends on the CPU's
            # LAPACK kernels (seen: one ulp between two machines on the same inputs), so it is held to the rounding scale of that
            # inverse, cond * 2^-24 * |centre| = 4.5e-6 < 5e-6 for these cameras (|centre| < 3, cond < 25): test_dataset_cpu's bound
            np.testing.assert_allclose(cam.camera_center.numpy(), z[key + "camera_center"], rtol=0, atol=5e-6)
            assert (cam.FoVx, cam.FoVy) == (r["FovX"], r["FovY"])                        # (the angles are not rescaled)


def test_records_without_fx_behave_as_before(golden):
    from relightable3dgaussian_amd import dataset, synthetic
    r = dict(name="a", path="a.png", R=np.eye(3), T=np.array([0.0, 0.0, 4.0]), FovX=0.7, FovY=0.5, width=8, height=6)
    cam = dataset.cameras_of([r], [(3, 4)], None, [2])[0]
    want = synthetic._projection(0.01, 100.0, 0.7, 0.5).transpose(0, 1)
    assert (cam.cx, cam.cy, cam.image_height, cam.image_width) == (2.0, 1.5, 3, 4)
    assert torch.equal(cam.full_proj_transform, cam.world_view_transform.unsqueeze(0).bmm(want.unsqueeze(0)).squeeze(0))


def test_initial_points_neilf_writes_the_rescaled_ply_byte_for_byte(golden, tmp_path):
    from relightable3dgaussian_amd import dataset
    z = golden
    root = scene_from_golden(z, tmp_path)
    points, colors, normals = dataset.initial_points_neilf(root)
    with open(os.path.join(root, "inputs", "model", "sparse_bbx_scale.ply"), "rb") as fh:
        assert fh.read() == z["scaled_ply_bytes"].tobytes()
    for got, want in ((points, z["ply_points"]), (colors, z["ply_colors"]), (normals, z["ply_normals"])):
        assert got.shape == (50, 3) and got.dtype == want.dtype and np.array_equal(got, want)


# ---- 2. pixels --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("resolution", RESOLUTIONS)
def test_yardsticks_are_the_reference_images_and_masks_bit_for_bit(golden, tmp_path, resolution):
    from relightable3dgaussian_amd import dataset
    z = golden
    root = scene_from_golden(z, tmp_path)
    seen_mask = set()
    for split, records in zip(("train", "test"), dataset.read_neilf_scene(root, eval=True)):
        for j, r in enumerate(records):
            from PIL import Image
            px = np.array(Image.open(r["path"]))
            if r["mask_path"] is None:
                image, mask = dataset.unpack_reference(px, (0, 0, 0), clamp=False)
            else:
                mb = np.array(Image.open(r["mask_path"]).convert("L"))
                seen_mask |= set(np.unique(mb).tolist())
                image, mask = dataset.unpack_masked_reference(px, mb, clamp=False)
                clamped = dataset.unpack_masked_reference(px, mb)
                assert torch.equal(clamped[0], image.clamp(0, 1)) and set(np.unique(mask.numpy()).tolist()) <= {0.0, 1.0}
            scale = dataset.view_scale(resolution, r["width"])
            if scale != 1:
                image, mask = dataset.resize_reference(image, mask, dataset.target_size(r["height"], r["width"], scale))
            key = "%s_%02d_r%d_" % (split, j, resolution)
            assert image.dtype == torch.float32 and tuple(image.shape) == z[key + "original_image"].shape
            assert np.array_equal(_bits(image.clamp(0.0, 1.0)), _bits(z[key + "original_image"])), key
            assert np.array_equal(_bits(mask), _bits(z[key + "image_mask"])), key
    assert {0, 1, 127, 255} <= seen_mask


def test_unpack_masked_reference_refuses_other_shapes():
    from relightable3dgaussian_amd import dataset
    px = np.zeros((4, 5, 3), np.uint8)
    for bad_px, bad_mask in ((np.zeros((4, 5, 4), np.uint8), np.zeros((4, 5), np.uint8)), (px, np.zeros((5, 4), np.uint8)),
                             (px, np.zeros((4, 5), np.float32))):
        with pytest.raises(RuntimeError):
            dataset.unpack_masked_reference(bad_px, bad_mask)


# ---- 3. the resolution rule ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("resolution,width,height,scale,size", [
    (1, 1600, 1200, 1, (1200, 1600)), (2, 1600, 1200, 2, (600, 800)), (4, 1600, 1200, 4, (300, 400)),
    (8, 1600, 1200, 8, (150, 200)), (2, 53, 37, 2, (18, 26)), (-1, 1600, 1200, 1, (1200, 1600)),
    # (1601 / (1601 / 1600) is 1599.99...: loadCam's int() makes the "1.6K" view of a 1601-pixel file 1599 wide)
    (-1, 1601, 1201, 1601 / 1600, (1200, 1599)), (-1, 3200, 2400, 2.0, (1200, 1600)), (-1, 800, 800, 1, (800, 800)),
    (1000, 1600, 1200, 1.6, (750, 1000)), (58, 70, 50, 70 / 58, (41, 58)), (1600, 1600, 1200, 1.0, (1200, 1600))])
def test_scale_and_target_size_are_load_cams(resolution, width, height, scale, size):
    from relightable3dgaussian_amd import dataset
    got = dataset.view_scale(resolution, width)
    assert got == scale and dataset.target_size(height, width, got) == size
    assert size == (int(height / scale), int(width / scale))


@pytest.mark.parametrize("resolution,width", [(1600, 800), (801, 800), (3, 100), (49, 800), (16, 1600)])
def test_upscaling_and_scales_above_16_raise(resolution, width):
    """801 on an 800-pixel file is upscaling; 3 on 100 is a scale of 33; 49 on 800 and 16 on 1600 are scales above 16."""
    from relightable3dgaussian_amd import dataset
    with pytest.raises(RuntimeError, match="upscaling" if resolution > width else "above 16"):
        dataset.view_scale(resolution, width)
    assert dataset.view_scale(50, 800) == 16.0                                            # (16 itself is built)


# ---- 4. what is refused --------------------------------------------------------------------------------------------------------------
def test_an_rgba_file_in_the_neilf_layout_raises_and_names_the_file(golden, tmp_path):
    from PIL import Image
    from relightable3dgaussian_amd import dataset
    root = scene_from_golden(golden, tmp_path)
    bad = os.path.join(root, "inputs", "images", str(golden["file_names"][3]))
    Image.fromarray(np.zeros((5, 7, 4), np.uint8)).save(bad)
    with pytest.raises(RuntimeError, match=os.path.basename(bad)):
        dataset.read_neilf_scene(root, eval=True)
    # ... and so does a store handed a mask file for an RGBA view, before it looks for a device
    with pytest.raises(RuntimeError, match="RGBA"):
        dataset.ViewStore([bad], device="cuda", mask_paths=[bad])
    with pytest.raises(RuntimeError, match="mask_paths"):
        dataset.ViewStore([bad], device="cuda", mask_paths=[None, None])
    with pytest.raises(RuntimeError, match="upscaling"):
        dataset.ViewStore([bad], device="cuda", resolution=20)


def test_layout_detection(golden, tmp_path):
    from relightable3dgaussian_amd import dataset, training
    neilf = tmp_path / "neilf"
    assert dataset.detect_layout(scene_from_golden(golden, neilf)) == "neilf"
    blender = tmp_path / "blender"
    blender.mkdir()
    (blender / "transforms_train.json").write_text("{}")
    assert dataset.detect_layout(str(blender)) == "blender"
    empty = tmp_path / "colmap"
    (empty / "sparse").mkdir(parents=True)
    with pytest.raises(RuntimeError, match=r"transforms_train\.json.*inputs/sfm_scene\.json"):
        dataset.detect_layout(str(empty))
    args = training.build_parser().parse_args(["-s", str(empty), "-m", str(tmp_path / "out")])
    with pytest.raises(RuntimeError, match=r"transforms_train\.json.*inputs/sfm_scene\.json"):
        training.read_scene(args)


# ---- 5. the driver's flags -------------------------------------------------------------------------------------------------------------
def _args(*extra):
    from relightable3dgaussian_amd import training
    return training.build_parser().parse_args(["-s", "/nonexistent/data", "-m", "/nonexistent/out"] + list(extra))


def test_parser_has_the_resolution_flag_with_the_reference_default():
    assert _args().resolution == -1 and _args("-r", "2").resolution == 2 and _args("--resolution", "800").resolution == 800


def test_the_flags_of_the_dtu_run_script_parse_and_reach_the_schedule_and_the_weights():
    from relightable3dgaussian_amd import training
    stage1 = _args("--eval", "--lambda_normal_render_depth", "0.01", "--lambda_normal_smooth", "0.01", "--lambda_mask_entropy", "0.1",
                   "--densify_grad_normal_threshold", "999", "--lambda_depth_var", "1e-2")
    assert training.schedule_of(stage1).densify_grad_normal_threshold == 999.0
    w = training.loss_weights_of(stage1)
    assert (w["normal_render_depth"], w["normal_smooth"], w["mask_entropy"], w["depth_var"]) == (0.01, 0.01, 0.1, 0.01)
    stage2 = _args("--eval", "-c", "chkpnt30000.pth", "--position_lr_init", "0", "--position_lr_final", "0", "--normal_lr", "0",
                   "--sh_lr", "0", "--opacity_lr", "0", "--scaling_lr", "0", "--rotation_lr", "0", "--iterations", "50000",
                   "--lambda_base_color_smooth", "1", "--lambda_roughness_smooth", "0.5", "--lambda_light_smooth", "1",
                   "--lambda_light", "0.01", "--light_init", "3.0", "-t", "neilf", "--sample_num", "32", "--lambda_env_smooth", "0.01",
                   "--env_resolution", "16", "--env_lr", "0.1", "--roughness_lr", "0.01")
    sch = training.schedule_of(stage2)
    assert (sch.position_lr_init, sch.position_lr_final, sch.normal_lr, sch.sh_lr, sch.opacity_lr, sch.scaling_lr,
            sch.rotation_lr) == (0.0,) * 7
    assert (sch.iterations, sch.env_lr, sch.roughness_lr, sch.light_init, stage2.sample_num, stage2.env_resolution) == \
        (50000, 0.1, 0.01, 3.0, 32, 16)
    w2 = training.loss_weights_of(stage2)
    assert (w2["base_color_smooth"], w2["roughness_smooth"], w2["light_smooth"], w2["light"], w2["env_smooth"], w2["pbr"]) == \
        (1.0, 0.5, 1.0, 0.01, 0.01, 1.0)


# ---- 6. the C ABI ------------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_two_entries_and_the_library_checks_their_arguments():
    from relightable3dgaussian_amd import _abi, _lib
    with open(os.path.join(ROOT, "include", "r3dg_hip.h")) as fh:
        header = fh.read()
    assert all(prototype in header for prototype in PROTOTYPES)
    p, i = C.c_void_p, C.c_int
    assert _abi.prototypes["r3dg_view_unpack_masked"] == (i, [p, i, i, p, p, p, p])
    assert _abi.prototypes["r3dg_view_resize"] == (i, [p, i, i, i, p, p, p, i, i, p, p])
    assert _abi.constants["R3DG_VIEW_RESIZE_MAX_SCALE"] == 16
    L = _lib.lib()
    # (nothing is launched: every call is refused or empty; 16 is a 16-byte-aligned address, 1 is not)
    f = L.r3dg_view_unpack_masked
    assert f(None, -1, 8, 1, 1, 1, 1) != 0 and f(None, 8, -1, 1, 1, 1, 1) != 0
    assert b"view_unpack_masked" in L.r3dg_last_error()
    assert f(None, 8, 8, None, 1, 1, 1) != 0 and f(None, 8, 8, 1, None, 1, 1) != 0 and f(None, 8, 8, 1, 1, None, 1) != 0
    assert f(None, 1 << 16, 1 << 15, 1, 1, 1, 1) != 0
    assert f(None, 0, 8, None, None, None, None) == 0 and f(None, 8, 0, None, None, None, None) == 0
    g = L.r3dg_view_resize
    assert g(None, 8, 8, 2, 16, None, 16, 4, 4, 16, None) != 0 and b"view_resize" in L.r3dg_last_error()
    assert g(None, 8, 8, 3, 16, None, None, 9, 4, 16, None) != 0 and g(None, 8, 8, 3, 16, None, None, 4, 9, 16, None) != 0   # upscaling
    assert b"upscaling" in L.r3dg_last_error()
    assert g(None, 8, 8, 3, 16, None, None, 0, 4, 16, None) != 0
    assert g(None, 33, 8, 3, 16, None, None, 2, 4, 16, None) != 0 and b"above 16" in L.r3dg_last_error()                    # 33 / 2
    assert g(None, 8, 33, 3, 16, None, None, 4, 2, 16, None) != 0
    assert g(None, 8, 8, 4, 16, None, None, 4, 4, 16, None) != 0                           # RGBA needs its background
    assert g(None, 8, 8, 4, 16, 16, 16, 4, 4, 16, None) != 0                               # ... and has no mask plane
    assert g(None, 8, 8, 3, None, None, None, 4, 4, 16, None) != 0 and g(None, 8, 8, 3, 16, None, None, 4, 4, None, None) != 0
    assert g(None, 8, 8, 3, 1, None, None, 4, 4, 16, None) != 0 and b"aligned" in L.r3dg_last_error()
    assert g(None, 8, 8, 3, 16, 8, None, 4, 4, 16, None) != 0
    assert g(None, 1 << 16, 1 << 15, 3, 16, None, None, 1 << 15, 1 << 14, 16, None) != 0


# ---- 7. kernel resources ---------------------------------------------------------------------------------------------------------------
def test_the_new_kernels_use_no_scratch_memory(tmp_path):
    """hipcc's metadata for gfx950, read as tests/test_kernel_resources_cpu.py reads it."""
    from relightable3dgaussian_amd import build as B, kernel_sources
    from tests.test_kernel_resources_cpu import _metadata
    if not os.path.exists(B.HIPCC):
        pytest.skip("no hipcc")
    assert B.EXTRA["view_resize.hip"] == ["-ffp-contract=off"]
    files = kernel_sources.kernel_files()
    assert files["view_unpack_masked_kernel"] == "view_store.hip" and files["view_resize_kernel"] == "view_resize.hip"
    _, kernels = _metadata("view_store.hip", str(tmp_path))
    masked = {k: v for k, v in kernels.items() if "view_unpack_masked_kernel" in k}
    _, kernels = _metadata("view_resize.hip", str(tmp_path))
    resize = {k: v for k, v in kernels.items() if "view_resize_kernel" in k}
    assert len(masked) == 1 and len(resize) == 3, (masked, resize)
    for found in (masked, resize):
        assert all(scratch == 0 for scratch, _ in found.values()), found
        assert all(0 < vgprs <= 128 for _, vgprs in found.values()), found
