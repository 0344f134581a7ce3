"""OpenEXR views on the GPU (csrc/exr_unpack.hip, relightable3dgaussian_amd/hdr_views.py, the Synthetic4Relight path of
training.py): r3dg_exr_unpack_chunks against exr.decode_reference bit for bit on every case of tests/exr_cases.py and on the
golden crop of the reference's envmap3.exr; r3dg_view_unpack_hdr against the float64 restatement exr_cases.unpack_hdr_reference;
the HdrViewStore's ring; the driver end to end on a `.../Synthetic4Relight/toy` directory the test writes.

Power-branch bound of r3dg_view_unpack_hdr, per element: |device - float64| <= (c_ref + 2) * 2^-24 * 1.055 * x^(1/2.4), where c_ref
is the reference's own float32 arithmetic measured against the same float64 values (tests/test_exr_cpu.py: 2.845 over the golden
crop), one unit is for a device powf that rounds differently from NumPy's and one for contraction of the multiply-subtract.
Measured on the MI355X (profiles/r14_exr_views.txt; the test prints it): the device's maximum is 3.181 units on the golden crop,
2.467 / 2.064 on the half / float noise case, 0.483 / 0.118 on the hand-picked samples, against the bound of 4.845."""
import json
import os

import numpy as np
import pytest
import torch

from tests import exr_cases, exr_writer

pytestmark = pytest.mark.gpu
DEV = "cuda"
CANARY = 0x5A
_CACHE = {}


def _device_decode(path, channels=("R", "G", "B")):
    """The product path on one file: exr.inflate_chunks on the host, r3dg_exr_unpack_chunks on the device -> uint8 tensor holding
    the planar [len(channels),H,W] samples, with 64 canary bytes on either side checked here."""
    from relightable3dgaussian_amd import _abi, _lib, exr
    h = exr.read_header(path)
    keep = exr.channel_indexes(h, channels)
    staging = np.zeros(exr.inflated_nbytes(h), np.uint8)
    table, used = exr.inflate_chunks(path, h, staging)
    tiles = -(-(h.rows_per_chunk * h.width * len(h.channels) * h.bytes_per_sample // 2) // _abi.constants["R3DG_EXR_TILE"])
    d_bytes = torch.from_numpy(staging[:used]).to(DEV)                                 # exact size: nothing to read past its end
    d_table = torch.from_numpy(table).to(DEV)
    d_keep = torch.tensor(keep, dtype=torch.int32, device=DEV)
    d_sums = torch.zeros(len(table) * 2 * tiles, dtype=torch.int32, device=DEV)
    n = len(keep) * h.height * h.width * h.bytes_per_sample
    out = torch.full((n + 128,), CANARY, dtype=torch.uint8, device=DEV)
    _lib.check(_lib.lib().r3dg_exr_unpack_chunks(
        _lib.current_stream(), h.width, h.height, len(h.channels), h.bytes_per_sample, len(table), h.rows_per_chunk,
        d_bytes.data_ptr(), used, d_table.data_ptr(), len(keep), d_keep.data_ptr(), d_sums.data_ptr(), d_sums.numel(),
        out.data_ptr() + 64), "exr_unpack_chunks")
    torch.cuda.synchronize()
    assert bool((out[:64] == CANARY).all()) and bool((out[64 + n:] == CANARY).all()), path
    return out[64:64 + n].clone(), h


def _same_bits(device_bytes, h, want):
    """device planar bytes against decode_reference's [H,W,K] array, on the int16 / int32 views."""
    kind = torch.int16 if h.bytes_per_sample == 2 else torch.int32
    got = device_bytes.cpu().view(kind).reshape(want.shape[2], h.height, h.width)
    want_t = torch.from_numpy(np.ascontiguousarray(exr_cases.bits_of(want).transpose(2, 0, 1)).view(
        np.int16 if h.bytes_per_sample == 2 else np.int32))
    return torch.equal(got, want_t)


# ---- 8. the chunk decode ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,kind,compression", exr_cases.CASES)
def test_exr_unpack_chunks_is_the_decoder_bit_for_bit(tmp_path, name, kind, compression):
    from relightable3dgaussian_amd import exr
    path, _planes, stored_raw = exr_cases.write_case(tmp_path, name, kind, compression)
    if name == "257x33_noise" and compression != "NONE":
        assert stored_raw >= 1
    got, h = _device_decode(path)
    assert _same_bits(got, h, exr.decode_reference(path)), (name, kind, compression)
    if name == "64x40_abgrz":                                                        # every channel, and one asked for twice
        for channels in (("A", "B", "G", "R", "Z"), ("Z", "R", "R")):
            got, h = _device_decode(path, channels)
            assert _same_bits(got, h, exr.decode_reference(path, channels)), channels


def test_exr_unpack_chunks_on_the_references_own_file():
    from relightable3dgaussian_amd import exr
    got, h = _device_decode(exr_cases.GOLDEN_EXR)
    assert (h.width, h.height, h.bytes_per_sample) == (500, 32, 4)
    assert _same_bits(got, h, exr.decode_reference(exr_cases.GOLDEN_EXR))


# ---- 9. the per-iteration launch ---------------------------------------------------------------------------------------------------------
def _unpack_hdr(view, mask_bytes, bg, want_mask=True):
    from relightable3dgaussian_amd import _lib
    _, H, W = view.shape
    d_view = torch.from_numpy(np.ascontiguousarray(view)).to(DEV)
    d_mask_bytes = None if mask_bytes is None else torch.from_numpy(mask_bytes).to(DEV)
    d_bg = torch.tensor(bg, dtype=torch.float32, device=DEV)
    image = torch.full((3, H, W), -7.5, device=DEV)
    mask = torch.full((1, H, W), -7.5, device=DEV) if want_mask else None
    _lib.check(_lib.lib().r3dg_view_unpack_hdr(
        _lib.current_stream(), W, H, int(view.dtype == np.float16), d_view.data_ptr(),
        None if d_mask_bytes is None else d_mask_bytes.data_ptr(), d_bg.data_ptr(), image.data_ptr(),
        None if mask is None else mask.data_ptr()), "view_unpack_hdr")
    torch.cuda.synchronize()
    return image.cpu().numpy(), None if mask is None else mask.cpu().numpy()


def _hdr_inputs():
    if "hdr" not in _CACHE:
        golden = exr_cases.golden_planes()                                             # [3,32,500] float32
        c_ref, _ = exr_cases.reference_deviation(golden)
        inputs = [("golden", golden)]
        for kind in ("HALF", "FLOAT"):
            planes = exr_cases.planes_of("257x33_noise", kind)
            inputs.append(("noise " + kind, np.stack([planes[c] for c in "RGB"])))
        picked = np.tile(exr_cases.HAND_PICKED.reshape(1, 1, -1), (3, 1, 1))
        inputs += [("picked FLOAT", picked), ("picked HALF", picked.astype(np.float16))]
        _CACHE["hdr"] = (c_ref, inputs)
    return _CACHE["hdr"]


@pytest.mark.parametrize("which", range(5))
def test_view_unpack_hdr_against_the_float64_restatement(which):
    c_ref, inputs = _hdr_inputs()
    label, view = inputs[which]
    _, H, W = view.shape
    mask_bytes = np.random.RandomState(9).choice(np.array([0, 1, 255], np.uint8), size=(H, W))
    x = view.astype(np.float32)
    finite = np.isfinite(x)                                                           # (nothing else is masked out of the comparison)
    linear = finite & ~(x > np.float32(0.0031308))
    power = finite & (x > np.float32(0.0031308))
    worst = 0.0
    for bg in ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0)):
        for mb in (mask_bytes, None):
            want_image, want_mask = exr_cases.unpack_hdr_reference(view, mb, bg)
            image, mask = _unpack_hdr(view, mb, bg)
            assert image.dtype == np.float32 and np.array_equal(mask, want_mask.astype(np.float32))
            assert set(np.unique(mask)) <= {0.0, 1.0}
            inside = np.ones((H, W), bool) if mb is None else mb > 0
            assert (image[:, ~inside] == np.float32(bg[0])).all()                     # masked out: the background exactly
            got = image[:, inside].astype(np.float64)
            want = want_image[:, inside]
            xs, lin, pw = x[:, inside], linear[:, inside], power[:, inside]
            # the linear branch: float32(12.92 * x) clamped -- one rounding of a product that is exact in float64
            exact = np.clip((np.float32(12.92) * xs[lin]).astype(np.float32), 0, 1)
            assert np.array_equal(got[lin].astype(np.float32), exact), label
            # both clamp ends, whichever branch: exactly 0 and exactly 1
            ends = np.isfinite(want) & ((want == 0.0) | (want == 1.0)) & np.isfinite(xs)
            assert np.array_equal(got[ends], want[ends]), label
            assert np.array_equal(np.isnan(got), np.isnan(want)), label               # a NaN stays one; inf clamps
            inf = np.isinf(xs)
            assert np.array_equal(got[inf], want[inf])
            if pw.any():
                units = np.abs(got[pw] - want[pw]) / exr_cases.power_unit(xs[pw])
                worst = max(worst, float(units.max()))
                assert (units <= c_ref + 2).all(), (label, float(units.max()), c_ref)
            image_only, no_mask = _unpack_hdr(view, mb, bg, want_mask=False)          # d_mask = NULL
            assert no_mask is None and np.array_equal(image_only.view(np.uint32), image.view(np.uint32))
    print("%s: device maximum %.3f units of 2^-24 * 1.055 * x^(1/2.4) on the power branch (c_ref %.3f, bound %.3f)"
          % (label, worst, c_ref, c_ref + 2))


# ---- 10. the store ---------------------------------------------------------------------------------------------------------------------------
def _toy_views(directory, n, W=40, H=24, masks=True, seed=5):
    """n half ZIP views `<i>_rgb.exr` (+ `<i>_mask.png` of 0 / 1 / 255 bytes) -> (paths, mask paths or None, planar views, masks)."""
    from PIL import Image
    rng = np.random.RandomState(seed)
    os.makedirs(str(directory), exist_ok=True)
    y, x = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    paths, mask_paths, views, mask_arrays = [], [], [], []
    for i in range(n):
        planes = {c: (np.round((1.0 + np.sin(0.3 * x + 0.2 * y + i + j)) * 48) / 64 + (x == 3) * 2.0).astype(np.float16)
                  for j, c in enumerate("RGB")}
        paths.append(os.path.join(str(directory), "%03d_rgb.exr" % i))
        exr_writer.write_exr(paths[-1], planes, "ZIP")
        views.append(np.stack([planes[c] for c in "RGB"]))
        grey = rng.choice(np.array([0, 1, 255], np.uint8), size=(H, W), p=[0.3, 0.1, 0.6])
        mask_arrays.append(grey)
        if masks:
            mask_paths.append(os.path.join(str(directory), "%03d_mask.png" % i))
            Image.fromarray(grey).save(mask_paths[-1])
    return paths, (mask_paths if masks else None), views, mask_arrays


def _matches(pair, view, mask_bytes, bg, c_ref):
    want_image, want_mask = exr_cases.unpack_hdr_reference(view, mask_bytes, bg)
    image, mask = pair[0].cpu().numpy().astype(np.float64), pair[1].cpu().numpy()
    tolerance = (c_ref + 2) * np.broadcast_to(exr_cases.power_unit(view.astype(np.float32)), want_image.shape)
    return bool((np.abs(image - want_image) <= tolerance).all()) and np.array_equal(mask, want_mask.astype(np.float32))


def test_hdr_view_store_serves_every_view_from_its_ring(tmp_path):
    from relightable3dgaussian_amd import hdr_views
    c_ref, _ = _hdr_inputs()
    paths, mask_paths, views, masks = _toy_views(tmp_path / "masked", 4)
    store = hdr_views.HdrViewStore(paths, DEV, slots=2, mask_paths=mask_paths)
    assert store.sizes == [(24, 40)] * 4 and store.scales == [1] * 4 and store.has_masks and store.unpack_launches == 4
    assert store.resident_nbytes() == 4 * 7 * 24 * 40 and store.float_nbytes() == 4 * 16 * 24 * 40       # (6 + 1 bytes per pixel;
    assert all(v.offset % 16 == 0 and v.mask_offset % 16 == 0 for v in store.views)                      # 960 pixels need no padding)
    assert set(store.load_seconds) == {"inflate", "upload", "inflate_cpu"} and 1 <= store.workers <= 8
    for bg in ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0)):
        for v in range(4):
            before = store.launches
            for got in (store.fetch(v, torch.tensor(bg, device=DEV)), store.fetch(v, bg)):
                assert _matches(got, views[v], masks[v], bg, c_ref), (v, bg)
            assert store.launches == before + 2                                      # one launch per fetch
    # the ring: a pair survives slots - 1 further fetches and is overwritten by the slots-th
    bg = (1.0, 1.0, 1.0)
    i0, m0 = store.fetch(0, bg)
    kept0, keptm0 = i0.clone(), m0.clone()
    i1, _ = store.fetch(1, bg)
    assert i1.data_ptr() != i0.data_ptr() and torch.equal(i0, kept0) and torch.equal(m0, keptm0)
    i2, m2 = store.fetch(2, bg)
    assert i2.data_ptr() == i0.data_ptr() and m2.data_ptr() == m0.data_ptr() and not torch.equal(i0, kept0)
    assert _matches((i0, m0), views[2], masks[2], bg, c_ref)
    # the sequences of the training loops: masks[v] behind images[v] is the mask of that same launch
    images, mask_seq = store.images(bg), store.masks(bg)
    before = store.launches
    image, mask = images[3], mask_seq[3]
    assert store.launches == before + 1 and len(images) == 4 and _matches((image, mask), views[3], masks[3], bg, c_ref)
    # no mask files: no masks sequence; an all-ones mask from fetch; 6 bytes per pixel
    paths, none, views, _ = _toy_views(tmp_path / "plain", 2, masks=False)
    plain = hdr_views.HdrViewStore(paths, DEV)
    assert plain.masks(bg) is None and not plain.has_masks and plain.resident_nbytes() == 2 * 6 * 24 * 40
    assert _matches(plain.fetch(1, bg), views[1], None, bg, c_ref)
    with pytest.raises(RuntimeError, match="HdrViewStore"):
        hdr_views.HdrViewStore(paths, DEV, resolution=2)


# ---- 11. the driver end to end ---------------------------------------------------------------------------------------------------------
def test_driver_trains_both_stages_from_a_synthetic4relight_directory(tmp_path):
    from PIL import Image
    from relightable3dgaussian_amd import dataset, hdr_views, synthetic as syn, training
    root, out = str(tmp_path / "Synthetic4Relight" / "toy"), str(tmp_path / "out")
    W, H = 40, 24
    _toy_views(os.path.join(root, "train"), 4, W, H)
    cams = syn.orbit_cameras(6, radius=4.0, width=W, height=H, fovx=0.69)
    c2w = []
    for cam in cams:                                                # camera-to-world in the OpenGL/Blender axes
        m = torch.linalg.inv(cam.world_view_transform.double().t())
        m[:3, 1:3] *= -1
        c2w.append(m.numpy().tolist())
    os.makedirs(os.path.join(root, "test"))
    rng = np.random.RandomState(3)
    for i in range(2):
        rgba = rng.randint(0, 256, size=(H, W, 4)).astype(np.uint8)
        rgba[:, : W // 2, 3] = 255
        Image.fromarray(rgba).save(os.path.join(root, "test", "%03d_rgba.png" % i))
    for split, ids in (("train", range(4)), ("test", range(4, 6))):
        frames = [{"file_path": "./%s/%03d" % (split, j), "transform_matrix": c2w[i]} for j, i in enumerate(ids)]
        with open(os.path.join(root, "transforms_%s.json" % split), "w") as fh:
            json.dump({"camera_angle_x": 0.69, "frames": frames}, fh)
    dataset.write_points_ply(os.path.join(root, "points3d.ply"), rng.random_sample((500, 3)) * 2.6 - 1.3,
                             rng.random_sample((500, 3)) * 255, np.zeros((500, 3)))
    parse = training.build_parser().parse_args
    r1 = training.train(parse(["-s", root, "-m", out, "-t", "render", "--iterations", "3", "--eval", "--log_interval", "1"]))
    assert isinstance(r1.store, hdr_views.HdrViewStore) and r1.store.has_masks and r1.store.launches >= 3 and r1.step.P == 500
    assert len(r1.cameras) == 4 and len(r1.test_cameras) == 2 and np.isfinite(float(r1.step.loss()))
    ck = os.path.join(out, "chkpnt3.pth")
    assert os.path.exists(ck) and os.path.exists(os.path.join(out, "point_cloud", "iteration_3", "point_cloud.ply"))
    with open(os.path.join(out, "metrics.json")) as fh:
        m1 = json.load(fh)
    assert m1["views"] == 2 and m1["iteration"] == 3 and all(np.isfinite(m1["render"][k]) for k in ("psnr", "ssim"))
    out2 = os.path.join(out, "neilf")
    r2 = training.train(parse(["-s", root, "-m", out2, "-t", "neilf", "-c", ck, "--iterations", "5", "--log_interval", "1",
                               "--position_lr_init", "0", "--position_lr_final", "0", "--normal_lr", "0", "--sh_lr", "0",
                               "--opacity_lr", "0", "--scaling_lr", "0", "--rotation_lr", "0", "--lambda_base_color_smooth", "1",
                               "--lambda_roughness_smooth", "0.5", "--lambda_light_smooth", "1", "--lambda_light", "0.01",
                               "--sample_num", "8", "--lambda_env_smooth", "0.01"]))
    assert r2.first_iteration == 3 and len(r2.views) == 2 and np.isfinite(float(r2.step.loss()))
    assert isinstance(r2.store, hdr_views.HdrViewStore)
    env_ck, env_it = torch.load(os.path.join(out2, "env_light_chkpnt5.pth"), map_location="cpu", weights_only=True)
    assert env_it == 5 and torch.isfinite(env_ck[0]).all()
