"""Views with a mask file of their own, views at another resolution, and the driver on a NeILF-format directory, on the GPU
(relightable3dgaussian_amd/dataset.py, training.py; csrc/view_store.hip, csrc/view_resize.hip).

r3dg_view_unpack_masked against dataset.unpack_masked_reference bit for bit -- which tests/test_neilf_dataset_cpu.py pins to the
reference's own reader.  Shapes (W, H): 1024 x 1 holding every byte value of every channel against the mask bytes 0, 1, 127, 255;
5, 6 and 35 pixels (one or two lanes and a tail of 1, 2, 3); 64 x 64 (four workgroups, no tail); 67 x 61 / 62 / 63 (more than one
workgroup with a tail, N % 4 = 3, 2, 1).  Every shape runs on exact-size tensors and on views 1 and 16 bytes / 1 and 4 floats into
larger buffers, with canaries around every output.

r3dg_view_resize against dataset.resize_reference.  MEASURED TOLERANCE: y32 and y64 are the yardstick (torch's antialiased bilinear
interpolate on CPU) in float32 and in float64 on the same float32 composite, d = max|y32 - y64| is the reference's own float32 error,
and the kernel must satisfy max|kernel - y64| <= 2 * max(d, 16 * 2^-24): as close to the exact filter as the reference's own float32
code, the factor 2 because a float32 sum in another order can be equally far on the other side.  d itself must stay below 2e-5.
Measured on the MI355X (profiles/r13_view_resize.txt): d between 7.4e-8 and 2.4e-6, the kernel between 5.6e-8 and 1.6e-7 from y64.
Masks are compared bit for bit with the nearest-neighbour yardstick."""
import json
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
CANARY = -7.5
WHITE = (1.0, 1.0, 1.0)
MASK_BYTES = np.array([0, 1, 127, 255], np.uint8)
UNPACK_SHAPES = [(1024, 1), (5, 1), (6, 1), (7, 5), (64, 64), (67, 61), (67, 62), (67, 63)]
# (H, W) -> `resolution`: scales 2, 4, 8, a target width (70 / 58), and a view larger than the 64 x 8 tile in both directions
RESIZE_CASES = [((37, 53), 2), ((37, 53), 4), ((64, 80), 8), ((50, 70), 58), ((130, 300), 2)]
KINDS = ("rgba", "rgb_mask", "rgb")
_CACHE = {}


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _unpack_case(W, H):
    """(pixels, mask bytes, image, mask) of a masked-unpack case: computed once, shared, never modified."""
    from relightable3dgaussian_amd import dataset
    if ("unpack", W, H) not in _CACHE:
        rng = np.random.RandomState(W * 100 + H)
        if (W, H) == (1024, 1):                       # every byte value of every channel against every mask byte
            v = np.repeat(np.arange(256), 4)
            px = np.stack([v, 255 - v, (7 * v + 13) % 256], -1).astype(np.uint8).reshape(1, 1024, 3)
            mb = np.tile(MASK_BYTES, 256).reshape(1, 1024)
        else:
            px = rng.randint(0, 256, size=(H, W, 3)).astype(np.uint8)
            mb = rng.choice(MASK_BYTES, size=(H, W))
        _CACHE[("unpack", W, H)] = (px, mb) + dataset.unpack_masked_reference(px, mb)
    return _CACHE[("unpack", W, H)]


def _unpack_masked(W, H, pixels, mask_bytes, image, mask):
    from relightable3dgaussian_amd import _lib
    _lib.check(_lib.lib().r3dg_view_unpack_masked(_lib.current_stream(), W, H, pixels.data_ptr(), mask_bytes.data_ptr(),
                                                  image.data_ptr(), None if mask is None else mask.data_ptr()), "view_unpack_masked")


# ---- 1. the masked unpack ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", UNPACK_SHAPES)
def test_view_unpack_masked_is_the_reference_reader_bit_for_bit(W, H):
    N = W * H
    px, mb, want_image, want_mask = _unpack_case(W, H)
    if N == 1024:
        for c in range(3):
            assert len({(int(a), int(b)) for a, b in zip(px[0, :, c], mb[0])}) == 1024
    d_px, d_mb = torch.from_numpy(px).to(DEV), torch.from_numpy(mb).to(DEV)
    image = torch.full((3, H, W), CANARY, device=DEV)
    mask = torch.full((1, H, W), CANARY, device=DEV)
    _unpack_masked(W, H, d_px, d_mb, image, mask)
    assert torch.equal(_bits(image), _bits(want_image)) and torch.equal(_bits(mask), _bits(want_mask))
    assert set(np.unique(mask.cpu().numpy()).tolist()) <= {0.0, 1.0}
    image2 = torch.full((3, H, W), CANARY, device=DEV)
    _unpack_masked(W, H, d_px, d_mb, image2, None)                                     # d_mask = NULL
    assert torch.equal(_bits(image2), _bits(want_image))
    # views into larger buffers: off every vector grid (1), and on it at a non-zero offset (16 bytes / 4 floats)
    for off in (1, 4):
        o = off if off == 1 else 16
        big_px = torch.zeros(N * 3 + 64, dtype=torch.uint8, device=DEV)
        big_mb = torch.full((N + 64,), 255, dtype=torch.uint8, device=DEV)
        big_px[o:o + N * 3] = d_px.reshape(-1)
        big_mb[o:o + N] = d_mb.reshape(-1)
        big_image = torch.full((3 * N + 2 * off + 8,), CANARY, device=DEV)
        big_mask = torch.full((N + 2 * off + 8,), CANARY, device=DEV)
        v_image, v_mask = big_image[off:off + 3 * N], big_mask[off:off + N]
        _unpack_masked(W, H, big_px[o:o + N * 3], big_mb[o:o + N], v_image, v_mask)
        assert torch.equal(_bits(v_image).reshape(-1), _bits(want_image).reshape(-1)), (W, H, off)
        assert torch.equal(_bits(v_mask).reshape(-1), _bits(want_mask).reshape(-1)), (W, H, off)
        for buf, n in ((big_image, 3 * N), (big_mask, N)):
            assert bool((buf[:off] == CANARY).all()) and bool((buf[off + n:] == CANARY).all()), (W, H, off)


# ---- 2. the resize ----------------------------------------------------------------------------------------------------------------
def _resize_case(H, W, resolution, kind):
    """Inputs, target size and the yardsticks of a resize case: computed once, shared, never modified."""
    from relightable3dgaussian_amd import dataset
    key = ("resize", H, W, resolution, kind)
    if key not in _CACHE:
        rng = np.random.RandomState(H * 1000 + W + resolution)
        px = rng.randint(0, 256, size=(H, W, 4 if kind == "rgba" else 3)).astype(np.uint8)
        mb = None
        if kind == "rgba":
            px[0, :, 3], px[1, :, 3] = 0, 255
            composite, mask = dataset.unpack_reference(px, WHITE, clamp=False)
        elif kind == "rgb_mask":
            mb = rng.choice(MASK_BYTES, size=(H, W), p=(0.3, 0.1, 0.1, 0.5))
            composite, mask = dataset.unpack_masked_reference(px, mb, clamp=False)
        else:
            composite, mask = dataset.unpack_reference(px, WHITE, clamp=False)
        scale = dataset.view_scale(resolution, W)
        size = dataset.target_size(H, W, scale)
        y32, want_mask = dataset.resize_reference(composite, mask, size)
        y64 = dataset.resize_reference(composite.double(), None, size)[0].clamp(0.0, 1.0)
        _CACHE[key] = (px, mb, size, y32.clamp(0.0, 1.0), y64, want_mask)
    return _CACHE[key]


def _assert_resized(tag, image, y32, y64):
    """The measured tolerance of the module docstring; prints both figures."""
    d = float((y32.double() - y64).abs().max())
    e = float((image.detach().cpu().double() - y64).abs().max())
    bound = 2.0 * max(d, 16.0 * 2.0 ** -24)
    print("%-40s d = max|y32 - y64| = %.3e   max|kernel - y64| = %.3e   bound %.3e" % (tag, d, e, bound))
    assert d <= 2e-5, (tag, d)
    assert e <= bound, (tag, e, bound)
    assert float(image.min()) >= 0.0 and float(image.max()) <= 1.0


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape,resolution", RESIZE_CASES)
def test_view_resize_is_the_reference_resize(shape, resolution, kind):
    from relightable3dgaussian_amd import _lib
    (H, W) = shape
    px, mb, (h, w), y32, y64, want_mask = _resize_case(H, W, resolution, kind)
    d_px = torch.from_numpy(px).to(DEV)                           # exact-size tensors: the kernel reads no byte outside them
    d_mb = None if mb is None else torch.from_numpy(mb).to(DEV)
    bg = torch.tensor(WHITE, device=DEV)
    pad = 8
    big_image = torch.full((3 * h * w + 2 * pad,), CANARY, device=DEV)
    big_mask = torch.full((h * w + 2 * pad,), CANARY, device=DEV)
    image, mask = big_image[pad:pad + 3 * h * w].view(3, h, w), big_mask[pad:pad + h * w].view(1, h, w)
    _lib.check(_lib.lib().r3dg_view_resize(_lib.current_stream(), W, H, px.shape[2], d_px.data_ptr(),
                                           None if d_mb is None else d_mb.data_ptr(), bg.data_ptr(), w, h, image.data_ptr(),
                                           mask.data_ptr()), "view_resize")
    _assert_resized("(%d,%d) -> (%d,%d) %s" % (H, W, h, w, kind), image, y32, y64)
    assert torch.equal(_bits(mask), _bits(want_mask))             # nearest neighbour: bit for bit (all ones for plain RGB)
    if kind == "rgb":
        assert bool((mask == 1).all())
    for buf, n in ((big_image, 3 * h * w), (big_mask, h * w)):
        assert bool((buf[:pad] == CANARY).all()) and bool((buf[pad + n:] == CANARY).all())
    image2 = torch.full((3, h, w), CANARY, device=DEV)            # d_mask = NULL
    _lib.check(_lib.lib().r3dg_view_resize(_lib.current_stream(), W, H, px.shape[2], d_px.data_ptr(),
                                           None if d_mb is None else d_mb.data_ptr(), bg.data_ptr(), w, h, image2.data_ptr(), None),
               "view_resize")
    assert torch.equal(_bits(image2), _bits(image))


# ---- 3. the store ------------------------------------------------------------------------------------------------------------------
def _save(path, array, mode=None):
    from PIL import Image
    Image.fromarray(array, mode=mode).save(path)
    return str(path)


def test_store_keeps_mask_files_as_one_byte_planes_at_aligned_offsets(tmp_path):
    """The second view lies at a 16-byte-aligned, non-zero offset behind an odd-sized one (105 + 35 bytes, padded to 112 + 48)."""
    from relightable3dgaussian_amd import dataset
    rng = np.random.RandomState(7)
    shapes = [(5, 7), (24, 24), (5, 7)]
    arrays = [rng.randint(0, 256, size=s + (3,)).astype(np.uint8) for s in shapes]
    mask_arrays = [rng.choice(MASK_BYTES, size=shapes[0]), rng.choice(MASK_BYTES, size=shapes[1]), None]
    paths = [_save(tmp_path / ("v%d.png" % i), a) for i, a in enumerate(arrays)]
    mask_paths = [None if m is None else _save(tmp_path / ("m%d.png" % i), m, "L") for i, m in enumerate(mask_arrays)]
    store = dataset.ViewStore(paths, DEV, mask_paths=mask_paths, slots=2)
    assert [(v.offset, v.mask_offset) for v in store.views] == [(0, 112), (160, 160 + 1728), (160 + 1728 + 576, None)]
    assert store.nbytes == 160 + 1728 + 576 + 112 and store.has_masks and not store.has_alpha and store.scales == [1, 1, 1]
    assert store.resident_nbytes() == store.nbytes and store.resizes == 0
    for v, (a, m) in enumerate(zip(arrays, mask_arrays)):
        want = dataset.unpack_reference(a, WHITE) if m is None else dataset.unpack_masked_reference(a, m)
        n = store.launches
        image, mask = store.fetch(v, WHITE)
        assert store.launches == n + 1
        assert torch.equal(_bits(image), _bits(want[0])) and torch.equal(_bits(mask), _bits(want[1]))
    masks = store.masks(WHITE)
    assert len(masks) == 3 and bool((masks[2] == 1).all())                       # a view without a mask file: all ones


def test_store_resizes_once_at_load_and_serves_resident_tensors(tmp_path):
    """Target width 40: the 80 x 60 views are resized at load, the 40 x 30 ones (scale 1) still go through the ring."""
    from relightable3dgaussian_amd import dataset
    rng = np.random.RandomState(8)
    big = [rng.randint(0, 256, size=(60, 80, 4)).astype(np.uint8) for _ in range(2)]
    small = [rng.randint(0, 256, size=(30, 40, 4)).astype(np.uint8) for _ in range(2)]
    paths = [_save(tmp_path / ("v%d.png" % i), a) for i, a in enumerate(big + small)]
    with pytest.raises(RuntimeError, match="background"):
        dataset.ViewStore(paths, DEV, resolution=40)                              # resized RGBA views need their background
    store = dataset.ViewStore(paths, DEV, resolution=40, background=WHITE, slots=2)
    assert store.sizes == [(30, 40)] * 4 and store.scales == [2.0, 2.0, 1.0, 1.0] and store.resizes == 2
    assert store.nbytes == 2 * 30 * 40 * 4 and store.resident_nbytes() == store.nbytes + 2 * 16 * 30 * 40
    white, black = torch.ones(3, device=DEV), torch.zeros(3, device=DEV)
    for v, a in enumerate(big):
        composite, mask = dataset.unpack_reference(a, WHITE, clamp=False)
        y32, want_mask = dataset.resize_reference(composite, mask, (30, 40))
        y64 = dataset.resize_reference(composite.double(), None, (30, 40))[0].clamp(0.0, 1.0)
        n = store.launches
        image, got_mask = store.fetch(v, white)
        again = store.fetch(v, WHITE)
        assert store.launches == n                                                # no launch ...
        assert again[0].data_ptr() == image.data_ptr() and again[1].data_ptr() == got_mask.data_ptr()     # ... and no ring
        _assert_resized("store view %d" % v, image, y32.clamp(0.0, 1.0), y64)
        assert torch.equal(_bits(got_mask), _bits(want_mask))
        with pytest.raises(RuntimeError, match="background"):
            store.fetch(v, black)
        with pytest.raises(RuntimeError, match="background"):
            store.fetch(v, (0.0, 0.0, 0.0))
    images, masks = store.images(white), store.masks(white)
    n = store.launches
    assert images[0].data_ptr() == store.views[0].image.data_ptr() and masks[0].data_ptr() == store.views[0].mask.data_ptr()
    assert store.launches == n
    # the views of scale 1: today's path, any background, through the ring of two slots
    for bg in (WHITE, (0.0, 0.0, 0.0)):
        for v, a in enumerate(small):
            want = dataset.unpack_reference(a, bg)
            n = store.launches
            image, mask = store.fetch(2 + v, bg)
            assert store.launches == n + 1
            assert torch.equal(_bits(image), _bits(want[0])) and torch.equal(_bits(mask), _bits(want[1]))
    first = store.fetch(2, WHITE)[0]
    store.fetch(3, WHITE)
    assert store.fetch(2, WHITE)[0].data_ptr() == first.data_ptr()                # the third fetch of that size reuses the slot


def test_store_resizes_views_with_mask_files_and_plain_rgb_views(tmp_path):
    from relightable3dgaussian_amd import dataset
    rng = np.random.RandomState(9)
    arrays = [rng.randint(0, 256, size=(37, 53, 3)).astype(np.uint8) for _ in range(2)]
    mb = rng.choice(MASK_BYTES, size=(37, 53))
    paths = [_save(tmp_path / ("v%d.png" % i), a) for i, a in enumerate(arrays)]
    store = dataset.ViewStore(paths, DEV, mask_paths=[_save(tmp_path / "m0.png", mb, "L"), None], resolution=2)
    assert store.sizes == [(18, 26)] * 2 and store.nbytes == 0 and store.has_masks and store.launches == 0
    composite, mask = dataset.unpack_masked_reference(arrays[0], mb, clamp=False)
    y32, want_mask = dataset.resize_reference(composite, mask, (18, 26))
    image, got_mask = store.fetch(0, (0.0, 0.0, 0.0))                            # (no background is baked into an RGB view)
    _assert_resized("store, mask file", image, y32.clamp(0, 1), dataset.resize_reference(composite.double(), None, (18, 26))[0].clamp(0, 1))
    assert torch.equal(_bits(got_mask), _bits(want_mask))
    composite = dataset.unpack_reference(arrays[1], WHITE, clamp=False)[0]
    image, got_mask = store.fetch(1, WHITE)
    _assert_resized("store, plain RGB", image, dataset.resize_reference(composite, None, (18, 26))[0].clamp(0, 1),
                    dataset.resize_reference(composite.double(), None, (18, 26))[0].clamp(0, 1))
    assert bool((got_mask == 1).all()) and store.launches == 0                   # beside a view with a mask: all ones
    plain = dataset.ViewStore(paths[1:], DEV, resolution=2)
    assert plain.masks(WHITE) is None and plain.fetch(0, WHITE)[1] is None and torch.equal(plain.fetch(0, WHITE)[0], image)


# ---- 4. the driver end to end ---------------------------------------------------------------------------------------------------------
def _teacher_scene(root, n=8, width=64, height=48, points=200):
    """A NeILF-format directory of n views of a small teacher scene with mask files (the rendered opacity, thresholded), principal
    points off the centre, and a sparse.ply of `points` points."""
    from relightable3dgaussian_amd import dataset, synthetic as syn
    from relightable3dgaussian_amd.bench_core import GaussianParams, render_stage1
    from tests.test_neilf_dataset_cpu import write_neilf_scene
    cams = syn.orbit_cameras(n, width=width, height=height)
    zero = torch.zeros(3, device=DEV)
    pixels, masks = [], []
    with torch.no_grad():
        teacher = GaussianParams(syn.make_scene(P=3000, seed=9, stage2=False, scale_log_mean=-2.4), DEV, False)
        for c in cams:
            outs = render_stage1(teacher, c.to(DEV), zero)
            pixels.append((outs[2].clamp(0, 1).permute(1, 2, 0) * 255.0).round().to(torch.uint8).cpu().numpy())
            masks.append(((outs[3].reshape(height, width) > 0.5) * 255).to(torch.uint8).cpu().numpy())
    focal = [(width / (2 * math.tan(c.FoVx / 2)), height / (2 * math.tan(c.FoVy / 2))) for c in cams]
    ppt = [(width / 2 + 1.5, height / 2 - 1.0)] * n
    extrinsics = [c.world_view_transform.double().t().numpy() for c in cams]
    bbox = np.diag([2.0, 1.0, 2.0, 1.0])                          # (its diagonal becomes max / 2 = 1: the scene keeps its size)
    rng = np.random.RandomState(2)
    model = os.path.join(root, "inputs", "model")
    os.makedirs(model)
    dataset.write_points_ply(os.path.join(model, "sparse.ply"), rng.random_sample((points, 3)) * 2.0 - 1.0,
                             rng.random_sample((points, 3)) * 255, np.zeros((points, 3)))
    write_neilf_scene(root, [str(i) for i in range(n)], [2] * n, ["%04d.png" % i for i in range(n)], pixels, masks, extrinsics,
                      focal, ppt, bbox)
    return ppt[0]


def test_driver_trains_both_stages_from_a_neilf_directory(tmp_path):
    from relightable3dgaussian_amd import checkpoint, training
    root, out = str(tmp_path / "data"), str(tmp_path / "out")
    cx, cy = _teacher_scene(root)
    parse = training.build_parser().parse_args
    stage1 = ["-s", root, "-t", "render", "--eval", "--iterations", "6", "--log_interval", "3", "--seed", "3",
              "--lambda_normal_render_depth", "0.01", "--lambda_normal_smooth", "0.01", "--lambda_mask_entropy", "0.1",
              "--densify_grad_normal_threshold", "999", "--lambda_depth_var", "1e-2"]
    results = {}
    for r in (2, 1):
        dest = os.path.join(out, "r%d" % r)
        res = results[r] = training.train(parse(stage1 + ["-r", str(r), "-m", dest]))
        assert len(res.views) == 6 and len(res.cameras) == 7 and len(res.test_cameras) == 1        # view "2" is the test split
        assert math.isfinite(float(res.step.loss()))
        assert all((c.image_height, c.image_width, c.cx, c.cy) == (48 // r, 64 // r, cx / r, cy / r)
                   for c in res.cameras + res.test_cameras)
        assert res.store.resizes == (7 if r == 2 else 0) and res.store.has_masks
        assert res.store.launches == 0 if r == 2 else res.store.launches >= 6          # (a dropped view is fetched again)
        assert checkpoint.restore(os.path.join(dest, "chkpnt6.pth")).iteration == 6
        assert os.path.exists(os.path.join(dest, "point_cloud", "iteration_6", "point_cloud.ply"))
        with open(os.path.join(dest, "metrics.json")) as fh:
            m = json.load(fh)
        assert m["views"] == 1 and m["iteration"] == 6 and all(np.isfinite(m["render"][k]) for k in ("psnr", "ssim"))
    assert os.path.exists(os.path.join(root, "inputs", "model", "sparse_bbx_scale.ply")) and results[2].step.P == 200
    # stage 2 from the checkpoint just written, with the flags of the reference's DTU run script
    ck = os.path.join(out, "r2", "chkpnt6.pth")
    out2 = os.path.join(out, "neilf")
    r2 = training.train(parse(["-s", root, "-m", out2, "-t", "neilf", "-c", ck, "--eval", "-r", "2", "--iterations", "10",
                               "--log_interval", "2", "--seed", "3", "--position_lr_init", "0", "--position_lr_final", "0",
                               "--normal_lr", "0", "--sh_lr", "0", "--opacity_lr", "0", "--scaling_lr", "0", "--rotation_lr", "0",
                               "--lambda_base_color_smooth", "1", "--lambda_roughness_smooth", "0.5", "--lambda_light_smooth", "1",
                               "--lambda_light", "0.01", "--light_init", "3.0", "--sample_num", "32", "--lambda_env_smooth", "0.01",
                               "--env_resolution", "16", "--env_lr", "0.1", "--roughness_lr", "0.01"]))
    assert r2.first_iteration == 6 and len(r2.views) == 4 and math.isfinite(float(r2.step.loss()))
    assert torch.equal(r2.step.xyz.detach().cpu(), checkpoint.restore(ck).xyz.cpu())              # (learning rates of 0)
    captured, iteration = torch.load(os.path.join(out2, "chkpnt10.pth"), map_location="cpu", weights_only=True)
    assert iteration == 10
    env_ck, env_it = torch.load(os.path.join(out2, "env_light_chkpnt10.pth"), map_location="cpu", weights_only=True)
    assert env_it == 10 and torch.isfinite(env_ck[0]).all() and not torch.equal(env_ck[0].detach(), r2.env_init)
    assert os.path.exists(os.path.join(out2, "point_cloud", "iteration_10", "point_cloud.ply"))
    with open(os.path.join(out2, "metrics.json")) as fh:
        m2 = json.load(fh)
    assert m2["views"] == 1 and all(np.isfinite(m2[key][k]) for key in ("render", "pbr") for k in ("psnr", "ssim")), m2
