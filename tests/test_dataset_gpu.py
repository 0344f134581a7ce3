"""The device view store and the training driver on the GPU (relightable3dgaussian_amd/dataset.py, training.py;
csrc/view_store.hip): r3dg_view_unpack against dataset.unpack_reference bit for bit -- which tests/test_dataset_cpu.py pins to the
reference's own reader -- the ViewStore's ring of output slots, training through the store against training on resident tensors,
and the driver end to end on a dataset the test writes.

Unpack shapes (W, H, C): one pixel; three RGB pixels (a lone tail lane); 7 x 5 (the fixture's size: 35 pixels, 8 full lanes and a
tail of 3, planes 1 and 2 off the 16-byte grid); 64 x 4 (exactly one wave of 4-pixel lanes); 67 x 61 (more than one workgroup
with a tail, N % 4 = 3); 256 x 256 RGBA holding every (byte, alpha) pair.  Every shape runs on exact-size tensors at aligned
addresses and on views one element into larger buffers (the narrow-access paths), with canaries around every output."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
BACKGROUNDS = ((1.0, 1.0, 1.0), (0.0, 0.0, 0.0), (0.25, 0.5, 0.75))
SHAPES = [(1, 1, 4), (3, 1, 3), (7, 5, 4), (7, 5, 3), (64, 4, 4), (67, 61, 4), (67, 61, 3), (256, 256, 4)]
CANARY = -7.5
_CACHE = {}


def _pixels(W, H, Cn):
    if (W, H, Cn) == (256, 256, 4):                      # R = x, A = y, G = 255 - x, B = (7x + 13y) mod 256: every (byte, alpha) pair
        y, x = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
        return np.stack([x, 255 - x, (7 * x + 13 * y) % 256, y], -1).astype(np.uint8)
    px = np.random.RandomState(W * 1000 + H * 10 + Cn).randint(0, 256, size=(H, W, Cn)).astype(np.uint8)
    if Cn == 4:
        px[0, 0, 3], px[-1, -1, 3] = 0, 255
    return px


def _reference(W, H, Cn, bg):
    """(pixels, image, mask) of a case: computed once, shared, never modified."""
    from relightable3dgaussian_amd import dataset
    key = (W, H, Cn, bg)
    if key not in _CACHE:
        px = _pixels(W, H, Cn)
        image, mask = dataset.unpack_reference(px, bg)
        _CACHE[key] = (px, image, mask)
    return _CACHE[key]


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _unpack(W, H, Cn, pixels, bg, image, mask):
    from relightable3dgaussian_amd import _lib
    _lib.check(_lib.lib().r3dg_view_unpack(_lib.current_stream(), W, H, Cn, pixels.data_ptr(), bg.data_ptr(), image.data_ptr(),
                                           None if mask is None else mask.data_ptr()), "view_unpack")


# ---- 1. the kernel ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H,Cn", SHAPES)
def test_view_unpack_is_the_reference_reader_bit_for_bit(W, H, Cn):
    N = W * H
    for bg in BACKGROUNDS:
        px, want_image, want_mask = _reference(W, H, Cn, bg)
        d_bg = torch.tensor(bg, dtype=torch.float32, device=DEV)
        # exact-size tensors (an access outside them is outside the allocation's live bytes), aligned addresses
        d_px = torch.from_numpy(px).to(DEV)
        image = torch.full((3, H, W), CANARY, device=DEV)
        mask = torch.full((1, H, W), CANARY, device=DEV)
        _unpack(W, H, Cn, d_px, d_bg, image, mask)
        assert torch.equal(_bits(image), _bits(want_image)), (W, H, Cn, bg)
        assert torch.equal(_bits(mask), _bits(want_mask)), (W, H, Cn, bg)
        # d_mask = NULL
        image2 = torch.full((3, H, W), CANARY, device=DEV)
        _unpack(W, H, Cn, d_px, d_bg, image2, None)
        assert torch.equal(_bits(image2), _bits(want_image))
        # views into larger buffers: `off` elements (floats / bytes) in; 1 = off every vector grid, 4 floats / 16 bytes = on it
        for off in (1, 4):
            big_px = torch.zeros(N * Cn + 64, dtype=torch.uint8, device=DEV)
            o_px = off if off == 1 else 16
            big_px[o_px:o_px + N * Cn] = d_px.reshape(-1)
            big_image = torch.full((3 * N + 2 * off + 8,), CANARY, device=DEV)
            big_mask = torch.full((N + 2 * off + 8,), CANARY, device=DEV)
            v_image, v_mask = big_image[off:off + 3 * N], big_mask[off:off + N]
            _unpack(W, H, Cn, big_px[o_px:o_px + N * Cn], d_bg, v_image, v_mask)
            assert torch.equal(_bits(v_image).reshape(-1), _bits(want_image).reshape(-1)), (W, H, Cn, bg, off)
            assert torch.equal(_bits(v_mask).reshape(-1), _bits(want_mask).reshape(-1)), (W, H, Cn, bg, off)
            for buf, n in ((big_image, 3 * N), (big_mask, N)):
                assert bool((buf[:off] == CANARY).all()) and bool((buf[off + n:] == CANARY).all()), (W, H, Cn, bg, off)
    if Cn == 4 and N == 65536:
        assert len({(int(a), int(b)) for a, b in zip(px[..., 0].reshape(-1), px[..., 3].reshape(-1))}) == 65536


# ---- 2. the store -------------------------------------------------------------------------------------------------------------------
def _write_png(path, px):
    from PIL import Image
    Image.fromarray(px).save(path)


def test_view_store_serves_every_view_from_its_ring(tmp_path):
    from relightable3dgaussian_amd import dataset
    rng = np.random.RandomState(4)
    arrays = [rng.randint(0, 256, size=(24, 24, 4)).astype(np.uint8) for _ in range(3)] + \
             [rng.randint(0, 256, size=(12, 20, 4)).astype(np.uint8) for _ in range(2)]
    paths = []
    for i, a in enumerate(arrays):
        paths.append(str(tmp_path / ("v%d.png" % i)))
        _write_png(paths[-1], a)
    store = dataset.ViewStore(paths, DEV, slots=2)
    assert store.sizes == [(24, 24)] * 3 + [(12, 20)] * 2 and store.has_alpha
    assert store.nbytes == 3 * 24 * 24 * 4 + 2 * 12 * 20 * 4 and store.pixels.numel() == store.nbytes
    assert all(v.offset % 16 == 0 for v in store.views) and store.float_nbytes() == 4 * store.nbytes
    assert set(store.load_seconds) == {"decode", "upload", "decode_cpu"} and all(s >= 0 for s in store.load_seconds.values())
    assert 1 <= store.workers <= 8
    for bg in BACKGROUNDS:
        d_bg = torch.tensor(bg, device=DEV)
        for v, a in enumerate(arrays):
            want = dataset.unpack_reference(a, bg)
            for got in (store.fetch(v, d_bg), store.fetch(v, bg)):                  # a device tensor or three numbers
                assert torch.equal(_bits(got[0]), _bits(want[0])) and torch.equal(_bits(got[1]), _bits(want[1]))
    # the ring: two slots per size
    bg = BACKGROUNDS[2]
    want = [dataset.unpack_reference(a, bg) for a in arrays]
    i0, m0 = store.fetch(0, bg)
    i1, _ = store.fetch(1, bg)
    i3, _ = store.fetch(3, bg)                                                       # (another size: another ring)
    assert i1.data_ptr() != i0.data_ptr() and tuple(i3.shape) == (3, 12, 20)
    assert torch.equal(_bits(i0), _bits(want[0][0])) and torch.equal(_bits(m0), _bits(want[0][1]))       # still view 0
    version = i0._version
    i2, m2 = store.fetch(2, bg)
    assert i2.data_ptr() == i0.data_ptr() and m2.data_ptr() == m0.data_ptr()         # reused by the third fetch of that size
    assert torch.equal(_bits(i0), _bits(want[2][0])) and i0._version == version      # (raw-pointer writes: the version stays)
    assert torch.equal(_bits(i1), _bits(want[1][0]))
    # the lazy sequences: one launch serves an images[v] / masks[v] pair
    images, masks = store.images(bg), store.masks(bg)
    assert len(images) == len(masks) == 5
    n = store.launches
    a, b = images[4], masks[4]
    assert store.launches == n + 1
    assert torch.equal(_bits(a), _bits(want[4][0])) and torch.equal(_bits(b), _bits(want[4][1]))
    assert torch.equal(_bits(masks[1]), _bits(want[1][1])) and store.launches == n + 2      # (a mask on its own fetches)
    assert torch.equal(_bits(images[-1]), _bits(want[4][0]))
    with pytest.raises(IndexError):
        images[5]
    assert [tuple(t.shape) for t in images] == [(3, 24, 24)] * 3 + [(3, 12, 20)] * 2          # iterable, as zip() needs


def test_view_store_of_rgb_files_has_no_masks_and_pads_its_views(tmp_path):
    from relightable3dgaussian_amd import dataset
    rng = np.random.RandomState(5)
    arrays = [rng.randint(0, 256, size=(5, 7, 3)).astype(np.uint8), rng.randint(0, 256, size=(24, 24, 3)).astype(np.uint8),
              rng.randint(0, 256, size=(5, 7, 3)).astype(np.uint8)]
    paths = []
    for i, a in enumerate(arrays):
        paths.append(str(tmp_path / ("c%d.png" % i)))
        _write_png(paths[-1], a)
    store = dataset.ViewStore(paths, DEV, workers=2)
    assert not store.has_alpha and store.masks((0, 0, 0)) is None
    assert store.nbytes == 112 + 24 * 24 * 3 + 112                                   # 105 bytes padded to 112
    assert [v.offset for v in store.views] == [0, 112, 112 + 1728]
    for bg in BACKGROUNDS:
        images = store.images(bg)
        for v, a in enumerate(arrays):
            want = dataset.unpack_reference(a, bg)
            image, mask = store.fetch(v, bg)
            assert torch.equal(_bits(image), _bits(want[0])) and torch.equal(_bits(mask), _bits(want[1]))
            assert bool((mask == 1).all()) and torch.equal(_bits(images[v]), _bits(want[0]))


# ---- 3. training through the store ----------------------------------------------------------------------------------------------------
def _teacher_views(n, res, seed=9):
    """n views of a small teacher scene as RGBA bytes (alpha = the rendered opacity), with their cameras."""
    from relightable3dgaussian_amd import synthetic as syn
    from relightable3dgaussian_amd.bench_core import GaussianParams, render_stage1
    cams = syn.orbit_cameras(n, width=res, height=res)
    zero = torch.zeros(3, device=DEV)
    arrays = []
    with torch.no_grad():
        teacher = GaussianParams(syn.make_scene(P=3000, seed=seed, stage2=False, scale_log_mean=-2.4), DEV, False)
        for c in cams:
            outs = render_stage1(teacher, c.to(DEV), zero)
            rgba = torch.cat([outs[2].clamp(0, 1), outs[3].reshape(1, res, res).clamp(0, 1)], 0)
            arrays.append((rgba.permute(1, 2, 0) * 255.0).round().to(torch.uint8).cpu().numpy())
    return cams, arrays


def test_training_through_the_store_is_training_on_resident_tensors(tmp_path):
    """The first iteration's loss is bit-identical; the final parameters after 6 iterations agree within 4 x the spread of two
    runs of the resident-tensor path against each other (float atomics in the backward set that spread: it is measured here)."""
    from relightable3dgaussian_amd import dataset, synthetic as syn, train_loop
    from relightable3dgaussian_amd.bench_core import GaussianParams
    cams, arrays = _teacher_views(3, 64)
    paths = []
    for i, a in enumerate(arrays):
        paths.append(str(tmp_path / ("t%d.png" % i)))
        _write_png(paths[-1], a)
    store = dataset.ViewStore(paths, DEV)
    cams = [c.to(DEV) for c in cams]
    bg = torch.ones(3, device=DEV)
    resident = [dataset.unpack_reference(a, (1.0, 1.0, 1.0)) for a in arrays]
    r_images, r_masks = [r[0].to(DEV) for r in resident], [r[1].to(DEV) for r in resident]
    scene = syn.make_random_init_scene(2000)
    names = ("xyz", "normal", "scaling", "rotation", "opacity", "shs")

    def run(images, masks):
        first = []
        hook = lambda it, step: first.append(step.loss().detach().clone()) if it == 1 else None
        step, _ = train_loop.train_stage1(GaussianParams(scene, DEV, False), cams, images, bg, extent=4.4, iterations=6, seed=1,
                                          masks=masks, on_iteration=hook)
        torch.cuda.synchronize()
        return first[0], {k: getattr(step, k).detach().clone() for k in names}

    loss_a, a = run(r_images, r_masks)
    loss_b, b = run(r_images, r_masks)
    loss_s, s = run(store.images(bg), store.masks(bg))
    print("first-iteration loss: resident %r, resident again %r, store %r" % (float(loss_a), float(loss_b), float(loss_s)))
    assert torch.equal(_bits(loss_s), _bits(loss_a))
    for k in names:
        spread = float((a[k] - b[k]).abs().max())
        diff = float((s[k] - a[k]).abs().max())
        print("%-9s spread of two resident runs %.3e, store against resident %.3e" % (k, spread, diff))
        assert torch.isfinite(s[k]).all() and diff <= 4.0 * spread, (k, diff, spread)
    assert not torch.equal(a["xyz"], GaussianParams(scene, DEV, False).xyz.detach())           # (it trained)


# ---- 4. the driver end to end ---------------------------------------------------------------------------------------------------------
def test_driver_trains_both_stages_and_writes_the_reference_files(tmp_path):
    from relightable3dgaussian_amd import checkpoint, dataset, ply, training
    from tests.test_dataset_cpu import write_split
    cams, arrays = _teacher_views(8, 48)
    root, out = str(tmp_path / "data"), str(tmp_path / "out")
    os.makedirs(root)
    c2w = []
    for cam in cams:                                                # camera-to-world in the OpenGL/Blender axes
        m = torch.linalg.inv(cam.world_view_transform.double().t())
        m[:3, 1:3] *= -1
        c2w.append(m.numpy())
    c2w, pixels = np.stack(c2w), np.stack(arrays)
    test_ids = [2, 6]
    train_ids = [i for i in range(8) if i not in test_ids]
    write_split(root, "train", pixels[train_ids], c2w[train_ids], cams[0].FoVx)
    write_split(root, "test", pixels[test_ids], c2w[test_ids], cams[0].FoVx)
    rng = np.random.RandomState(2)                                  # (a small points3d.ply instead of the reader's 100 000 points)
    dataset.write_points_ply(os.path.join(root, "points3d.ply"), rng.random_sample((3000, 3)) * 2.6 - 1.3,
                             rng.random_sample((3000, 3)) * 255, np.zeros((3000, 3)))
    parse = training.build_parser().parse_args
    r1 = training.train(parse(["-s", root, "-m", out, "-t", "render", "--eval", "-w", "--iterations", "24", "--densify_from_iter", "8",
                               "--densification_interval", "8", "--log_interval", "8", "--seed", "3"]))
    assert len(r1.views) == 24 and sorted(r1.views[:6]) == list(range(6)) and any(e == "densify" for _, e, _ in r1.history)
    ck = os.path.join(out, "chkpnt24.pth")
    restored = checkpoint.restore(ck)
    assert restored.iteration == 24 and restored.xyz.shape[0] == r1.step.P
    assert abs(restored.spatial_lr_scale - r1.extent) < 1e-6 * r1.extent
    cloud = ply.load(os.path.join(out, "point_cloud", "iteration_24", "point_cloud.ply"), DEV)
    assert cloud.xyz.shape == restored.xyz.shape and torch.equal(cloud.xyz.cpu(), restored.xyz.cpu())
    with open(os.path.join(out, "metrics.json")) as fh:
        m1 = json.load(fh)
    assert set(m1) == {"render", "iteration", "views"} and m1["views"] == 2 and m1["iteration"] == 24
    assert all(np.isfinite(m1["render"][k]) for k in ("psnr", "ssim")) and m1["render"]["psnr"] > 0
    assert not os.path.exists(os.path.join(out, "env_light_chkpnt24.pth"))

    stage2 = ["-s", root, "-t", "neilf", "-c", ck, "--eval", "-w", "--iterations", "32", "--sample_num", "8", "--log_interval", "4",
              "--seed", "3"]
    out2 = os.path.join(out, "neilf")
    r2 = training.train(parse(stage2 + ["-m", out2]))
    assert r2.first_iteration == 24 and len(r2.views) == 8
    captured, iteration = torch.load(os.path.join(out2, "chkpnt32.pth"), map_location="cpu", weights_only=True)
    assert iteration == 32 and len(captured) == 21
    env_ck, env_it = torch.load(os.path.join(out2, "env_light_chkpnt32.pth"), map_location="cpu", weights_only=True)
    assert env_it == 32 and tuple(env_ck[0].shape) == (1, 16, 32, 3) and env_ck[1]["param_groups"][0]["name"] == "env"
    assert torch.isfinite(env_ck[0]).all() and not torch.equal(env_ck[0].detach(), r2.env_init)          # (the texture trained)
    assert 1.0 <= float(env_ck[1]["state"][0]["step"]) <= 8.0                                             # (8 less the dropped views)
    assert os.path.exists(os.path.join(out2, "point_cloud", "iteration_32", "point_cloud.ply"))
    with open(os.path.join(out2, "metrics.json")) as fh:
        m2 = json.load(fh)
    for key in ("render", "pbr"):
        assert all(np.isfinite(m2[key][k]) for k in ("psnr", "ssim")), m2
    # the same seed: the same views in the same order, from the same texture
    r3 = training.train(parse(stage2 + ["-m", os.path.join(out, "neilf_again")]))
    assert r3.views == r2.views and torch.equal(r3.env_init, r2.env_init)
    assert tuple(r2.env_init.shape) == (1, 16, 32, 3) and float(r2.env_init.max()) <= 3.0
    # a texture saved beside the checkpoint is read instead
    torch.save(training.env_checkpoint(torch.full((1, 16, 32, 3), 0.5), None, None, 0, 0.1, 24),
               os.path.join(out, "env_light_chkpnt24.pth"))
    r4 = training.train(parse(stage2[:-2] + ["--seed", "4", "--iterations", "26", "-m", os.path.join(out, "neilf_env")]))
    assert bool((r4.env_init == 0.5).all()) and len(r4.views) == 2
