"""Golden vectors for the NeILF-format dataset reader and the resize of `--resolution` (relightable3dgaussian_amd/dataset.py),
produced by running the REFERENCE's own readNeILFInfo / loadCamsFromScene / getNerfppNorm / storePly / fetchPly
(scene/dataset_readers.py:45-66, :125-160, :315-432), loadCam (utils/camera_utils.py:13-74) and Camera (scene/cameras.py:8-73) on CPU.

    python tests/golden/make_neilf_golden.py      # needs the reference checkout (make_golden.REF); writes neilf_dataset_reference.npz

A small NeILF-format directory is written into a temporary directory (by tests/test_neilf_dataset_cpu.write_neilf_scene, the
function the tests rebuild it with) and read back by the reference: 14 valid cameras with the indexes "0" .. "13" (with --eval, 2 and
12 are the test split) and one with flg != 2; RGB views 9 wide x 6 high and 7 x 5; principal points off the centre, fx != fy; a bbox
transform with an uneven diagonal and a translation; pmasks files with the bytes 0, 1, 127 and 255 for two views of three, none for
the others; a sparse.ply of 50 points.  loadCam runs at `resolution` 1, 2 and 5 (a target width: scales 9 / 5 and 7 / 5).  The file
records the inputs (pixel and mask arrays, the numbers of sfm_scene.json, the bytes of sparse.ply) and what came out: names, R, T,
FovX / FovY, fx / fy / cx / cy, the Camera's world_view_transform / projection_matrix / full_proj_transform / camera_center,
original_image and image_mask per resolution, the extent, the bytes of sparse_bbx_scale.ply and what fetchPly returns from it.
imageio, plyfile and torchvision are absent here and come from the stand-ins of tools/reference_shims.py (PIL for the PNG reads;
Resize is the two torch.nn.functional.interpolate calls torchvision's tensor Resize makes).  Only inputs and outputs are stored;
nothing of the reference's source is copied."""
import os
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import make_golden as mg  # noqa: E402  (auto-mock finder + CPU factory patches)
from tools import reference_shims  # noqa: E402
from tests.test_neilf_dataset_cpu import RESOLUTIONS, write_neilf_scene  # noqa: E402

VALID, SIZES = 14, ((9, 6), (7, 5))                            # valid cameras; (width, height) of even / odd views


def main():
    for factory in (reference_shims._plyfile_module, reference_shims._imageio_module, reference_shims._torchvision_modules):
        sys.modules.update(factory())
    sys.meta_path.append(mg._Finder())
    sys.path.insert(0, mg.REF)
    for p in mg._cpu_factories():
        p.start()
    import scene.dataset_readers as readers
    from utils.camera_utils import loadCam
    from relightable3dgaussian_amd import synthetic as syn
    rng = np.random.RandomState(21)
    n = VALID + 1
    indexes = [str(i) for i in range(n)]
    flags = np.array([2] * VALID + [1])
    file_names = np.array(["%04d.png" % i for i in range(n)])
    cams = syn.orbit_cameras(n, radius=4.0, width=9, height=6)
    extrinsics = np.stack([c.world_view_transform.double().t().numpy() for c in cams])           # world-to-camera
    pixels, masks, focal, ppt = [], [], [], []
    for i in range(n):
        w, h = SIZES[i % 2]
        focal.append((11.0 + 0.25 * i, 9.5 + 0.125 * i))
        ppt.append((w / 2 + 0.75 - 0.1 * i, h / 2 - 0.5 + 0.05 * i))
        if i >= VALID:                                         # (the reader never opens the files of a camera it skips)
            pixels.append(None)
            masks.append(None)
            continue
        pixels.append(rng.randint(0, 256, size=(h, w, 3)).astype(np.uint8))
        mask = None
        if i % 3 != 0:
            mask = rng.choice(np.array([0, 1, 127, 255], np.uint8), size=(h, w))
            mask[0, :4] = (0, 1, 127, 255)
        masks.append(mask)
    bbox = np.array([[2.0, 0, 0, 0.1], [0, 3.0, 0, -0.2], [0, 0, 2.5, 0.3], [0, 0, 0, 1.0]])
    rec = dict(indexes=np.array(indexes), flags=flags, file_names=file_names, extrinsics=extrinsics, focal=np.array(focal),
               ppt=np.array(ppt), bbox=bbox)
    for i in range(VALID):
        rec["pixels_%02d" % i] = pixels[i]
        if masks[i] is not None:
            rec["maskbytes_%02d" % i] = masks[i]
    with tempfile.TemporaryDirectory() as root:
        xyz = rng.random_sample((50, 3)) * 2.6 - 1.3
        rgb = rng.random_sample((50, 3)) * 255
        normals = rng.randn(50, 3)
        normals /= np.linalg.norm(normals, axis=-1, keepdims=True)
        sparse = os.path.join(root, "sparse.ply")
        readers.storePly(sparse, xyz, rgb, normals)
        with open(sparse, "rb") as fh:
            rec["sparse_ply_bytes"] = np.frombuffer(fh.read(), np.uint8).copy()
        write_neilf_scene(root, indexes, flags, list(file_names), pixels, masks, extrinsics, focal, ppt, bbox,
                          rec["sparse_ply_bytes"].tobytes())
        everything = readers.readNeILFInfo(root, False, False)
        assert len(everything.train_cameras) == VALID and not everything.test_cameras
        rec["all_names"] = np.array([ci.image_name for ci in everything.train_cameras])
        info = readers.readNeILFInfo(root, False, True)
        assert [ci.uid for ci in info.test_cameras] == ["2", "12"]
        rec["extent"] = np.array(info.nerf_normalization["radius"])
        for split, infos in (("train", info.train_cameras), ("test", info.test_cameras)):
            rec[split + "_names"] = np.array([ci.image_name for ci in infos])
            for j, ci in enumerate(infos):
                key = "%s_%02d_" % (split, j)
                rec[key + "R"], rec[key + "T"] = np.asarray(ci.R, np.float64), np.asarray(ci.T, np.float64)
                rec[key + "fov"] = np.array([ci.FovX, ci.FovY], np.float64)
                rec[key + "intrinsics"] = np.array([ci.fx, ci.fy, ci.cx, ci.cy], np.float64)
                rec[key + "size"] = np.array([ci.height, ci.width])
                rec[key + "has_mask"] = np.array(masks[int(ci.uid)] is not None)
                for resolution in RESOLUTIONS:
                    cam = loadCam(types.SimpleNamespace(resolution=resolution, data_device="cpu"), j, ci, 1.0)
                    key = "%s_%02d_r%d_" % (split, j, resolution)
                    rec[key + "size"] = np.array([cam.image_height, cam.image_width])
                    rec[key + "intrinsics"] = np.array([cam.fx, cam.fy, cam.cx, cam.cy], np.float64)
                    for name in ("world_view_transform", "projection_matrix", "full_proj_transform", "camera_center",
                                 "original_image", "image_mask"):
                        rec[key + name] = getattr(cam, name).numpy()
                        assert rec[key + name].dtype == np.float32
        with open(os.path.join(root, "inputs", "model", "sparse_bbx_scale.ply"), "rb") as fh:
            rec["scaled_ply_bytes"] = np.frombuffer(fh.read(), np.uint8).copy()
        pcd = info.point_cloud
        rec.update(ply_points=np.asarray(pcd.points), ply_colors=np.asarray(pcd.colors), ply_normals=np.asarray(pcd.normals))
    out = os.path.join(HERE, "neilf_dataset_reference.npz")
    np.savez_compressed(out, **rec)
    print("neilf_dataset_reference.npz: %d arrays, %d KB" % (len(rec), os.path.getsize(out) // 1024))


if __name__ == "__main__":
    main()
