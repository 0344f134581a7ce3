"""Golden vectors for the Blender-format dataset reader (relightable3dgaussian_amd/dataset.py), produced by running the REFERENCE's
own readCamerasFromTransforms / getNerfppNorm / storePly / fetchPly (scene/dataset_readers.py:45-66, :125-160, :215-272), loadCam
(utils/camera_utils.py:13-74) and Camera (scene/cameras.py:8-73) on CPU in this container.

    python tests/golden/make_dataset_golden.py      # needs the reference checkout (make_golden.REF); writes dataset_reference.npz

Two small splits are written into a temporary directory and read back by the reference: `rgba` (3 views, 7 wide x 5 high, alpha
values 0, 255 and in between) and `rgb` (2 views, 6 x 6, no alpha channel), each for a white and a black background.  The file
records the PNG pixel arrays, the frames' matrices, what the reader and the Camera class made of them (R, T, FovX, FovY,
world_view_transform, full_proj_transform, camera_center, original_image, image_mask), the extent, and a points3d.ply of 50 points
written by storePly (raw bytes) with what fetchPly returns from it.  imageio, plyfile and torchvision are absent here and come from
the stand-ins of tools/reference_shims.py (PIL for the PNG read; at scale 1 the only Resize call keeps the mask's size).
Only inputs and outputs are stored; nothing of the reference's source is copied."""
import json
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

SPLITS = (("rgba", 3, 7, 5, 4), ("rgb", 2, 6, 6, 3))          # name, views, width, height, channels
FOVX = 0.6911112070083618


def write_split(root, name, pixels, c2w):
    from PIL import Image
    os.makedirs(os.path.join(root, name), exist_ok=True)
    frames = []
    for i in range(pixels.shape[0]):
        Image.fromarray(pixels[i]).save(os.path.join(root, name, "r_%d.png" % i))
        frames.append({"file_path": "./%s/r_%d" % (name, i), "transform_matrix": c2w[i].tolist()})
    with open(os.path.join(root, "transforms_%s.json" % name), "w") as fh:
        json.dump({"camera_angle_x": FOVX, "frames": frames}, fh, indent=1)


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
    rng = np.random.RandomState(20)
    rec = {"camera_angle_x": np.array(FOVX)}
    args = types.SimpleNamespace(resolution=1, data_device="cpu")
    with tempfile.TemporaryDirectory() as root:
        for name, V, W, H, C in SPLITS:
            pixels = rng.randint(0, 256, size=(V, H, W, C)).astype(np.uint8)
            if C == 4:
                pixels[:, 0, :, 3] = 0                       # a transparent row, an opaque row, the rest in between
                pixels[:, 1, :, 3] = 255
                pixels[0, 2, 0] = (255, 0, 128, 1)
                pixels[0, 2, 1] = (0, 255, 127, 254)
            cams = syn.orbit_cameras(7, radius=3.5 + 0.5 * len(name), width=W, height=H, fovx=FOVX)[:V]
            c2w = []
            for cam in cams:                                  # camera-to-world in the OpenGL/Blender axes, as the files hold it
                m = torch.linalg.inv(cam.world_view_transform.double().t())
                m[:3, 1:3] *= -1
                c2w.append(m.numpy())
            c2w = np.stack(c2w)
            write_split(root, name, pixels, c2w)
            rec.update({name + "_pixels": pixels, name + "_transform_matrix": c2w})
            for bg_name, white in (("white", True), ("black", False)):
                infos = readers.readCamerasFromTransforms(root, "transforms_%s.json" % name, white)
                assert len(infos) == V
                cameras = [loadCam(args, i, ci, 1.0) for i, ci in enumerate(infos)]
                rec[name + "_image_" + bg_name] = np.stack([c.original_image.numpy() for c in cameras])
                rec[name + "_mask_" + bg_name] = np.stack([c.image_mask.numpy() for c in cameras])
                assert rec[name + "_image_" + bg_name].dtype == np.float32 and rec[name + "_mask_" + bg_name].dtype == np.float32
            rec[name + "_R"] = np.stack([np.asarray(ci.R, np.float64) for ci in infos])
            rec[name + "_T"] = np.stack([np.asarray(ci.T, np.float64) for ci in infos])
            rec[name + "_fov"] = np.array([[ci.FovX, ci.FovY] for ci in infos], np.float64)
            rec[name + "_names"] = np.array([ci.image_name for ci in infos])
            for key in ("world_view_transform", "full_proj_transform", "camera_center"):
                rec[name + "_" + key] = np.stack([getattr(c, key).numpy() for c in cameras])
            norm = readers.getNerfppNorm(infos)
            rec[name + "_extent"] = np.array(norm["radius"])
            rec[name + "_translate"] = np.asarray(norm["translate"], np.float64)
        # points3d.ply as storePly writes it and fetchPly reads it
        xyz = rng.random_sample((50, 3)) * 2.6 - 1.3
        rgb = rng.random_sample((50, 3)) * 255
        normals = rng.randn(50, 3)
        normals /= np.linalg.norm(normals, axis=-1, keepdims=True)
        path = os.path.join(root, "points3d.ply")
        readers.storePly(path, xyz, rgb, normals)
        with open(path, "rb") as fh:
            rec["ply_bytes"] = np.frombuffer(fh.read(), np.uint8).copy()
        pcd = readers.fetchPly(path)
        rec.update(ply_points=np.asarray(pcd.points), ply_colors=np.asarray(pcd.colors), ply_normals=np.asarray(pcd.normals))
    out = os.path.join(HERE, "dataset_reference.npz")
    np.savez_compressed(out, **rec)
    print("dataset_reference.npz: %d arrays, %d KB" % (len(rec), os.path.getsize(out) // 1024))


if __name__ == "__main__":
    main()
