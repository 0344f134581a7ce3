"""Golden data for the OpenEXR reader (relightable3dgaussian_amd/exr.py) and the Synthetic4Relight reader
(dataset.read_syn4relight), cut from files of the REFERENCE checkout and produced by its own reader on CPU.

    python tests/golden/make_exr_golden.py        # needs the reference checkout (make_golden.REF)

envmap3_rows96_127.exr   the two chunks at y = 96 and y = 112 of the reference's env_map/envmap3.exr (single-part scanline, FLOAT,
                         ZIP, 500 x 250, channels B, G, R), re-headed as a 500 x 32 file: dataWindow and displayWindow rewritten,
                         each chunk's y rebased, a fresh offset table; the chunk payloads are byte for byte the reference's.
exr_reference.npz        png_rows uint8 [32,500,3]: rows 96..127 of the reference's env_map/envmap3.png as RGB -- what
                         env_map/convert.py made of pyexr's decode of that file (rgb_to_srgb, clip, * 255, astype(uint8)): the
                         reference's own record of the decode.
syn4relight_reference.npz  R, T, FovX, FovY, image_name, width, height of the reference's readCamerasFromTransforms3
                         (scene/dataset_readers.py:526-565) on a three-frame transforms_train.json written here, with its two image
                         loaders replaced by stand-ins that return arrays of the right shape (as make_dataset_golden.py treats the
                         Blender reader), plus the frames' matrices and camera_angle_x.
Only data the reference's programs read and wrote is stored; nothing of its source is copied."""
import json
import os
import struct
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import make_golden as mg  # noqa: E402

ROWS = (96, 128)
SYN4_SIZE = (40, 24)               # width, height of the stand-in images (not square: FovY differs from FovX)
FOVX = 0.6911112070083618


def crop_exr():
    from relightable3dgaussian_amd import exr
    src = os.path.join(mg.REF, "env_map", "envmap3.exr")
    header = exr.read_header(src)
    assert header.compression == "ZIP" and header.data_window == (0, 0, 499, 249) and header.line_order == "INCREASING_Y"
    with open(src, "rb") as fh:
        data = fh.read()
    chunks = []
    for offset in header.offsets.tolist():
        y, size = struct.unpack_from("<ii", data, offset)
        if ROWS[0] <= y < ROWS[1]:
            chunks.append((y - ROWS[0], data[offset + 8:offset + 8 + size]))
    assert [y for y, _ in chunks] == [0, 16]
    window = struct.pack("<4i", 0, 0, header.width - 1, ROWS[1] - ROWS[0] - 1)
    out = data[:8]
    for name, (kind, value) in header.attributes.items():
        value = window if name in ("dataWindow", "displayWindow") else value
        out += name.encode("latin-1") + b"\0" + kind.encode("latin-1") + b"\0" + struct.pack("<i", len(value)) + value
    out += b"\0"
    at = len(out) + 8 * len(chunks)
    offsets = []
    for _, payload in chunks:
        offsets.append(at)
        at += 8 + len(payload)
    out += struct.pack("<%dQ" % len(chunks), *offsets)
    for y, payload in chunks:
        out += struct.pack("<ii", y, len(payload)) + payload
    path = os.path.join(HERE, "envmap3_rows96_127.exr")
    with open(path, "wb") as fh:
        fh.write(out)
    from PIL import Image
    with Image.open(os.path.join(mg.REF, "env_map", "envmap3.png")) as im:
        png = np.array(im.convert("RGB"), dtype=np.uint8)
    np.savez_compressed(os.path.join(HERE, "exr_reference.npz"), png_rows=png[ROWS[0]:ROWS[1]])
    samples = exr.decode_reference(path)
    print("envmap3_rows96_127.exr: %d bytes, %d of chunk data; %.1f %% of the samples above 1.0, maximum %g"
          % (len(out), sum(len(p) for _, p in chunks), 100.0 * float((samples > 1.0).mean()), float(samples.max())))


def syn4_reader():
    from relightable3dgaussian_amd import synthetic as syn
    import torch
    sys.meta_path.append(mg._Finder())
    sys.path.insert(0, mg.REF)
    import scene.dataset_readers as readers
    W, H = SYN4_SIZE
    readers.load_img_rgb = lambda path: np.zeros((H, W, 4), np.float32)          # stand-ins: arrays of the right shape
    readers.load_mask_bool = lambda path: np.ones((H, W), np.float32)
    cams = syn.orbit_cameras(5, radius=4.0, width=W, height=H, fovx=FOVX)[:3]
    c2w = []
    for cam in cams:                                      # camera-to-world in the OpenGL/Blender axes, as the files hold it
        m = torch.linalg.inv(cam.world_view_transform.double().t())
        m[:3, 1:3] *= -1
        c2w.append(m.numpy())
    c2w = np.stack(c2w)
    frames = [{"file_path": "./train/%03d" % i, "transform_matrix": c2w[i].tolist()} for i in range(3)]
    with tempfile.TemporaryDirectory() as root:
        with open(os.path.join(root, "transforms_train.json"), "w") as fh:
            json.dump({"camera_angle_x": FOVX, "frames": frames}, fh, indent=1)
        infos = readers.readCamerasFromTransforms3(root, "transforms_train.json", False, "_rgb.exr")
    assert len(infos) == 3
    np.savez_compressed(os.path.join(HERE, "syn4relight_reference.npz"), camera_angle_x=np.array(FOVX), transform_matrix=c2w,
                        R=np.stack([np.asarray(ci.R, np.float64) for ci in infos]),
                        T=np.stack([np.asarray(ci.T, np.float64) for ci in infos]),
                        FovX=np.array([ci.FovX for ci in infos], np.float64), FovY=np.array([ci.FovY for ci in infos], np.float64),
                        image_name=np.array([ci.image_name for ci in infos]), width=np.array([ci.width for ci in infos]),
                        height=np.array([ci.height for ci in infos]))
    print("syn4relight_reference.npz: %d views, names %s" % (len(infos), [ci.image_name for ci in infos]))


if __name__ == "__main__":
    crop_exr()
    syn4_reader()
