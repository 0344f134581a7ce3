"""A NeRF-synthetic (Blender) or NeILF-format (DTU / TnT) dataset directory as what the fused iterations take: the reference's
readNerfSyntheticInfo / readCamerasFromTransforms (scene/dataset_readers.py:215-312) and readNeILFInfo / loadCamsFromScene
(:315-432), with the ground-truth views kept ON THE DEVICE as the 8-bit pixels their files hold.

    records = read_transforms(root, "train")                 # name, path, R, T, FovX, FovY (+ width, height) per frame
    train, test = read_neilf_scene(root, eval)               # ... the same plus fx, fy, cx, cy, mask_path (inputs/sfm_scene.json)
    store = ViewStore([r["path"] for r in records], device,  # one uint8 device buffer: 4 bytes per RGBA pixel instead of 16,
                      mask_paths=[r.get("mask_path") ...],   # 3 + 1 per pixel of an RGB view with a mask file
                      resolution=-1, background=bg)          # loadCam's `--resolution`
    cameras = cameras_of(records, store.sizes, device, store.scales)   # synthetic.SynthCamera, the matrices of scene/cameras.py:56-73
    train_loop.train_stage1(init, cameras, store.images(bg), bg, extent, masks=store.masks(bg),
                            view_order=reference_view_order(len(cameras), seed))

`ViewStore.fetch` is ONE launch (csrc/view_store.hip): r3dg_view_unpack composites the chosen view onto the background and splits
off its alpha channel as the mask, r3dg_view_unpack_masked applies the mask file of a NeILF view, bit for bit as the reference's
reader does on the host; `unpack_reference` / `unpack_masked_reference` are the same arithmetic in NumPy, the yardsticks of the GPU
tests.  A view whose `resolution` scale is not 1 is resized ONCE, at load, by r3dg_view_resize (csrc/view_resize.hip: composite,
antialiased bilinear filter, clamp; the mask by nearest neighbour) and stays resident as float tensors; `resize_reference` is the
yardstick -- the two torch.nn.functional.interpolate calls that torchvision's tensor Resize makes (torchvision itself is not
installed where this was written; tools/reference_shims.py stands in for it with the same calls).  `initial_points` /
`initial_points_neilf` are the readers' point clouds (fetchPly / storePly, :125-160; the 100 000 random points of :288-299; the
bbox-rescaled sparse.ply of :408-425), `reference_view_order` the view pick of train.py:115-119.

`read_syn4relight` is the Synthetic4Relight reader (readCamerasFromTransforms3, :526-565): its train split is OpenEXR views
(`<file_path>_rgb.exr` + `<file_path>_mask.png`), which hdr_views.HdrViewStore keeps on the device in the files' own sample type
(exr.py parses the container, csrc/exr_unpack.hip decodes); its test split (`<file_path>_rgba.png`) goes through ViewStore.

Out of scope: the COLMAP and Stanford-ORB readers; `resolution_scale` other than 1 and upscaling; MVS depth / normal maps
(`<root>/extra`); `cfg_args`, `cameras.json`.
"""
import collections
import collections.abc
import json
import math
import os
import random
import time
import types
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import _lib, synthetic

ALIGN = 16                     # every view starts at a multiple of this in the store's buffer (the kernel's 16-byte loads)
RANDOM_POINTS = 100_000        # dataset_readers.py:290
C0 = 0.28209479177387814       # SH2RGB (utils/sh_utils.py:134-135)
_PLY_FIELDS = (("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4"),
               ("red", "u1"), ("green", "u1"), ("blue", "u1"))                       # storePly, dataset_readers.py:145-147
_PLY_TYPES = {"float": "<f4", "float32": "<f4", "double": "<f8", "float64": "<f8", "uchar": "u1", "uint8": "u1", "char": "i1",
              "int8": "i1", "short": "<i2", "int16": "<i2", "ushort": "<u2", "uint16": "<u2", "int": "<i4", "int32": "<i4",
              "uint": "<u4", "uint32": "<u4"}


# ---- cameras ---------------------------------------------------------------------------------------------------------------
def probe(path):
    """(height, width, channels) of an image file from its header; RuntimeError naming the file for anything but 8-bit RGB / RGBA."""
    from PIL import Image
    with Image.open(path) as im:
        mode, (w, h) = im.mode, im.size
    if mode not in ("RGB", "RGBA"):
        raise RuntimeError("%s: image mode %r is not read (8-bit RGB or RGBA files only; no palette, grey, LA or 16-bit images)"
                           % (path, mode))
    return h, w, len(mode)


def read_transforms(root, split, extension=".png"):
    """`<root>/transforms_<split>.json` -> one dict per frame: name, path, R [3,3], T [3] (float64, as readCamerasFromTransforms
    makes them: columns 1..2 of `transform_matrix` flipped, inverted, R = w2c[:3,:3]^T), FovX = camera_angle_x, FovY =
    focal2fov(fov2focal(FovX, H), W) exactly as :264 writes it (the image HEIGHT is the focal-length base and the WIDTH goes back
    in: the true FovY only for square images, but what the reference trains with), and the file's width / height."""
    with open(os.path.join(root, "transforms_%s.json" % split)) as fh:
        contents = json.load(fh)
    fovx = contents["camera_angle_x"]
    records = []
    for frame in contents["frames"]:
        path = os.path.join(root, frame["file_path"] + extension)
        c2w = np.array(frame["transform_matrix"], dtype=np.float64)
        c2w[:3, 1:3] *= -1                                    # OpenGL/Blender camera axes -> COLMAP (Y down, Z forward)
        w2c = np.linalg.inv(c2w)
        h, w, _ = probe(path)
        focal = h / (2 * math.tan(fovx / 2))                  # fov2focal(fovx, image.shape[0])
        fovy = 2 * math.atan(w / (2 * focal))                 # focal2fov(., image.shape[1])
        records.append(dict(name=os.path.splitext(os.path.basename(path))[0], path=path, R=np.transpose(w2c[:3, :3]).copy(),
                            T=w2c[:3, 3].copy(), FovX=fovx, FovY=fovy, width=w, height=h))
    return records


NEILF_TEST_INDEXES = (2, 12, 17, 30, 34)      # readNeILFInfo's validation_indexes (dataset_readers.py:395)


def detect_layout(root):
    """"blender", "syn4relight" or "neilf", decided as scene/__init__.py:43-61 decides it (a transforms_train.json under a path that
    contains "Synthetic4Relight" is that dataset, :51); RuntimeError naming the layouts for anything else."""
    if os.path.exists(os.path.join(root, "transforms_train.json")):
        return "syn4relight" if "Synthetic4Relight" in str(root) else "blender"
    if os.path.exists(os.path.join(root, "inputs", "sfm_scene.json")):
        return "neilf"
    raise RuntimeError("%s: neither a Blender-format dataset (transforms_train.json) nor a NeILF-format one "
                       "(inputs/sfm_scene.json); these are the two layouts this driver reads" % root)


def read_syn4relight(root, split):
    """`<root>/transforms_<split>.json` of a Synthetic4Relight scene -> records as read_transforms makes them, restating
    readCamerasFromTransforms3 (scene/dataset_readers.py:526-565): the same flip of columns 1..2, inverse and transposed R; FovX =
    camera_angle_x and FovY = focal2fov(fov2focal(FovX, H), W) exactly as :557 writes it (the image HEIGHT is the focal-length
    base and the WIDTH goes back in).  split "train": path = `<file_path>_rgb.exr` (its size from the EXR header: exr.read_header,
    which raises for a file it cannot decode) and mask_path = `<file_path>_mask.png` when that file exists (else None) -- the views
    of hdr_views.HdrViewStore.  Any other split: path = `<file_path>_rgba.png`, no mask_path -- the views of ViewStore, whose mask
    is the alpha channel (the reference thresholds the file's grey value instead, :536,552; the two agree wherever colour sits
    only under non-zero alpha)."""
    from . import exr
    with open(os.path.join(root, "transforms_%s.json" % split)) as fh:
        contents = json.load(fh)
    fovx = contents["camera_angle_x"]
    records = []
    for frame in contents["frames"]:
        stem = os.path.join(root, frame["file_path"])
        c2w = np.array(frame["transform_matrix"], dtype=np.float64)
        c2w[:3, 1:3] *= -1                                    # OpenGL/Blender camera axes -> COLMAP (Y down, Z forward)
        w2c = np.linalg.inv(c2w)
        if split == "train":
            path, mask_path = stem + "_rgb.exr", stem + "_mask.png"
            header = exr.read_header(path)
            h, w = header.height, header.width
        else:
            path, mask_path = stem + "_rgba.png", None
            h, w, _ = probe(path)
        focal = h / (2 * math.tan(fovx / 2))                  # fov2focal(fovx, image.shape[0])
        fovy = 2 * math.atan(w / (2 * focal))                 # focal2fov(., image.shape[1])
        records.append(dict(name=os.path.splitext(os.path.basename(path))[0], path=path, R=np.transpose(w2c[:3, :3]).copy(),
                            T=w2c[:3, 3].copy(), FovX=fovx, FovY=fovy, width=w, height=h,
                            mask_path=mask_path if mask_path and os.path.exists(mask_path) else None))
    return records


def _bbox_transform(sfm_scene):
    """The scene's bbox transform with its diagonal replaced by max(diagonal) / 2 (loadCamsFromScene, :320-322)."""
    m = np.array(sfm_scene["bbox"]["transform"], dtype=np.float64).reshape(4, 4).copy()
    d = [0, 1, 2]
    m[d, d] = m[d, d].max() / 2
    return m


def _read_sfm_scene(root):
    with open(os.path.join(root, "inputs", "sfm_scene.json")) as fh:
        return json.load(fh)


def read_neilf_scene(root, eval=False):
    """`<root>/inputs/sfm_scene.json` -> (train records, test records) as loadCamsFromScene / readNeILFInfo make them: only the
    entries of camera_track_map.images with flg == 2; fx, fy = intrinsic.focal, cx, cy = intrinsic.ppt, FovX = focal2fov(fx, W),
    FovY = focal2fov(fy, H); the camera centre moved through the inverse of the bbox transform, R = extrinsic[:3,:3]^T,
    T = extrinsic[:3,3] (float64); path = inputs/<file_paths[index]>, mask_path = inputs/pmasks/<basename>.png when that file exists
    (else None).  With `eval` the views whose int(index) is in NEILF_TEST_INDEXES are the test split; without it all views train.
    A record is what read_transforms returns plus uid, fx, fy, cx, cy, mask_path.  An RGBA image raises and names the file: the
    reference's reader would hand the Camera a 4-channel image."""
    scene = _read_sfm_scene(root)
    inputs = os.path.join(root, "inputs")
    bbox_inv = np.linalg.inv(_bbox_transform(scene))
    file_paths = scene["image_path"]["file_paths"]
    test_indexes = NEILF_TEST_INDEXES if eval else ()
    train, test = [], []
    for index, info in scene["camera_track_map"]["images"].items():
        if info["flg"] != 2:                                  # (2: a valid camera)
            continue
        fx, fy = info["camera"]["intrinsic"]["focal"][:2]
        cx, cy = info["camera"]["intrinsic"]["ppt"][:2]
        extrinsic = np.array(info["camera"]["extrinsic"], dtype=np.float64).reshape(4, 4)
        c2w = np.linalg.inv(extrinsic)
        c2w[:3, 3] = (c2w[:4, 3] @ bbox_inv.T)[:3]
        extrinsic = np.linalg.inv(c2w)
        path = os.path.join(inputs, file_paths[index])
        h, w, channels = probe(path)
        if channels != 3:
            raise RuntimeError("%s: an RGBA image in a NeILF-format dataset is not read (the reference's reader would hand its "
                               "Camera a 4-channel image); the mask of this layout is inputs/pmasks/<name>.png" % path)
        mask_path = os.path.join(inputs, "pmasks", os.path.splitext(os.path.basename(file_paths[index]))[0] + ".png")
        record = dict(name=os.path.splitext(os.path.basename(path))[0], path=path, uid=index, R=np.transpose(extrinsic[:3, :3]).copy(),
                      T=extrinsic[:3, 3].copy(), FovX=2 * math.atan(w / (2 * fx)), FovY=2 * math.atan(h / (2 * fy)), width=w,
                      height=h, fx=fx, fy=fy, cx=cx, cy=cy, mask_path=mask_path if os.path.exists(mask_path) else None)
        (test if int(index) in test_indexes else train).append(record)
    return train, test


def _projection_center_shift(znear, zfar, cx, cy, fx, fy, w, h):
    """getProjectionMatrixCenterShift (utils/graphics_utils.py:171-189): the frustum of a pinhole with its principal point at
    (cx, cy) pixels."""
    top, bottom = cy / fy * znear, -(h - cy) / fy * znear
    left, right = -(w - cx) / fx * znear, cx / fx * znear
    Pm = torch.zeros(4, 4)
    Pm[0, 0] = 2.0 * znear / (right - left)
    Pm[1, 1] = 2.0 * znear / (top - bottom)
    Pm[0, 2] = (right + left) / (right - left)
    Pm[1, 2] = (top + bottom) / (top - bottom)
    Pm[3, 2] = 1.0
    Pm[2, 2] = zfar / (zfar - znear)
    Pm[2, 3] = -(zfar * znear) / (zfar - znear)
    return Pm


def cameras_of(records, sizes=None, device=None, scales=None):
    """records (read_transforms / read_neilf_scene) -> synthetic.SynthCamera list with the matrices of scene/cameras.py:56-73:
    world_view_transform = float32(getWorld2View2(R, T))^T, the projection of getProjectionMatrix(0.01, 100, FovX, FovY),
    full_proj_transform their product, camera_center from the inverse -- the conventions relighting.camera_of and
    synthetic.look_at_camera follow.  A record with `fx` (the NeILF layout) takes getProjectionMatrixCenterShift(0.01, 100, cx, cy,
    fx, fy, W, H) instead and carries its cx, cy; all four are first divided by the view's resize scale (camera_utils.py:60-69).
    `sizes`: (height, width) per view (ViewStore.sizes); None: the records' own.  `scales`: ViewStore.scales; None: all 1."""
    cams = []
    for i, r in enumerate(records):
        h, w = (r["height"], r["width"]) if sizes is None else sizes[i]
        scale = 1 if scales is None else scales[i]
        rt = np.zeros((4, 4))
        rt[:3, :3] = np.transpose(r["R"])
        rt[:3, 3] = r["T"]
        rt[3, 3] = 1.0
        if r.get("fx") is None:
            rt = np.float32(np.linalg.inv(np.linalg.inv(rt)))     # getWorld2View2 with no translation goes there and back
        else:
            # ... and does so in float32 (getWorld2View rounds first): bit for bit what the reference's Camera holds.  Records
            # without fx keep the float64 round trip they have always had (within one float32 ulp of this).
            c2w = np.linalg.inv(np.float32(rt))
            c2w[:3, 3] = (c2w[:3, 3] + np.zeros(3)) * 1.0
            rt = np.float32(np.linalg.inv(c2w))
        wvt = torch.from_numpy(rt).transpose(0, 1).contiguous()
        fovx, fovy = float(r["FovX"]), float(r["FovY"])
        if r.get("fx") is None:
            cx, cy = w / 2.0, h / 2.0
            proj = synthetic._projection(0.01, 100.0, fovx, fovy).transpose(0, 1)
        else:
            fx, fy, cx, cy = r["fx"] / scale, r["fy"] / scale, r["cx"] / scale, r["cy"] / scale
            proj = _projection_center_shift(0.01, 100.0, cx, cy, fx, fy, int(w), int(h)).transpose(0, 1)
        full = (wvt.unsqueeze(0).bmm(proj.unsqueeze(0))).squeeze(0).contiguous()
        cam = synthetic.SynthCamera(int(h), int(w), fovx, fovy, math.tan(fovx * 0.5), math.tan(fovy * 0.5), float(cx), float(cy),
                                    wvt, full, wvt.inverse()[3, :3].contiguous())
        cams.append(cam if device is None else cam.to(device))
    return cams


def reference_view_order(n_views, seed=0):
    """train.py:115-119 as a callable iteration -> view index: a stack of all views, refilled when empty, from which every
    iteration pops a random entry (`randint(0, len - 1)` of a random.Random(seed)).  Every block of n_views picks is a
    permutation.  The callable keeps the stack: call it once per iteration, in order (the iteration number is not read)."""
    rng = random.Random(seed)
    stack = []

    def pick(iteration=None):
        if not stack:
            stack.extend(range(n_views))
        return stack.pop(rng.randint(0, len(stack) - 1))
    return pick


# ---- pixels ----------------------------------------------------------------------------------------------------------------
def unpack_reference(pixels_u8, bg, clamp=True):
    """What the reference's reader makes of a file's pixels [H,W,C] uint8 (C = 3 or 4) over the background `bg` [3], in NumPy
    float64 (scene/utils.py:47-48: img / 255; dataset_readers.py:246-249: rgb * a + bg * (1 - a), mask = a, ones without an alpha
    channel; camera_utils.py:35,56: .float(); cameras.py:34: clamp(0, 1)) -> (image [3,H,W], mask [1,H,W]) float32 CPU tensors.
    The CPU restatement of r3dg_view_unpack.  `clamp=False`: the image as loadCam resizes it, before the Camera's clamp."""
    px = np.asarray(pixels_u8)
    if px.dtype != np.uint8 or px.ndim != 3 or px.shape[2] not in (3, 4):
        raise RuntimeError("unpack_reference: pixels must be uint8 [H,W,3] or [H,W,4]")
    img = px / 255
    bg = np.asarray(torch.as_tensor(bg).detach().cpu().numpy() if isinstance(bg, torch.Tensor) else bg, dtype=np.float64).reshape(3)
    mask = np.ones_like(img[..., 0])
    if px.shape[2] == 4:
        mask = img[:, :, 3]
        img = img[:, :, :3] * img[:, :, 3:4] + bg * (1 - img[:, :, 3:4])
    image = torch.from_numpy(np.ascontiguousarray(img)).float().permute(2, 0, 1)
    image = (image.clamp(0.0, 1.0) if clamp else image).contiguous()
    return image, torch.from_numpy(np.ascontiguousarray(mask)).float().unsqueeze(0).contiguous()


def unpack_masked_reference(rgb_u8, mask_u8, clamp=True):
    """What the reference's NeILF reader makes of a file's pixels [H,W,3] uint8 and its mask file's [H,W] uint8 (scene/utils.py:47-57:
    img / 255 in float64; the mask as float32 with `mask[mask > 0.5] = 1`; dataset_readers.py:364: image *= mask; no background;
    camera_utils.py:35,56: .float(); cameras.py:34: clamp(0, 1)) -> (image [3,H,W], mask [1,H,W]) float32 CPU tensors.  The CPU
    restatement of r3dg_view_unpack_masked.  `clamp=False`: the image as loadCam resizes it, before the Camera's clamp."""
    px, mb = np.asarray(rgb_u8), np.asarray(mask_u8)
    if px.dtype != np.uint8 or px.ndim != 3 or px.shape[2] != 3 or mb.dtype != np.uint8 or mb.shape != px.shape[:2]:
        raise RuntimeError("unpack_masked_reference: pixels must be uint8 [H,W,3] and the mask uint8 [H,W]")
    mask = mb.astype(np.float32)
    mask[mask > 0.5] = 1.0
    img = px / 255
    img *= mask[..., np.newaxis]
    image = torch.from_numpy(np.ascontiguousarray(img)).float().permute(2, 0, 1)
    image = (image.clamp(0.0, 1.0) if clamp else image).contiguous()
    return image, torch.from_numpy(np.ascontiguousarray(mask)).float().unsqueeze(0).contiguous()


MAX_SCALE = 16                 # R3DG_VIEW_RESIZE_MAX_SCALE: bounds the filter's tap count


def view_scale(resolution, width):
    """loadCam's scale of a view `width` pixels wide with resolution_scale = 1 (camera_utils.py:13-32): 1, 2, 4, 8 are the scale;
    -1 rescales files wider than 1600 pixels to 1600; any other value is the target width.  RuntimeError for a scale below 1
    (upscaling is not built) or above MAX_SCALE."""
    if resolution in (1, 2, 4, 8):
        scale = resolution
    elif resolution == -1:
        scale = width / 1600 if width > 1600 else 1
    else:
        scale = width / resolution
    if not 1 <= scale <= MAX_SCALE:
        raise RuntimeError("--resolution %r on a view %d pixels wide is a scale of %g: %s" % (
            resolution, width, scale, "upscaling is not built" if scale < 1 else "scales above %d are not built" % MAX_SCALE))
    return scale


def target_size(height, width, scale):
    """(height, width) of loadCam's resized view (camera_utils.py:33)."""
    return int(height / scale), int(width / scale)


def resize_reference(image, mask, size):
    """loadCam's resize on CPU: image [3,H,W] float -> [3,h,w] by the antialiased bilinear filter, mask [1,H,W] (or None) -> [1,h,w]
    by nearest neighbour.  These are exactly the calls torchvision's tensor Resize(size, antialias=True) and Resize(size,
    interpolation=NEAREST) make.  The image is NOT clamped here (cameras.py:34 does that afterwards)."""
    size = (int(size[0]), int(size[1]))
    out = torch.nn.functional.interpolate(image.cpu()[None], size=size, mode="bilinear", align_corners=False, antialias=True)[0]
    out_mask = None if mask is None else torch.nn.functional.interpolate(mask.cpu()[None], size=size, mode="nearest")[0]
    return out, out_mask


def _decode(path, mask_path=None):
    from PIL import Image
    with Image.open(path) as im:
        if im.mode not in ("RGB", "RGBA"):
            raise RuntimeError("%s: image mode %r is not read (8-bit RGB or RGBA files only)" % (path, im.mode))
        t0 = time.perf_counter()
        arr = np.array(im, dtype=np.uint8)                  # (a writable copy: torch.from_numpy wants one)
    mask = None
    if mask_path is not None:
        with Image.open(mask_path) as im:                   # imageio.imread(mode="L"): PIL's conversion to 8-bit grey
            mask = np.ascontiguousarray(np.array(im.convert("L"), dtype=np.uint8))
    return np.ascontiguousarray(arr), mask, time.perf_counter() - t0


class _ViewSequence(collections.abc.Sequence):
    """store.images(bg) / store.masks(bg): indexable, with a len; what train_stage1 / train_stage2 / evaluate_nvs index."""

    def __init__(self, store, background, part):
        self.store, self.background, self.part = store, background, part

    def __len__(self):
        return len(self.store.views)

    def __getitem__(self, v):
        n = len(self.store.views)
        if not isinstance(v, (int, np.integer)):
            raise TypeError("a view index is an integer")
        if v < -n or v >= n:
            raise IndexError(v)
        return self.store._pair(int(v) % n, self.background, fresh=self.part == 0)[self.part]


class ViewStore:
    """All views of a split on the device as the 8-bit pixels their files hold.

    Loading: the files are decoded by PIL on at most 8 worker threads (`workers`; never the machine's whole CPU count), copied
    through pinned staging buffers into ONE uint8 device buffer -- view v at the 16-byte-aligned offset `views[v].offset`, with its
    (height, width, channels); views may differ in size -- `nbytes` in all.  `load_seconds`: {"decode": seconds the loading thread
    waited for decoded files, "upload": seconds it spent staging and copying, "decode_cpu": decoder seconds summed over the worker
    threads}.  Modes RGB and RGBA only; anything else raises a RuntimeError naming the file.

    `fetch(v, background)` -> (image [3,H,W], mask [1,H,W]): one r3dg_view_unpack launch on the caller's current stream into one of
    `slots` preallocated output pairs of that size.
    RING CONTRACT: a returned pair holds view v until `slots` further fetches of views of the same size; everything that reads it
    must have been QUEUED on the device by then (stream order does the rest).  Both fused steps queue every reader of the
    ground truth inside the call that receives it, and evaluate.evaluate_nvs queues each view's metric job before it indexes the
    next view.  Keep a view longer with .clone().
    The kernel writes through raw pointers, so a returned tensor's `_version` never moves.  FusedStage2Step caches its MVS pixel
    count under the depth map's and mask's `_version` (`_sup_counts`); that cache is only consulted with an MVS depth map, the
    training driver offers none (no `depth` / `normal_mvs_depth` term), so nothing stale can be read.  Do not pair these masks
    with MVS supervision without cloning them.

    `mask_paths[v]`: the mask file of RGB view v (the NeILF layout's inputs/pmasks), or None.  It is decoded as 8-bit grey and kept
    as a one-byte plane behind the view's pixels at a 16-byte-aligned offset (`views[v].mask_offset`): 3 + 1 bytes per pixel
    resident; `fetch` is then one r3dg_view_unpack_masked launch, which reads no background.

    `resolution`: loadCam's `--resolution` (`view_scale`).  A view of scale 1 is kept as above, byte for byte.  Any other view is
    resized ONCE, at load: its full-size bytes go through a transient device buffer, one r3dg_view_resize launch writes the
    float32 [3,h,w] image (and the [1,h,w] mask of a view with an alpha channel or a mask file) into resident tensors, and `fetch`
    returns those with no launch and no ring (`launches` does not grow; they are never overwritten).  The composite is baked in, so
    a store with resized RGBA views is built for ONE `background` (3 floats, required then) and `fetch` with another raises.
    `sizes` are the sizes after the resize, `scales` the scales (what cameras_of divides the intrinsics by).

    `images(background)` / `masks(background)`: lazy sequences over the views; `images[v]` fetches, and the `masks[v]` that
    follows it is the mask of that same launch.  `masks` returns None when no view has an alpha channel or a mask file: the loops
    then run as with masks=None (the reference's mask is all ones there).  There is no CPU path."""

    def __init__(self, paths, device="cuda", workers=None, slots=4, mask_paths=None, resolution=1, background=None):
        paths = [str(p) for p in paths]
        if not paths:
            raise RuntimeError("ViewStore: no views")
        if int(slots) < 1:
            raise RuntimeError("ViewStore: slots must be at least 1")
        mask_paths = [None] * len(paths) if mask_paths is None else [None if m is None else str(m) for m in mask_paths]
        if len(mask_paths) != len(paths):
            raise RuntimeError("ViewStore: mask_paths has one entry (a file or None) per view")
        self.paths, self.mask_paths, self.slots = paths, mask_paths, int(slots)
        self.workers = max(1, min(8, workers or (os.cpu_count() or 1)))
        shapes = [probe(p) for p in paths]                          # (raises for a file that is not RGB / RGBA, before anything else)
        for (h, w, c), p, m in zip(shapes, paths, mask_paths):
            if m is not None and c != 3:
                raise RuntimeError("%s: an RGBA image with a mask file (%s): its mask is the alpha channel" % (p, m))
        self.scales = [view_scale(resolution, w) for _, w, _ in shapes]           # (raises for upscaling / a scale above 16)
        self.dev = torch.device(device)
        if self.dev.type != "cuda":
            raise RuntimeError("ViewStore needs a device (there is no CPU path; unpack_reference is the NumPy restatement)")
        if self.dev.index is None:
            self.dev = torch.device("cuda", torch.cuda.current_device())
        pad = lambda n: -(-n // ALIGN) * ALIGN
        self.views, offset = [], 0
        for (h, w, c), m, scale in zip(shapes, mask_paths, self.scales):
            th, tw = target_size(h, w, scale)
            view = types.SimpleNamespace(offset=None, mask_offset=None, height=th, width=tw, channels=c, scale=scale, source=(h, w),
                                         masked=m is not None, image=None, mask=None)
            if scale == 1:
                view.offset = offset
                offset += pad(h * w * c)
                if m is not None:
                    view.mask_offset = offset
                    offset += pad(h * w)
            elif th < 1 or tw < 1:
                raise RuntimeError("ViewStore: --resolution %r leaves nothing of a %d x %d view" % (resolution, w, h))
            self.views.append(view)
        self.nbytes = offset
        self.sizes = [(v.height, v.width) for v in self.views]
        self.has_alpha = any(v.channels == 4 for v in self.views)
        self.has_masks = self.has_alpha or any(v.masked for v in self.views)
        self.background = None                                      # the one background of resized RGBA views
        if any(v.scale != 1 and v.channels == 4 for v in self.views):
            if background is None:
                raise RuntimeError("ViewStore: resized RGBA views are composited at load: pass the `background` they are for")
            self.background = self._key(background)
        self.pixels = torch.empty(self.nbytes, dtype=torch.uint8, device=self.dev)
        self._backgrounds, self._checked = {}, set()
        self.resizes = 0                                             # r3dg_view_resize launches, all of them at load
        self._load()
        f = dict(dtype=torch.float32, device=self.dev)
        self._rings = {}                                             # (H, W) -> [next slot, [(image, mask)] * slots]
        for h, w in sorted(set((v.height, v.width) for v in self.views if v.scale == 1)):
            self._rings[(h, w)] = [0, [(torch.empty(3, h, w, **f), torch.empty(1, h, w, **f)) for _ in range(self.slots)]]
        self._last = None                                            # (view, background pointer, image, mask) of the last fetch
        self.launches = 0

    def _load(self):
        pad = lambda n: -(-n // ALIGN) * ALIGN
        nbytes = lambda v: pad(v.source[0] * v.source[1] * v.channels) + (v.source[0] * v.source[1] if v.masked else 0)
        stage = [types.SimpleNamespace(host=torch.empty(max(nbytes(v) for v in self.views), dtype=torch.uint8, pin_memory=True),
                                       done=None) for _ in range(2)]
        resized = [v for v in self.views if v.scale != 1]
        # the full-size bytes of a view being resized: pixels, then its mask plane at a 16-byte-aligned offset; reused by the next
        # one (the copy into it is queued on the stream behind the launch that read it)
        transient = torch.empty(max(nbytes(v) for v in resized), dtype=torch.uint8, device=self.dev) if resized else None
        bg = None if self.background is None else torch.tensor(self.background, dtype=torch.float32, device=self.dev)
        f = dict(dtype=torch.float32, device=self.dev)
        wait = upload = decode_cpu = 0.0
        window = 2 * self.workers                                    # decoded files alive at once: bounded host memory
        with ThreadPoolExecutor(max_workers=self.workers) as pool, torch.cuda.device(self.dev):
            pending = collections.deque(pool.submit(_decode, p, m) for p, m in zip(self.paths[:window], self.mask_paths[:window]))
            submitted = len(pending)
            for i, view in enumerate(self.views):
                t0 = time.perf_counter()
                arr, mask_arr, seconds = pending.popleft().result()
                t1 = time.perf_counter()
                if submitted < len(self.paths):
                    pending.append(pool.submit(_decode, self.paths[submitted], self.mask_paths[submitted]))
                    submitted += 1
                h, w = view.source
                if arr.shape != (h, w, view.channels):
                    raise RuntimeError("%s: decoded to %s, its header said %s" % (self.paths[i], arr.shape, (h, w, view.channels)))
                if mask_arr is not None and mask_arr.shape != (h, w):
                    raise RuntimeError("%s: the mask is %d x %d, its image %d x %d" % (self.mask_paths[i], mask_arr.shape[1],
                                                                                      mask_arr.shape[0], w, h))
                n, at = arr.size, pad(arr.size)
                s = stage[i % 2]
                if s.done is not None:
                    s.done.synchronize()                             # (the copy out of this staging buffer two views ago)
                s.host[:n].copy_(torch.from_numpy(arr).reshape(-1))
                if mask_arr is not None:
                    s.host[at:at + h * w].copy_(torch.from_numpy(mask_arr).reshape(-1))
                if view.scale == 1:
                    self.pixels[view.offset:view.offset + n].copy_(s.host[:n], non_blocking=True)
                    if mask_arr is not None:
                        self.pixels[view.mask_offset:view.mask_offset + h * w].copy_(s.host[at:at + h * w], non_blocking=True)
                else:
                    transient[:n].copy_(s.host[:n], non_blocking=True)
                    if mask_arr is not None:
                        transient[at:at + h * w].copy_(s.host[at:at + h * w], non_blocking=True)
                    view.image = torch.empty(3, view.height, view.width, **f)
                    if view.channels == 4 or view.masked:
                        view.mask = torch.empty(1, view.height, view.width, **f)
                    elif self.has_masks:                             # (beside views that have one: the reference's all-ones mask)
                        view.mask = torch.ones(1, view.height, view.width, **f)
                    _lib.check(_lib.lib().r3dg_view_resize(
                        _lib.current_stream(), w, h, view.channels, transient.data_ptr(),
                        transient.data_ptr() + at if view.masked else None, None if bg is None else bg.data_ptr(), view.width,
                        view.height, view.image.data_ptr(),
                        view.mask.data_ptr() if (view.channels == 4 or view.masked) else None), "view_resize")
                    self.resizes += 1
                s.done = torch.cuda.Event()
                s.done.record()
                wait += t1 - t0
                upload += time.perf_counter() - t1
                decode_cpu += seconds
            t1 = time.perf_counter()
            torch.cuda.current_stream().synchronize()
            upload += time.perf_counter() - t1
        self.load_seconds = dict(decode=wait, upload=upload, decode_cpu=decode_cpu)

    def _background(self, background):
        if isinstance(background, torch.Tensor) and background.device == self.dev and background.dtype == torch.float32 and \
                background.numel() == 3 and background.is_contiguous():
            return background
        key = self._key(background)
        t = self._backgrounds.get(key)
        if t is None:
            t = self._backgrounds[key] = torch.tensor(key, dtype=torch.float32, device=self.dev)
        return t

    @staticmethod
    def _key(background):
        key = tuple(float(x) for x in (background.detach().cpu().reshape(-1).tolist() if isinstance(background, torch.Tensor)
                                        else background))
        if len(key) != 3:
            raise RuntimeError("ViewStore: a background is 3 floats")
        return tuple(float(np.float32(x)) for x in key)

    def fetch(self, v, background):
        view = self.views[v]
        bg = self._background(background)
        if view.image is not None:                                   # resized at load: resident, no launch, no ring
            if view.channels == 4 and bg.data_ptr() not in self._checked:
                if self._key(bg) != self.background:                 # (one host read per background tensor, not per fetch)
                    raise RuntimeError("ViewStore: its resized RGBA views were composited over the background %s at load; "
                                       "fetch with another background (%s) needs another store"
                                       % (self.background, self._key(bg)))
                self._checked.add(bg.data_ptr())
            self._last = (v, bg.data_ptr(), view.image, view.mask)
            return view.image, view.mask
        ring = self._rings[(view.height, view.width)]
        image, mask = ring[1][ring[0]]
        ring[0] = (ring[0] + 1) % self.slots
        if view.masked:
            call = lambda: _lib.check(_lib.lib().r3dg_view_unpack_masked(
                _lib.current_stream(), view.width, view.height, self.pixels.data_ptr() + view.offset,
                self.pixels.data_ptr() + view.mask_offset, image.data_ptr(), mask.data_ptr()), "view_unpack_masked")
        else:
            call = lambda: _lib.check(_lib.lib().r3dg_view_unpack(
                _lib.current_stream(), view.width, view.height, view.channels, self.pixels.data_ptr() + view.offset,
                bg.data_ptr(), image.data_ptr(), mask.data_ptr()), "view_unpack")
        if torch.cuda.current_device() == self.dev.index:
            call()
        else:
            with torch.cuda.device(self.dev):
                call()
        self.launches += 1
        self._last = (v, bg.data_ptr(), image, mask)
        return image, mask

    def _pair(self, v, background, fresh):
        """(image, mask) of view v: a new launch for `fresh` (images[v]); the last launch's pair when it was this view over this
        background (the masks[v] behind an images[v]), else a new launch."""
        last = self._last
        if not fresh and last is not None and last[0] == v and last[1] == self._background(background).data_ptr():
            return last[2], last[3]
        return self.fetch(v, background)

    def images(self, background):
        return _ViewSequence(self, background, 0)

    def masks(self, background):
        return _ViewSequence(self, background, 1) if self.has_masks else None

    def float_nbytes(self):
        """Bytes the same views take as resident float images + masks (16 per pixel)."""
        return sum(16 * v.height * v.width for v in self.views)

    def resident_nbytes(self):
        """Bytes the views occupy on the device: the 8-bit buffer and the float tensors of the resized ones (the rings not counted)."""
        return self.nbytes + sum(t.numel() * 4 for v in self.views for t in (v.image, v.mask) if t is not None)


# ---- initial points --------------------------------------------------------------------------------------------------------
def read_points_ply(path):
    """A binary little-endian PLY with one vertex element of scalar properties (what storePly writes) -> structured array."""
    with open(path, "rb") as fh:
        data = fh.read()
    end = data.find(b"end_header\n")
    if not data.startswith(b"ply") or end < 0:
        raise RuntimeError("%s: not a PLY file" % path)
    fields, count, in_vertex = [], None, False
    for line in data[:end].decode("ascii", "replace").splitlines():
        tok = line.split()
        if tok[:1] == ["format"] and tok[1:2] != ["binary_little_endian"]:
            raise RuntimeError("%s: only binary_little_endian PLY files are read" % path)
        if tok[:1] == ["element"]:
            if count is not None and not in_vertex:
                break
            in_vertex = tok[1] == "vertex"
            if in_vertex:
                count = int(tok[2])
            elif count is None:
                raise RuntimeError("%s: the vertex element must come first" % path)
        elif tok[:1] == ["property"] and in_vertex:
            if len(tok) != 3 or tok[1] not in _PLY_TYPES:
                raise RuntimeError("%s: property %r is not a scalar this reader knows" % (path, line))
            fields.append((tok[2], _PLY_TYPES[tok[1]]))
    if count is None:
        raise RuntimeError("%s: no vertex element" % path)
    return np.frombuffer(data, dtype=np.dtype(fields), count=count, offset=end + len(b"end_header\n"))


def write_points_ply(path, xyz, rgb, normals):
    """storePly (dataset_readers.py:143-160): float xyz, float normals, uchar rgb (the colour floats truncated to bytes)."""
    elements = np.empty(xyz.shape[0], dtype=np.dtype(list(_PLY_FIELDS)))
    attributes = np.concatenate((xyz, normals, rgb), axis=1)
    for j, (name, _) in enumerate(_PLY_FIELDS):
        elements[name] = attributes[:, j]
    names = {"<f4": "float", "u1": "uchar"}
    header = ["ply", "format binary_little_endian 1.0", "element vertex %d" % xyz.shape[0]] + \
             ["property %s %s" % (names[t], n) for n, t in _PLY_FIELDS] + ["end_header"]
    with open(path, "wb") as fh:
        fh.write(("\n".join(header) + "\n").encode("ascii"))
        fh.write(elements.tobytes())


def initial_points(root, seed=0):
    """`<root>/points3d.ply` as fetchPly reads it (dataset_readers.py:125-140) -> (points [N,3] float32, colors [N,3] float32 in
    [0,1], normals [N,3]); all-zero normals are replaced by uniform random ones in [0,1) as :136-138 does.  A missing file is
    first written as :288-299 does: 100 000 points uniform in [-1.3, 1.3]^3, colours SH2RGB(random / 255) * 255 truncated to bytes,
    unit random normals.  Every draw comes from a NumPy generator seeded with `seed` (the reference uses the global one)."""
    rng = np.random.RandomState(seed)
    path = os.path.join(root, "points3d.ply")
    if not os.path.exists(path):
        xyz = rng.random_sample((RANDOM_POINTS, 3)) * 2.6 - 1.3
        shs = rng.random_sample((RANDOM_POINTS, 3)) / 255.0
        normals = rng.randn(*xyz.shape)
        normals /= np.linalg.norm(normals, axis=-1, keepdims=True)
        write_points_ply(path, xyz, (shs * C0 + 0.5) * 255, normals)
    v = read_points_ply(path)
    points = np.vstack([v["x"], v["y"], v["z"]]).T
    colors = np.vstack([v["red"], v["green"], v["blue"]]).T
    if colors.dtype == np.uint8:
        colors = colors.astype(np.float32)
        colors /= 255.0
    normals = np.vstack([v["nx"], v["ny"], v["nz"]]).T
    if np.all(normals == 0):
        normals = rng.random_sample(normals.shape)
    return points, colors, normals


def initial_points_neilf(root, seed=0):
    """The point cloud of readNeILFInfo (dataset_readers.py:408-425): `<root>/inputs/model/sparse.ply` read as fetchPly reads it,
    its positions moved through the inverse of the bbox transform (the one read_neilf_scene moves the cameras through), written
    to `inputs/model/sparse_bbx_scale.ply` exactly as storePly would (colours * 255 truncated to bytes) and read back.
    -> (points [N,3] float32, colors [N,3] float32 in [0,1], normals [N,3]), with all-zero normals replaced as in initial_points."""
    rng = np.random.RandomState(seed)
    model = os.path.join(root, "inputs", "model")

    def fetch(path):
        v = read_points_ply(path)
        colors = np.vstack([v["red"], v["green"], v["blue"]]).T
        if colors.dtype == np.uint8:
            colors = colors.astype(np.float32)
            colors /= 255.0
        normals = np.vstack([v["nx"], v["ny"], v["nz"]]).T
        if np.all(normals == 0):
            normals = rng.random_sample(normals.shape)
        return np.vstack([v["x"], v["y"], v["z"]]).T, colors, normals

    points, colors, normals = fetch(os.path.join(model, "sparse.ply"))
    inverse = np.linalg.inv(_bbox_transform(_read_sfm_scene(root)))
    xyz = (np.concatenate([points, np.ones_like(points[:, :1])], axis=-1) @ inverse.T)[:, :3]
    path = os.path.join(model, "sparse_bbx_scale.ply")
    write_points_ply(path, xyz, colors * 255, normals)
    return fetch(path)
