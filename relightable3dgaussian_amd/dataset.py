"""A NeRF-synthetic (Blender) dataset directory as what the fused iterations take: the reference's readNerfSyntheticInfo /
readCamerasFromTransforms (scene/dataset_readers.py:215-312), with the ground-truth views kept ON THE DEVICE as the 8-bit pixels
their files hold.

    records = read_transforms(root, "train")                 # name, path, R, T, FovX, FovY (+ width, height) per frame
    store = ViewStore([r["path"] for r in records], device)  # one uint8 device buffer, 4 bytes per RGBA pixel instead of 16
    cameras = cameras_of(records, store.sizes, device)       # synthetic.SynthCamera, the matrices of scene/cameras.py:56-73
    train_loop.train_stage1(init, cameras, store.images(bg), bg, extent, masks=store.masks(bg),
                            view_order=reference_view_order(len(cameras), seed))

`ViewStore.fetch` is ONE r3dg_view_unpack launch (csrc/view_store.hip) that composites the chosen view onto the background and
splits off its alpha channel as the mask, bit for bit as the reference's reader does on the host; `unpack_reference` is the same
arithmetic in NumPy, the yardstick of the GPU tests.  `initial_points` is the reader's points3d.ply (fetchPly / storePly, :125-160,
and the 100 000 random points of :288-299), `reference_view_order` the view pick of train.py:115-119.

Out of scope: the COLMAP, NeILF, Synthetic4Relight and Stanford-ORB readers; `--resolution` other than the files' own (the
reference resizes with torchvision's antialiased Resize); MVS depth / normal maps (`<root>/extra`); `cfg_args`, `cameras.json`.
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


def cameras_of(records, sizes=None, device=None):
    """records (read_transforms) -> synthetic.SynthCamera list with the matrices of scene/cameras.py:56-73: world_view_transform =
    float32(getWorld2View2(R, T))^T, the projection of getProjectionMatrix(0.01, 100, FovX, FovY), full_proj_transform their
    product, camera_center from the inverse -- the conventions relighting.camera_of and synthetic.look_at_camera follow.
    `sizes`: (height, width) per view (ViewStore.sizes); None: the records' own."""
    cams = []
    for i, r in enumerate(records):
        h, w = (r["height"], r["width"]) if sizes is None else sizes[i]
        rt = np.zeros((4, 4))
        rt[:3, :3] = np.transpose(r["R"])
        rt[:3, 3] = r["T"]
        rt[3, 3] = 1.0
        rt = np.float32(np.linalg.inv(np.linalg.inv(rt)))     # getWorld2View2 with no translation goes there and back
        wvt = torch.from_numpy(rt).transpose(0, 1).contiguous()
        fovx, fovy = float(r["FovX"]), float(r["FovY"])
        proj = synthetic._projection(0.01, 100.0, fovx, fovy).transpose(0, 1)
        full = (wvt.unsqueeze(0).bmm(proj.unsqueeze(0))).squeeze(0).contiguous()
        cam = synthetic.SynthCamera(int(h), int(w), fovx, fovy, math.tan(fovx * 0.5), math.tan(fovy * 0.5), w / 2.0, h / 2.0,
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
def unpack_reference(pixels_u8, bg):
    """What the reference's reader makes of a file's pixels [H,W,C] uint8 (C = 3 or 4) over the background `bg` [3], in NumPy
    float64 (scene/utils.py:47-48: img / 255; dataset_readers.py:246-249: rgb * a + bg * (1 - a), mask = a, ones without an alpha
    channel; camera_utils.py:35,56: .float(); cameras.py:34: clamp(0, 1)) -> (image [3,H,W], mask [1,H,W]) float32 CPU tensors.
    The CPU restatement of r3dg_view_unpack."""
    px = np.asarray(pixels_u8)
    if px.dtype != np.uint8 or px.ndim != 3 or px.shape[2] not in (3, 4):
        raise RuntimeError("unpack_reference: pixels must be uint8 [H,W,3] or [H,W,4]")
    img = px / 255
    bg = np.asarray(torch.as_tensor(bg).detach().cpu().numpy() if isinstance(bg, torch.Tensor) else bg, dtype=np.float64).reshape(3)
    mask = np.ones_like(img[..., 0])
    if px.shape[2] == 4:
        mask = img[:, :, 3]
        img = img[:, :, :3] * img[:, :, 3:4] + bg * (1 - img[:, :, 3:4])
    image = torch.from_numpy(np.ascontiguousarray(img)).float().permute(2, 0, 1).clamp(0.0, 1.0).contiguous()
    return image, torch.from_numpy(np.ascontiguousarray(mask)).float().unsqueeze(0).contiguous()


def _decode(path):
    from PIL import Image
    with Image.open(path) as im:
        if im.mode not in ("RGB", "RGBA"):
            raise RuntimeError("%s: image mode %r is not read (8-bit RGB or RGBA files only)" % (path, im.mode))
        t0 = time.perf_counter()
        arr = np.array(im, dtype=np.uint8)                  # (a writable copy: torch.from_numpy wants one)
    return np.ascontiguousarray(arr), time.perf_counter() - t0


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

    `images(background)` / `masks(background)`: lazy sequences over the views; `images[v]` fetches, and the `masks[v]` that
    follows it is the mask of that same launch.  `masks` returns None when no view has an alpha channel: the loops then run as
    with masks=None (the reference's mask is all ones there).  There is no CPU path."""

    def __init__(self, paths, device="cuda", workers=None, slots=4):
        paths = [str(p) for p in paths]
        if not paths:
            raise RuntimeError("ViewStore: no views")
        if int(slots) < 1:
            raise RuntimeError("ViewStore: slots must be at least 1")
        self.paths, self.slots = paths, int(slots)
        self.workers = max(1, min(8, workers or (os.cpu_count() or 1)))
        shapes = [probe(p) for p in paths]                          # (raises for a file that is not RGB / RGBA, before anything else)
        self.dev = torch.device(device)
        if self.dev.type != "cuda":
            raise RuntimeError("ViewStore needs a device (there is no CPU path; unpack_reference is the NumPy restatement)")
        if self.dev.index is None:
            self.dev = torch.device("cuda", torch.cuda.current_device())
        self.views, offset = [], 0
        for h, w, c in shapes:
            self.views.append(types.SimpleNamespace(offset=offset, height=h, width=w, channels=c))
            offset += -(-h * w * c // ALIGN) * ALIGN
        self.nbytes = offset
        self.sizes = [(v.height, v.width) for v in self.views]
        self.has_alpha = any(v.channels == 4 for v in self.views)
        self.pixels = torch.empty(self.nbytes, dtype=torch.uint8, device=self.dev)
        self._load()
        f = dict(dtype=torch.float32, device=self.dev)
        self._rings = {}                                             # (H, W) -> [next slot, [(image, mask)] * slots]
        for h, w in sorted(set(self.sizes)):
            self._rings[(h, w)] = [0, [(torch.empty(3, h, w, **f), torch.empty(1, h, w, **f)) for _ in range(self.slots)]]
        self._backgrounds = {}
        self._last = None                                            # (view, background pointer, image, mask) of the last fetch
        self.launches = 0

    def _load(self):
        largest = max(v.height * v.width * v.channels for v in self.views)
        stage = [types.SimpleNamespace(host=torch.empty(largest, dtype=torch.uint8, pin_memory=True), done=None) for _ in range(2)]
        wait = upload = decode_cpu = 0.0
        window = 2 * self.workers                                    # decoded files alive at once: bounded host memory
        with ThreadPoolExecutor(max_workers=self.workers) as pool, torch.cuda.device(self.dev):
            pending = collections.deque(pool.submit(_decode, p) for p in self.paths[:window])
            submitted = len(pending)
            for i, view in enumerate(self.views):
                t0 = time.perf_counter()
                arr, seconds = pending.popleft().result()
                t1 = time.perf_counter()
                if submitted < len(self.paths):
                    pending.append(pool.submit(_decode, self.paths[submitted]))
                    submitted += 1
                if arr.shape != (view.height, view.width, view.channels):
                    raise RuntimeError("%s: decoded to %s, its header said %s" % (self.paths[i], arr.shape,
                                                                                  (view.height, view.width, view.channels)))
                n = arr.size
                s = stage[i % 2]
                if s.done is not None:
                    s.done.synchronize()                             # (the copy out of this staging buffer two views ago)
                s.host[:n].copy_(torch.from_numpy(arr).reshape(-1))
                self.pixels[view.offset:view.offset + n].copy_(s.host[:n], non_blocking=True)
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
        key = tuple(float(x) for x in (background.detach().cpu().reshape(-1).tolist() if isinstance(background, torch.Tensor)
                                        else background))
        if len(key) != 3:
            raise RuntimeError("ViewStore: a background is 3 floats")
        t = self._backgrounds.get(key)
        if t is None:
            t = self._backgrounds[key] = torch.tensor(key, dtype=torch.float32, device=self.dev)
        return t

    def fetch(self, v, background):
        view = self.views[v]
        bg = self._background(background)
        ring = self._rings[(view.height, view.width)]
        image, mask = ring[1][ring[0]]
        ring[0] = (ring[0] + 1) % self.slots
        call = lambda: _lib.check(_lib.lib().r3dg_view_unpack(
            _lib.current_stream(), view.width, view.height, view.channels, self.pixels.data_ptr() + view.offset, bg.data_ptr(),
            image.data_ptr(), mask.data_ptr()), "view_unpack")
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
        return _ViewSequence(self, background, 1) if self.has_alpha else None

    def float_nbytes(self):
        """Bytes the same views take as resident float images + masks (16 per pixel)."""
        return sum(16 * v.height * v.width for v in self.views)


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
