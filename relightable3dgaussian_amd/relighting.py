"""The reference's composition and relighting tool (relighting.py) on the fast path:

    python -m relightable3dgaussian_amd.relighting -co configs/nerf_syn -e env.hdr --output out --capture_list pbr_env,normal

reads `transform.json`, `trajectory.json` and the optional `light_transform.json` of a reference config directory
(compose.load_scene_config), assembles the composite from the objects' PLY files on the device (compose.assemble), traces its
visibility once (RelightRenderer(device_visibility=True); with --bake: visibility_bake.bake_visibility on the composite and
RelightRenderer(baked_visibility=True)), walks the trajectory with the cameras of relighting.py:159-165 and each frame's light
transform, and writes OUTPUT/<capture>/frame_<idx>.png with the background rules of relighting.py:172-181.  Frames are quantised on
the device (r3dg_relight_quantize, the rounding of torchvision's save_image), copied asynchronously into a ring of pinned host
buffers and encoded by PIL on worker threads while the next frame renders; with --device_png the encoder runs on the device too
(png_device.py) and the workers only frame and write the files.  `render_trajectory` is the same loop as a generator
of device frames, for callers that want no files.

Arguments are those of relighting.py:88-101 plus --rotate-sh (compose.assemble), --fovx (the reference hard-codes
0.6911112070083618), --envmap_scale, --bake_iterations and --device_png.  --video is not offered (there is no cv2 here) and the `points`
capture raises.

Environment maps: `.npy` ([He,We,3] linear radiance) and Radiance `.hdr` (RGBE, flat or run-length encoded scanlines) are read
as LINEAR radiance; `.exr` raises (np.save("envmap3.npy", exr.read_image("envmap3.exr")) is the bridge for the
NONE / ZIPS / ZIP scanline files exr.py decodes; PIZ files, the reference's envmap6 / envmap12, are not decoded).  Note the
difference: the reference treats every non-EXR file as an 8-bit sRGB image (scene/envmap.py:23-24: srgb_to_rgb(imread(path) / 255)); this tool does not."""
import argparse
import math
import os
import queue
import types
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import _lib, compose, relight, synthetic

DEFAULT_FOVX = 0.6911112070083618
# the captures relighting.py:178-179 puts over the background (`normal` too, after * 0.5 + 0.5; everything else as rendered)
OVER_BACKGROUND = ("base_color", "roughness", "visibility")


def read_hdr(path):
    """Radiance RGBE picture (-Y H +X W; flat or new-style run-length encoded scanlines) -> float32 [H,W,3] linear radiance."""
    with open(path, "rb") as fh:
        data = fh.read()
    if not data.startswith(b"#?"):
        raise RuntimeError("%s: not a Radiance picture (no #? signature)" % path)
    end = data.find(b"\n\n")
    if end < 0:
        raise RuntimeError("%s: the Radiance header does not end" % path)
    if b"FORMAT=32-bit_rle_rgbe" not in data[:end]:
        raise RuntimeError("%s: only FORMAT=32-bit_rle_rgbe is read" % path)
    eol = data.find(b"\n", end + 2)
    tok = data[end + 2:eol].split()
    if len(tok) != 4 or tok[0] != b"-Y" or tok[2] != b"+X":
        raise RuntimeError("%s: resolution line %r: only `-Y H +X W` is read" % (path, data[end + 2:eol]))
    H, W = int(tok[1]), int(tok[3])
    raw = np.frombuffer(data, np.uint8, offset=eol + 1)
    out = np.empty((H, W, 4), np.uint8)
    pos = 0
    for y in range(H):
        if 8 <= W < 32768 and pos + 4 <= raw.size and raw[pos] == 2 and raw[pos + 1] == 2 and \
                (int(raw[pos + 2]) << 8 | int(raw[pos + 3])) == W:
            pos += 4
            for c in range(4):
                x = 0
                while x < W:
                    if pos >= raw.size:
                        raise RuntimeError("%s: scanline %d ends early" % (path, y))
                    n = int(raw[pos])
                    if n > 128:                                  # a run
                        n -= 128
                        if n == 0 or x + n > W or pos + 1 >= raw.size:
                            raise RuntimeError("%s: bad run in scanline %d" % (path, y))
                        out[y, x:x + n, c] = raw[pos + 1]
                        pos += 2
                    else:                                        # literals
                        if n == 0 or x + n > W or pos + 1 + n > raw.size:
                            raise RuntimeError("%s: bad literal block in scanline %d" % (path, y))
                        out[y, x:x + n, c] = raw[pos + 1:pos + 1 + n]
                        pos += 1 + n
                    x += n
        else:
            if pos + 4 * W > raw.size:
                raise RuntimeError("%s: scanline %d ends early" % (path, y))
            out[y] = raw[pos:pos + 4 * W].reshape(W, 4)
            pos += 4 * W
    e = out[..., 3].astype(np.int32)
    scale = np.where(e > 0, np.ldexp(1.0, e - 136), 0.0)
    return (out[..., :3].astype(np.float64) * scale[..., None]).astype(np.float32)


def load_envmap(path, scale=1.0, device="cuda"):
    """-> [He,We,3] float32 linear radiance on the device, times `scale`."""
    ext = os.path.splitext(str(path))[1].lower()
    if ext == ".npy":
        env = np.load(path)
    elif ext == ".hdr":
        env = read_hdr(path)
    else:
        raise RuntimeError("%s: environment maps are read from .npy ([He,We,3] linear radiance) or Radiance .hdr files; "
                           "%s is not supported (there is no EXR decoder here)" % (path, ext or "this file"))
    if env.ndim != 3 or env.shape[2] != 3:
        raise RuntimeError("%s: an environment map is [He,We,3], got %s" % (path, env.shape))
    return (torch.from_numpy(np.ascontiguousarray(env, dtype=np.float32)) * float(scale)).to(device).contiguous()


def camera_of(w2c, width, height, fovx=DEFAULT_FOVX, device=None):
    """The camera relighting.py:159-165 builds from a world-to-camera matrix [4,4] (R = w2c[:3,:3]^T, T = w2c[:3,3], FoVy from the
    focal length of FoVx) with the matrices of scene/cameras.py:62-73."""
    w2c = torch.as_tensor(np.asarray(w2c, dtype=np.float32).reshape(4, 4)).clone()
    w2c[3] = torch.tensor([0.0, 0.0, 0.0, 1.0])
    fovy = 2 * math.atan(height / (2 * (width / (2 * math.tan(fovx / 2)))))
    wvt = w2c.transpose(0, 1).contiguous()
    proj = synthetic._projection(0.01, 100.0, fovx, fovy).transpose(0, 1)
    full = (wvt.unsqueeze(0).bmm(proj.unsqueeze(0))).squeeze(0).contiguous()
    cam = synthetic.SynthCamera(height, width, fovx, fovy, math.tan(fovx * 0.5), math.tan(fovy * 0.5), width / 2.0, height / 2.0,
                                wvt, full, wvt.inverse()[3, :3].contiguous())
    return cam if device is None else cam.to(device)


def quantize(image, out=None):
    """r3dg_relight_quantize: [C,H,W] float32 on the device -> [H,W,C] uint8 as save_image rounds, clamp(x * 255 + 0.5, 0, 255)
    truncated."""
    if not isinstance(image, torch.Tensor) or not image.is_cuda or image.dtype != torch.float32 or image.dim() != 3 or \
            not 1 <= image.shape[0] <= 4:
        raise RuntimeError("quantize: the image must be float32 [C,H,W] with 1 <= C <= 4 on the device (there is no CPU path)")
    C, H, W = image.shape
    if out is None:
        out = torch.empty(H, W, C, dtype=torch.uint8, device=image.device)
    elif not out.is_cuda or out.dtype != torch.uint8 or tuple(out.shape) != (H, W, C) or not out.is_contiguous() or \
            out.device != image.device:
        raise RuntimeError("quantize: the output must be contiguous uint8 [H,W,C] on the image's device")
    image = image.contiguous()
    with torch.cuda.device(image.device):
        _lib.check(_lib.lib().r3dg_relight_quantize(_lib.current_stream(), W, H, C, image.data_ptr(), out.data_ptr()),
                   "relight_quantize")
    return out


class FrameWriter:
    """PNG output beside the renderer: `submit(image [C,H,W], path)` quantises on the device into one slot of a small ring,
    starts the asynchronous copy into the slot's pinned host buffer and hands the encoding (PIL) to a pool of at most 8 worker
    threads.  submit blocks only when every slot is still being encoded; `close` waits for the files and raises what a worker
    raised.  `submit_bytes(bytes [H,W,C] uint8, path)` takes a picture that is 8-bit already (training_vis) through the same ring,
    copy, event and workers without the quantise launch.

    `device_png=True` (opt-in) moves the encoder onto the device: submit quantises and encodes (png_device.encode: filter, deflate
    and Adler-32 in three launches), the slot's pinned buffer has the size of the stream's bound plus the length word, and the
    worker reads the length, frames the stream as a PNG file (png_device.wrap: one CRC-32) and writes it; PIL is not used.  The
    ring, the back-pressure, close() and the raising of a worker's error are the same."""

    def __init__(self, workers=None, slots=None, device_png=False):
        self.device_png = bool(device_png)
        self.workers = max(1, min(8, workers or (os.cpu_count() or 1)))
        self.pool = ThreadPoolExecutor(max_workers=self.workers)
        self.free = queue.Queue()
        for _ in range(slots or self.workers + 2):
            self.free.put(types.SimpleNamespace(dev=None, host=None))
        self.jobs = []

    def submit(self, image, path):
        if self.device_png:
            return self._submit_device(image, None, path)
        C, H, W = image.shape
        slot = self.free.get()
        if slot.dev is None or tuple(slot.dev.shape) != (H, W, C) or slot.dev.device != image.device:
            slot.dev = torch.empty(H, W, C, dtype=torch.uint8, device=image.device)
            slot.host = torch.empty(H, W, C, dtype=torch.uint8, pin_memory=True)
        quantize(image, slot.dev)
        slot.host.copy_(slot.dev, non_blocking=True)
        done = torch.cuda.Event()
        done.record()
        self.jobs.append(self.pool.submit(self._encode, slot, done, path))

    def submit_bytes(self, bytes_dev, path):
        """The same for a picture that is 8-bit already ([H,W,C] uint8 on the device, contiguous: r3dg_training_sheet's output): no
        quantise launch, the asynchronous copy goes from the caller's tensor straight into the slot's pinned host buffer.  The copy
        is queued on the current stream, so the caller may overwrite `bytes_dev` with later work of that stream."""
        if not isinstance(bytes_dev, torch.Tensor) or not bytes_dev.is_cuda or bytes_dev.dtype != torch.uint8 or \
                bytes_dev.dim() != 3 or not 1 <= bytes_dev.shape[2] <= 4 or not bytes_dev.is_contiguous():
            raise RuntimeError("submit_bytes: the picture must be a contiguous uint8 [H,W,C] with 1 <= C <= 4 on the device")
        if self.device_png:
            return self._submit_device(None, bytes_dev, path)
        slot = self.free.get()
        if slot.host is None or tuple(slot.host.shape) != tuple(bytes_dev.shape):
            slot.dev = None                  # (a slot that changes size drops the device half `submit` would have to match)
            slot.host = torch.empty(tuple(bytes_dev.shape), dtype=torch.uint8, pin_memory=True)
        slot.host.copy_(bytes_dev, non_blocking=True)
        done = torch.cuda.Event()
        done.record()
        self.jobs.append(self.pool.submit(self._encode, slot, done, path))

    def _encode(self, slot, done, path):
        from PIL import Image
        try:
            done.synchronize()
            arr = slot.host.numpy()
            Image.fromarray(arr[..., 0] if arr.shape[-1] == 1 else arr).save(path)
        finally:
            self.free.put(slot)

    def _submit_device(self, image, bytes_dev, path):
        """The device encoder's half of submit (an image [C,H,W] to quantise first) and submit_bytes (a picture [H,W,C])."""
        from . import png_device
        if bytes_dev is None:
            C, H, W = image.shape
            dev = image.device
        else:
            H, W, C = bytes_dev.shape
            dev = bytes_dev.device
        slot = self.free.get()
        try:
            if getattr(slot, "shape", None) != (H, W, C) or slot.stream.device != dev:
                n = 4 + png_device.zlib_bound(W, H, C)                  # the length word, then the stream
                slot.stream = torch.empty(n, dtype=torch.uint8, device=dev)
                slot.host = torch.empty(n, dtype=torch.uint8, pin_memory=True)
                slot.dev = torch.empty(H, W, C, dtype=torch.uint8, device=dev)
                slot.shape = (H, W, C)
            if bytes_dev is None:
                bytes_dev = quantize(image, slot.dev)
            png_device.encode(bytes_dev, out=(slot.stream[4:], slot.stream[:4].view(torch.int32)))
            slot.host.copy_(slot.stream, non_blocking=True)
            done = torch.cuda.Event()
            done.record()
        except BaseException:
            self.free.put(slot)
            raise
        self.jobs.append(self.pool.submit(self._write, slot, done, path))

    def _write(self, slot, done, path):
        from . import png_device
        try:
            done.synchronize()
            host = slot.host.numpy()
            n = int(host[:4].view(np.int32)[0])
            H, W, C = slot.shape
            data = png_device.wrap(host[4:4 + n].tobytes(), W, H, C)
            with open(path, "wb") as fh:
                fh.write(data)
        finally:
            self.free.put(slot)

    def close(self):
        self.pool.shutdown(wait=True)
        for j in self.jobs:
            j.result()


@torch.no_grad()
def render_trajectory(composite, envmap, cameras, light_transforms=None, captures=("pbr_env",), sample_num=64, bg=0.0,
                      bake=False, bake_iterations=1000, renderer=None):
    """Generator of (index, {capture: [C,H,W] device tensor}) over `cameras`.  `composite`: what compose.assemble returns (or a
    namespace of the same tensors); `light_transforms`: one [3,3] per camera, or None; `captures`: names of relighting.py's
    --capture_list (any output of RelightRenderer.frame; `normal`, `base_color`, `roughness`, `visibility` are put over `bg` as
    relighting.py:172-181 does).  The composite's visibility is traced once, on the device; `bake`: bake_visibility(composite)
    and the baked renderer instead."""
    captures = tuple(captures)
    for c in captures:
        if c == "points":
            raise RuntimeError("capture 'points' (the reference's point-splat debug view) is not offered")
        if c not in relight.CAPTURE_MAPS and c not in relight.COMPOSITES and c != "render":
            raise RuntimeError("unknown capture %r" % c)
    if renderer is None:
        model = types.SimpleNamespace(**composite) if isinstance(composite, dict) else composite
        if bake:
            from . import visibility_bake
            visibility_bake.bake_visibility(model, iterations=bake_iterations)
            renderer = relight.RelightRenderer(model, envmap, sample_num, baked_visibility=True)
        else:
            renderer = relight.RelightRenderer(model, envmap, sample_num, device_visibility=True)
    dev = renderer.dev
    background = torch.full((3,), float(bg), dtype=torch.float32, device=dev)
    outputs = tuple(c for c in captures if c != "render")
    if light_transforms is not None and len(light_transforms) != len(cameras):
        raise RuntimeError("render_trajectory needs one light transform per camera")
    for i, cam in enumerate(cameras):
        tr = None if light_transforms is None else light_transforms[i]
        res = renderer.frame(cam.to(dev), background, env_transform=tr, outputs=outputs)
        frames = {}
        for c in captures:
            img = res[c]
            if c == "normal":
                img = img * 0.5 + 0.5
                img = img + (1 - res["opacity"]) * float(bg)
            elif c in OVER_BACKGROUND:
                img = img + (1 - res["opacity"]) * float(bg)
            frames[c] = img
        yield i, frames


def build_parser():
    p = argparse.ArgumentParser(prog="python -m relightable3dgaussian_amd.relighting",
                                description="Composition and relighting of Relightable 3D Gaussian objects (PLY) on the device")
    p.add_argument("-co", "--config", required=True, help="the config root (transform.json, trajectory.json, light_transform.json)")
    p.add_argument("-e", "--envmap_path", required=True, help="environment map: .npy [He,We,3] or Radiance .hdr, linear radiance")
    p.add_argument("-bg", "--background_color", type=float, default=None, help="if set, the background colour")
    p.add_argument("--bake", action="store_true", help="bake the composite's visibility into SH and relight from it")
    p.add_argument("--output", default="./capture_trace", help="output directory")
    p.add_argument("--capture_list", default="pbr_env", help="comma-separated captures to write")
    p.add_argument("--sample_num", type=int, default=64)
    p.add_argument("--white_background", action="store_true")
    p.add_argument("--rotate-sh", dest="rotate_sh", action="store_true",
                   help="rotate the SH coefficients with each object (the reference does not)")
    p.add_argument("--fovx", type=float, default=DEFAULT_FOVX)
    p.add_argument("--envmap_scale", type=float, default=1.0)
    p.add_argument("--bake_iterations", type=int, default=1000)
    p.add_argument("--device", default="cuda")
    p.add_argument("--device_png", action="store_true",
                   help="encode the PNG files on the device (filter, deflate, Adler-32) instead of on PIL worker threads")
    return p


def main(argv=None):
    args = build_parser().parse_args(argv)
    captures = [c.strip() for c in args.capture_list.split(",") if c.strip()]
    if "points" in captures:
        raise RuntimeError("capture 'points' (the reference's point-splat debug view) is not offered")
    cfg = compose.load_scene_config(args.config)
    device = torch.device(args.device)
    envmap = load_envmap(args.envmap_path, args.envmap_scale, device)
    composite = compose.assemble([path for _, path, _ in cfg.objects], [t for _, _, t in cfg.objects],
                                 rotate_sh=args.rotate_sh, device=device)
    print("Totally %d points loaded." % composite["xyz"].shape[0])
    bg = args.background_color
    if bg is None:
        bg = 1.0 if args.white_background else 0.0
    cameras = [camera_of(w2c, cfg.width, cfg.height, args.fovx) for _, w2c in cfg.trajectory]
    keys = [idx for idx, _ in cfg.trajectory]
    lights = None if cfg.light_transforms is None else [cfg.light_transforms[idx] for idx in keys]
    for c in captures:
        os.makedirs(os.path.join(args.output, c), exist_ok=True)
    writer = FrameWriter(device_png=True) if args.device_png else FrameWriter()
    try:
        for i, frames in render_trajectory(composite, envmap, cameras, lights, captures, sample_num=args.sample_num, bg=bg,
                                           bake=args.bake, bake_iterations=args.bake_iterations):
            for c, img in frames.items():
                writer.submit(img, os.path.join(args.output, c, "frame_%s.png" % keys[i]))
    finally:
        writer.close()
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
