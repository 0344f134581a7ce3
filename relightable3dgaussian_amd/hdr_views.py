"""The views of a Synthetic4Relight train split on the device: OpenEXR files (`<name>_rgb.exr`, scene/dataset_readers.py:526-565) kept
RESIDENT in the files' own sample type -- 6 bytes per pixel of a half file + 1 for the mask file, against 16 as a float image +
mask -- and turned into the float image the fused steps read by ONE launch per iteration.  The interface is dataset.ViewStore's:

    store = HdrViewStore([r["path"] for r in records], device, mask_paths=[r["mask_path"] for r in records])
    image, mask = store.fetch(v, background)            # r3dg_view_unpack_hdr: sRGB curve, mask select, clamp
    train_loop.train_stage1(init, cameras, store.images(bg), bg, extent, masks=store.masks(bg), ...)

Loading: worker threads (at most 8) read each file and zlib-inflate its chunks straight into a pinned staging buffer of their own
(zlib releases the GIL; exr.inflate_chunks), `*_mask.png` is decoded by PIL to 8-bit grey behind them; the loading thread uploads
each staging buffer into a transient device buffer and queues one r3dg_exr_unpack_chunks (csrc/exr_unpack.hip: predictor,
byte un-split, de-planarisation) per view into ONE resident buffer.  Only the inflate is host work.  `exr.decode_reference` is the
NumPy restatement of the decode, tests/exr_cases.unpack_hdr_reference that of the fetch.

Out of scope: `--resolution` scales other than 1 (Synthetic4Relight is 800 x 800; an antialiased resize of float data is a
separate piece of work) -- they raise; everything exr.read_header refuses (PIZ and the other codecs, tiles, ...)."""
import collections
import os
import time
import types
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import _abi, _lib, dataset, exr

ALIGN = dataset.ALIGN
CHANNELS = ("R", "G", "B")
_TILE = _abi.constants["R3DG_EXR_TILE"]


def _pad(n):
    return -(-n // ALIGN) * ALIGN


def _staged_nbytes(header, masked):
    """Bytes of a view's pinned staging buffer: chunk bytes, mask bytes, chunk table (16 per chunk), kept-channel list."""
    return exr.inflated_nbytes(header) + (_pad(header.height * header.width) if masked else 0) + 16 * len(header.offsets) + 16


def _inflate(path, header, mask_path, keep, staging):
    """A worker's job: the file's chunks inflated into `staging` (the NumPy view of a pinned uint8 tensor), then, each at a
    16-byte-aligned offset, the mask file's grey bytes, the chunk table and the kept-channel list.
    -> (bytes of chunk data, mask offset or None, table offset, seconds spent)."""
    t0 = time.perf_counter()
    table, used = exr.inflate_chunks(path, header, staging)
    mask_at, at = None, used
    if mask_path is not None:
        from PIL import Image
        with Image.open(mask_path) as im:                   # imageio.imread(mode="L"): PIL's conversion to 8-bit grey
            grey = np.array(im.convert("L"), dtype=np.uint8)
        if grey.shape != (header.height, header.width):
            raise RuntimeError("%s: the mask is %d x %d, its image %d x %d" % (mask_path, grey.shape[1], grey.shape[0],
                                                                              header.width, header.height))
        mask_at = at
        staging[at:at + grey.size] = grey.reshape(-1)
        at += _pad(grey.size)
    small = np.concatenate([table.reshape(-1), np.asarray(keep, np.int32)]).view(np.uint8)
    staging[at:at + small.size] = small
    return used, mask_at, at, time.perf_counter() - t0


class HdrViewStore:
    """All views of a split on the device as the half / float samples their OpenEXR files hold (planar [3,H,W] R,G,B per view, its
    mask bytes [H,W] behind it; every part at a 16-byte-aligned offset of ONE uint8 buffer, `nbytes` in all).

    `fetch(v, background)` -> (image [3,H,W], mask [1,H,W]) float32: one r3dg_view_unpack_hdr launch on the caller's current
    stream into one of `slots` preallocated output pairs of that size.  RING CONTRACT (dataset.ViewStore's): a returned pair holds
    view v until `slots` further fetches of views of the same size; everything that reads it must have been queued on the device by
    then.  Keep a view longer with .clone().  The kernel writes through raw pointers: a returned tensor's `_version` never moves.
    A view without a mask file: the image alone and an all-ones mask.

    `images(background)` / `masks(background)`: the lazy sequences of dataset.ViewStore; `masks` is None when no view has a mask
    file.  `sizes`, `scales` (all 1), `launches` (fetch launches), `unpack_launches` (r3dg_exr_unpack_chunks calls, all at load),
    `load_seconds`: {"inflate": seconds the loading thread waited for inflated files, "upload": seconds it spent on copies and
    launches, "inflate_cpu": seconds summed over the worker threads}.  `resolution`: loadCam's `--resolution`; anything but a
    scale of 1 raises.  There is no CPU path."""

    def __init__(self, paths, device="cuda", workers=None, slots=4, mask_paths=None, resolution=1, background=None):
        paths = [str(p) for p in paths]
        if not paths:
            raise RuntimeError("HdrViewStore: no views")
        if int(slots) < 1:
            raise RuntimeError("HdrViewStore: slots must be at least 1")
        mask_paths = [None] * len(paths) if mask_paths is None else [None if m is None else str(m) for m in mask_paths]
        if len(mask_paths) != len(paths):
            raise RuntimeError("HdrViewStore: mask_paths has one entry (a file or None) per view")
        self.paths, self.mask_paths, self.slots = paths, mask_paths, int(slots)
        self.workers = max(1, min(8, workers or (os.cpu_count() or 1)))
        self.headers = [exr.read_header(p) for p in paths]             # (raises for a file that is not decoded, before anything else)
        self.scales = [dataset.view_scale(resolution, h.width) for h in self.headers]
        if any(s != 1 for s in self.scales):
            raise RuntimeError("HdrViewStore: --resolution %r would resize its views (scale %g); HDR views are kept at the size of "
                               "their files (no resize of float data is built)" % (resolution, max(self.scales)))
        self.dev = torch.device(device)
        if self.dev.type != "cuda":
            raise RuntimeError("HdrViewStore needs a device (there is no CPU path; exr.decode_reference is the NumPy restatement)")
        if self.dev.index is None:
            self.dev = torch.device("cuda", torch.cuda.current_device())
        self.views, offset = [], 0
        for h, m in zip(self.headers, mask_paths):
            view = types.SimpleNamespace(offset=offset, mask_offset=None, height=h.height, width=h.width,
                                         bytes_per_sample=h.bytes_per_sample, keep=exr.channel_indexes(h, CHANNELS), masked=m is not None)
            offset += _pad(3 * h.height * h.width * h.bytes_per_sample)
            if m is not None:
                view.mask_offset = offset
                offset += _pad(h.height * h.width)
            self.views.append(view)
        self.nbytes = offset
        self.sizes = [(v.height, v.width) for v in self.views]
        self.has_masks = any(v.masked for v in self.views)
        self.pixels = torch.zeros(self.nbytes, dtype=torch.uint8, device=self.dev)
        self._backgrounds = {}
        self.unpack_launches = 0
        self._load()
        f = dict(dtype=torch.float32, device=self.dev)
        self._rings = {}                                             # (H, W) -> [next slot, [(image, mask)] * slots]
        for h, w in sorted(set(self.sizes)):
            self._rings[(h, w)] = [0, [(torch.empty(3, h, w, **f), torch.empty(1, h, w, **f)) for _ in range(self.slots)]]
        self._last = None                                            # (view, background pointer, image, mask) of the last fetch
        self.launches = 0

    def _load(self):
        staged = [_staged_nbytes(h, m is not None) for h, m in zip(self.headers, self.mask_paths)]
        window = 2 * self.workers                                    # files being inflated at once: bounded host memory
        # one pinned staging buffer per file in flight and two more: a buffer goes back to a worker only after the copies out of it,
        # two views back, have been waited for (ViewStore's double buffer, widened to the workers that fill them directly)
        ring = [types.SimpleNamespace(host=torch.empty(max(staged), dtype=torch.uint8, pin_memory=True), done=None)
                for _ in range(min(len(self.views), window + 2))]
        for s in ring:
            s.array = s.host.numpy()
        # the transient device buffer of the view being decoded: chunk bytes, chunk table + kept-channel list, tile-sum scratch;
        # reused by the next view (its copies are queued on the stream behind the launches that read it)
        tiles = [-(-(h.rows_per_chunk * h.width * len(h.channels) * h.bytes_per_sample // 2) // _TILE) for h in self.headers]
        layout = [(exr.inflated_nbytes(h), 16 * len(h.offsets) + 16, 4 * len(h.offsets) * 2 * t) for h, t in zip(self.headers, tiles)]
        transient = torch.empty(max(sum(_pad(n) for n in sizes) for sizes in layout), dtype=torch.uint8, device=self.dev)
        wait = upload = inflate_cpu = 0.0
        submit = lambda pool, i: pool.submit(_inflate, self.paths[i], self.headers[i], self.mask_paths[i], self.views[i].keep,
                                             ring[i % len(ring)].array)
        with ThreadPoolExecutor(max_workers=self.workers) as pool, torch.cuda.device(self.dev):
            pending = collections.deque(submit(pool, i) for i in range(min(window, len(self.views))))
            submitted = len(pending)
            for i, (view, header) in enumerate(zip(self.views, self.headers)):
                t0 = time.perf_counter()
                used, mask_at, table_at, seconds = pending.popleft().result()
                t1 = time.perf_counter()
                s = ring[i % len(ring)]
                chunks, pixels = len(header.offsets), view.height * view.width
                n_chunk, n_small, n_sums = layout[i]
                transient[:used].copy_(s.host[:used], non_blocking=True)
                transient[n_chunk:n_chunk + n_small].copy_(s.host[table_at:table_at + n_small], non_blocking=True)
                if mask_at is not None:
                    self.pixels[view.mask_offset:view.mask_offset + pixels].copy_(s.host[mask_at:mask_at + pixels], non_blocking=True)
                base = transient.data_ptr()
                _lib.check(_lib.lib().r3dg_exr_unpack_chunks(
                    _lib.current_stream(), view.width, view.height, len(header.channels), view.bytes_per_sample, chunks,
                    header.rows_per_chunk, base, used, base + n_chunk, len(view.keep), base + n_chunk + 16 * chunks,
                    base + n_chunk + _pad(n_small), n_sums // 4, self.pixels.data_ptr() + view.offset), "exr_unpack_chunks")
                self.unpack_launches += 1
                s.done = torch.cuda.Event()
                s.done.record()
                if submitted < len(self.views):
                    nxt = ring[submitted % len(ring)]
                    if nxt.done is not None:
                        nxt.done.synchronize()                       # (the copies out of that staging buffer, two views back)
                    pending.append(submit(pool, submitted))
                    submitted += 1
                wait += t1 - t0
                upload += time.perf_counter() - t1
                inflate_cpu += seconds
            t1 = time.perf_counter()
            torch.cuda.current_stream().synchronize()
            upload += time.perf_counter() - t1
        self.load_seconds = dict(inflate=wait, upload=upload, inflate_cpu=inflate_cpu)

    def _background(self, background):
        if isinstance(background, torch.Tensor) and background.device == self.dev and background.dtype == torch.float32 and \
                background.numel() == 3 and background.is_contiguous():
            return background
        key = dataset.ViewStore._key(background)
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
        call = lambda: _lib.check(_lib.lib().r3dg_view_unpack_hdr(
            _lib.current_stream(), view.width, view.height, int(view.bytes_per_sample == 2), self.pixels.data_ptr() + view.offset,
            self.pixels.data_ptr() + view.mask_offset if view.masked else None, bg.data_ptr(), image.data_ptr(), mask.data_ptr()),
            "view_unpack_hdr")
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
        return dataset._ViewSequence(self, background, 0)

    def masks(self, background):
        return dataset._ViewSequence(self, background, 1) if self.has_masks else None

    def float_nbytes(self):
        """Bytes the same views take as resident float images + masks (16 per pixel)."""
        return sum(16 * v.height * v.width for v in self.views)

    def resident_nbytes(self):
        """Bytes the views occupy on the device: the sample planes and the mask bytes (the rings not counted)."""
        return self.nbytes
