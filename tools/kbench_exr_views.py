"""Time the OpenEXR view store (GPU only): VIEWS views at RES x RES, half R,G,B,A under ZIP (smooth content with a little noise,
written once by the test-side writer tests/exr_writer.py) with a mask file each, then
  load     hdr_views.HdrViewStore(paths, mask_paths=...): wall clock and its split (`load_seconds`: waiting for inflated files,
           staging + upload + launches); exr.decode_reference on one view as the host-only baseline; the resident bytes against
           the float image + mask bytes of the same views;
  decode   one r3dg_exr_unpack_chunks call (two launches) on one view by HIP events (median of REPS with min and max) and the bytes
           it moves per second (the inflated bytes read twice, the three kept planes written) against the 6.3 TB/s the part sustains;
  unpack   one r3dg_view_unpack_hdr launch by HIP events (median, min and max of REPS; 7 bytes read, 16 written per pixel);
  train    the fused stage-2 iteration of the bench's Synthetic4Relight configuration (POINTS Gaussians, K rays, the run_syn4.sh
           objective, frozen geometry) over the views in round-robin order, through store.images / store.masks against resident
           float tensors of the same views, alternating BLOCKS blocks of STEPS iterations of each inside this one process (the
           protocol of tools/kbench_view_store.py).
VIEWS=100  RES=800  REPS=21  POINTS=300000  K=64  STEPS=100  BLOCKS=4."""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import shutil, tempfile, time
from concurrent.futures import ThreadPoolExecutor
import numpy as np
import torch
from PIL import Image
from relightable3dgaussian_amd import _abi, _lib, bench_core as bc, exr, hdr_views, synthetic as syn, train_step
from relightable3dgaussian_amd.bench_core import GaussianParams
from relightable3dgaussian_amd.fused_step import FusedStage2Step
from tests import exr_writer
env = lambda k, d: int(os.environ.get(k, d))
VIEWS, RES, REPS, POINTS, K = env("VIEWS", 100), env("RES", 800), env("REPS", 21), env("POINTS", 300000), env("K", 64)
STEPS, BLOCKS = env("STEPS", 100), env("BLOCKS", 4)
dev = "cuda"
median = lambda t: sorted(t)[len(t) // 2]
event = lambda: torch.cuda.Event(enable_timing=True)
work = tempfile.mkdtemp(prefix="kbench_exr_")
paths = [os.path.join(work, "%03d_rgb.exr" % i) for i in range(VIEWS)]
mask_paths = [os.path.join(work, "%03d_mask.png" % i) for i in range(VIEWS)]
yy, xx = np.meshgrid(np.arange(RES), np.arange(RES), indexing="ij")


def write_view(i):
    rng = np.random.RandomState(i)
    inside = (xx - RES / 2) ** 2 + (yy - RES / 2) ** 2 < (0.4 * RES) ** 2
    planes = {c: ((0.6 + 0.5 * np.sin(0.011 * xx + 0.007 * yy + i + j)) * inside + 0.002 * rng.standard_normal((RES, RES)) * inside)
              .astype(np.float16) for j, c in enumerate("RGB")}
    planes["A"] = inside.astype(np.float16)
    exr_writer.write_exr(paths[i], planes, "ZIP")
    Image.fromarray((inside * 255).astype(np.uint8)).save(mask_paths[i])


with ThreadPoolExecutor(max_workers=8) as pool:
    list(pool.map(write_view, range(VIEWS)))
print("%d views %d x %d, half R,G,B,A under ZIP + mask files: %.1f MB of EXR files, %.1f MB inflated"
      % (VIEWS, RES, RES, sum(os.path.getsize(p) for p in paths) / 1e6, VIEWS * RES * RES * 8 / 1e6))

# ---- load
t0 = time.perf_counter()
host = exr.decode_reference(paths[0])
print("host     exr.decode_reference on one view (NumPy + zlib, one thread): %.3f s" % (time.perf_counter() - t0))
torch.zeros(1, device=dev); torch.cuda.synchronize()
t0 = time.perf_counter()
store = hdr_views.HdrViewStore(paths, dev, mask_paths=mask_paths)
wall = time.perf_counter() - t0
ls = store.load_seconds
print("load     %.3f s wall (%d inflate threads): waiting for inflated files %.3f s, staging + upload + device launches %.3f s; "
      "inflate time summed over the threads %.3f s" % (wall, store.workers, ls["inflate"], ls["upload"], ls["inflate_cpu"]))
print("bytes    resident %.1f MB (half samples + mask bytes) against %.1f MB as float image + mask: x %.2f"
      % (store.resident_nbytes() / 1e6, store.float_nbytes() / 1e6, store.float_nbytes() / store.resident_nbytes()))
got = store.pixels[:3 * RES * RES * 2].cpu().numpy().view(np.float16).reshape(3, RES, RES)
assert np.array_equal(got.view(np.uint16), np.ascontiguousarray(host.transpose(2, 0, 1)).view(np.uint16)), "device decode != host decode"

# ---- one r3dg_exr_unpack_chunks call
h = exr.read_header(paths[0])
staging = np.zeros(exr.inflated_nbytes(h), np.uint8)
table, used = exr.inflate_chunks(paths[0], h, staging)
tiles = -(-(h.rows_per_chunk * h.width * len(h.channels) * h.bytes_per_sample // 2) // _abi.constants["R3DG_EXR_TILE"])
d_bytes, d_table = torch.from_numpy(staging[:used]).to(dev), torch.from_numpy(table).to(dev)
d_keep = torch.tensor(exr.channel_indexes(h, "RGB"), dtype=torch.int32, device=dev)
d_sums = torch.zeros(len(table) * 2 * tiles, dtype=torch.int32, device=dev)
d_out = torch.zeros(3 * RES * RES * 2, dtype=torch.uint8, device=dev)
decode = lambda: _lib.check(_lib.lib().r3dg_exr_unpack_chunks(
    _lib.current_stream(), h.width, h.height, len(h.channels), h.bytes_per_sample, len(table), h.rows_per_chunk, d_bytes.data_ptr(),
    used, d_table.data_ptr(), 3, d_keep.data_ptr(), d_sums.data_ptr(), d_sums.numel(), d_out.data_ptr()), "exr_unpack_chunks")
for _ in range(8):
    decode()
torch.cuda.synchronize()
times = []
for r in range(REPS):
    e0, e1 = event(), event()
    e0.record(); decode(); e1.record()
    torch.cuda.synchronize()
    times.append(e0.elapsed_time(e1))
moved = 2 * used + d_out.numel()
print("decode   r3dg_exr_unpack_chunks, one view (%d chunks, %d tiles each, two launches): median %.4f ms (min %.4f max %.4f, %d reps)  "
      "%.1f MB moved -> %.2f TB/s (%.0f %% of 6.3 TB/s)" % (len(table), tiles, median(times), min(times), max(times), REPS, moved / 1e6,
                                                         moved / (median(times) * 1e-3) / 1e12, 100 * moved / (median(times) * 1e-3) / 6.3e12))

# ---- the per-iteration launch
bg = torch.ones(3, device=dev)
for v in range(8):
    store.fetch(v % VIEWS, bg)
torch.cuda.synchronize()
times = []
for r in range(REPS):
    e0, e1 = event(), event()
    e0.record(); store.fetch(r % VIEWS, bg); e1.record()
    torch.cuda.synchronize()
    times.append(e0.elapsed_time(e1))
moved = RES * RES * 23
print("unpack   r3dg_view_unpack_hdr, one view: median %.4f ms (min %.4f max %.4f, %d reps)  %.1f MB moved -> %.2f TB/s (%.0f %% of 6.3 TB/s)"
      % (median(times), min(times), max(times), REPS, moved / 1e6, moved / (median(times) * 1e-3) / 1e12,
         100 * moved / (median(times) * 1e-3) / 6.3e12))

# ---- the Synthetic4Relight stage-2 configuration through the store against resident tensors
cams = [c.to(dev) for c in syn.orbit_cameras(VIEWS, width=RES, height=RES)]
scene = syn.make_scene(P=POINTS, seed=0, stage2=True)
resident = [store.fetch(v, bg) for v in range(VIEWS)]
r_images, r_masks = [r[0].clone() for r in resident], [r[1].clone() for r in resident]
step = FusedStage2Step(GaussianParams(scene, dev, True), K, lr=1e-4, lrs=bc.SYN4_LRS, loss_weights=train_step.STAGE2_WEIGHTS_SYN4)
s_images, s_masks = store.images(bg), store.masks(bg)
for i in range(8):
    step(cams[i % VIEWS], bg, r_images[i % VIEWS], image_mask=r_masks[i % VIEWS])
    step(cams[i % VIEWS], bg, s_images[i % VIEWS], image_mask=s_masks[i % VIEWS])
rates = {"resident": [], "store": []}
n = 0
for b in range(BLOCKS):
    for name, images, masks in (("resident", r_images, r_masks), ("store", s_images, s_masks)):
        step.flush(); torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(STEPS):
            v = (n + i) % VIEWS
            step(cams[v], bg, images[v], image_mask=masks[v])
        step.flush(); torch.cuda.synchronize()
        rates[name].append(STEPS / (time.perf_counter() - t0))
    n += STEPS
dropped = step.poll_overflow()
for name in ("resident", "store"):
    r = rates[name]
    print("train    stage 2 (Synthetic4Relight objective, frozen geometry %s), %d Gaussians, K=%d, %d x %d, %d views, %-8s: median "
          "%7.1f it/s (blocks of %d: %s)" % (step.frozen_geometry, POINTS, K, RES, RES, VIEWS, name, median(r), STEPS,
                                             " ".join("%.1f" % x for x in r)))
mr, ms = median(rates["resident"]), median(rates["store"])
spread = max(max(r) - min(r) for r in rates.values())
print("train    store against resident: %+.1f it/s (%+.2f %%); largest block-to-block spread of one path %.1f it/s (%.2f %%); "
      "views dropped by the bounded forward since the last poll: %d" % (ms - mr, 100 * (ms - mr) / mr, spread, 100 * spread / mr, dropped))
shutil.rmtree(work, ignore_errors=True)
