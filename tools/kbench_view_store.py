"""Time the device view store (GPU only): VIEWS RGBA views at RES x RES (renders of a synthetic teacher, alpha = its opacity)
written once as PNG files, then
  load     dataset.ViewStore(paths): wall clock, and its split into the time the loading thread waited for decoded files and the
           time it spent staging and copying; the store's bytes against the float image + mask bytes of the same views;
  unpack   one r3dg_view_unpack launch by HIP events (median of REPS with min and max) and the bytes it moves per second
           (4 bytes read, 16 written per pixel) against the 6.3 TB/s the part sustains;
  train    the fused stage-2 iteration at the headline size (POINTS Gaussians, K rays) over the views in round-robin order, through
           store.images / store.masks against resident float tensors of the same views, alternating BLOCKS blocks of STEPS
           iterations of each inside this one process: it/s of every block, the medians, their difference next to the spread.
VIEWS=100  RES=800  REPS=21  POINTS=300000  K=64  STEPS=100  BLOCKS=4  RESIDENT_VIEWS=100."""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import shutil, tempfile, time
from concurrent.futures import ThreadPoolExecutor
import torch
from PIL import Image
from relightable3dgaussian_amd import dataset, synthetic as syn
from relightable3dgaussian_amd.bench_core import GaussianParams, render_stage1
from relightable3dgaussian_amd.fused_step import FusedStage2Step
env = lambda k, d: int(os.environ.get(k, d))
VIEWS, RES, REPS, POINTS, K = env("VIEWS", 100), env("RES", 800), env("REPS", 21), env("POINTS", 300000), env("K", 64)
STEPS, BLOCKS = env("STEPS", 100), env("BLOCKS", 4)
dev = "cuda"
median = lambda t: sorted(t)[len(t) // 2]
event = lambda: torch.cuda.Event(enable_timing=True)
work = tempfile.mkdtemp(prefix="kbench_views_")
cams = [c.to(dev) for c in syn.orbit_cameras(VIEWS, width=RES, height=RES)]
bg = torch.ones(3, device=dev)
scene = syn.make_scene(P=POINTS, seed=0, stage2=True)
with torch.no_grad():
    teacher = GaussianParams(syn.make_scene(P=POINTS, seed=0, stage2=False), dev, False)
    teacher.features_dc.add_(0.05 * torch.randn_like(teacher.features_dc))
    arrays = []
    for c in cams:
        outs = render_stage1(teacher, c, torch.zeros(3, device=dev))
        rgba = torch.cat([outs[2].clamp(0, 1), outs[3].reshape(1, RES, RES).clamp(0, 1)], 0)
        arrays.append((rgba.permute(1, 2, 0) * 255.0).round().to(torch.uint8).cpu().numpy())
    del teacher
paths = [os.path.join(work, "r_%d.png" % i) for i in range(VIEWS)]
with ThreadPoolExecutor(max_workers=8) as pool:
    list(pool.map(lambda ia: Image.fromarray(ia[1]).save(paths[ia[0]]), enumerate(arrays)))
file_mb = sum(os.path.getsize(p) for p in paths) / 1e6
torch.cuda.synchronize(); torch.cuda.empty_cache()
print("%d RGBA views %d x %d, %.1f MB of PNG files" % (VIEWS, RES, RES, file_mb))

# ---- load
t0 = time.perf_counter()
store = dataset.ViewStore(paths, dev)
wall = time.perf_counter() - t0
ls = store.load_seconds
print("load     %.3f s wall (%d decoder threads): waiting for decoded files %.3f s, staging + upload %.3f s; decoder time summed "
      "over the threads %.3f s" % (wall, store.workers, ls["decode"], ls["upload"], ls["decode_cpu"]))
print("bytes    store %.1f MB (8-bit pixels) against %.1f MB as float image + mask: x %.2f"
      % (store.nbytes / 1e6, store.float_nbytes() / 1e6, store.float_nbytes() / store.nbytes))

# ---- unpack launch
for v in range(8):
    store.fetch(v % VIEWS, bg)
torch.cuda.synchronize()
times = []
for r in range(REPS):
    e0, e1 = event(), event()
    e0.record(); store.fetch(r % VIEWS, bg); e1.record()
    torch.cuda.synchronize()
    times.append(e0.elapsed_time(e1))
moved = RES * RES * 20
print("unpack   r3dg_view_unpack, one view: median %.4f ms (min %.4f max %.4f, %d reps)  %.1f MB moved -> %.2f TB/s (%.0f %% of 6.3 TB/s)"
      % (median(times), min(times), max(times), REPS, moved / 1e6, moved / (median(times) * 1e-3) / 1e12,
         100 * moved / (median(times) * 1e-3) / 6.3e12))
t0 = time.perf_counter()
for r in range(1000):
    store.fetch(r % VIEWS, bg)
host = (time.perf_counter() - t0) / 1000
torch.cuda.synchronize()
print("unpack   host time of fetch(): %.1f us per call (1000 calls queued back to back)" % (host * 1e6))

# ---- training through the store against resident tensors
RESIDENT = min(VIEWS, env("RESIDENT_VIEWS", VIEWS))
resident = [store.fetch(v, bg) for v in range(RESIDENT)]
r_images, r_masks = [r[0].clone() for r in resident], [r[1].clone() for r in resident]
step = FusedStage2Step(GaussianParams(scene, dev, True), K, lr=1e-4)
s_images, s_masks = store.images(bg), store.masks(bg)
for i in range(8):
    step(cams[i % RESIDENT], bg, r_images[i % RESIDENT], image_mask=r_masks[i % RESIDENT])
    step(cams[i % RESIDENT], bg, s_images[i % RESIDENT], image_mask=s_masks[i % RESIDENT])
rates = {"resident": [], "store": []}
n = 0
for b in range(BLOCKS):
    for name, images, masks in (("resident", r_images, r_masks), ("store", s_images, s_masks)):
        step.flush(); torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(STEPS):
            v = (n + i) % RESIDENT
            step(cams[v], bg, images[v], image_mask=masks[v])
        step.flush(); torch.cuda.synchronize()
        rates[name].append(STEPS / (time.perf_counter() - t0))
    n += STEPS
dropped = step.poll_overflow()
for name in ("resident", "store"):
    r = rates[name]
    print("train    stage 2, %d Gaussians, K=%d, %d x %d, %d views, %-8s: median %7.1f it/s (blocks of %d: %s)"
          % (POINTS, K, RES, RES, RESIDENT, name, median(r), STEPS, " ".join("%.1f" % x for x in r)))
mr, ms = median(rates["resident"]), median(rates["store"])
spread = max(max(r) - min(r) for r in rates.values())
print("train    store against resident: %+.1f it/s (%+.2f %%); largest block-to-block spread of one path %.1f it/s (%.2f %%); "
      "views dropped by the bounded forward since the last poll: %d" % (ms - mr, 100 * (ms - mr) / mr, spread, 100 * spread / mr, dropped))
shutil.rmtree(work, ignore_errors=True)
