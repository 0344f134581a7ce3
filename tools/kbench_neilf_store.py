"""Time the device view store on a generated DTU-sized set (GPU only): VIEWS RGB views at W x H (renders of a synthetic teacher)
with a mask file each (its opacity, thresholded), written once as PNG files, then
  load     dataset.ViewStore(paths, mask_paths=...) at resolution 1 and at resolution 2: wall clock and its split (`load_seconds`);
           the resident bytes against the float image + mask bytes of the same views;
  unpack   one r3dg_view_unpack_masked launch by HIP events (median of REPS with min and max), 4 bytes read and 16 written per pixel;
  resize   one r3dg_view_resize launch W x H -> W/2 x H/2 by HIP events, 4 bytes read per source pixel and 16 written per target pixel;
  train    the fused stage-2 iteration of the bench's DTU configuration (POINTS Gaussians, K rays, the run_dtu.sh objective, frozen
           geometry) over the views in round-robin order, through store.images / store.masks against resident float tensors of the
           same views, alternating BLOCKS blocks of STEPS iterations of each inside this one process.
VIEWS=49  W=1600  H=1200  REPS=21  POINTS=300000  K=32  STEPS=200  BLOCKS=4."""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import shutil, tempfile, time
from concurrent.futures import ThreadPoolExecutor
import torch
from PIL import Image
from relightable3dgaussian_amd import _lib, bench_core as bc, dataset, synthetic as syn, train_step
from relightable3dgaussian_amd.bench_core import GaussianParams, render_stage1
from relightable3dgaussian_amd.fused_step import FusedStage2Step
env = lambda k, d: int(os.environ.get(k, d))
VIEWS, W, H, REPS, POINTS, K = env("VIEWS", 49), env("W", 1600), env("H", 1200), env("REPS", 21), env("POINTS", 300000), env("K", 32)
STEPS, BLOCKS = env("STEPS", 200), env("BLOCKS", 4)
dev = "cuda"
median = lambda t: sorted(t)[len(t) // 2]
event = lambda: torch.cuda.Event(enable_timing=True)
work = tempfile.mkdtemp(prefix="kbench_neilf_")
cams = [c.to(dev) for c in syn.orbit_cameras(VIEWS, width=W, height=H)]
bg = torch.ones(3, device=dev)
scene = syn.make_scene(P=POINTS, seed=0, stage2=True)
with torch.no_grad():
    teacher = GaussianParams(syn.make_scene(P=POINTS, seed=0, stage2=False), dev, False)
    teacher.features_dc.add_(0.05 * torch.randn_like(teacher.features_dc))
    arrays, mask_arrays = [], []
    for c in cams:
        outs = render_stage1(teacher, c, torch.zeros(3, device=dev))
        arrays.append((outs[2].clamp(0, 1).permute(1, 2, 0) * 255.0).round().to(torch.uint8).cpu().numpy())
        mask_arrays.append(((outs[3].reshape(H, W) > 0.5) * 255).to(torch.uint8).cpu().numpy())
    del teacher
paths = [os.path.join(work, "%04d.png" % i) for i in range(VIEWS)]
mask_paths = [os.path.join(work, "m%04d.png" % i) for i in range(VIEWS)]
with ThreadPoolExecutor(max_workers=8) as pool:
    list(pool.map(lambda i: (Image.fromarray(arrays[i]).save(paths[i]), Image.fromarray(mask_arrays[i], mode="L").save(mask_paths[i])),
                  range(VIEWS)))
file_mb = sum(os.path.getsize(p) for p in paths + mask_paths) / 1e6
torch.cuda.synchronize(); torch.cuda.empty_cache()
print("%d RGB views %d x %d with mask files, %.1f MB of PNG files" % (VIEWS, W, H, file_mb))


def load(resolution):
    t0 = time.perf_counter()
    s = dataset.ViewStore(paths, dev, mask_paths=mask_paths, resolution=resolution)
    wall = time.perf_counter() - t0
    ls = s.load_seconds
    print("load     resolution %d: %.3f s wall (%d decoder threads): waiting for decoded files %.3f s, staging + upload%s %.3f s; "
          "decoder time summed over the threads %.3f s" % (resolution, wall, s.workers, ls["decode"],
                                                           " + resize launches" if s.resizes else "", ls["upload"], ls["decode_cpu"]))
    print("bytes    resolution %d: resident %.1f MB against %.1f MB as float image + mask: x %.2f"
          % (resolution, s.resident_nbytes() / 1e6, s.float_nbytes() / 1e6, s.float_nbytes() / s.resident_nbytes()))
    return s


store = load(1)
half = load(2)
del half
torch.cuda.empty_cache()

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
moved = W * H * 20
print("unpack   r3dg_view_unpack_masked, one view: median %.4f ms (min %.4f max %.4f, %d reps)  %.1f MB moved -> %.2f TB/s"
      % (median(times), min(times), max(times), REPS, moved / 1e6, moved / (median(times) * 1e-3) / 1e12))

# ---- resize launch
view = store.views[0]
OW, OH = W // 2, H // 2
image, mask = torch.empty(3, OH, OW, device=dev), torch.empty(1, OH, OW, device=dev)
resize = lambda v: _lib.check(_lib.lib().r3dg_view_resize(
    _lib.current_stream(), W, H, 3, store.pixels.data_ptr() + store.views[v].offset, store.pixels.data_ptr() + store.views[v].mask_offset,
    None, OW, OH, image.data_ptr(), mask.data_ptr()), "view_resize")
for v in range(4):
    resize(v)
torch.cuda.synchronize()
times = []
for r in range(REPS):
    e0, e1 = event(), event()
    e0.record(); resize(r % VIEWS); e1.record()
    torch.cuda.synchronize()
    times.append(e0.elapsed_time(e1))
moved = W * H * 4 + OW * OH * 16
print("resize   r3dg_view_resize %d x %d -> %d x %d (RGB + mask plane): median %.4f ms (min %.4f max %.4f, %d reps)  %.1f MB moved -> "
      "%.1f GB/s" % (W, H, OW, OH, median(times), min(times), max(times), REPS, moved / 1e6, moved / (median(times) * 1e-3) / 1e9))

# ---- the DTU stage-2 configuration through the store against resident tensors
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
    print("train    stage 2 (DTU objective, frozen geometry %s), %d Gaussians, K=%d, %d x %d, %d views, %-8s: median %7.1f it/s "
          "(blocks of %d: %s)" % (step.frozen_geometry, POINTS, K, W, H, VIEWS, name, median(r), STEPS, " ".join("%.1f" % x for x in r)))
mr, ms = median(rates["resident"]), median(rates["store"])
spread = max(max(r) - min(r) for r in rates.values())
print("train    store against resident: %+.1f it/s (%+.2f %%); largest block-to-block spread of one path %.1f it/s (%.2f %%); "
      "views dropped by the bounded forward since the last poll: %d" % (ms - mr, 100 * (ms - mr) / mr, spread, 100 * spread / mr, dropped))
shutil.rmtree(work, ignore_errors=True)
