"""Time the assembly of a composite from PLY files (GPU only): SIZES synthetic stage-2 objects (130 columns, default
300000,300000,100000 rows) written once as PLY files, then assembled by two routes, alternating inside every repetition:
  (a) compose.assemble: memory-mapped records, one upload and one r3dg_scene_place_records launch per object into tensors
      allocated once;
  (b) the route available without it: NumPy column copies as the reference's load_ply makes them (scene/gaussian_model.py:568-665,
      one np.asarray per property into float64 arrays, torch.tensor(..., dtype=float) to the device, the transposes), then
      relight.compose_scenes (transform_object per object, torch.cat per group).
Wall clock from the open of the first file to a ready composite (synchronised), median of REPS with min and max;
torch.cuda.max_memory_allocated above the composite's own bytes; the placement launches alone (HIP events) with their achieved
bytes per second -- each row read once (A floats) and written once (130 floats) -- against the 6.3 TB/s the part sustains.
Then the driver: relighting.render_trajectory over FRAMES orbit frames at RES x RES with PNG output (relighting.FrameWriter) on and off.
SIZES="300000,300000,100000"  REPS=5  RES=800  FRAMES=60  K=64."""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import shutil, tempfile, time, types
import numpy as np
import torch
from relightable3dgaussian_amd import compose, ply, relight, relighting, synthetic as syn
from relightable3dgaussian_amd.bench_core import GaussianParams
SIZES = [int(x) for x in os.environ.get("SIZES", "300000,300000,100000").split(",")]
REPS = int(os.environ.get("REPS", 5)); RES = int(os.environ.get("RES", 800)); FRAMES = int(os.environ.get("FRAMES", 60))
K = int(os.environ.get("K", 64)); dev = "cuda"
median = lambda t: sorted(t)[len(t) // 2]
event = lambda: torch.cuda.Event(enable_timing=True)
work = tempfile.mkdtemp(prefix="kbench_scene_")
paths, transforms = [], []
for j, P in enumerate(SIZES):
    model = GaussianParams(syn.make_scene(P=P, seed=j, stage2=True), dev, True)        # raw parameters
    model.visibility_sh = (0.1 * torch.randn(P, 16, generator=torch.Generator().manual_seed(j))).to(dev)
    path = os.path.join(work, "object%d.ply" % j)
    ply.save(path, model)
    paths.append(path)
    a = 0.7 * j
    T = torch.eye(4)
    T[:3, :3] = (0.8 + 0.2 * j) * torch.tensor([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])
    T[:3, 3] = torch.tensor([1.6 * (j - 1), 0.3 * j, 0.0])
    transforms.append(T)
    del model
torch.cuda.synchronize(); torch.cuda.empty_cache()
total = sum(SIZES)
composite_bytes = total * 130 * 4


def load_ply_numpy(path):
    """load_ply's host work: a column copy per property into float64 arrays, then float32 tensors on the device."""
    rec = ply.read_records(path)
    col = {n: np.asarray(rec.array[:, i]) for i, n in enumerate(rec.names)}
    P = rec.count

    def stack(names):
        out = np.zeros((P, len(names)))
        for i, n in enumerate(names):
            out[:, i] = col[n]
        return out

    def sh(dc, rest, C):
        d = np.zeros((P, C, 1))
        for c in range(C):
            d[:, c, 0] = col["%s_%d" % (dc, c)]
        r = stack(["%s_%d" % (rest, i) for i in range(15 * C)]).reshape(P, C, 15)
        t = lambda x: torch.tensor(x, dtype=torch.float, device=dev).transpose(1, 2).contiguous()
        return t(d), t(r)
    t = lambda x: torch.tensor(x, dtype=torch.float, device=dev)
    out = dict(xyz=t(stack(["x", "y", "z"])), normal=t(stack(["nx", "ny", "nz"])))
    out["features_dc"], out["features_rest"] = sh("f_dc", "f_rest", 3)
    out.update(opacity=t(col["opacity"][..., None]), scaling=t(stack(["scale_%d" % i for i in range(3)])),
               rotation=t(stack(["rot_%d" % i for i in range(4)])), base_color=t(stack(["base_color_%d" % i for i in range(3)])),
               roughness=t(col["roughness"][..., None]))
    out["incidents_dc"], out["incidents_rest"] = sh("incidents_dc", "incidents_rest", 3)
    out["visibility_dc"], out["visibility_rest"] = sh("visibility_dc", "visibility_rest", 1)
    return out


def route_a():
    return compose.assemble(paths, transforms, device=dev)


def route_b():
    return relight.compose_scenes([load_ply_numpy(p) for p in paths], transforms)


routes = (("(a) compose.assemble", route_a), ("(b) numpy columns + compose_scenes", route_b))
for _, fn in routes:
    fn()
ms = {n: [] for n, _ in routes}; peak = {}
for rep in range(REPS):
    for n, fn in routes:
        torch.cuda.synchronize(); torch.cuda.empty_cache(); torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ms[n].append((time.perf_counter() - t0) * 1e3)
        peak[n] = max(peak.get(n, 0), torch.cuda.max_memory_allocated() - base - composite_bytes)
        del out
print("composite of %s = %d rows x 130 columns (%.1f MB)" % (" + ".join(str(s) for s in SIZES), total, composite_bytes / 2 ** 20))
for n, _ in routes:
    print("%-38s files -> ready composite: median %9.2f ms (min %9.2f max %9.2f, %d reps)   peak memory above the composite %8.1f MB"
          % (n, median(ms[n]), min(ms[n]), max(ms[n]), REPS, peak[n] / 2 ** 20))
a, b = route_a(), route_b()
for k in a:
    d = (a[k] - b[k]).abs().max().item()
    print("  %-16s max |(a) - (b)| %.3e" % (k, d))
del b
# the placement launches alone
uploads = [ply.upload(ply.read_records(p), dev) for p in paths]
pls = [compose.placement_of(T).to(dev) for T in transforms]
offsets = np.concatenate([[0], np.cumsum(SIZES)[:-1]])
for flags, label in ((compose.ZERO_INCIDENTS, "zero_incidents"), (0, "plain")):
    t = []
    for rep in range(REPS + 2):
        torch.cuda.synchronize()
        e0, e1 = event(), event()
        e0.record()
        for (rec, cmap, _), pl, off in zip(uploads, pls, offsets):
            ply.place_records(rec, cmap, a, int(off), pl, flags)
        e1.record(); torch.cuda.synchronize()
        if rep >= 2:
            t.append(e0.elapsed_time(e1))
    moved = total * 130 * 4 * 2
    print("r3dg_scene_place_records x %d (%s): median %7.3f ms (min %7.3f max %7.3f, %d reps)  %.1f MB moved -> %.2f TB/s "
          "(%.0f %% of 6.3 TB/s)" % (len(SIZES), label, median(t), min(t), max(t), REPS, moved / 2 ** 20,
                                     moved / median(t) / 1e9, 100 * moved / median(t) / 1e9 / 6.3))
del uploads
# the driver, PNG output on and off
envmap = (3.0 * torch.rand(256, 512, 3, generator=torch.Generator().manual_seed(7)) ** 2).to(dev)
cams = syn.orbit_cameras(FRAMES, width=RES, height=RES)
renderer = relight.RelightRenderer(types.SimpleNamespace(**a), envmap, K, device_visibility=True)
out_dir = os.path.join(work, "frames")
os.makedirs(out_dir)
for png in (False, True, False, True):
    writer = relighting.FrameWriter() if png else None
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i, frames in relighting.render_trajectory(a, envmap, cams, None, ("pbr_env",), sample_num=K, renderer=renderer):
        if png:
            writer.submit(frames["pbr_env"], os.path.join(out_dir, "frame_%d.png" % i))
    if png:
        writer.close()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    print("driver, %d frames %dx%d, %d rows, K=%d, PNG output %-3s: %7.1f frames / s (%d encoder threads)" % (
        FRAMES, RES, RES, total, K, "on" if png else "off", FRAMES / dt, writer.workers if png else 0))
shutil.rmtree(work, ignore_errors=True)
