"""Time what a relight renderer costs before its second frame (GPU only): relight.RelightRenderer(...) plus the first frame() --
the frame that builds the fixed-light cache -- with the default construction (train_step.update_visibility, r3dg_shade_build_taps +
r3dg_shade_build_transport) against device_visibility=True (train_step.update_visibility_device, r3dg_shade_build_transport_rayset),
P Gaussians x K samples on the synthetic stage-2 scene.  HIP events around the construction and around the first frame, WARMUP
untimed constructions per path first, the two paths alternating inside every repetition; peak memory =
torch.cuda.max_memory_allocated above what the inputs hold, resident = what is still allocated above them with the renderer alive.
Then the cache builders alone, on the renderers of the last repetition: the two-kernel path against the one launch, alternating.
CONFIGS="P:K,P:K"  RES=<frame width and height>.  Both paths live in one build, so one run compares them on the same machine in
the same minute."""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from relightable3dgaussian_amd import relight, shading_ops, synthetic as syn
from relightable3dgaussian_amd.bench_core import GaussianParams
CONFIGS = [tuple(int(x) for x in c.split(":")) for c in os.environ.get("CONFIGS", "300000:64,300000:384").split(",")]
WARMUP = int(os.environ.get("WARMUP", 2)); REPS = int(os.environ.get("REPS", 5)); RES = int(os.environ.get("RES", 800)); dev = "cuda"
PATHS = (("default", False), ("device_visibility", True))
event = lambda: torch.cuda.Event(enable_timing=True)
median = lambda t: sorted(t)[len(t) // 2]
envmap = (3.0 * torch.rand(256, 512, 3, generator=torch.Generator().manual_seed(7)) ** 2).to(dev)
cam = syn.orbit_cameras(100, width=RES, height=RES)[0].to(dev)
bg = torch.zeros(3, device=dev)
for P, K in CONFIGS:
    params = GaussianParams(syn.make_scene(P=P, seed=0, stage2=True), dev, True)
    ms = {n: dict(construct=[], frame=[], total=[]) for n, _ in PATHS}; peak, resident, last = {}, {}, {}
    for name, flag in PATHS:
        for _ in range(WARMUP):
            relight.RelightRenderer(params, envmap, K, device_visibility=flag).frame(cam, bg)
    for rep in range(REPS):
        for name, flag in PATHS:
            last.pop(name, None)
            torch.cuda.synchronize(); torch.cuda.empty_cache(); torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()           # (the other path's renderer of this repetition is alive: part of the base)
            e0, e1, e2 = event(), event(), event()
            e0.record(); r = relight.RelightRenderer(params, envmap, K, device_visibility=flag); e1.record()
            out = r.frame(cam, bg); e2.record(); torch.cuda.synchronize()
            ms[name]["construct"].append(e0.elapsed_time(e1)); ms[name]["frame"].append(e1.elapsed_time(e2))
            ms[name]["total"].append(e0.elapsed_time(e2))
            peak[name] = max(peak.get(name, 0), torch.cuda.max_memory_allocated() - base)
            del out
            resident[name] = torch.cuda.memory_allocated() - base
            last[name] = r
            del r
    for name, _ in PATHS:
        m = ms[name]
        print("P=%d K=%d %dx%d  %-18s construction median %8.2f ms  first frame %7.2f ms  together %8.2f ms (min %8.2f max %8.2f, "
              "%d reps)  peak memory %8.1f MB  resident %8.1f MB  visible %.3f" % (
                  P, K, RES, RES, name, median(m["construct"]), median(m["frame"]), median(m["total"]), min(m["total"]),
                  max(m["total"]), REPS, peak[name] / 2 ** 20, resident[name] / 2 ** 20,
                  (last[name].visibility > 0).float().mean().item()))
    a, b = last["default"], last["device_visibility"]
    diff = (a.shade_out - b.shade_out).abs()
    print("P=%d K=%d  first-frame shading outputs, device_visibility vs default (each on its own trace): mean |diff| %.2e, max %.2e "
          "(max |default| %.3g)" % (P, K, diff.mean().item(), diff.max().item(), a.shade_out.abs().max().item()))
    # the cache builders alone: same normals, incident light, map and (the default renderer's) visibility
    He, We = envmap.shape[0], envmap.shape[1]

    def two_kernels():
        rec = shading_ops.build_taps(a.incident_dirs, He, We, None, radiance_of=envmap)
        return rec, shading_ops.build_transport(a.a_normal, a.incidents, a.visibility, a.incident_dirs, None, a._uniform_area, rec)

    def one_launch():
        return shading_ops.build_transport_rayset(a.a_normal, a.incidents, a.visibility, b._zsamples, b._uniform_area, envmap)
    builders = (("build_taps + build_transport", two_kernels), ("build_transport_rayset", one_launch))
    tb = {n: [] for n, _ in builders}; res = {}
    for n, fn in builders:
        for _ in range(WARMUP):
            fn()
    for rep in range(REPS):
        for n, fn in builders:
            torch.cuda.synchronize()
            e0, e1 = event(), event()
            e0.record(); res[n] = fn(); e1.record(); torch.cuda.synchronize()
            tb[n].append(e0.elapsed_time(e1))
    want, got = res["build_taps + build_transport"][0].view(torch.float32), res["build_transport_rayset"][0]
    for n, _ in builders:
        print("P=%d K=%d  %-30s median %7.3f ms (min %7.3f max %7.3f, %d reps)" % (P, K, n, median(tb[n]), min(tb[n]), max(tb[n]), REPS))
    rdiff, top = (got.reshape(want.shape) - want).abs(), want.abs().max().item()
    print("P=%d K=%d  transport records, one launch vs two kernels: max |diff| %.2e, beyond 1e-4 max: %d of %d (max |two kernels| "
          "%.3g; this map's end columns differ, so a sample on the theta = +-pi seam may read either)" % (
              P, K, rdiff.max().item(), int((rdiff > 1e-4 * top).sum()), rdiff.numel(), top))
    del a, b, last, res, want, got, params
    torch.cuda.empty_cache()
