"""Time what a relight renderer costs before its second frame (GPU only): relight.RelightRenderer(...) plus the first frame() --
the frame that builds the fixed-light cache -- with the default construction (train_step.update_visibility, r3dg_shade_build_taps +
r3dg_shade_build_transport) against device_visibility=True (train_step.update_visibility_device, r3dg_shade_build_transport_rayset)
and baked_visibility=True (no trace: r3dg_shade_build_transport_baked on the coefficients visibility_bake.bake_visibility(...,
iterations=BAKE) fitted to the same scene), P Gaussians x K samples on the synthetic stage-2 scene.  HIP events around the construction and around the first frame, WARMUP
untimed constructions per path first, the two paths alternating inside every repetition; peak memory =
torch.cuda.max_memory_allocated above what the inputs hold, resident = what is still allocated above them with the renderer alive.
Then the cache builders alone, on the renderers of the last repetition: the two-kernel path against the one launch, alternating.
Then, baked against device_visibility on the renderers of the last repetition: steady-state frame time under a fixed and under a
turning light (BLOCKS blocks of FRAMES frames each, alternating, HIP events around a block) and the PSNR of the baked pbr_env
frames against the traced ones over 8 orbit views -- what the degree-3 SH costs.
CONFIGS="P:K,P:K"  RES=<frame width and height>.  All paths live in one build, so one run compares them on the same machine in
the same minute."""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import math
import torch
from relightable3dgaussian_amd import relight, shading_ops, synthetic as syn
from relightable3dgaussian_amd.visibility_bake import bake_visibility
from relightable3dgaussian_amd.bench_core import GaussianParams
CONFIGS = [tuple(int(x) for x in c.split(":")) for c in os.environ.get("CONFIGS", "300000:64,300000:384").split(",")]
WARMUP = int(os.environ.get("WARMUP", 2)); REPS = int(os.environ.get("REPS", 5)); RES = int(os.environ.get("RES", 800)); dev = "cuda"
BAKE = int(os.environ.get("BAKE", 1000)); BLOCKS = int(os.environ.get("BLOCKS", 7)); FRAMES = int(os.environ.get("FRAMES", 50))
PATHS = (("default", {}), ("device_visibility", dict(device_visibility=True)), ("baked", dict(baked_visibility=True)))
event = lambda: torch.cuda.Event(enable_timing=True)
median = lambda t: sorted(t)[len(t) // 2]
envmap = (3.0 * torch.rand(256, 512, 3, generator=torch.Generator().manual_seed(7)) ** 2).to(dev)
cam = syn.orbit_cameras(100, width=RES, height=RES)[0].to(dev)
bg = torch.zeros(3, device=dev)
for P, K in CONFIGS:
    params = GaussianParams(syn.make_scene(P=P, seed=0, stage2=True), dev, True)
    e0, e1 = event(), event()
    e0.record(); losses = bake_visibility(params, iterations=BAKE); e1.record(); torch.cuda.synchronize()
    print("P=%d  bake_visibility(iterations=%d): %.1f ms, L1 loss first / last 50 iterations %.4f / %.4f" % (
        P, BAKE, e0.elapsed_time(e1), losses[:50].mean().item(), losses[-50:].mean().item()))
    del losses
    torch.cuda.empty_cache()
    ms = {n: dict(construct=[], frame=[], total=[]) for n, _ in PATHS}; peak, resident, last = {}, {}, {}
    for name, flag in PATHS:
        for _ in range(WARMUP):
            relight.RelightRenderer(params, envmap, K, **flag).frame(cam, bg)
    for rep in range(REPS):
        for name, flag in PATHS:
            last.pop(name, None)
            torch.cuda.synchronize(); torch.cuda.empty_cache(); torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()           # (the other path's renderer of this repetition is alive: part of the base)
            e0, e1, e2 = event(), event(), event()
            e0.record(); r = relight.RelightRenderer(params, envmap, K, **flag); e1.record()
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
                  float("nan") if last[name].visibility is None else (last[name].visibility > 0).float().mean().item()))
    a, b, c = last["default"], last["device_visibility"], last["baked"]
    diff = (a.shade_out - b.shade_out).abs()
    print("P=%d K=%d  first-frame shading outputs, device_visibility vs default (each on its own trace): mean |diff| %.2e, max %.2e "
          "(max |default| %.3g)" % (P, K, diff.mean().item(), diff.max().item(), a.shade_out.abs().max().item()))
    diff = (c.shade_out - b.shade_out).abs()
    print("P=%d K=%d  first-frame shading outputs, baked (SH of %d bake iterations) vs device_visibility (traced): mean |diff| %.2e, "
          "max %.2e (max |device_visibility| %.3g); visibility column alone: mean |diff| %.2e" % (
              P, K, BAKE, diff.mean().item(), diff.max().item(), b.shade_out.abs().max().item(), diff[:, 18].mean().item()))
    # the cache builders alone: same normals, incident light, map and (the default renderer's) visibility
    He, We = envmap.shape[0], envmap.shape[1]

    def two_kernels():
        rec = shading_ops.build_taps(a.incident_dirs, He, We, None, radiance_of=envmap)
        return rec, shading_ops.build_transport(a.a_normal, a.incidents, a.visibility, a.incident_dirs, None, a._uniform_area, rec)

    def one_launch():
        return shading_ops.build_transport_rayset(a.a_normal, a.incidents, a.visibility, b._zsamples, b._uniform_area, envmap)

    def baked():
        return shading_ops.build_transport_baked(a.a_normal, a.incidents, c.visibility_sh, b._zsamples, b._uniform_area, envmap)
    builders = (("build_taps + build_transport", two_kernels), ("build_transport_rayset", one_launch), ("build_transport_baked", baked))
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
    # steady state, baked against device_visibility: the same per-frame kernels serve both
    orbit = [cm.to(dev) for cm in syn.orbit_cameras(8, width=RES, height=RES)]
    turns = [torch.tensor([[math.cos(t), -math.sin(t), 0.0], [math.sin(t), math.cos(t), 0.0], [0.0, 0.0, 1.0]], device=dev)
             for t in (0.05 * i for i in range(1, FRAMES + 1))]
    for light in ("fixed", "turning"):
        per = {"device_visibility": [], "baked": []}
        for blk in range(BLOCKS + 1):                                       # (the first block warms the caches of this light)
            for n, r in (("device_visibility", b), ("baked", c)):
                torch.cuda.synchronize()
                e0, e1 = event(), event()
                e0.record()
                for i in range(FRAMES):
                    r.frame(orbit[i % 8], bg, env_transform=turns[i] if light == "turning" else None)
                e1.record(); torch.cuda.synchronize()
                if blk:
                    per[n].append(e0.elapsed_time(e1) / FRAMES)
        for n in per:
            print("P=%d K=%d %dx%d  steady state, %-7s light  %-18s median %7.4f ms / frame (min %7.4f max %7.4f, %d blocks of %d frames)"
                  % (P, K, RES, RES, light, n, median(per[n]), min(per[n]), max(per[n]), BLOCKS, FRAMES))
    psnr = []
    for cm in orbit:
        fb, fc = b.frame(cm, bg)["pbr_env"], c.frame(cm, bg)["pbr_env"]
        psnr.append(-10.0 * math.log10(max((fb - fc).square().mean().item(), 1e-20)))
    print("P=%d K=%d %dx%d  PSNR of baked pbr_env frames against traced (device_visibility) ones, 8 orbit views: mean %.2f dB, "
          "min %.2f, max %.2f" % (P, K, RES, RES, sum(psnr) / len(psnr), min(psnr), max(psnr)))
    del a, b, c, last, res, want, got, params, orbit
    torch.cuda.empty_cache()
