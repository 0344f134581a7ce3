"""Time a whole visibility update (GPU only): train_step.update_visibility (PyTorch glue around the trace) against
train_step.update_visibility_device (leaf preparation and ray generation inside the kernels), P Gaussians x K rays each, on the
synthetic scene of kbench_trace.py.  HIP events around each call, WARMUP untimed calls per path first, the two paths alternating
inside every repetition; peak memory = torch.cuda.max_memory_allocated above what the inputs hold.  CONFIGS="P:K,P:K".
Both paths live in one build, so one run compares them on the same machine in the same minute."""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from relightable3dgaussian_amd import synthetic as syn
from relightable3dgaussian_amd.train_step import update_visibility, update_visibility_device
CONFIGS = [tuple(int(x) for x in c.split(":")) for c in os.environ.get("CONFIGS", "300000:64,300000:384").split(",")]
WARMUP = int(os.environ.get("WARMUP", 2)); REPS = int(os.environ.get("REPS", 5)); dev = "cuda"
PATHS = (("update_visibility", lambda a: update_visibility(*a)[0]),
         ("update_visibility_device", lambda a: update_visibility_device(*a)[0]),
         ("update_visibility_device want_dirs", lambda a: update_visibility_device(*a, want_dirs=True)[0]))
for P, K in CONFIGS:
    sc = syn.make_scene(P=P, seed=0, stage2=False)
    d = {k: v.to(dev) for k, v in sc.items() if torch.is_tensor(v)}
    args = (d["xyz"], d["scales"], d["rotations"], d["opacity"], d["normal"], K)
    ms = {n: [] for n, _ in PATHS}; peak = {}; vis = {}
    for name, fn in PATHS:
        for _ in range(WARMUP):
            fn(args)
    for rep in range(REPS):
        for name, fn in PATHS:
            torch.cuda.synchronize(); torch.cuda.empty_cache(); torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); out = fn(args); e1.record(); torch.cuda.synchronize()
            ms[name].append(e0.elapsed_time(e1)); peak[name] = max(peak.get(name, 0), torch.cuda.max_memory_allocated() - base)
            vis[name] = out
            del out
    ref = vis["update_visibility"]
    for name, _ in PATHS:
        t = sorted(ms[name]); med = t[len(t) // 2]
        diff = (vis[name] - ref).abs()
        print("P=%d K=%d  %-36s median %8.2f ms (min %8.2f max %8.2f, %d reps)  %7.1f Mrays/s  peak memory %8.1f MB  "
              "visible %.3f  vs update_visibility: mean |diff| %.2e, beyond 2e-5: %d of %d" % (
                  P, K, name, med, t[0], t[-1], len(t), P * K / med / 1e3, peak[name] / 2 ** 20,
                  (vis[name] > 0).float().mean().item(), diff.mean().item(), int((diff > 2e-5).sum()), diff.numel()))
    del vis, ref, d, args
    torch.cuda.empty_cache()
