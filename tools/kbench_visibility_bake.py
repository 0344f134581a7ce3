"""Time the visibility bake (GPU only) at P Gaussians, T iterations per chunk, on the synthetic scene of kbench_trace.py:
    trace   (a) bvh_ops.trace_hemisphere alone: P x T rays in one launch                      ms, Mrays/s
    fit     (b) r3dg_visibility_sh_fit alone (with and without the loss partials)             ms, bytes moved over time
    chunk   (c) one chunk end to end: VisibilityBaker.run(T) -- draws, trace, fit, loss sum   ms
    loop    (d) the same T iterations one at a time, the way the code before the bake had to: per iteration torch.randn +
                normalize / flip + RayTracer.trace_visibility + visibility_bake.fit_torch on the device    ms  <- the yardstick
HIP events around each repetition, WARMUP untimed repetitions first, medians.  Every leg runs in a child process of its own under
its own time limit (LEG_TIMEOUT seconds); the first leg that fails or runs out of time ends the run.  The report goes to OUT
(default profiles/r09_visibility_bake.txt).  P, T, WARMUP, REPS from the environment."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
P, T = int(os.environ.get("P", 300000)), int(os.environ.get("T", 64))
WARMUP, REPS = int(os.environ.get("WARMUP", 2)), int(os.environ.get("REPS", 7))
LEGS = ("trace", "fit", "chunk", "loop")


def _median_ms(fn):
    import torch
    for _ in range(WARMUP):
        fn()
    ms = []
    for _ in range(REPS):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    ms.sort()
    return ms[len(ms) // 2], ms[0], ms[-1]


def leg(name):
    import torch
    import torch.nn.functional as F
    from relightable3dgaussian_amd import _lib, bvh_ops, synthetic as syn, visibility_bake as vb
    dev = "cuda"
    sc = syn.make_scene(P=P, seed=0, stage2=False)
    d = {k: v.to(dev) for k, v in sc.items() if torch.is_tensor(v)}
    xyz, normal = d["xyz"], d["normal"]
    baker = vb.VisibilityBaker(xyz, d["scales"], d["rotations"], d["opacity"], normal, chunk=T)
    tracer, gen = baker.tracer, torch.Generator(device=dev).manual_seed(0)
    head = "P=%d T=%d  %-44s" % (P, T, name)
    if name in ("trace", "fit"):
        draws = torch.randn(T, P, 3, device=dev, generator=gen)
        vis, dirs = torch.empty(T, P, device=dev), torch.empty(T, P, 3, device=dev)
        bvh_ops.trace_hemisphere(tracer._records, tracer.tree, draws, vis, dirs)
    if name == "trace":
        med, lo, hi = _median_ms(lambda: bvh_ops.trace_hemisphere(tracer._records, tracer.tree, draws, vis, dirs))
        print("%s median %8.3f ms (min %8.3f max %8.3f, %d reps)  %7.1f Mrays/s  visible %.3f  stack overflow %d" % (
            head, med, lo, hi, REPS, P * T / med / 1e3, float((vis > 0).float().mean()), int(bvh_ops.trace_hemisphere.last_overflow)))
    elif name == "fit":
        L = _lib.lib()
        rows = int(L.r3dg_visibility_sh_fit_loss_rows(P))
        state = [torch.zeros(P, 16, device=dev) for _ in range(3)]
        part = torch.empty(rows, T, device=dev)
        moved = P * T * 16 + 2 * 3 * P * 64                           # directions + visibility read, the state read and written
        for tag, p in (("with loss partials", part), ("without", None)):
            def fit():
                _lib.check(L.r3dg_visibility_sh_fit(_lib.current_stream(), P, T, 0, dirs.data_ptr(), vis.data_ptr(), 1e-2, 0.9, 0.999,
                                                    1e-8, *[s.data_ptr() for s in state], _lib.ptr(p)), "visibility_sh_fit")
            med, lo, hi = _median_ms(fit)
            print("%s median %8.3f ms (min %8.3f max %8.3f, %d reps)  %6.1f MB moved  %7.1f GB/s" % (
                "P=%d T=%d  %-44s" % (P, T, "fit " + tag), med, lo, hi, REPS, moved / 1e6, moved / med / 1e6))
    elif name == "chunk":
        losses = []
        med, lo, hi = _median_ms(lambda: losses.append(baker.run(T, generator=gen)))
        print("%s median %8.3f ms (min %8.3f max %8.3f, %d reps)  loss %.4f at iteration 1, %.4f at iteration %d" % (
            head, med, lo, hi, REPS, float(losses[0][0]), float(losses[-1][-1]), baker.steps))
    elif name == "loop":
        op = d["opacity"][:, 0].contiguous()
        s = [torch.zeros(P, 16, device=dev), None, None]
        done = [0]

        def loop():
            for _ in range(T):
                z = F.normalize(torch.randn(P, 3, device=dev, generator=gen), dim=-1)
                z = torch.where(((z * normal).sum(-1) < 0)[:, None], -z, z)
                v = tracer.trace_visibility(xyz, z, xyz, tracer.covs_inv, op, normal)["visibility"][:, 0]
                s[0], s[1], s[2], _ = vb.fit_torch(z[None], v[None], s[0], s[1], s[2], steps_done=done[0])
                done[0] += 1
        med, lo, hi = _median_ms(loop)
        print("%s median %8.3f ms (min %8.3f max %8.3f, %d reps)  %d iterations one at a time" % (head, med, lo, hi, REPS, T))
    torch.cuda.synchronize()


def main():
    out = os.environ.get("OUT", os.path.join(ROOT, "profiles", "r09_visibility_bake.txt"))
    limit = int(os.environ.get("LEG_TIMEOUT", 240))
    lines = ["python tools/kbench_visibility_bake.py   (P=%d T=%d WARMUP=%d REPS=%d; HIP-event medians, one child process per leg)" % (
        P, T, WARMUP, REPS)]
    status = 0
    for name in LEGS:
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", name], capture_output=True, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            lines.append("%s: no result within %d s; stopped here" % (name, limit))
            status = 124
            break
        lines += [ln for ln in r.stdout.splitlines() if ln.startswith("P=")]
        if r.returncode != 0:
            lines.append("%s: exit status %d; stopped here\n%s" % (name, r.returncode, r.stderr[-2000:]))
            status = 1
            break
    if status == 0:
        ms = {ln.split()[2]: float(ln.split("median")[1].split()[0]) for ln in lines[1:]}
        lines.append("one chunk (c) / the same iterations one at a time (d): %.3f ms / %.3f ms = %.4f  (%.1f x)" % (
            ms["chunk"], ms["loop"], ms["chunk"] / ms["loop"], ms["loop"] / ms["chunk"]))
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as fh:
        fh.write(text)
    sys.stdout.write(text)
    return status


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--leg":
        leg(sys.argv[2])
    else:
        sys.exit(main())
