"""The device PNG encoder measured (profiles/r18_png_device.txt):

    python tools/kbench_png.py [--res 800] [--points 300000] [--frames 60] [--blocks 6] [--reps 30] [--skip-training]

kernel    r3dg_png_encode (three launches, HIP events around the call, median of `reps`) at res x res x 3 on a real pbr_env frame of
          the synthetic composite, a real 16-panel contact sheet and uniform noise (every segment stored): time per frame, bytes in
          and out, and the ratio to what the same bytes cost at the copy bandwidth of this run -- the filtered stream read once, the
          output written once, bandwidth = a 256 MB device-to-device copy (read + write) timed the same way; and the ratio to a
          copy of the picture itself, which at 1.9 MB is one launch and far from that bandwidth.
frames    relighting.render_trajectory over `frames` orbit frames of the 300k + 300k + 100k composite (the configuration of
          profiles/r11_scene_assembly.txt) through FrameWriter() and FrameWriter(device_png=True), alternating blocks of ONE
          process, files to the same directory; then the worker's host work per file (CRC-32 + framing, write) split by the clock.
sizes     the files of both writers over those frames and over the sheet: ratio device / PIL, mean and worst.
training  train_loop.train_stage2 with a sheet every `interval` iterations, blocks alternating between the PIL writer and the
          device encoder (the loop of tools/kbench_training_vis.py).
"""
import argparse
import os
import shutil
import statistics
import sys
import tempfile
import time
import types
import zlib

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def event():
    return torch.cuda.Event(enable_timing=True)


def timed(fn, reps):
    """Median and minimum of fn() in ms by HIP events, after three warm calls."""
    ms = []
    for i in range(reps + 3):
        a, b = event(), event()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        if i >= 3:
            ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms)


def composite_of(sizes, dev, work):
    from relightable3dgaussian_amd import compose, ply, synthetic as syn
    from relightable3dgaussian_amd.bench_core import GaussianParams
    paths, transforms = [], []
    for j, P in enumerate(sizes):
        model = GaussianParams(syn.make_scene(P=P, seed=j, stage2=True), dev, True)
        model.visibility_sh = (0.1 * torch.randn(P, 16, generator=torch.Generator().manual_seed(j))).to(dev)
        paths.append(os.path.join(work, "object%d.ply" % j))
        ply.save(paths[-1], model)
        a = 0.7 * j
        T = torch.eye(4)
        T[:3, :3] = (0.8 + 0.2 * j) * torch.tensor([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])
        T[:3, 3] = torch.tensor([1.6 * (j - 1), 0.3 * j, 0.0])
        transforms.append(T)
        del model
    return compose.assemble(paths, transforms, device=dev)


def kernel_rows(pictures, reps):
    from relightable3dgaussian_amd import png_device
    first = next(iter(pictures.values()))
    copy = torch.empty_like(first)
    copy_ms, _ = timed(lambda: copy.copy_(first), reps)
    small = 2 * first.numel() / (copy_ms * 1e-3)                            # bytes per second, read + write
    big = torch.empty(256 << 20, dtype=torch.uint8, device=first.device)
    big2 = torch.empty_like(big)
    big_ms, _ = timed(lambda: big2.copy_(big), 10)
    bandwidth = 2 * big.numel() / (big_ms * 1e-3)
    del big, big2
    print("copy: %d bytes device to device in %.4f ms -> %.2f TB/s read + write (a launch, not bandwidth); %d bytes in %.3f ms -> "
          "%.2f TB/s, the bandwidth of the ratios below" % (first.numel(), copy_ms, small / 1e12, 256 << 20, big_ms, bandwidth / 1e12))
    for name, x in pictures.items():
        H, W, C = x.shape
        out = (torch.empty(png_device.zlib_bound(W, H, C), dtype=torch.uint8, device=x.device),
               torch.empty(1, dtype=torch.int32, device=x.device))
        med, low = timed(lambda: png_device.encode(x, out=out), reps)
        n = int(out[1].item())
        stream = out[0][:n].cpu().numpy().tobytes()
        filtered = zlib.decompress(stream)
        assert len(filtered) == H * (W * C + 1)
        floor_ms = 1e3 * (len(filtered) + n) / bandwidth
        print("r3dg_png_encode %-8s %d x %d x %d: median %.4f ms (min %.4f, %d reps); %d bytes in, %d out (%.3f of raw); "
              "the filtered stream read once + the output written once at the copy bandwidth: %.4f ms -> ratio %.0f; "
              "against the copy of the picture itself (%.4f ms): %.1f"
              % (name, H, W, C, med, low, reps, x.numel(), n, n / x.numel(), floor_ms, med / floor_ms, copy_ms, med / copy_ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=800)
    ap.add_argument("--points", type=int, default=300_000)
    ap.add_argument("--sizes", default="300000,300000,100000")
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--blocks", type=int, default=6)
    ap.add_argument("--sample-num", type=int, default=64)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--interval", type=int, default=200)
    ap.add_argument("--train-blocks", type=int, default=8)
    ap.add_argument("--train-block", type=int, default=400)
    ap.add_argument("--skip-training", action="store_true")
    args = ap.parse_args()
    from relightable3dgaussian_amd import png_device, relight, relighting, synthetic as syn, train_loop, training_vis
    from relightable3dgaussian_amd.bench_core import GaussianParams, render_stage1
    dev = torch.device("cuda", 0)
    work = tempfile.mkdtemp(prefix="kbench_png_")
    RES, K = args.res, args.sample_num

    # ---- the pictures: a frame, a sheet, noise ----
    sizes = [int(v) for v in args.sizes.split(",")]
    composite = composite_of(sizes, dev, work)
    envmap = (3.0 * torch.rand(256, 512, 3, generator=torch.Generator().manual_seed(7)) ** 2).to(dev)
    cams = syn.orbit_cameras(args.frames, width=RES, height=RES)
    renderer = relight.RelightRenderer(types.SimpleNamespace(**composite), envmap, K, device_visibility=True)
    _, frames = next(iter(relighting.render_trajectory(composite, envmap, cams[:1], None, ("pbr_env",), sample_num=K,
                                                       renderer=renderer)))
    pictures = {"frame": relighting.quantize(frames["pbr_env"]).clone()}
    scene = syn.make_scene(P=args.points, seed=0, stage2=True)
    tcams = [c.to(dev) for c in syn.orbit_cameras(100, width=RES, height=RES)[:4]]
    bg = torch.ones(3, device=dev)
    params = GaussianParams(scene, dev, True)
    with torch.no_grad():
        teacher = GaussianParams(syn.make_scene(P=args.points, seed=0, stage2=False), dev, False)
        teacher.features_dc.add_(0.05 * torch.randn_like(teacher.features_dc))
        gts = [render_stage1(teacher, c, bg)[2].clone() for c in tcams]
        del teacher
    step, _ = train_loop.train_stage2(params, tcams, gts, bg, 2.6, K, iterations=50, poll_interval=0)
    sheets = training_vis.TrainingSheet(step, K)
    pictures["sheet"] = sheets.sheet(tcams[0], gts[0], bg).clone()
    pictures["noise"] = torch.randint(0, 256, (RES, RES, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(1)).to(dev)
    print("1. kernel time (%d x %d x 3)" % (RES, RES))
    kernel_rows(pictures, args.reps)

    # ---- frames to disk ----
    print("2. frames to disk: %d frames %d x %d, %d rows, K = %d, alternating blocks of one process" % (
        args.frames, RES, RES, sum(sizes), K))
    dirs = {False: os.path.join(work, "pil"), True: os.path.join(work, "device")}
    for d in dirs.values():
        os.makedirs(d)
    rates = {False: [], True: []}
    for b in range(args.blocks):
        device_png = b % 2 == 1
        writer = relighting.FrameWriter(device_png=True) if device_png else relighting.FrameWriter()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        in_submit = 0.0
        for i, fr in relighting.render_trajectory(composite, envmap, cams, None, ("pbr_env",), sample_num=K, renderer=renderer):
            t1 = time.perf_counter()
            writer.submit(fr["pbr_env"], os.path.join(dirs[device_png], "frame_%d.png" % i))
            in_submit += time.perf_counter() - t1
        t1 = time.perf_counter()
        writer.close()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        rate = args.frames / (t2 - t0)
        rates[device_png].append(rate)
        print("  block %-10s %8.1f frames / s (%d worker threads; host time inside submit() %.3f ms per frame, close() waited %.1f ms)"
              % ("device_png" if device_png else "PIL", rate, writer.workers, 1e3 * in_submit / args.frames, 1e3 * (t2 - t1)))
    t0 = time.perf_counter()
    for i, fr in relighting.render_trajectory(composite, envmap, cams, None, ("pbr_env",), sample_num=K, renderer=renderer):
        pass
    torch.cuda.synchronize()
    print("  no files   %8.1f frames / s" % (args.frames / (time.perf_counter() - t0)))
    for device_png, label in ((False, "PIL"), (True, "device_png")):
        r = rates[device_png]
        print("%-10s median %8.1f frames / s (min %.1f, max %.1f, %d blocks)" % (label, statistics.median(r), min(r), max(r), len(r)))
    # what a frame adds on the device: quantise + encode + the copy of the bound to pinned memory, by events on an idle device
    probe = relighting.FrameWriter(workers=1, slots=1, device_png=True)
    img = frames["pbr_env"]
    probe.submit(img, os.path.join(work, "probe.png"))
    probe.close()
    bound = png_device.zlib_bound(RES, RES, 3)
    zbuf = torch.empty(4 + bound, dtype=torch.uint8, device=dev)
    zhost = torch.empty(4 + bound, dtype=torch.uint8, pin_memory=True)
    qbytes = torch.empty(RES, RES, 3, dtype=torch.uint8, device=dev)

    def device_half():
        relighting.quantize(img, qbytes)
        png_device.encode(qbytes, out=(zbuf[4:], zbuf[:4].view(torch.int32)))
        zhost.copy_(zbuf, non_blocking=True)
    dev_ms, dev_min = timed(device_half, args.reps)
    print("per frame on the device: quantise + encode + copy of the bound to pinned memory %.3f ms (min %.3f, events)" % (dev_ms, dev_min))
    # the worker's host work on one frame
    zdev, ndev = png_device.encode(pictures["frame"])
    n = int(ndev.item())
    pinned = torch.empty(zdev.numel(), dtype=torch.uint8, pin_memory=True)
    copy_ms, _ = timed(lambda: pinned.copy_(zdev, non_blocking=True), 10)
    host = pinned.numpy()
    t_wrap, t_write = [], []
    for i in range(10):
        t0 = time.perf_counter()
        data = png_device.wrap(host[:n].tobytes(), RES, RES, 3)
        t1 = time.perf_counter()
        with open(os.path.join(work, "probe_%d.png" % i), "wb") as fh:
            fh.write(data)
        t2 = time.perf_counter()
        t_wrap.append(1e3 * (t1 - t0))
        t_write.append(1e3 * (t2 - t1))
    print("per file on the host: copy of the bound (%d bytes) to pinned memory %.3f ms, CRC-32 + framing of %d bytes %.3f ms, "
          "write() %.3f ms (medians of 10)" % (zdev.numel(), copy_ms, n, statistics.median(t_wrap), statistics.median(t_write)))

    # ---- sizes ----
    print("3. file sizes, device_png / PIL")
    ratios = []
    for i in range(args.frames):
        a = os.path.getsize(os.path.join(dirs[True], "frame_%d.png" % i))
        b = os.path.getsize(os.path.join(dirs[False], "frame_%d.png" % i))
        ratios.append(a / b)
    mean_pil = statistics.mean(os.path.getsize(os.path.join(dirs[False], "frame_%d.png" % i)) for i in range(args.frames))
    print("frames: mean ratio %.3f, worst %.3f over %d files (PIL mean %d bytes, raw %d)" % (
        statistics.mean(ratios), max(ratios), len(ratios), mean_pil, RES * RES * 3))
    for device_png, name in ((False, "sheet_pil.png"), (True, "sheet_device.png")):
        w = relighting.FrameWriter(workers=1, device_png=True) if device_png else relighting.FrameWriter(workers=1)
        w.submit_bytes(pictures["sheet"], os.path.join(work, name))
        w.close()
    a, b = (os.path.getsize(os.path.join(work, f)) for f in ("sheet_device.png", "sheet_pil.png"))
    print("sheet: %d bytes against PIL's %d -> ratio %.3f" % (a, b, a / b))
    from PIL import Image
    same = all(np.array_equal(np.asarray(Image.open(os.path.join(dirs[True], "frame_%d.png" % i))),
                              np.asarray(Image.open(os.path.join(dirs[False], "frame_%d.png" % i)))) for i in range(0, args.frames, 7))
    print("decoded pixels of every 7th frame equal between the writers: %s" % same)

    # ---- training ----
    if not args.skip_training:
        print("4. training_vis at %d Gaussians, %d x %d, K = %d; sheet every %d iterations; blocks of %d iterations, alternating"
              % (args.points, RES, RES, K, args.interval, args.train_block))
        total = args.train_block * (1 + args.train_blocks)
        st = dict(t0=None, rates=[], sheets={})

        def on_iteration(it, step):
            if it <= args.train_block:
                if it == args.train_block:
                    step.flush()
                    torch.cuda.synchronize()
                    st["t0"] = time.perf_counter()
                return
            b = (it - args.train_block - 1) // args.train_block
            kind = "device_png" if b % 2 else "PIL"
            if it % args.interval == 0:
                if kind not in st["sheets"]:
                    st["sheets"][kind] = training_vis.TrainingSheet(step, K)
                    st["sheets"][kind].device_png = kind == "device_png"
                v = (it - 1) % len(tcams)
                st["sheets"][kind].save(tcams[v], gts[v], bg, os.path.join(work, "%s_%06d.png" % (kind, it)))
            if (it - args.train_block) % args.train_block == 0:
                step.flush()
                torch.cuda.synchronize()
                st["rates"].append((kind, args.train_block / (time.perf_counter() - st["t0"])))
                st["t0"] = time.perf_counter()
        params2 = GaussianParams(scene, dev, True)
        train_loop.train_stage2(params2, tcams, gts, bg, 2.6, K, iterations=total, on_iteration=on_iteration, poll_interval=0)
        for s in st["sheets"].values():
            s.close()
        for kind, rate in st["rates"]:
            print("  block %-10s %8.1f it/s" % (kind, rate))
        for kind in ("PIL", "device_png"):
            r = [x for k, x in st["rates"] if k == kind]
            print("%-10s median %8.1f it/s  (min %.1f, max %.1f, %d blocks)" % (kind, statistics.median(r), min(r), max(r), len(r)))
    shutil.rmtree(work, ignore_errors=True)


if __name__ == "__main__":
    main()
