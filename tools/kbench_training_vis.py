"""What --save_training_vis costs a stage-2 run at the headline size (profiles/r15_training_vis.txt):

    python tools/kbench_training_vis.py [--points 300000] [--res 800] [--sample-num 64] [--interval 200] [--blocks 8] [--block 400]

rate   train_loop.train_stage2 -- the loop `python -m relightable3dgaussian_amd.training -t neilf` drives -- over `blocks` blocks of
       `block` iterations in ONE process, alternately with and without the driver's sheet hook (a sheet of the iteration's view
       whenever the iteration count is a multiple of `interval`, through TrainingSheet.save: frame, sheet launch, asynchronous copy,
       PNG on a worker thread); every block is closed by a device synchronisation, the writer is closed after the last one.
sheet  one TrainingSheet.sheet() split by HIP events into the eval frame and the r3dg_training_sheet launch; medians.
encode PIL's PNG encode of one finished sheet on this host, per file.
"""
import argparse
import os
import shutil
import statistics
import sys
import tempfile
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=300_000)
    ap.add_argument("--res", type=int, default=800)
    ap.add_argument("--sample-num", type=int, default=64)
    ap.add_argument("--interval", type=int, default=200)
    ap.add_argument("--blocks", type=int, default=8)
    ap.add_argument("--block", type=int, default=400)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    from relightable3dgaussian_amd import synthetic as syn, train_loop, training_vis
    from relightable3dgaussian_amd.bench_core import GaussianParams, render_stage1
    dev = torch.device("cuda", 0)
    scene = syn.make_scene(P=args.points, seed=0, stage2=True)
    cams = [c.to(dev) for c in syn.orbit_cameras(100, width=args.res, height=args.res)[:4]]
    bg = torch.ones(3, device=dev)
    params = GaussianParams(scene, dev, True)
    with torch.no_grad():
        teacher = GaussianParams(syn.make_scene(P=args.points, seed=0, stage2=False), dev, False)
        teacher.features_dc.add_(0.05 * torch.randn_like(teacher.features_dc))
        gts = [render_stage1(teacher, c, bg)[2].clone() for c in cams]
        del teacher
    out_dir = tempfile.mkdtemp(prefix="training_vis_")
    warm = args.block
    total = warm + args.blocks * args.block
    state = dict(sheets=None, t0=None, rates=[], files=0)

    def on_iteration(it, step):
        if it <= warm:
            if it == warm:
                step.flush()
                torch.cuda.synchronize()
                state["t0"] = time.perf_counter()
            return
        b = (it - warm - 1) // args.block
        if b % 2 == 0 and it % args.interval == 0:                  # (blocks 0, 2, ...: with sheets)
            if state["sheets"] is None:
                state["sheets"] = training_vis.TrainingSheet(step, args.sample_num)
            v = (it - 1) % len(cams)
            state["sheets"].save(cams[v], gts[v], bg, os.path.join(out_dir, "%06d.png" % it))
            state["files"] += 1
        if (it - warm) % args.block == 0:
            step.flush()
            torch.cuda.synchronize()
            t = time.perf_counter()
            state["rates"].append(("sheets" if b % 2 == 0 else "plain", args.block / (t - state["t0"])))
            state["t0"] = time.perf_counter()

    step, _ = train_loop.train_stage2(params, cams, gts, bg, 2.6, args.sample_num, iterations=total, on_iteration=on_iteration,
                                      poll_interval=0)
    t0 = time.perf_counter()
    state["sheets"].close()
    t_close = time.perf_counter() - t0
    print("training_vis at %d Gaussians, %d x %d, K = %d; sheet every %d iterations; blocks of %d iterations, alternating"
          % (args.points, args.res, args.res, args.sample_num, args.interval, args.block))
    for kind, rate in state["rates"]:
        print("  block %-6s %8.1f it/s" % (kind, rate))
    for kind in ("sheets", "plain"):
        r = [x for k, x in state["rates"] if k == kind]
        print("%-6s median %8.1f it/s  (min %.1f, max %.1f, %d blocks)" % (kind, statistics.median(r), min(r), max(r), len(r)))
    print("files written %d; writer.close() after the last block waited %.3f s" % (state["files"], t_close))

    # one sheet(), split
    sheets = state["sheets"]
    ev = lambda: torch.cuda.Event(enable_timing=True)
    frame_ms, sheet_ms, whole_ms = [], [], []
    H = W = args.res
    out_h, out_w = training_vis.sheet_size(16, H, W)[:2]
    out = torch.empty(out_h, out_w, 3, dtype=torch.uint8, device=dev)
    with torch.no_grad(), step._ctx:
        for i in range(args.reps + 3):
            a, b, c = ev(), ev(), ev()
            a.record()
            fr = sheets._frame_stage2(cams[i % 4], bg)
            b.record()
            training_vis.launch_sheet(1, fr["render"], gts[i % 4], fr["opacity"], fr["n_contrib"], fr["feature"],
                                      fr["pseudo_normal"], bg, fr["env"], out)
            c.record()
            torch.cuda.synchronize()
            if i >= 3:
                frame_ms.append(a.elapsed_time(b))
                sheet_ms.append(b.elapsed_time(c))
        for i in range(args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            sheets.sheet(cams[i % 4], gts[i % 4], bg)
            torch.cuda.synchronize()
            whole_ms.append(1e3 * (time.perf_counter() - t0))
    n = out_h * out_w * 3
    print("sheet(): eval frame median %.3f ms (min %.3f), r3dg_training_sheet %.4f ms (min %.4f; %d bytes written, %d x %d x 3), "
          "whole call with its synchronisation %.3f ms (host clock)"
          % (statistics.median(frame_ms), min(frame_ms), statistics.median(sheet_ms), min(sheet_ms), n, out_h, out_w,
             statistics.median(whole_ms)))
    from PIL import Image
    host = sheets.sheet(cams[0], gts[0], bg).cpu().numpy()
    enc = []
    for i in range(5):
        t0 = time.perf_counter()
        Image.fromarray(host).save(os.path.join(out_dir, "encode_%d.png" % i))
        enc.append(1e3 * (time.perf_counter() - t0))
    size = os.path.getsize(os.path.join(out_dir, "encode_0.png"))
    print("encode: PIL PNG of one %d x %d sheet median %.1f ms per file (min %.1f; %d bytes on disk)"
          % (out_w, out_h, statistics.median(enc), min(enc), size))
    shutil.rmtree(out_dir, ignore_errors=True)


if __name__ == "__main__":
    main()
