"""The reference's train.py for a NeRF-synthetic (Blender), a Synthetic4Relight or a NeILF-format (DTU / TnT) dataset directory, on
the fused iterations:

    python -m relightable3dgaussian_amd.training -s DATA -m OUT -t render --eval
    python -m relightable3dgaussian_amd.training -s DATA -m OUT/neilf -t neilf -c OUT/chkpnt30000.pth --iterations 40000 --eval

The layout is picked as scene/__init__.py:43-61 picks it: `transforms_train.json` -> Blender (dataset.read_transforms,
dataset.initial_points), or Synthetic4Relight when the path contains that name (:51; dataset.read_syn4relight: the train split
is OpenEXR views, kept on the device as half / float samples by hdr_views.HdrViewStore and decoded there; the test split's
`_rgba.png` files go through dataset.ViewStore; the same initial points); `inputs/sfm_scene.json` -> NeILF (dataset.read_neilf_scene, dataset.initial_points_neilf, the views' mask
files, the off-centre projection of their fx, fy, cx, cy); anything else raises.  `-r / --resolution` (default -1, as
arguments/__init__.py:45) is loadCam's, for the 8-bit layouts and for the test split (an HdrViewStore raises for a scale other than 1): dataset.ViewStore resizes such views once, at load.
UNDER THE DEFAULT, FILES WIDER THAN 1600 PIXELS ARE NOW RESCALED TO 1600 as the reference rescales them (before, every file trained
at its own size); files up to 1600 pixels wide are treated exactly as before.

Stage 1 (`-t render`): the train split's images into a dataset.ViewStore (the views stay on the device as 8-bit
pixels; one unpack launch per iteration), the extent of synthetic.cameras_extent, the initial points ->
train_loop.create_from_points -> train_loop.train_stage1 with the view pick of train.py:115-119.  Stage 2 (`-t neilf -c CKPT`,
train.py:52-72): checkpoint.restore(CKPT, pbr=True), the environment texture light_init * rand(1, R, 2R, 3) (or the texture of
`env_light_<basename of CKPT>` beside CKPT), train_loop.train_stage2 for `--iterations` minus the checkpoint's iteration count,
the xyz rate continuing along its decay from there.

Written at the save / checkpoint intervals and at the end: OUT/chkpnt<it>.pth (checkpoint.capture),
OUT/point_cloud/iteration_<it>/point_cloud.ply (ply.save), for stage 2 OUT/env_light_chkpnt<it>.pth (`env_checkpoint`: the layout
of DirectLightMap.capture() inside train.py:197), and with --eval OUT/metrics.json: PSNR / SSIM of `render` on the test split
(evaluate.evaluate_nvs) and, after stage 2, of `pbr` from a relight.RelightRenderer on the learned texture softplus(env).
One progress line every --log_interval iterations (step.loss(): the only host read of the loop besides the overflow poll).

`--save_training_vis` [`--save_training_vis_iteration N`, default 1000] (every script the reference ships passes it): the contact
sheet of train.py:276-317, OUT/visualize/%06d.png, of the iteration's own view whenever the iteration count is a multiple of N
and at the run's first iteration -- one eval frame of the live step and one r3dg_training_sheet launch (training_vis), encoded
off the training thread; the writer is closed, and its errors raised, before --eval and before train() returns.  Without the flag
nothing of it exists: no directory, no launch, no import.  ONE DIFFERENCE: the fused step has applied Adam when the loop's hook
runs, so sheet g shows the state AFTER iteration g; the reference's shows the state before its optimizer step.

Arguments carry the names and defaults of the reference's arguments/__init__.py.  The lambdas the fused steps implement become
their loss weights; every other non-zero lambda RAISES before anything is loaded (`loss_weights_of`).

Out of scope: the COLMAP / Stanford-ORB readers; OpenEXR files other than NONE / ZIPS / ZIP scanline files (PIZ above all); `resolution_scale` other than 1 and upscaling; MVS depth /
normal maps (hence no lambda_depth / lambda_normal_mvs_depth); cfg_args, cameras.json, TensorBoard (training_report's grids too),
LPIPS; --video and the eval/ image folders of eval_render; data parallelism in this
driver (train_loop's loops take a process group; this command does not start one).  THE ONE KNOWN DIFFERENCE FROM THE REFERENCE
SCHEDULE: train.py:107-108 raises the active SH degree by one every 1000 iterations, the fused steps train degree 3 from the
first iteration.
"""
import argparse
import json
import os
import types

import torch

from . import checkpoint, dataset, evaluate, ply, synthetic, train_loop
from .train_step import STAGE1_WEIGHTS, STAGE2_WEIGHTS

# arguments/__init__.py:108-134
LAMBDA_DEFAULTS = dict(depth=0.0, depth_smooth=0.0, mask_entropy=0.0, opacity=0.0, surface=0.0, normal_render_depth=0.0,
                       normal_mvs_depth=0.0, normal_smooth=0.0, point_entropy=0.0, orientation=0.0, depth_var=0.0, scaling=0.0,
                       dssim=0.2, pbr=1.0, light=0.0, base_color=0.0, base_color_smooth=0.0, roughness_smooth=0.0,
                       light_smooth=0.0, visibility_smooth=0.0, visibility=0.0, env_smooth=0.0)
# --lambda_<flag> -> key of train_step.STAGE1_WEIGHTS / STAGE2_WEIGHTS
STAGE1_LAMBDAS = dict(mask_entropy="mask_entropy", normal_render_depth="normal_render_depth", normal_smooth="normal_smooth",
                      depth_var="depth_var", depth_smooth="depth_smooth", point_entropy="point_entropy",
                      orientation="orientation", scaling="scaling")
STAGE2_LAMBDAS = dict(pbr="pbr", normal_render_depth="normal", light="light", env_smooth="env_smooth",
                      base_color_smooth="base_color_smooth", roughness_smooth="roughness_smooth", light_smooth="light_smooth")
assert set(STAGE1_LAMBDAS.values()) <= set(STAGE1_WEIGHTS) and set(STAGE2_LAMBDAS.values()) <= set(STAGE2_WEIGHTS)
_NOT_SCHEDULE = ("iterations", "lambda_orientation_from_iter")


def loss_weights_of(args):
    """The `loss_weights` of the fused step of `args.type` from the --lambda_* flags; RuntimeError naming the flag for a non-zero
    lambda the step does not implement (under `render` the stage-2 default lambda_pbr = 1 is the one that is passed over)."""
    table = STAGE1_LAMBDAS if args.type == "render" else STAGE2_LAMBDAS
    if float(args.lambda_dssim) != 0.2:
        raise RuntimeError("--lambda_dssim %g: the fused steps have the reference's 0.2 built in" % args.lambda_dssim)
    weights = {}
    for flag in LAMBDA_DEFAULTS:
        value = float(getattr(args, "lambda_" + flag))
        if flag == "dssim" or (flag == "pbr" and args.type == "render"):
            continue
        if flag in table:
            weights[table[flag]] = value
        elif value != 0.0:
            why = "the driver reads no MVS maps" if flag in ("depth", "normal_mvs_depth") else \
                "the fused %s step does not implement it" % ("stage-1" if args.type == "render" else "stage-2")
            raise RuntimeError("--lambda_%s %g is not supported with -t %s: %s" % (flag, value, args.type, why))
    if args.type == "render":
        weights["orientation_from_iter"] = int(args.lambda_orientation_from_iter)
    return weights


def build_parser():
    p = argparse.ArgumentParser(prog="python -m relightable3dgaussian_amd.training",
                                description="Train Relightable 3D Gaussians from a Blender-, Synthetic4Relight- or NeILF-format dataset on the fused "
                                            "iterations")
    p.add_argument("-s", "--source_path", required=True,
                   help="dataset root: Blender format (transforms_train.json, transforms_test.json) or NeILF format "
                        "(inputs/sfm_scene.json)")
    p.add_argument("-r", "--resolution", type=int, default=-1,
                   help="1, 2, 4, 8: downscale by that factor; -1: rescale files wider than 1600 pixels to 1600; else the target width")
    p.add_argument("-m", "--model_path", required=True, help="output directory")
    p.add_argument("-t", "--type", choices=["render", "neilf"], default="render")
    p.add_argument("-c", "--checkpoint", default=None, help="chkpnt<it>.pth to start from (required for -t neilf)")
    p.add_argument("--eval", action="store_true")
    p.add_argument("-w", "--white_background", action="store_true")
    p.add_argument("--iterations", type=int, default=30_000)
    p.add_argument("--sample_num", type=int, default=64)
    p.add_argument("--env_resolution", type=int, default=16)
    p.add_argument("--save_interval", type=int, default=5000)
    p.add_argument("--checkpoint_interval", type=int, default=5000)
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--log_interval", type=int, default=100, help="0: no progress lines")
    p.add_argument("--visibility_interval", type=int, default=0, help="re-trace the visibility every N stage-2 iterations")
    p.add_argument("--save_training_vis", action="store_true",
                   help="write the contact sheet OUT/visualize/<iteration>.png of the iteration's view (training_vis)")
    p.add_argument("--save_training_vis_iteration", type=int, default=1000, help="... every N iterations, and at the first")
    p.add_argument("--device_png", action="store_true",
                   help="encode the contact sheets on the device (png_device) instead of on a PIL worker thread")
    p.add_argument("--device", default="cuda")
    for name, value in sorted(vars(train_loop.Schedule()).items()):              # learning rates, light_init, densification
        if name not in _NOT_SCHEDULE and not name.startswith("lambda_"):
            p.add_argument("--" + name, type=type(value), default=value)
    for flag, value in LAMBDA_DEFAULTS.items():
        p.add_argument("--lambda_" + flag, type=float, default=value)
    p.add_argument("--lambda_orientation_from_iter", type=int, default=5000)
    return p


def schedule_of(args):
    fields = {k: getattr(args, k) for k in vars(train_loop.Schedule()) if k not in _NOT_SCHEDULE and not k.startswith("lambda_")}
    return train_loop.Schedule(iterations=args.iterations, **fields)         # (the lambdas travel as loss_weights)


def env_checkpoint(env, exp_avg, exp_avg_sq, steps, lr, iteration):
    """The object train.py:197 saves for the environment light: `(DirectLightMap.capture(), iteration)` = `([env Parameter
    [1,R,2R,3], state_dict of Adam([{"params": [env], "lr": env_lr, "name": "env"}], lr=0.0, eps=1e-15)], iteration)`
    (scene/direct_light_map.py:18-35).  `exp_avg` / `exp_avg_sq`: the texture's Adam moments, `steps` the optimizer's step count
    (0: no state yet).  Plain PyTorch on whatever device the tensors live on."""
    param = torch.nn.Parameter(env.detach().clone().contiguous().requires_grad_(True))
    optimizer = torch.optim.Adam([{"params": [param], "lr": float(lr), "name": "env"}], lr=0.0, eps=1e-15)
    if steps > 0:
        optimizer.state[param] = {"step": torch.tensor(float(steps)), "exp_avg": exp_avg.detach().clone().reshape(param.shape),
                                  "exp_avg_sq": exp_avg_sq.detach().clone().reshape(param.shape)}
    return [param, optimizer.state_dict()], int(iteration)


def read_env_checkpoint(path, resolution=None):
    """The texture [1,R,2R,3] of an env_light_chkpnt file (DirectLightMap.create_from_ckpt)."""
    (captured, _iteration) = torch.load(path, map_location="cpu", weights_only=True)
    env = captured[0].detach().float()
    if env.dim() != 4 or env.shape[0] != 1 or env.shape[3] != 3 or (resolution and env.shape[1] != resolution):
        raise RuntimeError("%s: not an environment texture [1,R,2R,3]%s: %s" % (
            path, " of --env_resolution %d" % resolution if resolution else "", tuple(env.shape)))
    return env.contiguous()


class _Stage1Model:
    """A FusedStage1Step's parameters behind the getters bench_core.render_stage1 calls (activations of gaussian_model.py:183-232)."""

    def __init__(self, step):
        self.step, self.xyz = step, step.xyz.detach()

    def get_normal(self):
        return torch.nn.functional.normalize(self.step.normal.detach(), dim=-1, eps=1e-3)

    def get_opacity(self):
        return torch.sigmoid(self.step.opacity.detach())

    def get_scaling(self):
        return torch.exp(self.step.scaling.detach())

    def get_rotation(self):
        return torch.nn.functional.normalize(self.step.rotation.detach())

    def get_shs(self):
        return self.step.shs.detach()


def _split(args, records, device, background):
    """records -> (records, view store at --resolution, cameras with the intrinsics of the resized views).  Records of OpenEXR
    files (the Synthetic4Relight train split) get an hdr_views.HdrViewStore, all others a dataset.ViewStore."""
    if all(r["path"].endswith(".exr") for r in records):
        from . import hdr_views
        kind = hdr_views.HdrViewStore
    else:
        kind = dataset.ViewStore
    store = kind([r["path"] for r in records], device, mask_paths=[r.get("mask_path") for r in records],
                 resolution=args.resolution, background=background)
    return records, store, dataset.cameras_of(records, store.sizes, device, store.scales)


def read_scene(args):
    """(layout, train records, test records or None, initial points callable) of --source_path, the layout picked as
    scene/__init__.py:43-61 picks it: transforms_train.json -> Blender (Synthetic4Relight under a path of that name),
    inputs/sfm_scene.json -> NeILF, else a RuntimeError."""
    root = args.source_path
    layout = dataset.detect_layout(root)
    if layout in ("blender", "syn4relight"):
        read = dataset.read_transforms if layout == "blender" else dataset.read_syn4relight
        train = read(root, "train")
        test = read(root, "test") if args.eval else None
        return layout, train, test, lambda: dataset.initial_points(root, args.seed)
    train, test = dataset.read_neilf_scene(root, args.eval)
    return layout, train, (test if args.eval else None), lambda: dataset.initial_points_neilf(root, args.seed)


@torch.no_grad()
def evaluate_step(step, args, cameras, store, background):
    """{"render": {"psnr", "ssim"} [, "pbr": ...]} of a trained step on a held-out split: `render` through evaluate.evaluate_nvs;
    for a stage-2 step also `pbr` from a RelightRenderer on the learned texture softplus(env), with the view's mask."""
    step.flush()
    gts = store.images(background)
    if args.type == "render":
        from .bench_core import render_stage1
        model = _Stage1Model(step)
        return {"render": evaluate.evaluate_nvs(lambda cam, bg: render_stage1(model, cam, bg)[2], cameras, gts, background)}
    from . import relight
    envmap = torch.nn.functional.softplus(step.env.detach())[0].contiguous()
    renderer = relight.RelightRenderer(step, envmap, args.sample_num)
    out = {"render": evaluate.evaluate_nvs(renderer, cameras, gts, background)}
    ev = evaluate.Evaluator(len(cameras), step.dev)
    for v, cam in enumerate(cameras):
        pbr = renderer.frame(cam, background, outputs=("pbr",))["pbr"]
        gt, mask = store.fetch(v, background)
        if store.has_masks:
            ev.add("pbr", pbr, gt, mask, background)
        else:
            ev.add("pbr", pbr, gt)
    out["pbr"] = ev.result()["pbr"]
    return out


def train(args):
    """Run the command described by `args` (build_parser().parse_args(...)).  -> namespace: step, history, views (the view of
    every iteration), files (what was written), metrics (None without --eval), first_iteration, env_init (stage 2), store, cameras,
    test_cameras (None without --eval)."""
    weights = loss_weights_of(args)                                   # (raises before anything is loaded)
    stage2 = args.type == "neilf"
    if stage2 and not args.checkpoint:
        raise RuntimeError("-t neilf starts from a stage-1 checkpoint: pass -c .../chkpnt<it>.pth (train.py:35-37)")
    device = torch.device(args.device)
    if device.type != "cuda":
        raise RuntimeError("training runs on the device (there is no CPU path)")
    sch = schedule_of(args)
    value = 1.0 if args.white_background else 0.0
    background = torch.full((3,), value, dtype=torch.float32, device=device)
    _layout, train_records, test_records, initial_points = read_scene(args)
    records, store, cameras = _split(args, train_records, device, background)
    test = _split(args, test_records, device, background) if args.eval else None
    extent, _ = synthetic.cameras_extent(cameras)
    masks = store.masks(background)
    seen, files = [], []
    pick = dataset.reference_view_order(len(cameras), args.seed)

    def view_order(it):
        seen.append(pick(it))
        return seen[-1]

    os.makedirs(args.model_path, exist_ok=True)
    result = types.SimpleNamespace(views=seen, files=files, metrics=None, env_init=None, store=store, extent=extent, cameras=cameras,
                                   test_cameras=test[2] if test else None)
    first = 0
    vis = types.SimpleNamespace(sheet=None)                           # the training_vis.TrainingSheet, made at the first sheet
    if args.save_training_vis:
        if args.save_training_vis_iteration < 1:
            raise RuntimeError("--save_training_vis_iteration %d: an interval of at least 1" % args.save_training_vis_iteration)
        os.makedirs(os.path.join(args.model_path, "visualize"), exist_ok=True)

    def save_sheet(it, g, step):
        # train.py:279: every N iterations and at the run's first; the view of THIS iteration, its pair out of the store's ring
        # while the ring still holds it (no second unpack launch)
        if not (g % args.save_training_vis_iteration == 0 or it == 1):
            return
        if vis.sheet is None:
            from . import training_vis
            vis.sheet = training_vis.TrainingSheet(step, args.sample_num if stage2 else None)
            if args.device_png:
                vis.sheet.device_png = True
        v = seen[-1]
        path = os.path.join(args.model_path, "visualize", "%06d.png" % g)
        vis.sheet.save(cameras[v], store._pair(v, background, fresh=False)[0], background, path)
        files.append(path)

    def close_sheets():
        if vis.sheet is not None:
            vis.sheet.close()                                         # (waits for the files; raises what an encoder raised)

    def on_iteration(it, step):
        g = first + it
        if args.save_training_vis:
            save_sheet(it, g, step)
        if args.log_interval and it % args.log_interval == 0:
            if getattr(step, "last_outs", None) is None:
                # (a densification replaced the step's buffers, the loss sums among them, after this iteration's backward)
                print("[ITER %d] densified: points %d" % (g, step.P), flush=True)
            else:
                print("[ITER %d] loss %.6f  points %d" % (g, float(step.loss()), step.P), flush=True)
        last = g == args.iterations
        save, keep = last or g % args.save_interval == 0, last or g % args.checkpoint_interval == 0
        if save or keep:
            step.flush()
        if save:
            path = os.path.join(args.model_path, "point_cloud", "iteration_%d" % g, "point_cloud.ply")
            ply.save(path, step)
            files.append(path)
        if keep:
            path = os.path.join(args.model_path, "chkpnt%d.pth" % g)
            torch.save(checkpoint.capture(step, g, spatial_lr_scale=extent), path)
            files.append(path)
            if stage2:
                group = step.opt.groups[step._opt_order.index("env")]
                path = os.path.join(args.model_path, "env_light_chkpnt%d.pth" % g)
                torch.save(env_checkpoint(step.env, group["exp_avg"], group["exp_avg_sq"], step.opt.step_count, group["lr"], g),
                           path)
                files.append(path)

    if not stage2:
        points, colors, normals = initial_points()
        init = train_loop.create_from_points(torch.from_numpy(points.copy()), torch.from_numpy(colors.copy()),
                                             torch.from_numpy(normals.copy()), device=device)
        step, history = train_loop.train_stage1(init, cameras, store.images(background), background, extent, schedule=sch,
                                                iterations=args.iterations, seed=args.seed,
                                                white_background=args.white_background, on_iteration=on_iteration, masks=masks,
                                                loss_weights=weights, view_order=view_order)
    else:
        restored = checkpoint.restore(args.checkpoint, device=device, pbr=True)
        first = restored.iteration
        if args.iterations <= first:
            raise RuntimeError("--iterations %d: the checkpoint already stands at iteration %d" % (args.iterations, first))
        beside = os.path.join(os.path.dirname(args.checkpoint), "env_light_" + os.path.basename(args.checkpoint))
        if os.path.exists(beside):
            env = read_env_checkpoint(beside, args.env_resolution)
        else:
            R = args.env_resolution                                    # DirectLightMap.__init__, scene/direct_light_map.py:14
            env = args.light_init * torch.rand(1, R, 2 * R, 3, generator=torch.Generator().manual_seed(args.seed))
        restored.env = env.to(device).contiguous()
        result.env_init = env.clone()
        step, history = train_loop.train_stage2(restored, cameras, store.images(background), background, extent,
                                                args.sample_num, schedule=sch, iterations=args.iterations - first,
                                                visibility_interval=args.visibility_interval, masks=masks, loss_weights=weights,
                                                on_iteration=on_iteration, view_order=view_order, first_iteration=first)
    result.step, result.history, result.first_iteration = step, history, first
    close_sheets()                                                    # (before --eval, and before train() returns)
    if args.eval:
        _, test_store, test_cameras = test
        metrics = evaluate_step(step, args, test_cameras, test_store, background)
        metrics.update(iteration=args.iterations, views=len(test_cameras))
        path = os.path.join(args.model_path, "metrics.json")
        with open(path, "w") as fh:
            json.dump(metrics, fh, indent=1)
        files.append(path)
        result.metrics = metrics
        print("[EVAL] " + "  ".join("%s PSNR %.3f SSIM %.4f" % (k, m["psnr"], m["ssim"]) for k, m in metrics.items()
                                    if isinstance(m, dict)), flush=True)
    return result


def main(argv=None):
    train(build_parser().parse_args(argv))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
