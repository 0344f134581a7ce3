"""Scores of held-out views, on the device: what the reference's eval_nvs.py:49-82 and eval_relighting_syn4.py:140-224 print --
PSNR (utils/image_utils.py:24-29) and SSIM (utils/loss_utils.py:39-63) of a rendered map against its ground truth, both
composited onto a background or onto the environment through the view's mask, and the per-channel albedo scale (:201).

    ev = Evaluator(n_slots, device)          # owns a [n_slots, R3DG_EVAL_ROW] float64 table on the device + scratch
    ev.add("pbr", pred, gt, mask, fill)      # r3dg_eval_image_metrics: queued on the current stream, no synchronisation
    ev.add_albedo_scale(albedo, gt_albedo, mask)     # r3dg_eval_median_ratio: likewise
    ev.result()                              # the ONLY host read: {"pbr": {"psnr", "ssim"}, ..., "albedo_scale": [n,3]}

`evaluate_nvs` and `evaluate_relighting` are the two loops over views; `reference_metrics`, `reference_albedo_scale` and
`capture_reference` are the same arithmetic in plain PyTorch ops -- the yardstick of the tests, as relight.frame_reference is
for RelightRenderer.frame.  LPIPS, the third number of the reference's scripts, is NOT computed: its network weights are a
blob this repository does not have, and SURVEY.md section 2 leaves it out of scope.
"""
import torch

from . import _abi, _lib
from .train_step import rgb_to_srgb, ssim as _ssim

ROW = _abi.constants["R3DG_EVAL_ROW"]
_STATE_WORDS = _abi.constants["R3DG_EVAL_MEDIAN_STATE_WORDS"]


def _image(t, dev):
    return t.detach().to(dev, torch.float32).contiguous()


class Evaluator:
    """`n_slots`: views x quantities that can be queued before `result()` (one table row each)."""

    def __init__(self, n_slots, device="cuda"):
        self.dev = torch.device(device)
        if self.dev.type != "cuda":
            raise RuntimeError("Evaluator needs a device (there is no CPU path; reference_metrics is the PyTorch restatement)")
        self.table = torch.zeros(int(n_slots), ROW, dtype=torch.float64, device=self.dev)
        self._state = torch.zeros(_STATE_WORDS, dtype=torch.int32, device=self.dev)
        self._tile_sums = None
        self._rows = []                              # (name or None for an albedo scale, row)

    def _next_row(self, name):
        if len(self._rows) >= self.table.shape[0]:
            raise RuntimeError("Evaluator: all %d slots are taken" % self.table.shape[0])
        self._rows.append(name)
        return self.table[len(self._rows) - 1]

    def add(self, name, pred, gt, mask=None, fill=None):
        """Queue PSNR / SSIM of `pred` against `gt` [C,H,W] (C <= 3) under `name`.  With `mask` [H,W] or [1,H,W] both images are
        composited as x * mask + fill * (1 - mask) inside the kernel's load stage; `fill`: a colour [C], an image [C,H,W], or
        None (0)."""
        dev = self.dev
        pred, gt = _image(pred, dev), _image(gt, dev)
        if pred.dim() != 3 or pred.shape != gt.shape:
            raise RuntimeError("Evaluator.add: pred and gt must both be [C,H,W]")
        C, H, W = pred.shape
        if mask is not None:
            mask = _image(mask, dev)
            if mask.numel() != H * W:
                raise RuntimeError("Evaluator.add: mask must be [H,W]")
        fill_is_image = 0
        if fill is not None:
            if mask is None:
                raise RuntimeError("Evaluator.add: a fill needs a mask")
            fill = _image(torch.as_tensor(fill), dev)
            if fill.numel() == C * H * W and fill.dim() == 3:
                fill_is_image = 1
            elif fill.numel() != C:
                raise RuntimeError("Evaluator.add: fill must be [C] or [C,H,W]")
        need = 2 * C * ((W + 31) // 32) * ((H + 31) // 32)
        if self._tile_sums is None or self._tile_sums.numel() < need:
            # (kernels queued earlier on this stream are done with the old buffer before anything reuses its memory)
            self._tile_sums = torch.empty(need, dtype=torch.float64, device=dev)
        row = self._next_row(str(name))
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().r3dg_eval_image_metrics(
                _lib.current_stream(), W, H, C, pred.data_ptr(), gt.data_ptr(), _lib.ptr(mask), _lib.ptr(fill), fill_is_image,
                self._tile_sums.data_ptr(), row.data_ptr()), "eval_image_metrics")

    def add_albedo_scale(self, pred_albedo, gt_albedo, mask=None):
        """Queue the masked per-channel lower median of gt_albedo / clamp(pred_albedo, 1e-6, 1) (both [3,H,W], mask > 0 selects)."""
        dev = self.dev
        pred, gt = _image(pred_albedo, dev), _image(gt_albedo, dev)
        if pred.dim() != 3 or pred.shape[0] != 3 or pred.shape != gt.shape:
            raise RuntimeError("Evaluator.add_albedo_scale: both images must be [3,H,W]")
        _, H, W = pred.shape
        if mask is not None:
            mask = _image(mask, dev)
            if mask.numel() != H * W:
                raise RuntimeError("Evaluator.add_albedo_scale: mask must be [H,W]")
        row = self._next_row(None)
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().r3dg_eval_median_ratio(
                _lib.current_stream(), W, H, _lib.ptr(pred), _lib.ptr(gt), None if mask is None else mask.data_ptr(),
                self._state.data_ptr(), row.data_ptr()), "eval_median_ratio")

    def result(self):
        """The one host read.  {name: {"psnr", "ssim"}}: float64 means over that name's views (the reference's `.double()`
        sums divided by the view count), and "albedo_scale" [n_views,3] (float32) when scales were queued.  Raises if a queued
        albedo scale saw an empty mask (the reference's median of nothing fails there too)."""
        n = len(self._rows)
        t = self.table[:n].cpu()
        out, scales = {}, []
        for i, name in enumerate(self._rows):
            if name is None:
                if float(t[i, 3]) == 0.0:
                    raise RuntimeError("Evaluator: the albedo scale of queued view %d has an empty mask" % len(scales))
                scales.append(t[i, :3])
            else:
                out.setdefault(name, []).append(t[i, 4:6])
        res = {}
        for name, rows in out.items():
            m = torch.stack(rows).sum(0) / len(rows)
            res[name] = {"psnr": float(m[0]), "ssim": float(m[1])}
        if scales:
            res["albedo_scale"] = torch.stack(scales).to(torch.float32)
        return res


def _render_of(render_fn_or_renderer, cam, bg):
    if hasattr(render_fn_or_renderer, "frame"):          # a RelightRenderer
        return render_fn_or_renderer.frame(cam, bg, outputs=())["render"]
    out = render_fn_or_renderer(cam, bg)
    return out["render"] if isinstance(out, dict) else out


@torch.no_grad()
def evaluate_nvs(render_fn_or_renderer, cameras, gts, bg):
    """eval_nvs.py:49-82 without LPIPS: mean PSNR and SSIM of the rendered image against each view's ground truth.
    `render_fn_or_renderer` is ONE of two things, nothing else is recognised: a callable (cam, bg) -> image [3,H,W] or dict with
    "render", or an object with RelightRenderer's `frame`.  A training step object (FusedStage2Step, FusedStage1Step) is neither:
    it holds the raw parameters a RelightRenderer is built from, or wrap its rasterizer call in a callable.
    -> {"psnr", "ssim"}."""
    ev = Evaluator(len(cameras), gts[0].device if gts[0].is_cuda else "cuda")
    for cam, gt in zip(cameras, gts):
        ev.add("render", _render_of(render_fn_or_renderer, cam, bg), gt[0:3])
    return ev.result()["render"]


@torch.no_grad()
def evaluate_relighting(renderer, cameras, gt_images, gt_albedos, masks, bg, env_transforms=None):
    """eval_relighting_syn4.py:140-224 without LPIPS, per view one RelightRenderer.frame and four queued device jobs:
      "pbr"         results["pbr"] against the ground truth, both masked onto `bg`                                  (:167,172,190-191)
      "base_color"  results["base_color"] against the ground-truth albedo, both masked onto `bg`                    (:165,177,194-195)
      "pbr_env"     the same pbr against the ground truth, both filled with the frame's env_only instead            (:169,186)
                    -- a score of THIS project: the script only saves these two images, it prints no number for them
      "albedo_scale" per view the masked median of gt_albedo / clamp(base_color, 1e-6, 1)                          (:201; the script
                    prints it for the first view only)
    The composites happen inside the metric kernel, each from the UNcomposited map.  (Where a mask is strictly between 0 and 1
    AND bg is not black the script's two pbr_env images carry bg * mask * (1 - mask) on top: its gt_pbr_env composites the ground
    truth it has already put onto bg, and its pbr_env takes render_pkg["pbr"], which an earlier "pbr" entry of the capture list
    has already put onto bg as well; and its median divides the composited images -- on a mask of zeros and ones all of these
    are what is computed here.)
    -> Evaluator.result()."""
    dev = renderer.dev
    bg = torch.as_tensor(bg, dtype=torch.float32).to(dev).reshape(3)
    ev = Evaluator(4 * len(cameras), dev)
    for i, cam in enumerate(cameras):
        tr = None if env_transforms is None else env_transforms[i]
        res = renderer.frame(cam, bg, env_transform=tr, outputs=("pbr", "base_color", "env_only"))
        ev.add("pbr", res["pbr"], gt_images[i], masks[i], bg)
        ev.add("base_color", res["base_color"], gt_albedos[i], masks[i], bg)
        ev.add("pbr_env", res["pbr"], gt_images[i], masks[i], res["env_only"])
        ev.add_albedo_scale(res["base_color"], gt_albedos[i], masks[i])
    return ev.result()


# ---- the same arithmetic in plain PyTorch ops (CPU tests; yardstick of the GPU tests) ---------------------------------------
def composite(x, mask, fill=None):
    """x * mask + fill * (1 - mask) (eval_relighting_syn4.py:161-186); fill: None (0), a colour [C] or an image [C,H,W]."""
    if mask is None:
        return x
    mask = mask.reshape(1, x.shape[-2], x.shape[-1])
    if fill is None:
        fill = torch.zeros(x.shape[0], dtype=x.dtype, device=x.device)
    fill = torch.as_tensor(fill, dtype=x.dtype).to(x.device)
    if fill.dim() == 1:
        fill = fill[:, None, None]
    return x * mask + fill * (1 - mask)


def reference_metrics(pred, gt, mask=None, fill=None):
    """-> {"psnr", "ssim", "mse"} (float64 tensors) of the composited pair: the composites and the SSIM in float32 exactly as the
    reference forms them, the mean squared error of the float32 images in float64 (psnr = mean_c 20 log10(1 / sqrt(mse_c)))."""
    x, y = composite(pred.float(), mask, fill), composite(gt.float(), mask, fill)
    mse = ((x.double() - y.double()) ** 2).reshape(x.shape[0], -1).mean(1)
    psnr = (20 * torch.log10(1.0 / torch.sqrt(mse))).mean()
    return {"psnr": psnr, "ssim": _ssim(x, y).double(), "mse": mse}


def reference_albedo_scale(pred_albedo, gt_albedo, mask=None):
    """(gt / pred.clamp(1e-6, 1))[:, mask > 0].median(dim=1).values (eval_relighting_syn4.py:201)."""
    ratio = gt_albedo / pred_albedo.clamp(1e-6, 1)
    sel = torch.ones_like(ratio[0], dtype=torch.bool) if mask is None else mask.reshape(ratio.shape[1:]) > 0
    return ratio[:, sel].median(dim=1).values


def capture_reference(feature, opacity, num_contrib, bg, mask=None):
    """The capture maps of neilf.py:146-182 from the rasterizer's raw 28-channel feature image, and the mask composite of
    eval_relighting_syn4.py:161-167 on every map but depth_var: what r3dg_relight_capture writes."""
    op = opacity.reshape(1, *feature.shape[1:])
    feat = feature / op.clamp_min(1e-5) * (num_contrib.reshape(op.shape) > 0)
    bg = torch.as_tensor(bg, dtype=feature.dtype).to(feature.device).reshape(3)
    maps = dict(pbr=rgb_to_srgb(feat[2:5] * op + (1 - op) * bg[:, None, None]), normal=feat[5:8],
                base_color=rgb_to_srgb(feat[8:11]), roughness=feat[11:12], diffuse=rgb_to_srgb(feat[12:15]),
                specular=rgb_to_srgb(feat[15:18]), lights=rgb_to_srgb(feat[18:21]), local_lights=rgb_to_srgb(feat[21:24]),
                global_lights=rgb_to_srgb(feat[24:27]), visibility=feat[27:28])
    if mask is not None:
        maps = {k: composite(v, mask, bg if v.shape[0] == 3 else bg[:1]) for k, v in maps.items()}
    maps["depth_var"] = feat[1:2] - feat[0:1].square()
    return maps
