"""The training contact sheet on the GPU (relightable3dgaussian_amd/training_vis.py, training.py --save_training_vis,
csrc/training_sheet.hip): r3dg_training_sheet on synthetic raw maps, TrainingSheet on small live steps of both stages, and the
driver end to end -- every byte of every sheet under the acceptance rule of tests/training_vis_reference.py (`accept`), which
tests/test_training_vis_cpu.py shows the reference's own float32 output to pass.

THE RULE.  A byte b passes when quantise(v - tol) <= b <= quantise(v + tol), v the float64 restatement: tol = 0 for render, gt,
opacity and padding (exact); 1e-6 |v| + 1e-7 for the linear panels and 4e-4 behind the sRGB curve (the project's figures for
r3dg_relight_capture, tests/test_evaluate_gpu.py:17-18); on the depth panel b must be the quantised `turbo` entry of a bin in
[bin(t - TOL_T), bin(t + TOL_T)].  TOL_T is derived, not measured (tests/training_vis_reference.py holds the derivation beside the
constant): the float32 roundings of the quotient feature / opacity and of the sum depth + eps (2^-24 each, carried through the
logarithm as absolute errors), logf's documented 1 ulp and the rounding of the difference c - c_far at magnitudes below 32
(2^-19, 2^-20), all divided by |c_far - c_near| = 4.174, plus the division's own half ulp of a t in [0, 1] (2^-24): 7.7e-7.
No share of the bytes is left out.

Kernel shapes (H x W): 13 x 11 (the grid is scaled UP to 800 rows: 25 sheet rows per grid row), 401 x 5 and 201 x 7 (grids of 808
and 814 rows: the downsampling path, some grid rows are skipped), 37 x 50 with a 16 x 32 texture, and a 7 x 5 sheet of a 13 x 11
frame whose 105 bytes end in a lane with one byte (the 800-row sheets are whole words).  Every input pointer is 4 bytes off the
allocation's alignment; the sheet has canaries on both sides."""
import os

import numpy as np
import pytest
import torch

from tests import training_vis_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
# (layout, H, W, texture rows, background, sheet size or None = sheet_size)
CASES = [(0, 13, 11, 0, 0.0, None), (0, 401, 5, 0, 1.0, None), (1, 13, 11, 4, 1.0, None), (1, 37, 50, 16, 0.0, None),
         (1, 201, 7, 4, 0.0, None), (0, 13, 11, 0, 1.0, (7, 5)), (1, 13, 11, 4, 0.0, (9, 11))]
_TABLE = []


def _table():
    if not _TABLE:
        _TABLE.append(R.turbo_table())
    return _TABLE[0]


def _off_grid(a):
    """The array on the device, 4 bytes past the start of its allocation."""
    flat = torch.empty(a.size + 1, dtype=torch.from_numpy(a).dtype, device=DEV)
    flat[1:] = torch.from_numpy(np.ascontiguousarray(a)).reshape(-1).to(DEV)
    return flat[1:].reshape(a.shape)


def _check(sheet, ref):
    ok, lines = R.accept(sheet, ref, _table())
    print("\n".join(lines))
    assert ok.all(), "\n".join(lines)


@pytest.mark.parametrize("layout,H,W,rows,bg,size", CASES)
def test_the_kernel_writes_the_reference_sheet(layout, H, W, rows, bg, size):
    from relightable3dgaussian_amd import training_vis
    m = R.synthetic_maps(layout, H, W, R=max(rows, 1), seed=1, background=bg)
    out_h, out_w = size or training_vis.sheet_size(R.PANELS[layout], H, W)[:2]
    assert size is not None or (out_h, out_w) == R.sheet_size(R.PANELS[layout], H, W)[:2]
    d = {k: _off_grid(v) for k, v in m.items()}
    assert all(t.data_ptr() % 16 == 4 for t in d.values())
    n = out_h * out_w * 3
    guarded = torch.full((n + 32,), 0xA5, dtype=torch.uint8, device=DEV)
    out = guarded[16:16 + n].reshape(out_h, out_w, 3)
    training_vis.launch_sheet(layout, d["render"], d["gt"], d["opacity"], d["n_contrib"], d["feature"], d["pseudo_normal"],
                              d["background"], d.get("env"), out)
    torch.cuda.synchronize()
    host = guarded.cpu().numpy()
    assert (host[:16] == 0xA5).all() and (host[16 + n:] == 0xA5).all(), "bytes outside the sheet were written"
    ref = R.sheet_reference(layout, m, out_h, out_w, _table())
    assert set(np.unique(ref["panel"]).tolist()) >= set(range(R.PANELS[layout])) or size is not None
    _check(host[16:16 + n].reshape(out_h, out_w, 3), ref)


class _Spy:
    """The library, with the name of every entry point that is looked up for a call."""

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        if name.startswith("r3dg_"):
            self.calls.append(name)
        return getattr(self._lib, name)


def _sheet_of_live_step(monkeypatch, step, stage, cam, gt, bg):
    from relightable3dgaussian_amd import _lib, training_vis
    sheets = training_vis.TrainingSheet(step, 8 if stage == 2 else None)
    spy = _Spy(_lib.lib())
    monkeypatch.setattr(_lib, "lib", lambda: spy)
    got = sheets.sheet(cam, gt, bg)
    monkeypatch.undo()
    torch.cuda.synchronize()
    H, W = cam.image_height, cam.image_width
    assert tuple(got.shape) == training_vis.sheet_size(R.PANELS[stage - 1], H, W)[:2] + (3,) and got.dtype == torch.uint8
    assert spy.calls.count("r3dg_training_sheet") == 1
    assert not [c for c in spy.calls if c.startswith("r3dg_bvh_")], spy.calls        # nothing is traced, no BVH is built or walked
    fr = sheets.frame_outputs
    m = {k: fr[k].detach().cpu().numpy() for k in ("render", "opacity", "n_contrib", "feature", "pseudo_normal")}
    m.update(gt=gt.cpu().numpy(), background=bg.cpu().numpy())
    if stage == 2:
        m["env"] = fr["env"].cpu().numpy()
        assert fr["feature"].shape[0] == 28 and "r3dg_shade_forward_cached" in spy.calls
        assert torch.equal(fr["env"], torch.nn.functional.softplus(step.env.detach())[0])
    assert (m["n_contrib"] > 0).any() and (m["n_contrib"] == 0).any()               # an object in front of a background
    _check(got.cpu().numpy(), R.sheet_reference(stage - 1, m, got.shape[0], got.shape[1], _table()))
    again = sheets.sheet(cam, gt, bg)
    assert again.data_ptr() == got.data_ptr()                                       # the buffer of that size, allocated once
    return sheets, spy


def _small_scene(stage2):
    from relightable3dgaussian_amd import synthetic as syn
    from relightable3dgaussian_amd.bench_core import GaussianParams, render_stage1
    dev = torch.device("cuda", 0)
    cams = [c.to(dev) for c in syn.orbit_cameras(3, width=40, height=30)]
    bg = torch.ones(3, device=dev)
    params = GaussianParams(syn.make_scene(P=3000, seed=1, stage2=stage2, scale_log_mean=-3.0), dev, stage2)
    with torch.no_grad():
        gts = [(render_stage1(params, c, bg)[2] * 0.9).clamp(0, 1).clone() for c in cams]
    return params, cams, gts, bg


def test_sheet_of_a_live_stage1_step(monkeypatch):
    from relightable3dgaussian_amd.fused_stage1 import FusedStage1Step
    params, cams, gts, bg = _small_scene(False)
    step = FusedStage1Step(params, lr=1e-3)
    for c, gt in zip(cams, gts):
        step(c, bg, gt)
    _sheet_of_live_step(monkeypatch, step, 1, cams[1], gts[1], bg)


@pytest.mark.parametrize("device_visibility", [False, True])
def test_sheet_of_a_live_stage2_step(monkeypatch, device_visibility):
    """On the step's own tensors and its own traced visibility: with resident direction caches, and on the device path where the
    step holds no direction tensor (the sheet regenerates one from the step's snapshot normals and never hands it to the step).
    The sheet leaves every parameter, the visibility and the kind of the sample set as they were, and training goes on."""
    from relightable3dgaussian_amd.fused_step import FusedStage2Step
    params, cams, gts, bg = _small_scene(True)
    step = FusedStage2Step(params, 8, lr=1e-3, device_visibility=device_visibility)
    for c, gt in zip(cams, gts):
        step(c, bg, gt)
    step.flush()
    names = ("xyz", "normal", "scaling", "rotation", "opacity", "shs", "base_color", "roughness", "env", "incidents")
    before = {k: (getattr(step, k), getattr(step, k).data_ptr(), getattr(step, k).detach().clone()) for k in names}
    holds_dirs = step._samples.incident_dirs is not None
    assert holds_dirs == (not device_visibility)
    visibility, seen = step._samples.visibility, step._samples.visibility.clone()
    _sheet_of_live_step(monkeypatch, step, 2, cams[1], gts[1], bg)
    assert (step._samples.incident_dirs is not None) == holds_dirs
    assert step._samples.visibility is visibility and torch.equal(visibility, seen)
    for k, (tensor, address, values) in before.items():             # the same tensors (none cloned, none replaced), the same values
        assert getattr(step, k) is tensor and tensor.data_ptr() == address and torch.equal(tensor, values), k
    step(cams[2], bg, gts[2])
    assert np.isfinite(float(step.loss()))


def test_a_sheet_at_another_sample_count_is_refused():
    from relightable3dgaussian_amd import training_vis
    from relightable3dgaussian_amd.fused_step import FusedStage2Step
    params, _, _, _ = _small_scene(True)
    with pytest.raises(RuntimeError, match="another ray set"):
        training_vis.TrainingSheet(FusedStage2Step(params, 8, lr=1e-3), 16)


def test_driver_writes_the_sheets_of_both_stages(tmp_path):
    """--iterations 3 --save_training_vis --save_training_vis_iteration 2 writes exactly 000001.png and 000002.png at the size
    sheet_size gives; stage 2 from that run's checkpoint counts on from it (000004, 000006); without the flag no visualize/."""
    from PIL import Image
    from relightable3dgaussian_amd import dataset, training, training_vis
    from tests.test_dataset_cpu import write_split
    from tests.test_dataset_gpu import _teacher_views
    cams, arrays = _teacher_views(4, 48)
    root = str(tmp_path / "data")
    os.makedirs(root)
    c2w = []
    for cam in cams:                                                # camera-to-world in the OpenGL/Blender axes
        mat = torch.linalg.inv(cam.world_view_transform.double().t())
        mat[:3, 1:3] *= -1
        c2w.append(mat.numpy())
    write_split(root, "train", np.stack(arrays), np.stack(c2w), cams[0].FoVx)
    rng = np.random.RandomState(2)
    dataset.write_points_ply(os.path.join(root, "points3d.ply"), rng.random_sample((3000, 3)) * 2.6 - 1.3,
                             rng.random_sample((3000, 3)) * 255, np.zeros((3000, 3)))
    parse = training.build_parser().parse_args
    base = ["-s", root, "-t", "render", "-w", "--iterations", "3", "--log_interval", "0", "--seed", "3"]
    plain = str(tmp_path / "plain")
    r0 = training.train(parse(base + ["-m", plain]))
    assert not os.path.exists(os.path.join(plain, "visualize")) and not any("visualize" in f for f in r0.files)
    out = str(tmp_path / "out")
    r1 = training.train(parse(base + ["-m", out, "--save_training_vis", "--save_training_vis_iteration", "2"]))
    assert sorted(os.listdir(os.path.join(out, "visualize"))) == ["000001.png", "000002.png"]
    assert [os.path.basename(f) for f in r1.files if "visualize" in f] == ["000001.png", "000002.png"]
    out_h, out_w = training_vis.sheet_size(7, 48, 48)[:2]
    for name in ("000001.png", "000002.png"):
        with Image.open(os.path.join(out, "visualize", name)) as im:
            assert im.size == (out_w, out_h) and im.mode == "RGB"
            px = np.asarray(im)
        assert px[:, :, :].any() and not px[0].any()               # panels, under the grid's top border
    assert r1.views == r0.views and r1.step.P == r0.step.P         # (the same run beside the sheets)
    out2 = str(tmp_path / "neilf")
    r2 = training.train(parse(["-s", root, "-t", "neilf", "-c", os.path.join(out, "chkpnt3.pth"), "-w", "--iterations", "6",
                               "--sample_num", "8", "--log_interval", "0", "--seed", "3", "-m", out2, "--save_training_vis",
                               "--save_training_vis_iteration", "2"]))
    assert r2.first_iteration == 3 and sorted(os.listdir(os.path.join(out2, "visualize"))) == ["000004.png", "000006.png"]
    with Image.open(os.path.join(out2, "visualize", "000006.png")) as im:
        assert im.size == tuple(reversed(training_vis.sheet_size(16, 48, 48)[:2]))
