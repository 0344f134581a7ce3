"""What FusedStage2Step launches, call by call, against a recording of the same scenario (tests/golden/fused_samples_call_trace.json,
written by tests/golden/make_fused_samples_call_trace.py from the commit whose hash the file holds): the check that moving the
step's sample-set state (visibility, ray set, lookup cache) into its owner, fused_samples.SampleSet, changed nothing an
iteration launches.

The scenario (P=6, K=8, a 4x4 camera, a 16x32 environment texture; the recording library of tests/helpers.py, the stream, event,
rasterizer and ray-set fakes of test_host_mirrors_cpu.py's three-stream test) runs a step built with device_visibility False and
one built with True through construction, three whole iterations, a texture of another size the fake ray set takes (8x16), one it
refuses (4x8), a swapped direction tensor, refresh_visibility(), one more iteration and the first texture size again.  Recorded:
  * per C-ABI call the entry point, scalars as they are, NULL as None, a stream by its role (main / order / early; "current" for
    the raw current stream) and every other pointer as the NAME of the step attribute (first) or owner attribute whose buffer it
    points into (+ the byte offset inside it), "other" for a buffer that belongs to none, "ref" for a ctypes object;
  * stream contexts entered and left, torch-level joins and events;
  * the fake ray sets' events (taps, rotate, forward, backward, chain), each with the serial number of the ray set, and the
    calls of FixedRaySet(...), FixedRaySet.try_build, build_taps, update_visibility and update_visibility_device (want_dirs)."""
import ctypes
import json
import os
import sys
import types

import pytest
import torch

from tests.helpers import recording_library
from tests.test_relight_call_sequences_cpu import pack, unpack  # noqa: F401  (pack: for the generator of the golden file)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fused_samples_call_trace.json")
P, K, H, W = 6, 8, 4, 4
STEPS = {"traced": False, "device": True}
TAKEN_SIZES = ((16, 32), (8, 16))
# the step's buffers, in the order in which a pointer is looked up among them; then the owner's (a buffer that moved there is
# still found under the step's name, through the step's forwarding property)
STEP_BUFFERS = ("xyz", "normal", "scaling", "rotation", "opacity", "shs", "base_color", "roughness", "_incidents", "env",
                "a_scales", "a_rot", "a_opacity", "a_normal", "a_base", "a_rough", "a_viewdirs", "shade_out", "features", "sums",
                "d_pbr", "d_diffuse", "_absmax", "_flag", "_acc", "_env_c", "_d_env", "_overflow_count",
                "visibility", "incident_dirs", "incident_areas", "_taps", "_ray_normals")
OWNER_BUFFERS = ("visibility", "incident_dirs", "incident_areas", "taps", "ray_normals")


@pytest.fixture(autouse=True)
def _no_side_streams_shared_between_tests():
    from relightable3dgaussian_amd import fused_step
    saved = dict(fused_step._STREAMS)
    fused_step._STREAMS.clear()
    yield
    fused_step._STREAMS.clear()
    fused_step._STREAMS.update(saved)


class _Namer:
    """Turns the arguments of a recorded call into names (module docstring)."""

    def __init__(self):
        self.step, self.view, self.streams = None, {}, {}

    def candidates(self):
        s = self.step
        yield from self.view.items()
        for k, t in getattr(s, "grads", {}).items():
            yield "grads." + k, t
        for k in STEP_BUFFERS:
            yield k, getattr(s, k, None)
        for i, g in enumerate(getattr(getattr(s, "opt", None), "groups", ())):
            for k in ("exp_avg", "exp_avg_sq"):
                yield "opt.%s.%s" % (s._opt_order[i], k), g.get(k)
        owner = getattr(s, "_samples", None)
        for k in OWNER_BUFFERS:
            yield "_samples." + k, getattr(owner, k, None)

    def name_of(self, ptr):
        if ptr is None:
            return None
        if not isinstance(ptr, int):
            return "ref"
        if ptr in self.streams:
            return self.streams[ptr]
        for k, t in self.candidates():
            if isinstance(t, torch.Tensor) and t.numel():
                off = ptr - t.data_ptr()
                if 0 <= off < t.numel() * t.element_size():
                    return k if off == 0 else "%s+%d" % (k, off)
        return "other"

    def tensor(self, t):
        return None if t is None else self.name_of(t.data_ptr())

    def record(self, name, args):
        from relightable3dgaussian_amd import _abi
        types_ = _abi.prototypes[name][1]
        assert len(types_) == len(args), (name, len(types_), len(args))
        out = ["current" if i == 0 and a == 0 and ty is ctypes.c_void_p else self.name_of(a) if ty is ctypes.c_void_p
               else a if isinstance(a, (int, float, str, type(None))) else "ref" for i, (ty, a) in enumerate(zip(types_, args))]
        return [name, out]


def scenario(monkeypatch):
    """-> {step name: [[entry point or event, [argument, ...]] or ["#", stage of the scenario], ...]}"""
    import contextlib
    from relightable3dgaussian_amd import fused_step, rasterizer_ops, shading_ops
    namer = _Namer()
    trace = recording_library(monkeypatch, P, convert=namer.record, returns={"r3dg_bounded_forward_supported": 1}).calls
    log = lambda what, *args: trace.append([what, list(args)])
    z = torch.zeros
    role = lambda s: namer.streams.get(getattr(s, "cuda_stream", s), "other")

    class FakeStream:
        def __init__(self, name=None):
            self.cuda_stream = 1000 + len(namer.streams)
            namer.streams[self.cuda_stream] = name or "side%d" % len(namer.streams)

        def wait_stream(self, other):
            log("torch.wait_stream", role(self), role(other))

        def wait_event(self, ev):
            log("torch.wait_event", role(self))

    class FakeEvent:
        def record(self, stream):
            log("event.record", role(stream))

    @contextlib.contextmanager
    def stream_context(s):
        log("enter", role(s))
        yield
        log("exit", role(s))

    class FakeRaySet:
        n_invalid, made = 2, 0

        def __init__(self, normals=None, sample_num=None, how="FixedRaySet", dirs=None):
            FakeRaySet.made += 1
            self.serial = FakeRaySet.made
            log(how, self.serial, namer.tensor(normals), sample_num if dirs is None else namer.tensor(dirs))

        @classmethod
        def try_build(cls, normals, dirs, **k):
            return cls(normals, how="try_build", dirs=dirs)

        supported = staticmethod(lambda K_, M_, He, We: (He, We) in TAKEN_SIZES)

        def taps(self, He, We):
            log("frs.taps", self.serial, He, We)

        def rotate(self, incidents):
            log("frs.rotate", self.serial, namer.tensor(incidents))

        def forward(self, *a, uniform_area=None, leave_room=False, listed_stream=None, rotated=False, feature_rows=None):
            log("frs.forward", self.serial, [namer.tensor(t) for t in a], uniform_area, leave_room,
                None if listed_stream is None else role(listed_stream), rotated, namer.tensor(feature_rows))

        def backward(self, *a, uniform_area=None, out_incidents=None, out_env=None, block_absmax=None, rotate_stream=None,
                     rotation_back=True):
            log("frs.backward", self.serial, [namer.tensor(t) for t in a], uniform_area, namer.tensor(out_incidents),
                namer.tensor(out_env), namer.tensor(block_absmax), None if rotate_stream is None else role(rotate_stream),
                rotation_back)
            return z(P, 3), z(P, 1), z(P, 3), out_incidents, out_env

        def incident_chain(self, incidents, grad, m, v, lr, lr_tail, betas, eps, step, grad_scale=1.0, skip_flag=None):
            log("frs.chain", self.serial, [namer.tensor(t) for t in (incidents, grad, m, v)], lr, lr_tail, list(betas), eps, step,
                grad_scale, namer.tensor(skip_flag))

    def traced(*a, group=None, **k):
        log("update_visibility", [namer.tensor(t) for t in a[:5]], a[5])
        return torch.ones(P, K, 1), torch.ones(P, K, 3), torch.full((P, K, 1), 2.0), None

    def traced_on_device(*a, group=None, want_dirs=False):
        log("update_visibility_device", [namer.tensor(t) for t in a[:5]], a[5], want_dirs)
        return torch.ones(P, K, 1), torch.ones(P, K, 3) if want_dirs else None, None

    def build_taps(dirs, He, We, *a, **k):
        log("build_taps", namer.tensor(dirs), He, We)
        return z(P * K * 3)

    class Pending:
        def finish(self, ordering_stream=None):
            log("raster.finish", None if ordering_stream is None else role(ordering_stream))
            return (17, z(H, W, dtype=torch.int32), z(3, H, W), z(1, H, W), z(1, H, W), z(16, H, W), z(3, H, W), z(3, H, W),
                    z(P, 1), z(P, dtype=torch.int32), z(64, dtype=torch.uint8), z(8, dtype=torch.uint8), z(8, dtype=torch.uint8))

    def begin(*a, **k):
        log("raster.begin", k.get("capacity"), None if k.get("ordering_stream") is None else role(k["ordering_stream"]),
            namer.tensor(k.get("overflow_flag")))
        return Pending()

    def backward(*a, **k):
        log("raster.backward", None if k.get("geometry_stream") is None else role(k["geometry_stream"]), list(k["active_features"]))
        return (z(P, 3), z(P, 3), z(P, 1), z(P, 3), z(P, 16), z(P, 6), z(P, 16, 3), z(P, 3), z(P, 4))

    main = FakeStream("main")
    roles = iter(("order", "early"))
    monkeypatch.setattr(torch.cuda, "stream", stream_context)
    monkeypatch.setattr(torch.cuda, "Stream", lambda device=None: FakeStream(next(roles, None)))
    monkeypatch.setattr(torch.cuda, "Event", lambda *a, **k: FakeEvent())
    monkeypatch.setattr(torch.cuda, "current_stream", lambda *a: main)
    # the two traces are replaced in every module of the package that imported them by name: wherever the step's code calls them
    # from, on the recorded commit and on this one
    for name, mod in list(sys.modules.items()):
        if name.startswith("relightable3dgaussian_amd.") and hasattr(mod, "update_visibility_device"):
            monkeypatch.setattr(mod, "update_visibility", traced)
            monkeypatch.setattr(mod, "update_visibility_device", traced_on_device)
    monkeypatch.setattr(shading_ops, "FixedRaySet", FakeRaySet)
    monkeypatch.setattr(shading_ops, "build_taps", build_taps)
    monkeypatch.setattr(rasterizer_ops, "rasterize_gaussians_begin", begin)
    monkeypatch.setattr(rasterizer_ops, "rasterize_gaussians_backward", backward)
    monkeypatch.setattr(rasterizer_ops, "num_rendered_of", lambda geom, P_: torch.tensor(17))
    cam = types.SimpleNamespace(image_height=H, image_width=W, world_view_transform=torch.eye(4), full_proj_transform=torch.eye(4),
                                camera_center=z(3), tanfovx=0.5, tanfovy=0.5, cx=2.0, cy=2.0)
    bg, gt = torch.ones(3), z(3, H, W)
    namer.view = dict(viewmatrix=cam.world_view_transform, campos=cam.camera_center, bg=bg, gt=gt)

    def resize_env(step, He, We):
        """Another environment texture, its gradient and its Adam group (the texture's group follows the tensor)."""
        step.env = z(1, He, We, 3)
        step.grads["env"] = torch.zeros_like(step.env)
        g = step.opt.groups[step._opt_order.index("env")]
        g["param"], g["exp_avg"], g["exp_avg_sq"] = step.env, torch.zeros_like(step.env), torch.zeros_like(step.env)

    traces = {}
    for name, on_device in STEPS.items():
        del trace[:]
        stage = lambda s: trace.append(["#", s])
        FakeRaySet.made = 0
        params = types.SimpleNamespace(xyz=z(P, 3), normal=z(P, 3), scaling=z(P, 3), rotation=z(P, 4), opacity=z(P, 1),
                                       features_dc=z(P, 1, 3), features_rest=z(P, 15, 3), base_color=z(P, 3), roughness=z(P, 1),
                                       incidents_dc=z(P, 1, 3), incidents_rest=z(P, 15, 3), env=z(1, 16, 32, 3))
        stage("construction")
        step = namer.step = fused_step.FusedStage2Step.__new__(fused_step.FusedStage2Step)
        step.__init__(params, K, device_visibility=on_device)
        stage("three iterations")
        for _ in range(3):
            step(cam, bg, gt)
        stage("a texture size the ray set takes")
        resize_env(step, 8, 16)
        step(cam, bg, gt)
        stage("a texture size the ray set refuses")
        resize_env(step, 4, 8)
        step(cam, bg, gt)
        stage("swapped directions")
        step.incident_dirs = torch.ones(P, K, 3)
        step(cam, bg, gt)
        stage("refresh_visibility")
        step.refresh_visibility()
        stage("one more iteration")
        step(cam, bg, gt)
        stage("the first texture size again")
        resize_env(step, 16, 32)
        step(cam, bg, gt)
        step(cam, bg, gt)
        stage("the state afterwards")
        log("state", step.visibility_refreshes, step.device_visibility, namer.tensor(step.incident_dirs), step._uniform_area,
            getattr(step._frs, "serial", None), namer.tensor(step._taps))
        traces[name] = [list(c) for c in trace]
    return traces


def test_both_kinds_of_step_launch_what_the_recorded_commit_launched(monkeypatch):
    with open(GOLDEN) as fh:
        doc = json.load(fh)
    assert len(doc["parent"]) == 40
    want = unpack(doc)
    got = json.loads(json.dumps(scenario(monkeypatch)))                 # (tuples as lists, as the file holds them)
    assert sorted(got) == sorted(want) == sorted(STEPS)
    for name in STEPS:
        for i, (g, w) in enumerate(zip(got[name], want[name])):
            assert g == w, "%s, call %d (after %s)" % (name, i, [c[1] for c in want[name][:i + 1] if c[0] == "#"][-1])
        assert len(got[name]) == len(want[name]), name
        assert got[name] == want[name]
