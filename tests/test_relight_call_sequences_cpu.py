"""What RelightRenderer launches, call by call, against a recording of the same scenario (tests/golden/relight_call_trace.json,
written by tests/golden/make_relight_call_trace.py from the commit whose hash the file holds): the check that a change of the
renderer's host code changes nothing a frame launches.  And the recipe by which bench_core.relight_bench clones a renderer for
its radiance-cache measurement, which only reports a failure instead of raising one.

The scenario (P=7, K=8, an 8x16 map, a 4x4 camera; the recording library of tests/helpers.py) runs seven renderers -- traced,
device and baked visibility, transport and radiance cache, stored and regenerated directions -- through construction, a fixed
light, a swapped visibility, a light that turns on the host and on the device, a light that stops, an edited map, a scaled
transform and a frame with capture maps.  Per C-ABI call the entry point, the scalars as they are, NULL as None and every
pointer as the NAME of the renderer attribute (or `_split` entry) whose buffer it is at the time of the call are recorded;
"other" for a buffer that belongs to none.  One name is given by value instead of by owner: a [K,3] table that
sampling.fibonacci_z_samples made is "ray_table" wherever it is kept (`_zsamples`, the split cache's `zsamples`, a local) --
every such table holds the same values, and which copy a launch reads is not behaviour."""
import json
import os

import torch

from tests.helpers import dt, recording_library, relight_camera, relight_model, z_rotation

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "relight_call_trace.json")
P, K = 7, 8
RENDERERS = {
    "traced/transport": dict(),
    "traced/transport/stored_dirs": dict(regenerate_dirs=False),
    "traced/radiance": dict(cache="radiance"),
    "device/transport": dict(device_visibility=True),
    "device/radiance": dict(device_visibility=True, cache="radiance"),
    "baked/transport": dict(baked_visibility=True),
    "baked/radiance": dict(baked_visibility=True, cache="radiance"),
}
# the renderer's buffers, in the order in which a pointer is looked up among them
ATTRIBUTES = ("xyz", "normal", "scaling", "rotation", "opacity", "base_color", "roughness", "shs", "incidents", "envmap",
              "a_scales", "a_rot", "a_opacity", "a_normal", "a_base", "a_rough", "a_viewdirs", "shade_out", "features",
              "visibility", "incident_dirs", "incident_areas", "visibility_sh", "_taps", "_consts")
SPLIT_ENTRIES = ("perm", "lt", "vis_t", "consts", "env4")


class _Namer:
    """Turns the arguments of a recorded call into names (module docstring)."""

    def __init__(self):
        self.renderer, self.frame_tensors, self.tables = None, {}, []

    def ray_table(self, *a, **k):
        """sampling.fibonacci_z_samples: the real [1,3,K] table as a transposed view of a contiguous [K,3] one, so that the
        `[0].t().contiguous()` of its callers is that tensor and no copy; a new tensor per call, like the real one."""
        table = self.real_z_samples(*a, **k)[0].t().contiguous()
        self.tables.append(table)
        return table.t()[None]

    def name_of(self, ptr):
        if ptr is None:
            return None
        if any(t.data_ptr() == ptr for t in self.tables):
            return "ray_table"
        for k, t in self.frame_tensors.items():
            if t is not None and t.data_ptr() == ptr:
                return k
        r = self.renderer
        for k in ATTRIBUTES:
            t = getattr(r, k, None)
            if isinstance(t, torch.Tensor) and t.data_ptr() == ptr:
                return k
        sp = getattr(r, "_split", None)
        if isinstance(sp, dict):
            for k in SPLIT_ENTRIES:
                if sp.get(k) is not None and sp[k].data_ptr() == ptr:
                    return "_split." + k
        return "other"

    def record(self, name, args):
        import ctypes
        from relightable3dgaussian_amd import _abi
        types = _abi.prototypes[name][1]
        assert len(types) == len(args), (name, len(types), len(args))
        out = ["stream" if i == 0 and ty is ctypes.c_void_p else self.name_of(a) if ty is ctypes.c_void_p else a
               for i, (ty, a) in enumerate(zip(types, args))]
        return [name, out]


def scenario(monkeypatch):
    """-> {renderer name: [[entry point, [argument, ...]] or ["#", step], ...]}"""
    from relightable3dgaussian_amd import relight, sampling
    namer = _Namer()
    trace = recording_library(monkeypatch, P, convert=namer.record).calls
    namer.real_z_samples = sampling.fibonacci_z_samples
    monkeypatch.setattr(relight.sampling, "fibonacci_z_samples", namer.ray_table)
    two_pi = 2.0 * 3.141592653589793
    monkeypatch.setattr(relight, "update_visibility", lambda *a, **k: (
        torch.ones(P, K, 1), torch.ones(P, K, 3), torch.full((P, K, 1), two_pi), None))
    monkeypatch.setattr(relight, "update_visibility_device", lambda *a, group=None, want_dirs=False: (
        torch.ones(P, K, 1), torch.ones(P, K, 3) if want_dirs else None, None))
    coeffs = torch.randn(P, 16, generator=torch.Generator().manual_seed(1))
    cam, bg = relight_camera(), torch.zeros(3)

    def frame(r, env_transform=None, **kw):
        namer.frame_tensors = dict(viewmatrix=cam.world_view_transform, campos=cam.camera_center, env_transform=env_transform,
                                   mask=kw.get("mask"))
        r.frame(cam, bg, env_transform=env_transform, **kw)

    traces = {}
    for name, kw in RENDERERS.items():
        del trace[:]
        step = lambda s: trace.append(["#", s])
        step("construction")
        model = relight_model(P, visibility_dc=coeffs[:, :1, None].clone(), visibility_rest=coeffs[:, 1:, None].clone())
        r = namer.renderer = relight.RelightRenderer.__new__(relight.RelightRenderer)
        r.__init__(model, dt(torch.zeros(8, 16, 3)), K, **kw)
        step("fixed light")
        for _ in range(3):
            frame(r)
        step("swapped visibility")
        if kw.get("baked_visibility"):
            r.visibility_sh = r.visibility_sh.clone()
        else:
            r.visibility = torch.ones(P, K, 1)
        for _ in range(2):
            frame(r)
        step("host rotations")
        for i in range(1, 5):
            frame(r, z_rotation(i))
        step("device rotations")
        for i in range(6):
            frame(r, dt(z_rotation(10 + i)))
        step("one device rotation")
        fixed = dt(z_rotation(30))
        for _ in range(3):
            frame(r, fixed)
        step("map edited in place")
        r.envmap.add_(1.0)
        frame(r, dt(z_rotation(40)))
        step("scaled host transform")
        frame(r, torch.eye(3) * 2.0)
        step("capture maps and a mask")
        frame(r, outputs=("pbr_env", "normal", "visibility"), mask=torch.ones(4, 4))
        traces[name] = [list(c) for c in trace]
    return traces


def pack(traces, parent):
    """The JSON form: every distinct call once, the traces as indices into that table."""
    table, index = [], {}
    packed = {}
    for name, calls in traces.items():
        packed[name] = []
        for c in calls:
            key = json.dumps(c)
            if key not in index:
                index[key] = len(table)
                table.append(c)
            packed[name].append(index[key])
    return dict(parent=parent, calls=table, traces=packed)


def unpack(doc):
    return {name: [doc["calls"][i] for i in idx] for name, idx in doc["traces"].items()}


def test_every_renderer_launches_what_the_recorded_commit_launched(monkeypatch):
    with open(GOLDEN) as fh:
        doc = json.load(fh)
    assert len(doc["parent"]) == 40
    want = unpack(doc)
    got = json.loads(json.dumps(scenario(monkeypatch)))                 # (tuples as lists, as the file holds them)
    assert sorted(got) == sorted(want) == sorted(RENDERERS)
    for name in RENDERERS:
        for i, (g, w) in enumerate(zip(got[name], want[name])):
            assert g == w, "%s, call %d (after %s)" % (name, i, [c[1] for c in want[name][:i + 1] if c[0] == "#"][-1])
        assert len(got[name]) == len(want[name]), name
        assert got[name] == want[name]


def test_the_benchmark_clone_rebuilds_a_radiance_cache_and_leaves_the_original_alone(monkeypatch):
    """The statements of bench_core.relight_bench that turn a transport-cache renderer into a radiance-cache one (they sit in a
    try/except there: a break would be reported as a failed side measurement, or as wrong numbers)."""
    from relightable3dgaussian_amd import relight, shading_ops
    rec = recording_library(monkeypatch, P)
    monkeypatch.setattr(relight, "update_visibility", lambda *a, **k: (torch.ones(P, K, 1), torch.ones(P, K, 3),
                                                                       torch.full((P, K, 1), 2.0), None))
    built = []
    monkeypatch.setattr(shading_ops, "build_taps", lambda dirs, He, We, tr=None, radiance_of=None:
                        built.append(tr) or torch.zeros(P * K * 3))
    cam, bg = relight_camera(), torch.zeros(3)
    renderer = relight.RelightRenderer(relight_model(P), dt(torch.zeros(8, 16, 3)), K)
    for _ in range(3):
        renderer.frame(cam, bg)
    records = renderer._taps
    assert len(built) == 1 and rec.names().count("r3dg_shade_build_transport") == 1

    r2 = relight.RelightRenderer.__new__(relight.RelightRenderer)
    r2.__dict__.update(renderer.__dict__)
    r2.cache = "radiance"
    r2._taps = r2._taps_key = r2._taps_ref = r2._light_key = r2._light_ref = None
    r2._light_changes, r2._area_key = 0, None
    r2.shade_out, r2.features = torch.empty_like(renderer.shade_out), torch.empty_like(renderer.features)

    del rec.calls[:]
    r2.frame(cam, bg)
    assert len(built) == 2
    assert not [n for n in rec.names() if n.startswith("r3dg_shade_build_transport")]
    assert "r3dg_shade_forward_transport" not in rec.names()
    (cached,) = rec.args_of("r3dg_shade_forward_cached")
    assert cached[-2] == shading_ops.TAPS_ARE_RADIANCE and cached[-3] == r2._taps.data_ptr() and cached[-1] == r2.shade_out.data_ptr()
    assert renderer._taps is records and r2._taps is not records

    del rec.calls[:]
    renderer.frame(cam, bg)
    n = rec.names()
    assert len(built) == 2 and n.count("r3dg_shade_forward_transport") == 1 and "r3dg_shade_forward_cached" not in n
    assert not [x for x in n if x.startswith("r3dg_shade_build")]
    assert rec.args_of("r3dg_shade_forward_transport")[0][7] == records.data_ptr() and renderer._taps is records
