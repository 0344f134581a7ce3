"""RelightRenderer(device_visibility=True) without a GPU: the C ABI declaration of r3dg_shade_build_transport_rayset and its
derived ctypes signature, and the renderer's host logic against a recording library (the technique of
tests/test_host_mirrors_cpu.py): which trace it calls with which arguments, which builder, and that no direction pointer
reaches the per-frame kernels."""
import ctypes as C
import math
import os

import pytest
import torch

from tests.helpers import dt, recording_library, relight_camera, relight_model, z_rotation as rot

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROTOTYPE = """\
int r3dg_shade_build_transport_rayset(void* stream, int P, int K, int M, const float* d_normals, const float* d_incidents,
                                      const float* d_visibility, const float* d_zsamples, float uniform_area,
                                      const float* d_env, int He, int We, const float* d_env_transform,
                                      float* d_transport, float* d_consts);
"""


def test_header_declares_the_builder_and_the_binding_follows():
    from relightable3dgaussian_amd import _abi
    with open(os.path.join(ROOT, "include", "r3dg_hip.h")) as fh:
        assert PROTOTYPE in fh.read()
    res, args = _abi.prototypes["r3dg_shade_build_transport_rayset"]
    p, i, f = C.c_void_p, C.c_int, C.c_float
    assert res is C.c_int and args == [p, i, i, i, p, p, p, p, f, p, i, i, p, p, p]
    assert len(_abi.options) == 13


def test_device_visibility_host_logic_with_a_recording_library(monkeypatch):
    from relightable3dgaussian_amd import relight, shading_ops
    P, K = 7, 8
    rec = recording_library(monkeypatch, P)
    calls, names = rec.calls, rec.names
    glue, device, taps_built = [], [], []
    monkeypatch.setattr(relight, "update_visibility", lambda *a, **k: glue.append(k) or (
        torch.ones(P, K, 1), torch.ones(P, K, 3), torch.full((P, K, 1), 2.0), None))
    tracer = object()
    vis = torch.ones(P, K, 1)
    monkeypatch.setattr(relight, "update_visibility_device", lambda *a, **k: device.append((a, k)) or (vis, None, tracer))
    monkeypatch.setattr(shading_ops, "build_taps", lambda dirs, He, We, tr=None, radiance_of=None:
                        taps_built.append(tr) or torch.zeros(P * K * 3))
    z = torch.zeros
    model, cam, env = relight_model(P), relight_camera(), dt(z(8, 16, 3))

    # the default renderer never asks for the device trace
    relight.RelightRenderer(model, env, K)
    assert len(glue) == 1 and not device
    del glue[:]

    # the device renderer: one device trace, `group` and `want_dirs` forwarded, no direction / area tensor
    group = object()
    r = relight.RelightRenderer(model, env, K, process_group=group, device_visibility=True)
    assert not glue and len(device) == 1
    a, k = device[0]
    assert len(a) == 6 and a[5] == K and k == dict(group=group, want_dirs=False)
    assert r.visibility is vis and r.tracer is tracer and r.incident_dirs is None and r.incident_areas is None
    assert r._uniform_area == 2.0 * math.pi
    relight.RelightRenderer(model, env, K, cache="radiance", device_visibility=True)
    assert device[1][1] == dict(group=None, want_dirs=True)
    with pytest.raises(RuntimeError):
        relight.RelightRenderer(model, env, K, device_visibility=True, regenerate_dirs=False)

    # fixed light: ONE builder launch for three frames, no taps, no two-kernel builder, a NULL direction pointer per frame
    calls.clear()
    for _ in range(3):
        out = r.frame(cam, z(3))
    n = names()
    assert n.count("r3dg_shade_build_transport_rayset") == 1 and n.count("r3dg_shade_forward_transport") == 3
    assert "r3dg_shade_build_transport" not in n and "r3dg_shade_forward_cached" not in n and not taps_built and not glue
    b = [c for c in calls if c[0] == "r3dg_shade_build_transport_rayset"][0][1]
    assert len(b) == 15 and b[1:4] == (P, K, 16) and b[7] == r._zsamples.data_ptr() and b[8] == pytest.approx(2.0 * math.pi)
    assert b[9] == r.envmap.data_ptr() and b[10:12] == (8, 16) and b[12] is None
    assert b[13] == r._taps.data_ptr() and b[14] == r._consts.data_ptr() and b[6] == vis.data_ptr()
    assert tuple(r._taps.shape) == (P, K, 3) and r._taps.dtype == torch.float32 and tuple(r._consts.shape) == (P, 16)
    for c in calls:
        if c[0] == "r3dg_shade_forward_transport":
            assert len(c[1]) == 12 and c[1][10] is None and c[1][7] == r._taps.data_ptr() and c[1][9] == r._zsamples.data_ptr()
    assert out["num_rendered"] == 3 and r.incident_dirs is None

    # the keys work without a direction tensor: swapped visibility rebuilds (into the same record buffer), nothing else does
    buf = r._taps.data_ptr()
    r.visibility = torch.ones(P, K, 1)
    r.frame(cam, z(3))
    r.frame(cam, z(3))
    assert names().count("r3dg_shade_build_transport_rayset") == 2 and r._taps.data_ptr() == buf
    assert r._taps_ref[1][0] is r.visibility and r._taps_ref[1][1] is r.normal            # references what it keys on

    # the light turns: first change builds once more (with the rotation), from the second on the split transport with NULL
    # directions, and still no direction tensor
    calls.clear()
    for i in range(1, 5):
        r.frame(cam, z(3), env_transform=rot(i))
    n = names()
    assert n.count("r3dg_shade_build_transport_rayset") == 1 and n.count("r3dg_shade_build_split") == 1
    assert n.count("r3dg_shade_forward_split") == 3 and "r3dg_shade_forward_cached" not in n
    assert [c for c in calls if c[0] == "r3dg_shade_build_transport_rayset"][0][1][12] is not None
    sp = [c for c in calls if c[0] == "r3dg_shade_build_split"][0][1]
    assert len(sp) == 13 and sp[7] is None and sp[8] is not None and sp[9] == pytest.approx(2.0 * math.pi)
    assert not taps_built and not glue and "r3dg_shade_build_transport" not in n and r.incident_dirs is None
