"""RelightRenderer(baked_visibility=True) without a GPU: the C ABI declarations of r3dg_visibility_sh_expand and
r3dg_shade_build_transport_baked, their derived ctypes signatures and the built library's exports; the refusals of the two host
mirrors and of the constructor, which must come before the library is touched; where the coefficients are taken from; and the
renderer's host logic against a recording library (the technique of tests/test_relight_device_visibility_cpu.py): no trace, one
baked builder launch under a fixed light, a transient expansion in front of the split cache under a turning one."""
import ctypes as C
import math
import os
import types

import pytest
import torch

from tests.helpers import dt, recording_library, relight_camera, relight_model as _model, z_rotation as rot

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROTOTYPES = """\
int r3dg_shade_build_transport_baked(void* stream, int P, int K, int M, const float* d_normals, const float* d_incidents,
                                     const float* d_visibility_sh, const float* d_zsamples, float uniform_area,
                                     const float* d_env, int He, int We, const float* d_env_transform,
                                     float* d_transport, float* d_consts);
int r3dg_visibility_sh_expand(void* stream, int P, int K, const float* d_normals, const float* d_zsamples,
                              const float* d_visibility_sh, float* d_visibility_out);
"""


def test_header_declares_both_functions_and_the_library_exports_them():
    from relightable3dgaussian_amd import _abi, _lib
    with open(os.path.join(ROOT, "include", "r3dg_hip.h")) as fh:
        assert PROTOTYPES in fh.read()
    p, i, f = C.c_void_p, C.c_int, C.c_float
    res, args = _abi.prototypes["r3dg_shade_build_transport_baked"]
    assert res is C.c_int and args == [p, i, i, i, p, p, p, p, f, p, i, i, p, p, p]
    # (the traced builder's signature: the baked one replaces a pointer by a pointer)
    assert args == _abi.prototypes["r3dg_shade_build_transport_rayset"][1]
    res, args = _abi.prototypes["r3dg_visibility_sh_expand"]
    assert res is C.c_int and args == [p, i, i, p, p, p, p]
    L = _lib.lib()
    assert L.r3dg_visibility_sh_expand is not None and L.r3dg_shade_build_transport_baked is not None


z = torch.zeros


def _no_library(monkeypatch):
    from relightable3dgaussian_amd import _lib

    def lib():
        raise AssertionError("the library was touched before the arguments were refused")
    monkeypatch.setattr(_lib, "lib", lib)


def test_mirrors_refuse_before_touching_the_library(monkeypatch):
    from relightable3dgaussian_amd import shading_ops as so
    _no_library(monkeypatch)
    P, K = 5, 4
    n, zs, v, inc, env = dt(z(P, 3)), dt(z(K, 3)), dt(z(P, 16)), dt(z(P, 16, 3)), dt(z(8, 16, 3))
    good = dict(normals=n, visibility_sh=v, zsamples=zs)
    for bad in (dict(normals=z(P, 3)), dict(visibility_sh=z(P, 16)), dict(zsamples=z(K, 3)),             # CPU tensors
                dict(visibility_sh=dt(z(P, 9))), dict(visibility_sh=dt(z(P + 1, 16))), dict(visibility_sh=dt(z(P, 16, 2))),
                dict(visibility_sh=dt(z(P, 16, dtype=torch.float64))), dict(normals=dt(z(P, 3, dtype=torch.float16))),
                dict(normals=dt(z(P, 4))), dict(zsamples=dt(z(3, K)))):
        kw = dict(good, **bad)
        with pytest.raises(RuntimeError):
            so.expand_visibility(**kw)
        with pytest.raises(RuntimeError):
            so.build_transport_baked(kw["normals"], inc, kw["visibility_sh"], kw["zsamples"], 2.0 * math.pi, env)
    for out in (dt(z(P, K + 1, 1)), z(P, K, 1), dt(z(P, K, 1, dtype=torch.float64))):
        with pytest.raises(RuntimeError):
            so.expand_visibility(n, v, zs, out=out)
    for kw in (dict(transport=dt(z(P, K, 2))), dict(transport=dt(z(K, P, 3))),
               dict(transport=dt(z(P, K, 3, dtype=torch.float64))), dict(consts=dt(z(P, 13)))):
        with pytest.raises(RuntimeError):
            so.build_transport_baked(n, inc, v, zs, 2.0 * math.pi, env, **kw)
    with pytest.raises(RuntimeError):
        so.build_transport_baked(n, z(P, 16, 3), v, zs, 2.0 * math.pi, env)                              # CPU incident light
    with pytest.raises(RuntimeError):
        so.build_transport_baked(n, inc, v, zs, 2.0 * math.pi, z(8, 16, 3))                               # CPU map


def test_constructor_refuses_before_touching_the_library(monkeypatch):
    from relightable3dgaussian_amd import relight
    _no_library(monkeypatch)
    P, K = 7, 8
    env = dt(z(8, 16, 3))
    coeffs = dict(visibility_dc=z(P, 1, 1), visibility_rest=z(P, 15, 1))
    with pytest.raises(RuntimeError, match="baked visibility SH"):
        relight.RelightRenderer(_model(P), env, K, baked_visibility=True)
    with pytest.raises(RuntimeError, match="baked visibility SH"):
        relight.RelightRenderer(_model(P, visibility_dc=z(P, 1, 1)), env, K, baked_visibility=True)      # half of the pair
    with pytest.raises(RuntimeError, match="regenerate_dirs"):
        relight.RelightRenderer(_model(P, **coeffs), env, K, baked_visibility=True, regenerate_dirs=False)
    with pytest.raises(RuntimeError, match="device_visibility"):
        relight.RelightRenderer(_model(P, **coeffs), env, K, baked_visibility=True, device_visibility=True)
    with pytest.raises(RuntimeError):
        relight.RelightRenderer(_model(P, visibility_sh=z(P, 9)), env, K, baked_visibility=True)
    with pytest.raises(RuntimeError):
        relight.RelightRenderer(_model(P, visibility_sh=z(P + 1, 16)), env, K, baked_visibility=True)
    with pytest.raises(RuntimeError):
        relight.RelightRenderer(_model(P, visibility_sh=z(P, 16, dtype=torch.float64)), env, K, baked_visibility=True)
    cpu = _model(P, **coeffs)
    cpu.xyz = z(P, 3)
    with pytest.raises(RuntimeError):
        relight.RelightRenderer(cpu, env, K, baked_visibility=True)


def test_visibility_sh_of_reads_every_form_a_model_holds_them_in():
    from relightable3dgaussian_amd import checkpoint, relight
    P = 6
    coeffs = torch.randn(P, 16, generator=torch.Generator().manual_seed(3))
    pair = types.SimpleNamespace(visibility_dc=coeffs[:, :1, None].clone(), visibility_rest=coeffs[:, 1:, None].clone())
    for model in (pair, types.SimpleNamespace(visibility_sh=coeffs.clone()), types.SimpleNamespace(visibility_sh=coeffs[..., None].clone())):
        got = relight._visibility_sh_of(model)
        assert tuple(got.shape) == (P, 16) and got.is_contiguous() and torch.equal(got, coeffs)
    assert relight._visibility_sh_of(types.SimpleNamespace()) is None
    restored = checkpoint.restore(os.path.join(ROOT, "tests", "golden", "checkpoint_reference_stage2.pth"), pbr=True)
    got = relight._visibility_sh_of(restored)
    n = restored.xyz.shape[0]
    assert tuple(got.shape) == (n, 16) and got.dtype == torch.float32
    assert torch.equal(got[:, 0], restored.visibility_dc.reshape(n)) and torch.equal(got[:, 1:], restored.visibility_rest.reshape(n, 15))


def test_baked_host_logic_with_a_recording_library(monkeypatch):
    from relightable3dgaussian_amd import relight, shading_ops
    P, K = 7, 8
    rec = recording_library(monkeypatch, P)
    calls, names = rec.calls, rec.names
    traced = []
    monkeypatch.setattr(relight, "update_visibility", lambda *a, **k: traced.append("glue"))
    monkeypatch.setattr(relight, "update_visibility_device", lambda *a, **k: traced.append("device"))
    monkeypatch.setattr(shading_ops, "build_taps", lambda *a, **k: traced.append("taps"))
    coeffs = torch.randn(P, 16, generator=torch.Generator().manual_seed(1))
    model = _model(P, visibility_dc=coeffs[:, :1, None].clone(), visibility_rest=coeffs[:, 1:, None].clone())
    cam, env = relight_camera(), dt(z(8, 16, 3))

    # construction: a snapshot of the coefficients, no trace of either kind, nothing per sample
    r = relight.RelightRenderer(model, env, K, baked_visibility=True)
    assert not traced and names() == ["r3dg_stage2_activate"]
    assert r.tracer is None and r.visibility is None and r.incident_dirs is None and r.incident_areas is None
    assert r._uniform_area == 2.0 * math.pi
    assert torch.equal(r.visibility_sh, coeffs)
    model.visibility_dc.add_(1.0)
    assert torch.equal(r.visibility_sh, coeffs)

    # fixed light: ONE baked builder launch for three frames, fed the coefficient snapshot; no expansion, no [P,K] visibility
    calls.clear()
    for _ in range(3):
        r.frame(cam, z(3))
    n = names()
    assert n.count("r3dg_shade_build_transport_baked") == 1 and n.count("r3dg_shade_forward_transport") == 3
    for other in ("r3dg_shade_build_transport_rayset", "r3dg_shade_build_transport", "r3dg_visibility_sh_expand", "r3dg_shade_forward_cached"):
        assert other not in n
    b = [c for c in calls if c[0] == "r3dg_shade_build_transport_baked"][0][1]
    assert len(b) == 15 and b[1:4] == (P, K, 16) and b[6] == r.visibility_sh.data_ptr() and b[7] == r._zsamples.data_ptr()
    assert b[8] == pytest.approx(2.0 * math.pi) and b[9] == r.envmap.data_ptr() and b[10:12] == (8, 16) and b[12] is None
    assert b[13] == r._taps.data_ptr() and b[14] == r._consts.data_ptr()
    assert tuple(r._taps.shape) == (P, K, 3) and r._taps.dtype == torch.float32 and r.visibility is None and not traced
    assert r._taps_ref[1][0] is r.visibility_sh and r._taps_ref[1][1] is r.normal                 # references what it keys on

    # swapped coefficients rebuild, into the same record buffer
    buf = r._taps.data_ptr()
    r.visibility_sh = r.visibility_sh.clone()
    r.frame(cam, z(3))
    r.frame(cam, z(3))
    assert names().count("r3dg_shade_build_transport_baked") == 2 and r._taps.data_ptr() == buf

    # the light turns: one more baked build (with the rotation), then ONE expansion in front of ONE split build; the expansion
    # is not kept
    calls.clear()
    for i in range(1, 5):
        r.frame(cam, z(3), env_transform=rot(i))
    n = names()
    assert n.count("r3dg_shade_build_transport_baked") == 1 and n.count("r3dg_visibility_sh_expand") == 1
    assert n.count("r3dg_shade_build_split") == 1 and n.count("r3dg_shade_forward_split") == 3 and "r3dg_shade_forward_cached" not in n
    assert n.index("r3dg_visibility_sh_expand") < n.index("r3dg_shade_build_split")
    assert [c for c in calls if c[0] == "r3dg_shade_build_transport_baked"][0][1][12] is not None
    ex = [c for c in calls if c[0] == "r3dg_visibility_sh_expand"][0][1]
    sp = [c for c in calls if c[0] == "r3dg_shade_build_split"][0][1]
    assert len(ex) == 7 and ex[1:3] == (P, K) and ex[5] == r.visibility_sh.data_ptr() and sp[6] == ex[6] and sp[7] is None
    assert r.visibility is None and r.incident_dirs is None and not traced

    # the radiance cache materialises the [P,K] visibility once, on the first frame, and keeps it
    monkeypatch.setattr(shading_ops, "build_taps", lambda dirs, He, We, tr=None, radiance_of=None: torch.zeros(P * K * 3))
    monkeypatch.setattr(relight.sampling, "fibonacci_sphere_sampling", lambda nrm, k: (torch.zeros(nrm.shape[0], k, 3), None))
    c = relight.RelightRenderer(model, env, K, cache="radiance", baked_visibility=True)
    assert c.visibility is None
    calls.clear()
    c.frame(cam, z(3))
    held = c.visibility
    c.frame(cam, z(3))
    n = names()
    assert n.count("r3dg_visibility_sh_expand") == 1 and n.count("r3dg_shade_forward_cached") == 2 and c.visibility is held
    assert tuple(held.shape) == (P, K, 1)
    assert [a[1][13] for a in calls if a[0] == "r3dg_shade_forward_cached"] == [held.data_ptr()] * 2


def test_the_ray_set_kernels_use_no_scratch_memory(tmp_path):
    """hipcc's metadata for gfx950 (read as tests/test_kernel_resources_cpu.py reads it for the hot kernels): the two new kernels
    and both instances of the builder keep their per-lane arrays (16 basis values, 13 sums) in registers."""
    from relightable3dgaussian_amd import build as B
    from tests.test_kernel_resources_cpu import _metadata
    if not os.path.exists(B.HIPCC):
        pytest.skip("no hipcc")
    _, kernels = _metadata("shading_relight_rayset.hip", str(tmp_path))
    found = {}
    for name, (scratch, vgprs) in kernels.items():
        for key in ("visibility_sh_expand_kernel", "shade_build_transport_rayset_kernelILb0", "shade_build_transport_rayset_kernelILb1"):
            if key in name:
                found[key] = (scratch, vgprs)
    assert len(found) == 3, kernels
    assert all(scratch == 0 for scratch, _ in found.values()), found
    assert all(0 < vgprs <= 128 for _, vgprs in found.values()), found          # (at least 4 waves per SIMD)
