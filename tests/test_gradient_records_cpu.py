"""The gradient-record entry points' argument checks and the host side of the switch; nothing here reaches a launch."""
import ctypes as C

import torch

from relightable3dgaussian_amd import _abi, _lib

N = _abi.constants["R3DG_GRAD_RECORD_LAYOUT_INTS"]


def _layout(nvp=16, lean=True, features=((2, 9), (3, 10), (4, 11))):
    """A layout as the library hands it out: width | r g b | S_x S_y depth | S_xx S_xy S_yy opacity | 36 feature columns."""
    vc = 5 if lean else 6
    ints = [nvp, 0, 1, 2, 3, 4, -1 if lean else 5, vc, vc + 1, vc + 2, vc + 3] + [-1] * 36
    for col, ch in features:
        ints[11 + col] = ch
    return (C.c_int * N)(*ints)


def test_layout_size_is_the_struct_of_the_header():
    assert N == 1 + 3 + 3 + 4 + _lib.lib().r3dg_max_features_backward()


Scene, Backward, AdamGroup = (_abi.structs[n] for n in ("r3dg_raster_scene", "r3dg_raster_backward", "r3dg_adam_group"))
NO_ADAM = (None, 0.0, 0.0, 0.0, 1, 1.0, None)


def _call(n_act=3, act=(2, 3, 4), **fields):
    """(scene, backward) of a call on 5 Gaussians, S = 16, an 8x8 image: every pointer a dummy 1 (nothing here reaches a launch)
    except the optional inputs and the depth gradient; `fields` overrides by NAME in whichever struct has the field."""
    scene = dict(P=5, S=16, D=3, M=16, width=8, height=8, d_background=1, d_means3D=1, d_shs=16, d_features=1, d_scales=1,
                 scale_modifier=1.0, d_rotations=1, d_viewmatrix=1, d_projmatrix=1, d_campos=1, tan_fovx=0.5, tan_fovy=0.5)
    back = dict(R=9, d_radii=1, d_geom_buffer=1, d_binning_buffer=1, d_img_buffer=1, d_dL_dpix=1, d_dL_dpix_o=1, d_dL_dpix_f=1,
                d_dL_dmean2D=1, d_dL_dmean3D=1, d_dL_dcov3D=1, d_dL_dsh=1, d_dL_dscale=1, d_dL_drot=1, backward_geometry=1,
                debug=0, n_active_features=n_act)
    for k, v in fields.items():
        (scene if hasattr(Scene, k) else back)[k] = v
    keep = (C.c_int * max(1, len(act)))(*act) if act is not None else None
    back["active_features"] = C.addressof(keep) if keep is not None else None
    return Scene(**scene), Backward(**back), keep


def _split(scene, back, adam=NO_ADAM, outs=(None, None, None)):
    return _lib.lib().r3dg_rasterize_backward_split(None, None, C.byref(scene), C.byref(back), *adam, *outs)


def test_records_backward_reports_unsupported_instances_without_an_error():
    rows, ok, layout = C.c_void_p(123), C.c_int(7), (C.c_int * N)()
    outs = (C.byref(rows), layout, C.byref(ok))
    # all 16 channels live: 32-float records
    s, b, _k = _call(-1, None)
    assert _split(s, b, outs=outs) == 0 and ok.value == 0 and rows.value is None
    # 7 active channels WITH a depth gradient: no instance without the depth slot, 18 channels
    ok.value = 7
    s, b, _k = _call(7, (0, 2, 3, 4, 5, 6, 7), d_dL_dpix_d=1)
    assert _split(s, b, outs=outs) == 0 and ok.value == 0
    # P == 0: nothing to do, nothing supported, the records pointer reset
    ok.value, rows.value = 7, 123
    s, b, _k = _call(P=0)
    assert _split(s, b, outs=outs) == 0 and ok.value == 0
    assert rows.value is None
    # bad arguments
    s, b, _k = _call()
    assert _split(s, b, outs=(C.byref(rows), layout, None)) != 0                  # no place for the answer
    s, b, _k = _call(d_dL_dmean2D=None)
    assert _split(s, b, outs=outs) != 0                                           # no dL_dmean2D
    s, b, _k = _call(3, (2, 3, 16))
    assert _split(s, b, outs=outs) != 0                                           # channel out of range


def test_one_entry_checks_the_sh_adam_arguments_on_both_paths_and_the_outputs_together():
    """sh_adam given: step counts from 1, the group is the SH tensor itself, and SH is the colour input -- with record outputs
    and without; record outputs come all three or not at all."""
    EINVAL = _abi.constants["R3DG_EINVAL"]
    rows, ok, layout = C.c_void_p(), C.c_int(0), (C.c_int * N)()
    group = AdamGroup(param=16, exp_avg=32, exp_avg_sq=48, n=5 * 3 * 16, lr=1e-3, lr_tail=1e-4, period=48, split=3)
    other = AdamGroup(param=64, exp_avg=32, exp_avg_sq=48, n=5 * 3 * 16, lr=1e-3, lr_tail=1e-4, period=48, split=3)
    adam = lambda g, step: (C.addressof(g), 0.9, 0.999, 1e-15, step, 1.0, None)
    for outs in ((None, None, None), (C.byref(rows), layout, C.byref(ok))):
        s, b, _k = _call()
        assert _split(s, b, adam(group, 0), outs) == EINVAL and b"step counts from 1" in _lib.lib().r3dg_last_error()
        assert _split(s, b, adam(other, 1), outs) == EINVAL and b"SH tensor itself" in _lib.lib().r3dg_last_error()
        s, b, _k = _call(d_colors_precomp=1)
        assert _split(s, b, adam(group, 1), outs) == EINVAL and b"needs SH input" in _lib.lib().r3dg_last_error()
    s, b, _k = _call()
    assert _split(s, b, outs=(None, None, C.byref(ok))) == EINVAL


def test_readers_refuse_what_is_not_a_layout_of_16_float_records():
    L = _lib.lib()
    good = _layout()
    scatter = lambda P, S, rows, lay: L.r3dg_gradient_records_scatter(None, P, S, rows, lay, 1, 1, 1, 1, 1)
    unpack = lambda P, rows, lay: L.r3dg_stage2_unpack_gradients_records(None, P, rows, lay, 1, 0.1, 1, 1, None, None)
    chain = lambda P, rows, lay, g_xyz=1: L.r3dg_stage2_activate_backward_with_records(
        None, P, 1, 1, 1, 1, 1, 1, 1, 1, 1, rows, lay, 1, 1, 1, 1, 1, 1, g_xyz, 1, 1, 1, 1, 1, 1, 0, 0, None, None, None, 0.0,
        None, None, 0)
    assert scatter(0, 16, None, None) == 0 and unpack(0, None, None) == 0 and chain(0, None, None) == 0       # nothing to do
    for bad in (None,                                                     # no layout
                _layout(nvp=24),                                          # not a record width
                _layout(features=((2, 9), (3, 9))),                       # two columns in one channel
                _layout(features=((2, 9), (3, 11))),                      # a hole in the channels
                _layout(features=((2, 8),)),                              # a feature in the opacity channel
                _layout(features=((2, 16),))):                            # past the record
        assert scatter(5, 16, 1, bad) != 0 and unpack(5, 1, bad) != 0 and chain(5, 1, bad) != 0
    wide = _layout(nvp=32, lean=False, features=tuple((c, 10 + c) for c in range(16)))
    assert unpack(5, 1, wide) != 0 and chain(5, 1, wide) != 0             # 32-float rows: the scatter pass only
    assert scatter(5, 2, 1, good) != 0                                    # a column the caller's S does not have
    assert scatter(5, 16, None, good) != 0 and unpack(5, None, good) != 0 and chain(5, None, good) != 0       # no rows
    assert chain(5, 1, good, g_xyz=None) != 0                             # frozen geometry has no records
    assert b"frozen geometry" in L.r3dg_last_error()


def test_whole_iterations_ask_for_records_and_bare_calls_do_not(monkeypatch):
    """FusedStage2Step._reads_gradient_records: the switch, frozen geometry, and a backward that does not take the argument."""
    from relightable3dgaussian_amd import rasterizer_ops
    from relightable3dgaussian_amd.fused_step import FusedStage2Step
    step = FusedStage2Step.__new__(FusedStage2Step)
    step.frozen_geometry = False
    monkeypatch.delenv("R3DG_GRADIENT_RECORDS", raising=False)
    assert step._reads_gradient_records()
    monkeypatch.setenv("R3DG_GRADIENT_RECORDS", "0")
    assert not step._reads_gradient_records()
    monkeypatch.setenv("R3DG_GRADIENT_RECORDS", "1")
    step.frozen_geometry = True
    assert not step._reads_gradient_records()
    step.frozen_geometry = False
    monkeypatch.setattr(rasterizer_ops, "rasterize_gaussians_backward", lambda *a, **k: None)
    assert not step._reads_gradient_records()
    rows = rasterizer_ops.GradientRecords()
    assert not rows and rows.ptr is None and isinstance(torch.zeros(1), torch.Tensor)
