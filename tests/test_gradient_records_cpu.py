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


def test_records_backward_reports_unsupported_instances_without_an_error():
    L = _lib.lib()
    rows, ok, layout = C.c_void_p(123), C.c_int(7), (C.c_int * N)()
    args = lambda n_act, act, depth: (
        None, None, 5, 16, 3, 16, 9, 1, 8, 8, 1, 1, 1, None, 1, 1.0, 1, None, 1, 1, 1, 0.5, 0.5, 1, 1, 1, 1, 1, 1, depth, 1,
        1, 1, 1, 1, 1, 1, 1, 0, n_act, act, None, 0.0, 0.0, 0.0, 1, 1.0, None, C.byref(rows), layout, C.byref(ok))
    # all 16 channels live: 32-float records
    assert L.r3dg_rasterize_backward_split_records(*args(-1, None, None)) == 0 and ok.value == 0 and rows.value is None
    # 7 active channels WITH a depth gradient: no instance without the depth slot, 18 channels
    ok.value = 7
    act = (C.c_int * 7)(0, 2, 3, 4, 5, 6, 7)
    assert L.r3dg_rasterize_backward_split_records(*args(7, act, 1)) == 0 and ok.value == 0
    # P == 0: nothing to do, nothing supported
    ok.value = 7
    a = list(args(3, (C.c_int * 3)(2, 3, 4), None))
    a[2] = 0
    assert L.r3dg_rasterize_backward_split_records(*a) == 0 and ok.value == 0
    # bad arguments
    a = list(args(3, (C.c_int * 3)(2, 3, 4), None))
    a[-1] = None
    assert L.r3dg_rasterize_backward_split_records(*a) != 0                       # no place for the answer
    a = list(args(3, (C.c_int * 3)(2, 3, 4), None))
    a[31] = None
    assert L.r3dg_rasterize_backward_split_records(*a) != 0                       # no dL_dmean2D
    assert L.r3dg_rasterize_backward_split_records(*args(3, (C.c_int * 3)(2, 3, 16), None)) != 0   # channel out of range


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
