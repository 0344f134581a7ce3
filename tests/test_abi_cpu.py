"""relightable3dgaussian_amd/_abi.py reads include/r3dg_hip.h; the C compiler reads the same header and is the witness."""
import ctypes as C
import subprocess

import pytest

from relightable3dgaussian_amd import _abi, densify, fused_adam

_i, _f, _p, _A = C.c_int, C.c_float, C.c_void_p, _abi.ALLOC_FN


def test_c_compiler_agrees_on_structs_constants_and_options(tmp_path):
    """A C program generated from the reader's own name lists (a name the compiler rejects fails too) prints the size, and per
    field the offset, size and type, of the six structs, every integer #define and every R3DG_OPT_* enumerator."""
    assert set(_abi.structs) == {"r3dg_adam_group", "r3dg_densify_config", "r3dg_densify_group", "r3dg_raster_scene",
                                 "r3dg_raster_outputs", "r3dg_raster_backward"}
    assert (fused_adam.AdamGroup, densify.DensifyConfig, densify.DensifyGroup) == tuple(
        _abi.structs[n] for n in ("r3dg_adam_group", "r3dg_densify_config", "r3dg_densify_group"))
    assert len(_abi.constants) >= 15 and len(_abi.options) == 13
    kind = "_Generic(%s, float: 'f', int: 'i', unsigned int: 'I', unsigned long: 'L', default: 'P')"   # ctypes' own type codes
    rows = []                                                       # (what, C expression, the reader's value)
    for tag, S in _abi.structs.items():
        rows.append(("sizeof " + tag, "sizeof(%s)" % tag, C.sizeof(S)))
        for name, ctype in S._fields_:
            member, field = "((%s*)0)->%s" % (tag, name), getattr(S, name)
            rows += [("%s.%s offset" % (tag, name), "offsetof(%s, %s)" % (tag, name), field.offset),
                     ("%s.%s size" % (tag, name), "sizeof(%s)" % member, field.size),
                     ("%s.%s type" % (tag, name), kind % member, ord(ctype._type_))]
    rows += [(n, "(intptr_t)(%s)" % n, v) for n, v in _abi.constants.items()]
    rows += [("R3DG_OPT_" + n, "R3DG_OPT_" + n, i) for i, n in enumerate(_abi.options + ("COUNT",))]
    src = tmp_path / "abi_witness.c"
    src.write_text('#include <stdio.h>\n#include "r3dg_hip.h"\nint main(void) {\n%s    return 0;\n}\n' % "".join(
        '    printf("%%lld\\n", (long long)(%s));\n' % expr for _, expr, _ in rows))
    exe = str(tmp_path / "abi_witness")
    r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", _abi.HEADER.rsplit("/", 1)[0], str(src), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()
    assert [(what, int(o)) for (what, _, _), o in zip(rows, out)] == [(what, v) for what, _, v in rows] and len(out) == len(rows)


def test_type_rule_on_one_prototype_of_each_kind():
    P = _abi.prototypes
    assert P["r3dg_last_error"] == (C.c_char_p, [])
    assert P["r3dg_context_destroy"] == (None, [_p])
    assert P["r3dg_context_create"] == (_p, [])
    assert P["r3dg_geometry_state_offsets"] == (_i, [_i, C.POINTER(C.c_size_t)])
    assert P["r3dg_binning_state_bytes"] == (C.c_size_t, [C.c_int64])
    assert P["r3dg_rasterize_forward"] == (_i, [_p, _A, _A, _A, _p, _i, _i, _i, _i, _p, _i, _i] + [_p] * 6 + [_f] + [_p] * 5 +
                                           [_f] * 4 + [_i, _i] + [_p] * 8 + [_i, C.POINTER(_i)])
    assert P["r3dg_rasterize_backward_split"] == (_i, [_p] * 5 + [_f] * 3 + [_i, _f, _p, C.POINTER(_p), C.POINTER(_i),
                                                         C.POINTER(_i)])
    assert P["r3dg_context_make_current"] == (_i, [_p, C.POINTER(_p)])
    assert P["r3dg_adam_step"] == (_i, [_p, _i, _p, _f, _f, _f, _i, _f, _p])
    assert P["r3dg_profile_read"] == (_i, [C.POINTER(C.c_double), C.POINTER(_i)])
    assert P["r3dg_shade_frs_incident_chain"] == (_i, [_p, _i] + [_p] * 8 + [_f] * 5 + [_i, _f, _p, _i])


@pytest.mark.parametrize("line", [
    "int r3dg_x(struct foo f);",                            # a struct by value
    "int r3dg_y(int (*cb)(int));",                          # a function pointer that is not r3dg_alloc_fn
    "#define R3DG_Z foo",                                   # a value that is no integer expression
    "int r3dg_w(void* stream, int);",                       # a parameter without a name
    "int r3dg_v(int a[3]);",                                # an array
    "int r3dg_u(short s);",                                 # an unknown scalar
    "int r3dg_t(float* out);",                              # a pointer that is neither device memory nor a known host out-pointer
    "short r3dg_s(void);",                                  # an unknown return type
    "static inline int r3dg_r(void) { return 0; }",         # r3dg_*( outside a prototype
    "typedef struct r3dg_q { const r3dg_adam_group* g; } r3dg_q;",      # a struct field that points to another struct
])
def test_reader_fails_loudly_naming_the_line(line):
    header = open(_abi.HEADER).read()
    _abi.parse(header + "\n")                                                       # (the extra line is what raises)
    with pytest.raises(ValueError, match=r"r3dg_hip\.h:%d: " % (header.count("\n") + 1)):
        _abi.parse(header + line + "\n")
