"""include/r3dg_hip.h as ctypes: the header is the ONE declaration of the C ABI, this module reads it (once per process; neither
the built library nor a GPU is needed) and nothing in the package restates it.  The header is flat C -- prototypes, plain structs,
one enum, integer #defines -- and `parse` raises, naming the line, on anything it cannot classify: nothing defaults to a pointer.

    prototypes  {name: (restype, [argtypes])}     constants  {"R3DG_*": int}
    options     names of enum r3dg_option, in order, without R3DG_OPT_ and COUNT       structs  {"r3dg_*": ctypes.Structure}

Pointer rule: `void*`, a parameter named d_* (device memory) and a pointer to an r3dg_* struct are c_void_p; `T**` is
POINTER(c_void_p); `int* / size_t* / double* / uint64_t*` under any other name is a host out-pointer, POINTER(T); any other
pointer raises."""
import ctypes as C
import os
import re

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "r3dg_hip.h")
ALLOC_FN = C.CFUNCTYPE(C.c_void_p, C.c_void_p, C.c_size_t)
_ALLOC_FN_DECL = "typedef void* (*r3dg_alloc_fn)(void* user, size_t bytes)"

_SCALARS = {"int": C.c_int, "unsigned int": C.c_uint, "long long": C.c_longlong, "unsigned long long": C.c_ulonglong,
            "float": C.c_float, "double": C.c_double, "size_t": C.c_size_t, "int32_t": C.c_int32, "uint32_t": C.c_uint32,
            "int64_t": C.c_int64, "uint64_t": C.c_uint64, "uint8_t": C.c_uint8}
_RETURNS = dict(_SCALARS, **{"void": None, "void *": C.c_void_p, "const char *": C.c_char_p})
_HOST_POINTEES = ("int", "size_t", "double", "uint64_t")
_INT_EXPR = r"(?:0[xX][0-9a-fA-F]+|\d+|<<|>>|[\s()+\-*|&~])+"


def parse(text):
    """-> (prototypes, constants, options, structs) of a header text."""
    def fail(pos, what):
        raise ValueError("r3dg_hip.h:%d: %s" % (text.count("\n", 0, pos) + 1, what))

    def blank(m):                                   # (removed text keeps its newlines: positions stay line numbers)
        return "\n" * m.group(0).count("\n")

    def declarator(pos, decl, what):                # "const float* d_x" -> ("float", 1, "d_x")
        tok = decl.replace("*", " * ").split()
        name = tok.pop() if tok else ""
        stars = tok.count("*")
        base = " ".join(t for t in tok if t not in ("const", "*"))
        if not re.fullmatch(r"[A-Za-z_]\w*", name) or name in _SCALARS or not base or tok[len(tok) - stars:] != ["*"] * stars:
            fail(pos, "%s %r is not `type name`" % (what, decl.strip()))
        return base, stars, name

    text = re.sub(r"/\*.*?\*/", blank, text, flags=re.S)
    text = re.sub(r"^#ifdef __cplusplus\n.*?^#endif", blank, text, flags=re.S | re.M)       # (what a C compiler sees)
    prototypes, constants, structs = {}, {}, {}

    def define(m):
        name, value = m.group(1), m.group(2).strip()
        if name.startswith("R3DG_") and value:
            if name == "R3DG_SHADE_NO_ROTATION_BACK":                                       # the one pointer-valued define
                value = "-1"
            if not re.fullmatch(_INT_EXPR, value):
                fail(m.start(), "#define %s: %r is not an integer expression" % (name, value))
            constants[name] = int(eval(value, {"__builtins__": {}}))
        return ""
    text = re.sub(r"^#[ \t]*define[ \t]+(\w+)(.*)$", define, text, flags=re.M)
    text = re.sub(r"^#.*$", "", text, flags=re.M)

    def struct(m):
        fields = []
        for decl in filter(str.strip, m.group(2).split(";")):
            first, *more = decl.split(",")                                                  # `float lr, lr_tail;`
            for d in [first] + [declarator(m.start(), first, "field")[0] + " " + d for d in more]:
                base, stars, name = declarator(m.start(), d, "field")
                if stars > 1 or (base not in _SCALARS and (base, stars) != ("void", 1)):
                    fail(m.start(), "field %r: unknown type" % d.strip())
                fields.append((name, C.c_void_p if stars else _SCALARS[base]))
        structs[m.group(1)] = type(m.group(1), (C.Structure,), {"_fields_": fields})
        return blank(m)
    text = re.sub(r"typedef\s+struct\s+(r3dg_\w+)\s*\{([^{}]*)\}\s*\1\s*;", struct, text)

    enum = re.search(r"enum\s+r3dg_option\s*\{([^{}]*)\}\s*;", text)
    entries = [[s.strip() for s in e.split("=")] for e in enum.group(1).split(",")] if enum else [[""]]
    if any(not re.fullmatch(r"R3DG_OPT_[A-Z0-9_]+", e[0]) or e[1:] not in ([], [str(i)]) for i, e in enumerate(entries)) or \
            entries[-1][0] != "R3DG_OPT_COUNT":
        fail(enum.start() if enum else 0, "enum r3dg_option: expected R3DG_OPT_* numbered from 0, R3DG_OPT_COUNT last")
    options = tuple(e[0][len("R3DG_OPT_"):] for e in entries[:-1])
    text = text[:enum.start()] + blank(enum) + text[enum.end():]

    for m in re.finditer(r"\s*([^;]*[^;\s])\s*;?", text):               # every remaining statement is a prototype, or an error
        stmt, at = " ".join(m.group(1).split()), m.start(1)
        if stmt == _ALLOC_FN_DECL:
            continue
        p = re.fullmatch(r"([\w\s*]+?)\s*\b(r3dg_\w+)\s*\(([^()]*)\)", stmt)
        ret = " ".join(p.group(1).replace("*", " * ").split()) if p else None
        if ret not in _RETURNS:
            fail(at, "not a prototype this reader understands: %r" % stmt)
        args = []
        for decl in ([] if p.group(3).strip() == "void" else p.group(3).split(",")):
            base, stars, name = declarator(at, decl, p.group(2) + ": parameter")
            known = base in _SCALARS or (base == "void" and stars > 0)
            if stars == 0 and (known or base == "r3dg_alloc_fn"):
                args.append(ALLOC_FN if base == "r3dg_alloc_fn" else _SCALARS[base])
            elif stars == 2 and known:
                args.append(C.POINTER(C.c_void_p))
            elif stars == 1 and (base == "void" or base in structs or (known and name.startswith("d_"))):
                args.append(C.c_void_p)
            elif stars == 1 and base in _HOST_POINTEES:
                args.append(C.POINTER(_SCALARS[base]))
            else:
                fail(at, "%s: cannot classify parameter %r" % (p.group(2), decl.strip()))
        prototypes[p.group(2)] = (_RETURNS[ret], args)
    return prototypes, constants, options, structs


with open(HEADER) as _f:
    prototypes, constants, options, structs = parse(_f.read())
