"""The reference's point-cloud PLY, both ways (scene/gaussian_model.py:507-561 save_ply, :568-665 load_ply): one `vertex`
element, `format binary_little_endian 1.0`, every property `property float NAME`, 62 columns for a stage-1 model and 130 with
the PBR groups, in the order of construct_list_of_attributes (COLUMNS below).  The *_dc / *_rest columns are channel-major in
the file (f_rest_{c*15+i} is coefficient i+1 of channel c) and coefficient-major in a model ([P,15,3]).

The host side is NumPy and touches no tensor: `read_header`, `read_records` (the body as a memory-mapped [P,A] float32 array),
`column_map` (where each canonical column sits in the file).  The split into the 13 parameter groups and its inverse run on the
device (r3dg_scene_place_records / r3dg_scene_pack_records, csrc/scene_assembly.hip): `load` uploads the body once, `save`
copies the packed records to the host once.  There is no CPU split: a CPU target raises."""
import os
import types

import numpy as np

from . import _abi, _lib

STAGE1_COLUMNS = (["x", "y", "z", "nx", "ny", "nz"] + ["f_dc_%d" % i for i in range(3)] + ["f_rest_%d" % i for i in range(45)] +
                  ["opacity"] + ["scale_%d" % i for i in range(3)] + ["rot_%d" % i for i in range(4)])
PBR_COLUMNS = (["base_color_%d" % i for i in range(3)] + ["roughness"] + ["incidents_dc_%d" % i for i in range(3)] +
               ["incidents_rest_%d" % i for i in range(45)] + ["visibility_dc_0"] + ["visibility_rest_%d" % i for i in range(15)])
COLUMNS = STAGE1_COLUMNS + PBR_COLUMNS
# the 13 groups in the order of the C ABI's group tables (include/r3dg_hip.h "scene assembly"), with their per-row shapes
GROUPS = (("xyz", (3,)), ("normal", (3,)), ("features_dc", (1, 3)), ("features_rest", (15, 3)), ("opacity", (1,)),
          ("scaling", (3,)), ("rotation", (4,)), ("base_color", (3,)), ("roughness", (1,)), ("incidents_dc", (1, 3)),
          ("incidents_rest", (15, 3)), ("visibility_dc", (1, 1)), ("visibility_rest", (15, 1)))
GROUP_NAMES = tuple(n for n, _ in GROUPS)
N_STAGE1_GROUPS = 7
MAX_COLUMNS = _abi.constants["R3DG_SCENE_MAX_COLUMNS"]
assert len(COLUMNS) == _abi.constants["R3DG_SCENE_COLUMNS"] and len(STAGE1_COLUMNS) == _abi.constants["R3DG_SCENE_STAGE1_COLUMNS"]
assert len(GROUPS) == _abi.constants["R3DG_SCENE_GROUPS"]


def read_header(path):
    """-> (row count, property names in file order, byte offset of the body).  Raises RuntimeError naming the offending line for
    anything but one `vertex` element of float properties in binary little-endian."""
    def bad(n, line, why):
        return RuntimeError("%s: header line %d (%r): %s" % (path, n, line, why))
    count, names, fmt = None, [], None
    with open(path, "rb") as fh:
        first = fh.readline()
        if first.rstrip(b"\r\n") != b"ply":
            raise RuntimeError("%s: header line 1 (%r): not a PLY file" % (path, first[:40]))
        n = 1
        while True:
            raw = fh.readline()
            n += 1
            if not raw:
                raise RuntimeError("%s: the header ends at line %d without end_header" % (path, n - 1))
            try:
                line = raw.decode("ascii").rstrip("\n")
            except UnicodeDecodeError:
                raise bad(n, raw[:40], "not ASCII")
            tok = line.split()
            if not raw.endswith(b"\n") or line.endswith("\r"):
                raise bad(n, line, "header lines end in a single newline character")
            if not tok or tok[0] in ("comment", "obj_info"):
                continue
            if tok[0] == "format":
                if tok[1:] != ["binary_little_endian", "1.0"]:
                    raise bad(n, line, "only `format binary_little_endian 1.0` is read (not ascii, not big-endian)")
                fmt = tok[1]
            elif tok[0] == "element":
                if len(tok) != 3 or tok[1] != "vertex" or count is not None:
                    raise bad(n, line, "exactly one element, `vertex`, is read")
                try:
                    count = int(tok[2])
                except ValueError:
                    count = -1
                if count < 0:
                    raise bad(n, line, "bad row count")
            elif tok[0] == "property":
                if count is None:
                    raise bad(n, line, "a property before `element vertex`")
                if len(tok) > 1 and tok[1] == "list":
                    raise bad(n, line, "list properties are not read")
                if len(tok) != 3 or tok[1] not in ("float", "float32"):
                    raise bad(n, line, "every property must be `property float NAME` (property %r is not)" % (tok[-1],))
                if tok[2] in names:
                    raise bad(n, line, "property %r is declared twice" % tok[2])
                names.append(tok[2])
            elif tok[0] == "end_header":
                break
            else:
                raise bad(n, line, "unknown header keyword")
        offset = fh.tell()
    if fmt is None or count is None:
        raise RuntimeError("%s: the header has no %s line" % (path, "format" if fmt is None else "element vertex"))
    return count, names, offset


class Records:
    """The body of a PLY: `array` [P,A] little-endian float32 (a read-only memory map of the file where possible), the property
    `names` in file order and the `path` it came from."""

    def __init__(self, array, names, path=None):
        self.array, self.names, self.path = array, list(names), path

    @property
    def count(self):
        return self.array.shape[0]


def read_records(path):
    """-> Records.  Raises RuntimeError when the body is shorter than the header promises."""
    count, names, offset = read_header(path)
    A = len(names)
    have = os.path.getsize(path) - offset
    if have < count * A * 4:
        raise RuntimeError("%s: the body holds %d bytes, the header promises %d rows x %d float properties = %d (truncated file)"
                           % (path, have, count, A, count * A * 4))
    if count == 0 or A == 0:
        return Records(np.zeros((count, A), "<f4"), names, path)
    try:
        arr = np.memmap(path, dtype="<f4", mode="r", offset=offset, shape=(count, A))
    except (OSError, ValueError):
        with open(path, "rb") as fh:
            fh.seek(offset)
            arr = np.frombuffer(fh.read(count * A * 4), dtype="<f4").reshape(count, A)
    return Records(arr, names, path)


def column_map(names):
    """int32 [130]: for every canonical column (COLUMNS) its column in a file with the property `names`, -1 where absent.  The
    order in the file is free and unknown properties are skipped; the 62 stage-1 columns are required; the 68 PBR columns are all
    present or all absent (`visibility_rest_15` and up, the reference's degree-4 padding of relighting.py:43-47, are skipped)."""
    names = list(names)
    if len(set(names)) != len(names):
        raise RuntimeError("a property is named twice: %s" % sorted(n for n in set(names) if names.count(n) > 1))
    if len(names) > MAX_COLUMNS:
        raise RuntimeError("%d float properties: at most %d are read" % (len(names), MAX_COLUMNS))
    where = {n: i for i, n in enumerate(names)}
    m = np.array([where.get(n, -1) for n in COLUMNS], dtype=np.int32)
    missing = [n for n, c in zip(STAGE1_COLUMNS, m) if c < 0]
    if missing:
        raise RuntimeError("required properties are missing: %s" % ", ".join(missing))
    pbr = m[len(STAGE1_COLUMNS):]
    missing = [n for n, c in zip(PBR_COLUMNS, pbr) if c < 0]
    if missing and len(missing) != len(PBR_COLUMNS):
        raise RuntimeError("the PBR properties are all present or all absent; missing: %s" % ", ".join(missing))
    return m


def has_pbr(cmap):
    return bool(cmap[len(STAGE1_COLUMNS)] >= 0)


def _group_table(tensors):
    """13 tensors / None -> the host table of device pointers the C ABI takes."""
    import ctypes as C
    return (C.c_void_p * len(GROUPS))(*[None if t is None else t.data_ptr() for t in tensors])


def _check_groups(what, tensors, P, n_required, device=None):
    """The refusals of the host mirrors: device float32 contiguous tensors of the group shapes with P rows; entries past
    `n_required` may be None, all of them or none."""
    import torch
    rest = [t is not None for t in tensors[n_required:]]
    if len(tensors) != len(GROUPS) or (any(rest) and not all(rest)):
        raise RuntimeError("%s: 13 groups, the six PBR groups all present or all absent" % what)
    for (name, shape), t in zip(GROUPS, tensors):
        if t is None:
            if GROUP_NAMES.index(name) < n_required:
                raise RuntimeError("%s: group %s is missing" % (what, name))
            continue
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise RuntimeError("%s: group %s must be a device tensor (there is no CPU path)" % (what, name))
        if t.dtype != torch.float32 or tuple(t.shape) != (P,) + shape or not t.is_contiguous():
            raise RuntimeError("%s: group %s must be contiguous float32 %s, got %s %s" % (
                what, name, (P,) + shape, t.dtype, tuple(t.shape)))
        if device is not None and t.device != device:
            raise RuntimeError("%s: group %s is on %s, expected %s" % (what, name, t.device, device))


def allocate_groups(P, device, fill=None):
    """The 13 group tensors for P rows (uninitialised, or filled)."""
    import torch
    make = (lambda s: torch.empty(s, dtype=torch.float32, device=device)) if fill is None else \
        (lambda s: torch.full(s, float(fill), dtype=torch.float32, device=device))
    return {name: make((P,) + shape) for name, shape in GROUPS}


def upload(records, device):
    """(records tensor [P,A] on the device, column map int32 [130] on the device, has_pbr): ONE copy of the body."""
    import torch
    cmap = column_map(records.names)
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("ply: the records are split on the device; %s is no device target (there is no CPU path)" % device)
    import warnings
    with warnings.catch_warnings():                 # (a read-only memory map: the tensor over it is only ever read)
        warnings.simplefilter("ignore")
        body = torch.from_numpy(np.ascontiguousarray(records.array, dtype=np.float32))
    return body.to(device), torch.from_numpy(cmap).to(device), has_pbr(cmap)


def place_records(d_records, d_column_map, dst, row_offset=0, placement=None, flags=0):
    """r3dg_scene_place_records: rows of `d_records` [P,A] (device float32) through `d_column_map` (device int32 [130]) into
    rows [row_offset, row_offset + P) of the 13 tensors `dst` (dict or sequence in GROUPS order)."""
    import torch
    dst = [dst[n] for n in GROUP_NAMES] if isinstance(dst, dict) else list(dst)
    for what, t, dtype in (("records", d_records, torch.float32), ("column map", d_column_map, torch.int32)):
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != dtype or not t.is_contiguous():
            raise RuntimeError("place_records: the %s must be a contiguous %s device tensor" % (what, dtype))
    if d_records.dim() != 2 or not len(STAGE1_COLUMNS) <= d_records.shape[1] <= MAX_COLUMNS:
        raise RuntimeError("place_records: records must be [P,A] with %d <= A <= %d, got %s" % (
            len(STAGE1_COLUMNS), MAX_COLUMNS, tuple(d_records.shape)))
    if tuple(d_column_map.shape) != (len(COLUMNS),):
        raise RuntimeError("place_records: the column map holds %d entries" % len(COLUMNS))
    P, total = d_records.shape[0], _rows_of(dst)
    _check_placement_args("place_records", P, row_offset, total, placement, flags)
    _check_groups("place_records", dst, total, len(GROUPS), d_records.device)
    with torch.cuda.device(d_records.device):
        _lib.check(_lib.lib().r3dg_scene_place_records(
            _lib.current_stream(), P, d_records.shape[1], d_records.data_ptr(), d_column_map.data_ptr(), _lib.ptr(placement),
            int(flags), int(row_offset), _group_table(dst)), "scene_place_records")


def place_groups(src, dst, row_offset=0, placement=None, flags=0):
    """r3dg_scene_place_groups: the 13 tensors `src` of an in-memory model (the six PBR ones may all be None) into rows
    [row_offset, row_offset + P) of `dst`."""
    import torch
    src = [src.get(n) for n in GROUP_NAMES] if isinstance(src, dict) else list(src)
    dst = [dst[n] for n in GROUP_NAMES] if isinstance(dst, dict) else list(dst)
    if not src or not isinstance(src[0], torch.Tensor):
        raise RuntimeError("place_groups: group xyz is missing")
    P, total = src[0].shape[0], _rows_of(dst)
    _check_placement_args("place_groups", P, row_offset, total, placement, flags)
    _check_groups("place_groups (source)", src, P, N_STAGE1_GROUPS)
    _check_groups("place_groups", dst, total, len(GROUPS), src[0].device)
    with torch.cuda.device(src[0].device):
        _lib.check(_lib.lib().r3dg_scene_place_groups(
            _lib.current_stream(), P, _group_table(src), _lib.ptr(placement), int(flags), int(row_offset), _group_table(dst)),
            "scene_place_groups")


def pack_records(src, columns):
    """r3dg_scene_pack_records: the groups of a model -> [P,columns] records on the device (columns 62 or 130)."""
    import torch
    src = [src.get(n) for n in GROUP_NAMES] if isinstance(src, dict) else list(src)
    if columns not in (len(STAGE1_COLUMNS), len(COLUMNS)):
        raise RuntimeError("pack_records: a record holds 62 or 130 columns, not %r" % (columns,))
    if not src or not isinstance(src[0], torch.Tensor):
        raise RuntimeError("pack_records: group xyz is missing")
    P = src[0].shape[0]
    _check_groups("pack_records", src, P, N_STAGE1_GROUPS if columns == len(STAGE1_COLUMNS) else len(GROUPS))
    out = torch.empty(P, columns, dtype=torch.float32, device=src[0].device)
    with torch.cuda.device(out.device):
        _lib.check(_lib.lib().r3dg_scene_pack_records(_lib.current_stream(), P, columns, _group_table(src), out.data_ptr()),
                   "scene_pack_records")
    return out


def _rows_of(dst):
    t = dst[0] if dst else None
    if t is None or not hasattr(t, "shape") or len(t.shape) < 1:
        raise RuntimeError("the destination group xyz is missing")
    return t.shape[0]


def _check_placement_args(what, P, row_offset, total, placement, flags):
    import torch
    n = _abi.constants["R3DG_SCENE_PLACEMENT_FLOATS"]
    if row_offset < 0 or row_offset + P > total:
        raise RuntimeError("%s: rows [%d, %d) do not fit a composite of %d rows" % (what, row_offset, row_offset + P, total))
    if placement is not None and (not isinstance(placement, torch.Tensor) or not placement.is_cuda or
                                  placement.dtype != torch.float32 or tuple(placement.shape) != (n,) or
                                  not placement.is_contiguous()):
        raise RuntimeError("%s: the placement must be a contiguous float32 [%d] device tensor" % (what, n))
    if flags & ~(_abi.constants["R3DG_SCENE_ZERO_INCIDENTS"] | _abi.constants["R3DG_SCENE_ROTATE_SH"]):
        raise RuntimeError("%s: unknown flag" % what)
    if flags & _abi.constants["R3DG_SCENE_ROTATE_SH"] and placement is None:
        raise RuntimeError("%s: rotate_sh needs a placement" % what)


def load(path, device):
    """A PLY -> namespace of the 13 parameter groups on `device` under the names checkpoint.restore uses (xyz, normal,
    features_dc, features_rest, scaling, rotation, opacity, base_color, roughness, incidents_dc, incidents_rest, visibility_dc,
    visibility_rest) + `has_pbr`.  The PBR groups of a stage-1 file come back zero, as checkpoint.restore(pbr=True) returns them."""
    import torch
    if torch.device(device).type != "cuda":
        raise RuntimeError("ply.load splits the records on the device; %s is no device target (there is no CPU path)" % (device,))
    rec = read_records(path)
    d_rec, d_map, pbr = upload(rec, device)
    groups = allocate_groups(rec.count, d_rec.device)
    place_records(d_rec, d_map, groups)
    return types.SimpleNamespace(has_pbr=pbr, **groups)


def groups_of(model):
    """The 13 group tensors (contiguous; None for absent PBR groups) of a dict / namespace of raw parameters: features_dc /
    features_rest or one `shs` [P,16,3]; incidents_dc / incidents_rest or one `incidents`; visibility_dc / visibility_rest or
    one `visibility_sh` [P,16]."""
    get = (lambda k: model.get(k)) if isinstance(model, dict) else (lambda k: getattr(model, k, None))
    out = {n: get(n) for n in GROUP_NAMES}
    for joined, dc, rest in (("shs", "features_dc", "features_rest"), ("incidents", "incidents_dc", "incidents_rest")):
        j = get(joined)
        if j is not None and (out[dc] is None or out[rest] is None):
            out[dc], out[rest] = j.detach()[:, :1], j.detach()[:, 1:]
    v = get("visibility_sh")
    if v is not None and (out["visibility_dc"] is None or out["visibility_rest"] is None):
        v = v.detach().reshape(v.shape[0], 16, 1)
        out["visibility_dc"], out["visibility_rest"] = v[:, :1], v[:, 1:]
    return [None if out[n] is None else out[n].detach().contiguous() for n in GROUP_NAMES]


def header_bytes(count, names):
    lines = ["ply", "format binary_little_endian 1.0", "element vertex %d" % count] + ["property float %s" % n for n in names]
    return ("\n".join(lines + ["end_header"]) + "\n").encode("ascii")


def save(path, model):
    """A model (dict / namespace of raw parameters, see groups_of) -> the file the reference's save_ply writes for the same
    values, byte for byte: packed on the device, ONE copy to the host.  A model without the PBR groups -- or one `load` marked
    `has_pbr = False`, whose PBR groups are the zero stand-ins -- writes 62 columns."""
    src = groups_of(model)
    flag = model.get("has_pbr") if isinstance(model, dict) else getattr(model, "has_pbr", None)       # (what `load` recorded)
    pbr = all(t is not None for t in src[N_STAGE1_GROUPS:]) and flag is not False
    columns = len(COLUMNS) if pbr else len(STAGE1_COLUMNS)
    if columns == len(STAGE1_COLUMNS):
        src = src[:N_STAGE1_GROUPS] + [None] * (len(GROUPS) - N_STAGE1_GROUPS)
    body = pack_records(src, columns).cpu().numpy()
    d = os.path.dirname(os.path.abspath(path))
    os.makedirs(d, exist_ok=True)
    with open(path, "wb") as fh:
        fh.write(header_bytes(body.shape[0], COLUMNS[:columns]))
        fh.write(body.astype("<f4", copy=False).tobytes())
