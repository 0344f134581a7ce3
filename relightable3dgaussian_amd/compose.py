"""Assembly of a composite from files: scene_composition (relighting.py:28-52) without per-object tensors.

`assemble` takes the objects of a reference `transform.json` -- PLY paths, record handles (ply.read_records) or in-memory models
(dicts / namespaces of raw parameters: checkpoint.restore, a live fused step) -- allocates the composite's 13 group tensors ONCE
from the row counts and places every object with one launch (r3dg_scene_place_records / r3dg_scene_place_groups,
csrc/scene_assembly.hip): unpack through the column map, the transposes, the similarity transform of relight.transform_object and
the incident-light reset in one pass over the rows.  No per-object group tensors, no torch.cat, nothing per property on the host;
an object named twice is uploaded once and placed twice.  relight.compose_scenes / transform_object stay the oracle.

The one deliberate difference from the reference is opt-in: `rotate_sh=True` rotates bands 1..3 of the colour, incident-light
and visibility SH with the object, so that sum_i c'_i Y_i(d) = sum_i c_i Y_i(R^T d).  The reference (and the default here) leaves
the coefficients in the object's old frame."""
import functools
import json
import os
import types

import numpy as np
import torch

from . import _abi, ply, relight

ZERO_INCIDENTS = _abi.constants["R3DG_SCENE_ZERO_INCIDENTS"]
ROTATE_SH = _abi.constants["R3DG_SCENE_ROTATE_SH"]
PLACEMENT_FLOATS = _abi.constants["R3DG_SCENE_PLACEMENT_FLOATS"]
_C0, _C1 = 0.28209479177387814, 0.4886025119029199
_BANDS = ((1, 4), (4, 9), (9, 16))


def sh_basis64(d):
    """Real SH basis of degree 3 in the reference's sign convention (utils/sh_utils.py:92-127), float64: d [...,3] -> [...,16]."""
    d = np.asarray(d, np.float64)
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
    Y = [_C0 + 0 * x, -_C1 * y, _C1 * z, -_C1 * x,
         1.0925484305920792 * xy, -1.0925484305920792 * yz, 0.31539156525252005 * (2 * zz - xx - yy),
         -1.0925484305920792 * xz, 0.5462742152960396 * (xx - yy),
         -0.5900435899266435 * y * (3 * xx - yy), 2.890611442640554 * xy * z, -0.4570457994644658 * y * (4 * zz - xx - yy),
         0.3731763325901154 * z * (2 * zz - 3 * xx - 3 * yy), -0.4570457994644658 * x * (4 * zz - xx - yy),
         1.445305721320277 * z * (xx - yy), -0.5900435899266435 * x * (xx - 3 * yy)]
    return np.stack(Y, -1)


@functools.lru_cache(maxsize=None)
def _rotation_point_sets(trials=4000):
    """Per band the 2l+1 sample directions p_j and A_l^{-1}, A_l[j][i] = Y_{l,i}(p_j): the seeded search for well-conditioned
    point sets of tools/gen_sh_rotation_tables.py (same seeds, same sets as csrc/sh_rotation_tables.hpp), in float64."""
    out = []
    for a, b in _BANDS:
        rng = np.random.default_rng(100 + a)
        best = (np.inf, None)
        for _ in range(trials):
            p = rng.standard_normal((b - a, 3))
            p /= np.linalg.norm(p, axis=-1, keepdims=True)
            c = np.linalg.cond(sh_basis64(p)[:, a:b])
            if c < best[0]:
                best = (c, p)
        out.append((best[1], np.linalg.inv(sh_basis64(best[1])[:, a:b])))
    return tuple(out)


def sh_rotation_matrices(R):
    """The band-wise matrices M_1 [3,3], M_2 [5,5], M_3 [7,7] (float64) of the rotation R [3,3]: with c'_l = M_l c_l,
    sum_i c'_i Y_i(d) = sum_i c_i Y_i(R^T d) for every d.  By sampling: the band-l part of the rotated function at the points
    p_j is f_j = sum_i c_i Y_{l,i}(R^T p_j), and c'_l = A_l^{-1} f."""
    R = np.asarray(R, np.float64).reshape(3, 3)
    out = []
    for (a, b), (p, ainv) in zip(_BANDS, _rotation_point_sets()):
        B = sh_basis64(p @ R)[:, a:b]              # rows p_j R = (R^T p_j)^T
        out.append(ainv @ B)
    return out


def placement_of(transform, rotate_sh=False):
    """The R3DG_SCENE_PLACEMENT_FLOATS floats the placement kernels read for the similarity transform T [4,4] (include/r3dg_hip.h):
    the upper 3x4 of T, the per-axis scale, R and its quaternion -- computed once, in float32, with the expressions of
    relight.transform_object -- and, with `rotate_sh`, the three SH rotation matrices of R rounded to float32.  `rotate_sh`
    raises when R^T R differs from the identity by more than 1e-4 in any entry (shear, non-uniform scale in the object's frame),
    when the per-axis scales differ by more than 1e-4 (non-uniform scale in the world's frame) or when R is a reflection."""
    T = torch.as_tensor(transform, dtype=torch.float32).detach().cpu().reshape(4, 4)
    scale = T[:3, :3].norm(dim=-1)
    R = T[:3, :3] / scale[:, None]
    q = relight._quaternion_of(R[None])[0]
    out = torch.zeros(PLACEMENT_FLOATS, dtype=torch.float32)
    out[0:12], out[12:15], out[15:24], out[24:28] = T[:3].reshape(-1), scale, R.reshape(-1), q
    if rotate_sh:
        R64 = R.double().numpy()
        spread = float(scale.max() / scale.min()) - 1.0          # (a per-axis scale in the world's frame leaves R a rotation)
        if np.abs(R64.T @ R64 - np.eye(3)).max() > 1e-4 or np.linalg.det(R64) < 0 or spread > 1e-4:
            raise RuntimeError("rotate_sh: the transform's linear part is no rotation x uniform scale (R^T R - I reaches %.3g, "
                               "det R = %.3g, scale spread %.3g): SH coefficients cannot follow a shear, a non-uniform scale or "
                               "a reflection" % (np.abs(R64.T @ R64 - np.eye(3)).max(), np.linalg.det(R64), spread))
        M = sh_rotation_matrices(R64)
        out[28:] = torch.from_numpy(np.concatenate([m.reshape(-1) for m in M])).float()
    return out


def _upload_placement(placement, device):
    return placement.to(device)


def _is_path(o):
    return isinstance(o, (str, bytes)) or hasattr(o, "__fspath__")


@torch.no_grad()
def assemble(objects, transforms, rotate_sh=False, zero_incidents=True, device=None):
    """-> dict of the composite's 13 group tensors (ply.GROUP_NAMES; what compose_scenes returns for objects holding those keys),
    every object under its own 4x4 transform (None: placed as it is), rows in the order given.  `objects`: PLY paths, ply.Records
    or dicts / namespaces of device tensors, mixed freely.  The PBR groups of an object without them (a stage-1 PLY) are zero;
    `visibility_rest` keeps 15 columns.  `zero_incidents`: the incident-light reset of relighting.py:49-50."""
    if not objects or len(objects) != len(transforms):
        raise RuntimeError("assemble needs one transform per object")
    sources, counts, uses = [], [], {}
    for o in objects:
        if _is_path(o):
            key = os.path.abspath(os.fspath(o))
        elif isinstance(o, ply.Records):
            key = id(o)
        else:
            groups = ply.groups_of(o)
            if groups[0] is None:
                raise RuntimeError("assemble: an in-memory object holds no xyz")
            if device is None:
                device = groups[0].device
            sources.append(("groups", groups))
            counts.append(groups[0].shape[0])
            continue
        if key not in uses:
            rec = ply.read_records(o) if _is_path(o) else o
            ply.column_map(rec.names)                       # (refuse a bad file before anything is allocated)
            uses[key] = [0, rec, None]
        uses[key][0] += 1
        sources.append(("records", key))
        counts.append(uses[key][1].count)
    device = torch.device("cuda" if device is None else device)
    if device.type != "cuda":
        raise RuntimeError("assemble places the objects on the device; %s is no device target (there is no CPU path)" % device)
    placements = [None if t is None else placement_of(t, rotate_sh) for t in transforms]
    flags = (ZERO_INCIDENTS if zero_incidents else 0)
    out = ply.allocate_groups(sum(counts), device)
    offset = 0
    for (kind, what), n, pl in zip(sources, counts, placements):
        f = flags | (ROTATE_SH if rotate_sh and pl is not None else 0)
        d_pl = None if pl is None else _upload_placement(pl, device)
        if kind == "groups":
            ply.place_groups(what, out, offset, d_pl, f)
        else:
            entry = uses[what]
            if entry[2] is None:
                entry[2] = ply.upload(entry[1], device)[:2]           # one upload per file, however often it is placed
            ply.place_records(entry[2][0], entry[2][1], out, offset, d_pl, f)
            entry[0] -= 1
            if entry[0] == 0:
                entry[2] = None                                      # (resident: the composite + one object's records)
        offset += n
    return out


def load_scene_config(config_dir):
    """The three JSON files of a reference config directory (configs/*; relighting.py:106-112) -> namespace with `objects`
    [(name, path, transform [4,4] float32)] in file order, `width`, `height`, `trajectory` [(frame key, w2c [4,4] float32)] and
    `light_transforms` {frame key: [3,3] float32} or None (light_transform.json is optional, relighting.py:17-25)."""
    def read(name, required):
        path = os.path.join(config_dir, name)
        if not os.path.exists(path):
            if required:
                raise RuntimeError("%s: no %s in the config directory" % (config_dir, name))
            return None
        with open(path, "r", encoding="UTF-8") as fh:
            return json.load(fh)
    scene, traj, light = read("transform.json", True), read("trajectory.json", True), read("light_transform.json", False)
    objects = [(name, entry["path"], torch.tensor(entry["transform"], dtype=torch.float32).reshape(4, 4))
               for name, entry in scene.items()]
    trajectory = [(idx, np.array(cam, dtype=np.float32).reshape(4, 4)) for idx, cam in traj["trajectory"].items()]
    lights = None
    if light is not None:
        lights = {idx: torch.tensor(m, dtype=torch.float32).reshape(3, 3) for idx, m in light["transform"].items()}
    return types.SimpleNamespace(objects=objects, width=int(traj["camera"]["width"]), height=int(traj["camera"]["height"]),
                                 trajectory=trajectory, light_transforms=lights)
