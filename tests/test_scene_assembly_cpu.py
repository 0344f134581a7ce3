"""Scene assembly without a GPU (relightable3dgaussian_amd/ply.py, compose.py, relighting.py): the PLY header / record readers
and the column map on the reference-written fixtures (tests/golden/make_ply_golden.py), every refusal of the reader, the C ABI
declarations with their derived ctypes signatures and the library's exports, the refusals of the host mirrors (before the library
is touched), compose.assemble's host logic against a recording library (the technique of tests/test_relight_baked_cpu.py), the
SH rotation matrices and their guard, the Radiance RGBE reader, the config reader and the driver's refusals, and hipcc's
resource metadata for the new kernels."""
import contextlib
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
STAGE1, STAGE2 = (os.path.join(GOLDEN, "ply_reference_%s.ply" % t) for t in ("stage1", "stage2"))

PROTOTYPES = """\
int r3dg_scene_place_records(void* stream, int P, int A, const float* d_records, const int32_t* d_column_map,
                             const float* d_placement, int flags, long long row_offset, void** dst_groups);
int r3dg_scene_place_groups(void* stream, int P, void** src_groups, const float* d_placement, int flags,
                            long long row_offset, void** dst_groups);
int r3dg_scene_pack_records(void* stream, int P, int columns, void** src_groups, float* d_records);
"""
QUANTIZE = "int r3dg_relight_quantize(void* stream, int width, int height, int channels, const float* d_image, uint8_t* d_bytes);\n"


# ---- 1. the reader --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path,P,A", [(STAGE2, 97, 130), (STAGE1, 33, 62)])
def test_header_and_records_of_the_fixtures(path, P, A):
    from relightable3dgaussian_amd import ply
    count, names, offset = ply.read_header(path)
    assert count == P and names == ply.COLUMNS[:A]
    with open(path, "rb") as fh:
        data = fh.read()
    assert data[:offset] == ply.header_bytes(P, names) and data[offset - 11:offset] == b"end_header\n"
    rec = ply.read_records(path)
    assert rec.count == P and rec.names == names and rec.array.shape == (P, A) and rec.array.dtype == np.dtype("<f4")
    assert np.asarray(rec.array).tobytes() == data[offset:] and len(data) == offset + 4 * P * A
    cmap = ply.column_map(names)
    assert cmap.dtype == np.int32 and cmap.shape == (130,)
    assert list(cmap[:A]) == list(range(A)) and list(cmap[A:]) == [-1] * (130 - A)          # the identity for the fixtures
    assert ply.has_pbr(cmap) == (A == 130)
    z = np.load(os.path.join(GOLDEN, "ply_reference.npz"))
    tag = "stage2" if A == 130 else "stage1"
    assert list(z[tag + "_columns"]) == names
    assert np.array_equal(np.asarray(rec.array)[:, :3], z[tag + "_xyz"])
    # channel-major in the file, coefficient-major in the model: f_rest_{c*15+i} is coefficient i+1 of channel c
    assert np.array_equal(np.asarray(rec.array)[:, 9 + 1 * 15 + 4], z[tag + "_features_rest"][:, 4, 1])


def _write(path, names, body=None, count=3, fmt="binary_little_endian", before="", after_vertex="", prop="property float %s"):
    lines = ["ply", "format %s 1.0" % fmt] + ([before] if before else []) + ["element vertex %d" % count] + \
        [(prop % n) if "%s" in prop else prop for n in names] + ([after_vertex] if after_vertex else []) + ["end_header"]
    with open(path, "wb") as fh:
        fh.write(("\n".join(lines) + "\n").encode("ascii"))
        fh.write(np.zeros((count, len(names)), "<f4").tobytes() if body is None else body)
    return str(path)


def test_column_map_of_a_shuffled_file_with_extra_properties(tmp_path):
    from relightable3dgaussian_amd import ply
    rec = ply.read_records(STAGE2)
    rng = np.random.default_rng(3)
    names = list(rec.names) + ["confidence", "semantic_0"]
    body = np.concatenate([np.asarray(rec.array), rng.standard_normal((rec.count, 2)).astype("<f4")], 1)
    perm = rng.permutation(len(names))
    path = _write(tmp_path / "s.ply", [names[i] for i in perm], np.ascontiguousarray(body[:, perm]).tobytes(), rec.count)
    got = ply.read_records(path)
    cmap = ply.column_map(got.names)
    assert got.array.shape == (97, 132) and sorted(cmap) == sorted(set(range(132)) - {int(np.where(perm == 130)[0][0]),
                                                                                     int(np.where(perm == 131)[0][0])})
    assert np.array_equal(np.asarray(got.array)[:, cmap], np.asarray(rec.array))
    # the reference's degree-4 padding of visibility_rest (relighting.py:43-47): the first 15 are taken
    padded = ply.column_map(ply.COLUMNS + ["visibility_rest_%d" % i for i in range(15, 24)])
    assert list(padded) == list(range(130))


def test_reader_refusals_name_their_reason(tmp_path):
    from relightable3dgaussian_amd import ply
    S1 = ply.STAGE1_COLUMNS
    cases = [
        (_write(tmp_path / "ascii.ply", S1, fmt="ascii"), "ascii"),
        (_write(tmp_path / "big.ply", S1, fmt="binary_big_endian"), "big_endian"),
        (_write(tmp_path / "face.ply", S1, before="element face 0"), "element face 0"),
        (_write(tmp_path / "after.ply", S1, after_vertex="element face 0"), "element face 0"),
        (_write(tmp_path / "list.ply", S1, after_vertex="property list uchar int vertex_indices"), "list"),
        (_write(tmp_path / "extra.ply", S1 + ["red"]), None),
        (_write(tmp_path / "double.ply", ["x"], prop="property double %s"), "'x'"),
        (_write(tmp_path / "twice.ply", S1 + ["x"]), "'x'"),
        (_write(tmp_path / "short.ply", S1, body=np.zeros((3, 62), "<f4").tobytes()[:-5]), "truncated"),
    ]
    for path, reason in cases:
        if reason is None:
            ply.read_records(path)                                  # (an extra float property is fine)
            continue
        with pytest.raises(RuntimeError, match=reason):
            ply.read_records(path)
    with open(tmp_path / "uchar2.ply", "wb") as fh:
        fh.write(b"ply\nformat binary_little_endian 1.0\nelement vertex 1\nproperty float x\nproperty uchar red\nend_header\n")
    with pytest.raises(RuntimeError, match="red"):
        ply.read_header(str(tmp_path / "uchar2.ply"))
    with open(tmp_path / "noend.ply", "wb") as fh:
        fh.write(b"ply\nformat binary_little_endian 1.0\nelement vertex 1\nproperty float x\n")
    with pytest.raises(RuntimeError, match="end_header"):
        ply.read_header(str(tmp_path / "noend.ply"))
    with open(tmp_path / "crlf.ply", "wb") as fh:
        fh.write(b"ply\r\nformat binary_little_endian 1.0\r\nelement vertex 1\r\nproperty float x\r\nend_header\r\n")
    with pytest.raises(RuntimeError, match="newline"):
        ply.read_header(str(tmp_path / "crlf.ply"))
    with pytest.raises(RuntimeError, match="not a PLY"):
        ply.read_header(os.path.join(GOLDEN, "ply_reference.npz"))
    # the column rules
    with pytest.raises(RuntimeError, match="rot_3"):
        ply.column_map([n for n in ply.COLUMNS if n != "rot_3"])
    with pytest.raises(RuntimeError, match=r"missing: roughness$"):
        ply.column_map([n for n in ply.COLUMNS if n != "roughness"])
    with pytest.raises(RuntimeError, match="visibility_rest_14"):                          # fewer than 15 visibility_rest_*
        ply.column_map([n for n in ply.COLUMNS if n != "visibility_rest_14"])
    with pytest.raises(RuntimeError, match="at most"):
        ply.column_map(ply.COLUMNS + ["extra_%d" % i for i in range(200)])


# ---- 2. the C ABI -----------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_functions_and_the_library_exports_them():
    from relightable3dgaussian_amd import _abi, _lib
    with open(os.path.join(ROOT, "include", "r3dg_hip.h")) as fh:
        text = fh.read()
    assert PROTOTYPES in text and QUANTIZE in text
    p, i, ll, pp = C.c_void_p, C.c_int, C.c_longlong, C.POINTER(C.c_void_p)
    assert _abi.prototypes["r3dg_scene_place_records"] == (i, [p, i, i, p, p, p, i, ll, pp])
    assert _abi.prototypes["r3dg_scene_place_groups"] == (i, [p, i, pp, p, i, ll, pp])
    assert _abi.prototypes["r3dg_scene_pack_records"] == (i, [p, i, i, pp, p])
    assert _abi.prototypes["r3dg_relight_quantize"] == (i, [p, i, i, i, p, p])
    k = _abi.constants
    assert (k["R3DG_SCENE_COLUMNS"], k["R3DG_SCENE_STAGE1_COLUMNS"], k["R3DG_SCENE_GROUPS"]) == (130, 62, 13)
    assert k["R3DG_SCENE_PLACEMENT_FLOATS"] == 12 + 3 + 9 + 4 + 9 + 25 + 49
    # a 64-row tile of the widest row and the kernel's static tables fit the 64 KiB of LDS a workgroup may ask for
    assert 64 * (k["R3DG_SCENE_MAX_COLUMNS"] | 1) * 4 + 4 * (130 + k["R3DG_SCENE_PLACEMENT_FLOATS"]) <= 65536
    L = _lib.lib()
    for name in ("r3dg_scene_place_records", "r3dg_scene_place_groups", "r3dg_scene_pack_records", "r3dg_relight_quantize"):
        assert getattr(L, name) is not None
    EINVAL = k.get("R3DG_EINVAL", None)
    table = (C.c_void_p * 13)(*([1] * 13))
    # argument checks of the entry points themselves (nothing is launched: every call is refused or empty)
    assert L.r3dg_scene_place_records(None, 0, 130, None, None, None, 0, 0, None) == 0                       # empty object
    for bad in ((5, 61, 1, 1, None, 0, 0, table), (5, 251, 1, 1, None, 0, 0, table), (-1, 130, 1, 1, None, 0, 0, table),
                (5, 130, 1, 1, None, 0, -1, table), (5, 130, 1, 1, None, 2, 0, table), (5, 130, 1, 1, None, 4, 0, table),
                (5, 130, None, 1, None, 0, 0, table), (5, 130, 1, None, None, 0, 0, table), (5, 130, 1, 1, None, 0, 0, None),
                (5, 130, 2, 1, None, 0, 0, table)):
        st = L.r3dg_scene_place_records(None, *bad)
        assert st != 0 and (EINVAL is None or st == EINVAL), bad
    half = (C.c_void_p * 13)(*([1] * 9 + [None] * 4))
    assert L.r3dg_scene_place_groups(None, 5, half, None, 0, 0, table) != 0                                   # a partial PBR set
    assert L.r3dg_scene_place_groups(None, 5, table, None, 0, 0, half) != 0
    assert L.r3dg_scene_pack_records(None, 5, 100, table, 1) != 0
    stage1 = (C.c_void_p * 13)(*([1] * 7 + [None] * 6))
    assert L.r3dg_scene_pack_records(None, 5, 130, stage1, 1) != 0
    assert L.r3dg_scene_pack_records(None, 0, 62, None, None) == 0
    assert L.r3dg_relight_quantize(None, 8, 8, 5, 1, 1) != 0 and L.r3dg_relight_quantize(None, 8, 8, 3, None, 1) != 0
    assert L.r3dg_relight_quantize(None, 1 << 16, 1 << 15, 3, 1, 1) != 0 and L.r3dg_relight_quantize(None, 0, 8, 3, None, None) == 0
    assert b"scene_" in L.r3dg_last_error() or b"relight_quantize" in L.r3dg_last_error()


# ---- 3. the host mirrors ------------------------------------------------------------------------------------------------------------------
class DeviceTensor(torch.Tensor):            # a CPU tensor that claims to be a device tensor
    is_cuda = property(lambda self: True)


dt = lambda t: t.as_subclass(DeviceTensor)
z = torch.zeros


def _no_library(monkeypatch):
    from relightable3dgaussian_amd import _lib

    def lib():
        raise AssertionError("the library was touched before the arguments were refused")
    monkeypatch.setattr(_lib, "lib", lib)


def _groups(P, device=True, **replace):
    from relightable3dgaussian_amd import ply
    out = {n: (dt(z(P, *s)) if device else z(P, *s)) for n, s in ply.GROUPS}
    out.update(replace)
    return out


def test_mirrors_refuse_before_touching_the_library(monkeypatch):
    from relightable3dgaussian_amd import compose, ply, relighting
    _no_library(monkeypatch)
    P = 5
    rec, cmap = dt(z(P, 130)), dt(z(130, dtype=torch.int32))
    pl = dt(z(111))
    bad_groups = [_groups(9, device=False), _groups(9, xyz=dt(z(9, 4))), _groups(9, features_rest=dt(z(9, 3, 15))),
                  _groups(9, opacity=dt(z(9, 1, dtype=torch.float64))), _groups(9, rotation=dt(z(8, 4))),
                  _groups(9, normal=dt(z(9, 6))[:, ::2]), _groups(9, roughness=None), _groups(9, visibility_rest=dt(z(9, 24, 1)))]
    for dst in bad_groups:
        with pytest.raises(RuntimeError):
            ply.place_records(rec, cmap, dst)
        with pytest.raises(RuntimeError):
            ply.place_groups(_groups(P), dst)
    for kw in (dict(d_records=z(P, 130)), dict(d_records=dt(z(P, 61))), dict(d_records=dt(z(P, 251))), dict(d_records=dt(z(P * 130))),
               dict(d_records=dt(z(P, 130, dtype=torch.float64))), dict(d_column_map=z(130, dtype=torch.int32)),
               dict(d_column_map=dt(z(130, dtype=torch.int64))), dict(d_column_map=dt(z(62, dtype=torch.int32))),
               dict(row_offset=5), dict(row_offset=-1), dict(placement=z(111)), dict(placement=dt(z(110))),
               dict(placement=dt(z(111, dtype=torch.float64))), dict(flags=4), dict(flags=2), dict(flags=8, placement=pl)):
        args = dict(d_records=rec, d_column_map=cmap, dst=_groups(9), row_offset=0, placement=None, flags=0)
        args.update(kw)
        with pytest.raises(RuntimeError):
            ply.place_records(**args)
    for src in (_groups(P, device=False), _groups(P, base_color=None), _groups(P, scaling=dt(z(P + 1, 3))), {}):
        with pytest.raises(RuntimeError):
            ply.place_groups(src, _groups(9))
    with pytest.raises(RuntimeError):
        ply.place_groups(_groups(P), _groups(9), row_offset=5)
    stage1 = dict(_groups(P), **{n: None for n in ply.GROUP_NAMES[7:]})
    for src, cols in ((_groups(P), 100), (stage1, 130), (_groups(P, device=False), 130), (_groups(P, xyz=dt(z(P, 2))), 62)):
        with pytest.raises(RuntimeError):
            ply.pack_records(src, cols)
    for img in (z(3, 4, 4), dt(z(5, 4, 4)), dt(z(4, 4)), dt(z(3, 4, 4, dtype=torch.float64))):
        with pytest.raises(RuntimeError):
            relighting.quantize(img)
    for out in (z(4, 4, 3, dtype=torch.uint8), dt(z(3, 4, 4, dtype=torch.uint8)), dt(z(4, 4, 3))):
        with pytest.raises(RuntimeError):
            relighting.quantize(dt(z(3, 4, 4)), out)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ply.load(STAGE2, "cpu")
    with pytest.raises(RuntimeError, match="no CPU path"):
        compose.assemble([STAGE2], [torch.eye(4)], device="cpu")
    with pytest.raises(RuntimeError, match="one transform per object"):
        compose.assemble([STAGE2, STAGE1], [torch.eye(4)])
    with pytest.raises(RuntimeError, match="no xyz"):
        compose.assemble([STAGE1, {"normal": dt(z(3, 3))}], [None, None])


def test_assemble_host_logic_with_a_recording_library(monkeypatch):
    from relightable3dgaussian_amd import _lib, compose, ply
    calls, uploads, allocations = [], [], []

    class Recorder:
        def __getattr__(self, name):
            def fn(*args):
                calls.append((name, args))
                return 0
            return fn

    monkeypatch.setattr(_lib, "lib", lambda: Recorder())
    monkeypatch.setattr(_lib, "current_stream", lambda: 0)
    monkeypatch.setattr(torch.cuda, "device", lambda d: contextlib.nullcontext())
    # (the uploads are kept: assemble drops each after its launch, and the addresses compared below are only distinct while
    # both tensors live)
    placed = []
    monkeypatch.setattr(compose, "_upload_placement", lambda pl, device: placed.append(dt(pl.clone())) or placed[-1])

    def upload(records, device):
        uploads.append(records.path)
        cmap = ply.column_map(records.names)
        return dt(torch.from_numpy(np.array(records.array))), dt(torch.from_numpy(cmap)), ply.has_pbr(cmap)

    def allocate(P, device, fill=None):
        allocations.append(P)
        return {n: dt(torch.zeros(P, *s)) for n, s in ply.GROUPS}
    monkeypatch.setattr(ply, "upload", upload)
    monkeypatch.setattr(ply, "allocate_groups", allocate)

    live = {n: dt(torch.zeros(5, *s)) for n, s in ply.GROUPS[:7]}                  # a stage-1 model in memory
    handle = ply.read_records(STAGE1)
    T = [torch.eye(4), None, 2 * torch.eye(4), torch.eye(4), torch.eye(4)]
    T[2][3, 3] = 1.0
    out = compose.assemble([STAGE2, live, STAGE2, handle, STAGE1], T, rotate_sh=True, device="cuda")
    assert allocations == [97 + 5 + 97 + 33 + 33] and all(t.shape[0] == 265 for t in out.values())
    assert list(out) == list(ply.GROUP_NAMES)
    assert uploads == [STAGE2, STAGE1, STAGE1]       # the path named twice: one upload; a handle and a path are two objects
    names = [c[0] for c in calls]
    assert names == ["r3dg_scene_place_records", "r3dg_scene_place_groups", "r3dg_scene_place_records",
                     "r3dg_scene_place_records", "r3dg_scene_place_records"]            # one launch per object, nothing else
    rec = [c[1] for c in calls if c[0] == "r3dg_scene_place_records"]
    grp = [c[1] for c in calls if c[0] == "r3dg_scene_place_groups"][0]
    assert [a[7] for a in rec] == [0, 102, 199, 232] and grp[5] == 97                    # row offsets 0, P0, P0+P1, ...
    assert [a[1:3] for a in rec] == [(97, 130), (97, 130), (33, 62), (33, 62)]
    assert rec[0][3] == rec[1][3] and rec[0][4] == rec[1][4]                             # placed twice from ONE device buffer
    assert rec[0][5] is not None and rec[0][5] != rec[1][5]                              # each under its own placement
    assert [a[5] for a in rec] == [t.data_ptr() for t in placed[:4]]
    assert [a[6] for a in rec] == [3, 3, 3, 3] and grp[4] == 1 and grp[3] is None       # no transform: no SH rotation
    dst = [t.data_ptr() for t in out.values()]
    for a in rec:
        assert list(a[8]) == dst
    assert list(grp[6]) == dst and list(grp[2])[:7] == [t.data_ptr() for t in live.values()] and list(grp[2])[7:] == [None] * 6
    calls.clear()
    compose.assemble([STAGE2], [torch.eye(4)], zero_incidents=False, device="cuda")
    assert calls[0][1][6] == 0


# ---- 4. SH rotation on the host -----------------------------------------------------------------------------------------------------------
def _rotation(seed):
    rng = np.random.default_rng(seed)
    A = np.linalg.qr(rng.standard_normal((3, 3)))[0]
    return A * np.sign(np.linalg.det(A)), rng


@pytest.mark.parametrize("seed", [11, 12, 13, 14, 15])
def test_sh_rotation_matrices_satisfy_the_invariance(seed):
    from relightable3dgaussian_amd import compose
    R, rng = _rotation(seed)
    M = compose.sh_rotation_matrices(R)
    assert [m.shape for m in M] == [(3, 3), (5, 5), (7, 7)] and all(m.dtype == np.float64 for m in M)
    d = rng.standard_normal((256, 3))
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    c = rng.standard_normal(16)
    rot = c.copy()
    for (a, b), m in zip(((1, 4), (4, 9), (9, 16)), M):
        rot[a:b] = m @ c[a:b]
        assert np.abs(m @ m.T - np.eye(b - a)).max() < 1e-12                              # orthogonal, as a rotation of a band is
    assert np.abs(compose.sh_basis64(d) @ rot - compose.sh_basis64(d @ R) @ c).max() < 1e-12
    from relightable3dgaussian_amd.visibility_bake import sh_basis                       # the project's basis, the same functions
    assert np.abs(sh_basis(torch.from_numpy(d)).numpy() - compose.sh_basis64(d)).max() < 1e-15


def test_placement_layout_and_the_rotate_sh_guard():
    from relightable3dgaussian_amd import compose, relight
    R, rng = _rotation(21)
    T = torch.eye(4)
    T[:3, :3] = torch.from_numpy(R).float() * 1.7
    T[:3, 3] = torch.tensor([0.3, -1.2, 2.0])
    p = compose.placement_of(T, rotate_sh=True)
    assert p.dtype == torch.float32 and tuple(p.shape) == (111,)
    scale = T[:3, :3].norm(dim=-1)
    Rf = T[:3, :3] / scale[:, None]
    assert torch.equal(p[:12], T[:3].reshape(-1)) and torch.equal(p[12:15], scale) and torch.equal(p[15:24], Rf.reshape(-1))
    assert torch.equal(p[24:28], relight._quaternion_of(Rf[None])[0])
    M = compose.sh_rotation_matrices(Rf.double().numpy())
    assert torch.equal(p[28:], torch.from_numpy(np.concatenate([m.reshape(-1) for m in M])).float())
    assert not bool(compose.placement_of(T)[28:].any())
    shear = T.clone()
    shear[0, 1] += 0.4
    compose.placement_of(shear)                                                           # (the reference's behaviour: taken)
    stretched, squashed, mirrored = T.clone(), T.clone(), T.clone()
    stretched[:3, 1] *= 2.0                                       # non-uniform scale in the object's frame: rows no longer orthogonal
    squashed[1, :3] *= 0.5                                        # non-uniform scale in the world's frame: R stays a rotation
    mirrored[0, :3] *= -1.0                                       # a reflection: R^T R = I, det R = -1
    for bad in (shear, stretched, squashed, mirrored):
        with pytest.raises(RuntimeError, match="rotate_sh"):
            compose.placement_of(bad, rotate_sh=True)
    with pytest.raises(RuntimeError, match="rotate_sh"):
        compose.assemble([STAGE2], [shear], rotate_sh=True, device="cuda")


# ---- 5. the driver's host side --------------------------------------------------------------------------------------------------------------
def _rgbe(rng, H, W, runs):
    px = rng.integers(0, 256, (H, W, 4), dtype=np.uint8)
    px[..., 3] = rng.integers(120, 140, (H, W))
    if runs:
        px[:, 3:W // 2] = px[:, 3:4]                             # long runs in every channel
        px[0, :] = px[0, :1]                                     # a whole scanline of one value (a run longer than 127)
    px[1, 1, 3] = 0                                              # exponent 0: black
    return px


def _encode_rle(row):
    out = bytearray([2, 2, row.shape[0] >> 8, row.shape[0] & 255])
    for c in range(4):
        v, x, W = row[:, c], 0, row.shape[0]
        while x < W:
            n = 1
            while x + n < W and n < 127 and v[x + n] == v[x]:
                n += 1
            if n >= 3:
                out += bytes([128 + n, int(v[x])])
                x += n
                continue
            e = x
            while e < W and e - x < 128 and not (e + 2 < W and v[e] == v[e + 1] == v[e + 2]):
                e += 1
            out += bytes([e - x]) + bytes(v[x:e].tolist())
            x = e
    return bytes(out)


@pytest.mark.parametrize("rle", [False, True])
def test_rgbe_reader_round_trip(tmp_path, rle):
    from relightable3dgaussian_amd import relighting
    rng = np.random.default_rng(7)
    H, W = 6, 200
    px = _rgbe(rng, H, W, rle)
    body = b"".join(_encode_rle(px[y]) for y in range(H)) if rle else px.tobytes()
    assert not rle or len(body) < px.nbytes
    path = str(tmp_path / "env.hdr")
    with open(path, "wb") as fh:
        fh.write(b"#?RADIANCE\n# written by the test\nFORMAT=32-bit_rle_rgbe\n\n-Y %d +X %d\n" % (H, W) + body)
    want = px[..., :3].astype(np.float64) * np.where(px[..., 3:] > 0, np.ldexp(1.0, px[..., 3:].astype(np.int32) - 136), 0.0)
    got = relighting.read_hdr(path)
    assert got.dtype == np.float32 and got.shape == (H, W, 3) and np.array_equal(got, want.astype(np.float32))
    assert not got[1, 1].any()
    with open(path, "wb") as fh:
        fh.write(b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n-Y %d +X %d\n" % (H, W) + body[:-7])
    with pytest.raises(RuntimeError, match="scanline|run|literal"):
        relighting.read_hdr(path)


def test_config_reader_and_the_driver_refusals(tmp_path):
    from relightable3dgaussian_amd import compose, relighting
    cfg = tmp_path / "cfg"
    cfg.mkdir()
    T = np.eye(4)
    T[:3, 3] = [1, 2, 3]
    (cfg / "trajectory.json").write_text(json.dumps({"camera": {"height": 48, "width": 64, "fov": 39.6},
                                                     "trajectory": {"0": np.eye(4).reshape(-1).tolist(), "7": T.tolist()}}))
    with pytest.raises(RuntimeError, match="transform.json"):
        compose.load_scene_config(str(cfg))
    with pytest.raises(RuntimeError, match="transform.json"):
        relighting.main(["-co", str(cfg), "-e", str(tmp_path / "env.npy"), "--output", str(tmp_path / "out")])
    (cfg / "transform.json").write_text(json.dumps({"a": {"path": STAGE2, "transform": T.tolist()},
                                                    "b": {"path": STAGE2, "transform": np.eye(4).reshape(-1).tolist()}}))
    c = compose.load_scene_config(str(cfg))
    assert [(n, p) for n, p, _ in c.objects] == [("a", STAGE2), ("b", STAGE2)] and c.light_transforms is None
    assert torch.equal(c.objects[0][2], torch.from_numpy(T).float()) and (c.width, c.height) == (64, 48)
    assert [k for k, _ in c.trajectory] == ["0", "7"] and c.trajectory[1][1].dtype == np.float32
    (cfg / "light_transform.json").write_text(json.dumps({"transform": {"0": np.eye(3).tolist(), "7": np.eye(3).reshape(-1).tolist()}}))
    c = compose.load_scene_config(str(cfg))
    assert set(c.light_transforms) == {"0", "7"} and tuple(c.light_transforms["7"].shape) == (3, 3)
    with pytest.raises(RuntimeError, match=r"\.npy.*\.hdr"):
        relighting.main(["-co", str(cfg), "-e", str(tmp_path / "env.exr"), "--output", str(tmp_path / "out")])
    with pytest.raises(RuntimeError, match="points"):
        relighting.main(["-co", str(cfg), "-e", str(tmp_path / "env.npy"), "--capture_list", "pbr_env,points"])
    with pytest.raises(SystemExit):
        relighting.main(["-co", str(cfg), "-e", "x.npy", "--video"])
    cam = relighting.camera_of(T, 64, 48)
    g = np.load(os.path.join(GOLDEN, "camera_reference.npz"))
    assert cam.image_width == 64 and cam.image_height == 48 and tuple(cam.world_view_transform.shape) == (4, 4)
    assert torch.equal(cam.world_view_transform, torch.from_numpy(T).float().t())
    # the reference's Camera for the same world-to-camera matrix (tests/golden/camera_reference.npz, built as relighting.py:159-165)
    W, H = (int(v) for v in g["cam1_size"])
    ref = relighting.camera_of(g["cam1_world_view_transform"].T, W, H)
    assert np.allclose(ref.full_proj_transform.numpy(), g["cam1_full_proj_transform"], rtol=0, atol=1e-6)
    assert np.allclose(ref.camera_center.numpy(), g["cam1_camera_center"], rtol=0, atol=1e-5)
    assert abs(ref.FoVy - float(g["cam1_fovy"])) < 1e-12


# ---- 6. kernel resources --------------------------------------------------------------------------------------------------------------------
def test_the_scene_assembly_kernels_use_no_scratch_memory(tmp_path):
    """hipcc's metadata for gfx950 (read as tests/test_kernel_resources_cpu.py reads it for the hot kernels): the three instances
    of the tile kernel keep the 15 + 15 coefficients of an SH vector in registers, and the quantiser has nothing to spill."""
    from relightable3dgaussian_amd import build as B
    from tests.test_kernel_resources_cpu import _metadata
    if not os.path.exists(B.HIPCC):
        pytest.skip("no hipcc")
    _, kernels = _metadata("scene_assembly.hip", str(tmp_path))
    found = {}
    for name, (scratch, vgprs) in kernels.items():
        for key in ("scene_tile_kernelILb1ELb0", "scene_tile_kernelILb0ELb0", "scene_tile_kernelILb0ELb1", "relight_quantize_kernel"):
            if key in name:
                found[key] = (scratch, vgprs)
    assert len(found) == 4, kernels
    assert all(scratch == 0 for scratch, _ in found.values()), found
    assert all(0 < vgprs <= 128 for _, vgprs in found.values()), found          # (at least 4 waves per SIMD)
