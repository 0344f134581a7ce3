"""Golden PLY files, written and read back by the REFERENCE's own `GaussianModel.save_ply` / `load_ply`
(scene/gaussian_model.py:507-561, :568-665) on CPU in this container, through the `plyfile` stand-in of tools/reference_shims.py.

    python tests/golden/make_ply_golden.py      # needs the reference checkout (make_golden.REF); writes tests/golden/ply_reference*

    ply_reference_stage2.ply   P = 97, 130 columns (render_type neilf)
    ply_reference_stage1.ply   P = 33, 62 columns (render_type render)
    ply_reference.npz          the tensors load_ply produced from each file, under the names checkpoint.restore uses

The header of each file is asserted to be, line for line, what the PLY specification (and the real `plyfile`) gives for one
`vertex` element of float properties: if that ever fails the fixture is pinned to the stand-in and not to the format.
Only inputs and outputs are stored; nothing of the reference's source is copied."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import make_golden as mg  # noqa: E402  (auto-mock finder + CPU factory patches)
import make_densify_golden as mdg  # noqa: E402  (group names, attributes and shapes of the reference's model)
from tools import reference_shims  # noqa: E402

LOADED = dict(xyz="_xyz", normal="_normal", features_dc="_shs_dc", features_rest="_shs_rest", scaling="_scaling",
              rotation="_rotation", opacity="_opacity", base_color="_base_color", roughness="_roughness",
              incidents_dc="_incidents_dc", incidents_rest="_incidents_rest", visibility_dc="_visibility_dc",
              visibility_rest="_visibility_rest")


def one(GaussianModel, tag, P, stage2, seed, rec):
    from torch import nn
    g = torch.Generator().manual_seed(seed)
    render_type = "neilf" if stage2 else "render"
    m = GaussianModel(3, render_type=render_type)
    names = mdg.GROUPS_STAGE2 if stage2 else mdg.GROUPS_STAGE1
    for n in names:
        v = 0.5 * torch.randn(P, *mdg.SHAPES[n], generator=g)
        if n == "rotation":
            v = torch.nn.functional.normalize(torch.randn(P, 4, generator=g), dim=-1)
        setattr(m, mdg.ATTR[n], nn.Parameter(v.clone().requires_grad_(True)))
    path = os.path.join(HERE, "ply_reference_%s.ply" % tag)
    m.save_ply(path)
    columns = m.construct_list_of_attributes()
    expect = "\n".join(["ply", "format binary_little_endian 1.0", "element vertex %d" % P] +
                       ["property float %s" % c for c in columns] + ["end_header"]) + "\n"
    with open(path, "rb") as fh:
        data = fh.read()
    assert data[:len(expect)] == expect.encode("ascii"), "the header is not what the PLY specification gives"
    assert len(data) == len(expect) + 4 * P * len(columns), "the body is not P x columns little-endian floats"
    back = GaussianModel(3, render_type=render_type)
    back.load_ply(path)
    for ours, attr in LOADED.items():
        if stage2 or ours in ("xyz", "normal", "features_dc", "features_rest", "scaling", "rotation", "opacity"):
            rec["%s_%s" % (tag, ours)] = getattr(back, attr).detach().numpy().copy()
    rec["%s_columns" % tag] = np.array(columns)
    print("%-28s P %d, %d columns, %d KB" % (os.path.basename(path), P, len(columns), len(data) // 1024))


def main():
    sys.modules.update(reference_shims._plyfile_module())            # the functional stand-in, not the auto-mock
    sys.meta_path.append(mg._Finder())
    sys.path.insert(0, mg.REF)
    for p in mg._cpu_factories():
        p.start()
    from scene.gaussian_model import GaussianModel
    rec = {}
    one(GaussianModel, "stage2", 97, True, 61, rec)
    one(GaussianModel, "stage1", 33, False, 62, rec)
    np.savez_compressed(os.path.join(HERE, "ply_reference.npz"), **rec)


if __name__ == "__main__":
    main()
