"""The inputs of the fused image-tail test (tests/image_tail_cases.py) deliver what tests/test_image_tail_gpu.py relies on, checked
without a GPU: on every pixel of every case the float32 and the float64 restatement take the same decisions (the sRGB knee and
clip, the 1e-5 opacity clamp, n_contrib > 0, the signs of image - gt and srgb - gt) -- no pixel is exempt from any comparison of
the GPU test, so the generator has to deliver that on its own --; the crafted pixels and the blocks are where the docstring says; and
the composed reference is well conditioned: d = max |ref32 - ref64| / scale stays below the 1e-5 the tolerance rule asks for, for
every output (the pseudo normals are the oracle path's here, the kernel's in the GPU test)."""
import numpy as np
import pytest
import torch

from tests import glue_cases as gc
from tests import glue_reference as gr
from tests import image_tail_cases as tc
from tests import stencil_cases as sc


def test_shapes_cover_the_ssim_shapes_and_the_tile_seams():
    assert all(s in tc.SHAPES for s in sc.SSIM_SHAPES)
    T = tc.TILE
    assert all(s in tc.SHAPES for s in [(T + 11, 11), (11, T + 11), (2 * T + 1, 6), (6, 2 * T + 6)])
    assert len(set(tc.SHAPES)) == len(tc.SHAPES)


@pytest.mark.parametrize("W,H", tc.SHAPES)
def test_both_precisions_take_the_same_decisions_at_every_pixel(W, H):
    c = tc.tail_case(W, H)
    d32, d64 = tc.decisions(c, torch.float32), tc.decisions(c, torch.float64)
    for k in d64:
        assert torch.equal(d32[k], d64[k]), "%dx%d: %s differs at %d elements" % (W, H, k, int((d32[k] != d64[k]).sum()))
    assert not bool(tc._pbr_sign_offenders(c)[:, :c["HW"] - c["n_edge"]].any())
    # and the kernel's own form of them: lin = x <= knee, unclipped = 0 <= curve <= 1 -- the complements of the above
    assert c["image"].dtype == c["gt"].dtype == c["opacity"].dtype == c["feature"].dtype == torch.float32


@pytest.mark.parametrize("W,H", tc.SHAPES)
def test_crafted_pixels_and_blocks_are_in_place(W, H):
    c = tc.tail_case(W, H)
    HW, ne = c["HW"], c["n_edge"]
    edge = gc.s2_edge_pixels()[:HW]
    assert ne == len(edge)
    for i, (o, n, F3, im, t) in enumerate(edge):
        p = HW - ne + i
        assert float(c["opacity"][p]) == gr.f32(o) and int(c["n_contrib"][p]) == n
        assert torch.equal(c["feature"][2:5, p], torch.tensor(F3)) and torch.equal(c["image"][:, p], torch.tensor(im))
        assert torch.equal(c["gt"][:, p], torch.tensor(t))
    blocks = sc.ssim_blocks(W, H)
    if blocks and HW - ne >= W * 16:              # block 0 in the zero-padded corner: image and target exactly 0
        x0, y0 = blocks[0]
        rows = min(16, (HW - ne) // W)
        assert not c["image"].reshape(3, H, W)[:, y0:y0 + rows, x0:x0 + 16].any()
    # every kind of decision occurs in the larger cases
    if HW >= 300:
        d = tc.decisions(c, torch.float64)
        assert d["knee"].any() and (~d["knee"]).any() and d["clip_high"].any() and (~d["covered"]).any()
        assert (d["sign_pbr"] == 0).any() and (d["sign_pbr"] > 0).any() and (d["sign_pbr"] < 0).any()


def _pseudo(c):
    from oracle import torch_rasterizer as trz
    W, H = c["W"], c["H"]
    n, _ = trz.pseudo_normal(c["opacity"].reshape(1, H, W), c["depth"].reshape(1, H, W), c["viewmatrix"].reshape(4, 4),
                             W / (2.0 * tc.TAN_FOVX), H / (2.0 * tc.TAN_FOVY), c["cx"], c["cy"])
    return n.reshape(3, W * H).float()


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("W,H", tc.SHAPES)
def test_composed_reference_is_well_conditioned(W, H, masked):
    c = tc.tail_case(W, H)
    s0, s1 = sc.ssim_scales(W, H, 3)
    args = (W, H, c["image"], c["opacity"], c["feature"], _pseudo(c), c["n_contrib"], c["gt"], c["bg"],
            c["mask"] if masked else None) + tc.weights(W, H) + (s0, s1)
    r64, r32 = tc.tail_reference(*gr.widen(args, torch.float64)), tc.tail_reference(*args)
    assert sorted(r64) == ["dL_dfeature", "dL_dimage", "dL_dopacity", "ssim_image", "ssim_pbr", "sum_l1", "sum_normal", "sum_pbr"]
    for k in r64:
        v64, s64 = (np.asarray(t.detach().double()) for t in r64[k])
        d, _ = gr.tolerance(v64, np.asarray(r32[k][0].detach().double()), s64, 1)
        assert d < 1e-5, "%dx%d %s: d = %.3e" % (W, H, k, d)
        assert np.isfinite(v64).all() and (s64 >= 0).all()
    # the two SSIM terms pull with opposite signs, and both reach their gradients
    assert s0 > 0 > s1
    assert bool((r64["dL_dimage"][0].abs() > 0).any()) and bool((r64["dL_dfeature"][0][2:5].abs() > 0).any())
