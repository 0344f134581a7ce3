"""r3dg_shade_frs_incident_chain with R3DG_CHAIN_NO_GRADIENT_OUT (FixedRaySet.incident_chain(write_gradient=False)): the chain
kernel of a whole single-GPU iteration keeps the rotated-back gradient row on chip.  The two instantiations differ in ONE store,
so everything else they write is compared bit for bit: the updated coefficients, both moments and the rotated new coefficients.
The gradient buffer is pre-filled with a sentinel; with the write off it comes back untouched -- also on the rows of the
Gaussians off the rotated path (valid == 0), whose world-frame gradient the kernel READS from that buffer in place."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
K = 16
# one Gaussian; a wave's 64 Gaussians minus one, exactly, plus one; more than one 256-Gaussian workgroup
SIZES = (1, 63, 64, 65, 257)
# normals on and next to -z, where the rotation into the ray frame is ill-conditioned: those Gaussians are off the rotated path
OFF_PATH = ((0.0, 0.0, -1.0), (1e-4, 0.0, -1.0), (0.0, 3e-3, -1.0))


@pytest.mark.parametrize("P", SIZES)
def test_chain_without_the_gradient_row_writes_everything_else_bit_for_bit(P):
    from relightable3dgaussian_amd import sampling
    from relightable3dgaussian_amd import shading_ops as so
    g = torch.Generator().manual_seed(11 * P)
    rnd = lambda *sh: torch.randn(*sh, generator=g).to(DEV)
    normals = torch.nn.functional.normalize(rnd(P, 3), dim=-1)
    if P > 1:       # (rows 1.., the last one included when it fits: the ragged tail of a wave)
        rows = [1, min(P - 1, 40), P - 1][:len(OFF_PATH)]
        normals[rows] = torch.nn.functional.normalize(torch.tensor(OFF_PATH, device=DEV), dim=-1)[:len(rows)]
    dirs, _areas = sampling.fibonacci_sphere_sampling(normals, K)
    frs = so.FixedRaySet.try_build(normals, dirs)
    assert frs is not None and so.FixedRaySet.chain_gradient_optional
    off = frs.valid[:P] == 0
    # (which of the three the classifier takes off the rotated path is its threshold's business: at least one, not all rows)
    assert P == 1 or (frs.n_invalid >= 1 and int(off.sum()) == frs.n_invalid and bool((~off).any())), \
        "the fixture needs rows on and off the rotated path"
    inc0, m0, v0 = 0.3 * rnd(P, 16, 3), 0.01 * rnd(P, 16, 3), (0.01 * rnd(P, 16, 3)) ** 2
    dcp, sentinel = rnd(P, 16, 3), rnd(P, 16, 3) + 100.0
    lr, lr_tail, betas, eps, step = 1e-3, 1e-4, (0.9, 0.999), 1e-15, 3

    def run(write):
        frs.dcprime.copy_(dcp.reshape(P, 48))
        frs.cprime.fill_(float("nan"))
        inc, m, v, grad = inc0.clone(), m0.clone(), v0.clone(), sentinel.clone()
        frs.incident_chain(inc, grad, m, v, lr, lr_tail, betas, eps, step, write_gradient=write)
        torch.cuda.synchronize()
        return inc, m, v, frs.cprime[:P].clone(), grad
    inc_w, m_w, v_w, cp_w, grad_w = run(True)
    inc_n, m_n, v_n, cp_n, grad_n = run(False)
    assert not torch.equal(inc_w, inc0) and bool(torch.isfinite(cp_w).all())
    for name, a, b in (("incidents", inc_w, inc_n), ("exp_avg", m_w, m_n), ("exp_avg_sq", v_w, v_n), ("cprime", cp_w, cp_n)):
        assert torch.equal(a, b), "%s differs by up to %.3e" % (name, float((a - b).abs().max()))
    assert torch.equal(grad_n, sentinel), "the gradient buffer was written although the write is off"
    # with the write on: the rotated rows are replaced, the rows read in place are written back as they were
    assert torch.equal(grad_w[off], sentinel[off])
    if bool((~off).any()):
        assert not bool((grad_w[~off] == sentinel[~off]).any())
    # the rows off the rotated path DID drive their update from the buffer: another buffer, another update on exactly those rows
    if bool(off.any()):
        frs.dcprime.copy_(dcp.reshape(P, 48))
        inc2, m2, v2 = inc0.clone(), m0.clone(), v0.clone()
        frs.incident_chain(inc2, (sentinel + 1.0), m2, v2, lr, lr_tail, betas, eps, step, write_gradient=False)
        torch.cuda.synchronize()
        assert torch.equal(m2[~off], m_n[~off]) and not bool((m2[off] == m_n[off]).any())
    # a dropped view: nothing moves, with the write off as with it on
    flag = torch.ones(1, device=DEV)
    inc3, m3, v3, grad3 = inc0.clone(), m0.clone(), v0.clone(), sentinel.clone()
    frs.incident_chain(inc3, grad3, m3, v3, lr, lr_tail, betas, eps, step, skip_flag=flag, write_gradient=False)
    torch.cuda.synchronize()
    assert torch.equal(inc3, inc0) and torch.equal(m3, m0) and torch.equal(v3, v0) and torch.equal(grad3, sentinel)
