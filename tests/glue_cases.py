"""Seeded inputs of the glue-kernel tests (tests/test_glue_kernels_gpu.py; checked on the CPU by tests/test_glue_reference_cpu.py):
CPU float32 tensors, crafted EDGE ROWS first, random rows behind them.

Random rows keep every decision quantity at least 64 * 2^-24 * (its own scale, from the reference) away from its threshold, so that
the kernel, the float32 yardstick and the float64 reference take the same branch; offending elements are re-drawn from the same
generator (deterministically) until none is left.  In the edge rows the decision quantity is exact by construction instead
(opacity 1 or 0 per pixel: x = F exactly; the raw value itself per Gaussian)."""
import numpy as np
import torch

from tests import glue_reference as gr

CLEAR = 64.0 * gr.U32
BG = (1.0, 0.5, 0.2)


def step32(x, k):
    """The float32 k steps above (k > 0) or below (k < 0) float32(x)."""
    v = np.float32(x)
    for _ in range(abs(k)):
        v = np.nextafter(v, np.float32(np.inf if k > 0 else -np.inf), dtype=np.float32)
    return float(v)


def clip_hi():
    """The smallest float32 x whose float64 curve is at least 16 * 2^-24 above 1 -- "the next one up" from x = 1.0 (the largest x
    whose curve is <= 1) at which the clip is DECIDED under the tolerance rule: 16 >= the n = 13 of the curve, so a kernel within
    its bound clips there too; the floats in between are inside the curve's own float32 rounding (ref32 itself still says <= 1
    at 1 + 2^-23) and would be badly conditioned inputs for the derivative."""
    x = np.float32(1.0)
    while float(gr.srgb_curve(torch.tensor(float(x), dtype=torch.float64))) < 1.0 + 16.0 * gr.U32:
        x = np.nextafter(x, np.float32(2.0), dtype=np.float32)
    return float(x)


def near(q, thresholds, scale):
    """Elements of the decision quantity q closer than CLEAR * scale to one of the thresholds."""
    bad = torch.zeros_like(q, dtype=torch.bool)
    for t in thresholds:
        bad |= (q - t).abs() < CLEAR * scale
    return bad


# ---- stage 2, per pixel -------------------------------------------------------------------------------------------------------------
def s2_edge_pixels():
    """Rows (opacity, n_contrib, F[3], image[3], gt[3]); F are the feature maps 2..4 -- with opacity 1, x = F exactly."""
    k, hi = gr.KNEE, clip_hi()
    r = [(1.0, 1, (step32(k, -1), k, step32(k, 1)), (1.0, 0.0, 0.3), (1.0, 0.0, 0.7)),          # knee; image == gt (1.0, 0.0)
         (1.0, 1, (0.0, -0.25, 0.999), (0.2, 0.4, 0.6), (0.0, 0.1, 0.9)),                       # x = 0 with srgb == gt; negative
         (1.0, 3, (1.0, hi, 4.0), (0.5, 0.5, 0.5), (0.3, 0.3, 1.0)),                            # clip; srgb == gt == 1
         (1.0, 2, (1e4, 0.5, 0.5), (0.1, 0.1, 0.1), (0.9, 0.2, 0.6)),
         (0.5, 0, (0.3, 0.2, 0.1), (0.3, 0.6, 0.9), (0.4, 0.5, 0.8))]                           # n_contrib == 0, feature != 0
    for op in (0.0, 9e-6, step32(gr.OP_MIN, -1), gr.OP_MIN, step32(gr.OP_MIN, 1), 0.5, 1.0):
        r.append((op, 5, (0.7 * op, 0.2 * op, 1.3 * op), (0.3, 0.6, 0.9), (0.4, 0.5, 0.8)))
    return r


def s2_pixels(HW, seed):
    """Inputs of r3dg_stage2_loss / _pbr_srgb / _normals_srgb's sRGB half for HW pixels.  Random rows: opacity ~ U(0,1),
    F = U(0,1.6) * opacity (21 % of the pixels clip), n_contrib = 0 on 10 %, image / gt ~ U(0,1), pseudo normal ~ unit vectors,
    the other feature maps ~ N(0,1) * opacity, soft mask ~ U(0,1), extra gradients ~ N(0,1) / HW."""
    g = torch.Generator().manual_seed(seed)
    U = lambda *s: torch.rand(*s, generator=g)
    N = lambda *s: torch.randn(*s, generator=g)
    bg = torch.tensor(BG)
    op = U(HW)
    nc = torch.where(U(HW) < 0.1, torch.zeros(HW, dtype=torch.int32), (1 + (U(HW) * 40)).to(torch.int32))
    feature = N(16, HW) * op
    feature[2:5] = U(3, HW) * 1.6 * op
    image, gt = U(3, HW), U(3, HW)
    edge = s2_edge_pixels()[:HW]
    for i, (o, n, F3, im, t) in enumerate(edge):
        op[i], nc[i] = o, n
        feature[2:5, i], image[:, i], gt[:, i] = torch.tensor(F3), torch.tensor(im), torch.tensor(t)
    ne = len(edge)
    for _ in range(100):
        bad = s2_offenders(op, feature, nc, bg)
        bad[:ne] = False
        if not bad.any():
            break
        n = int(bad.sum())
        op[bad] = U(n)
        feature[2:5, bad] = U(3, n) * 1.6 * op[bad]
    else:
        raise AssertionError("s2_pixels: could not clear the thresholds")
    pn = torch.nn.functional.normalize(N(3, HW), dim=0)
    return dict(HW=HW, n_edge=ne, image=image, opacity=op, feature=feature, pseudo=pn, n_contrib=nc, gt=gt, bg=bg, mask=U(HW),
                extra_dimage=N(3, HW) / HW, extra_dsrgb=N(3, HW) / HW)


def s2_offenders(op, feature, nc, bg):
    """Pixels with a decision quantity inside its keep-clear margin (float64 on the widened inputs)."""
    o, f, b = op.double(), feature.double(), bg.double()
    x, sx = gr.pbr_x(o, f, nc, b)
    curve = gr.srgb_curve(x)
    sc = torch.where(x > gr.KNEE, 1.055 * torch.pow(x.clamp_min(gr.KNEE), 1.0 / 2.4) + 0.055, 12.92 * sx)
    bad = near(x, (gr.KNEE,), sx).any(0) | near(curve, (0.0, 1.0), sc).any(0) | near(o, (gr.OP_MIN,), o.abs())
    return bad


# ---- stage 1, per pixel -------------------------------------------------------------------------------------------------------------
def s1_edge_pixels():
    """Rows (opacity, n_contrib, mask, D, var): the entropy clamps at every mask value, then the variance clamp (opacity 1:
    D = F3 and D2 = F4 exactly; var exactly 0, negative, well above 1e-6)."""
    r = []
    for lit in (gr.ENT_LO, gr.ENT_HI):
        for k in (-1, 0, 1):
            for m in (0.0, 0.3, 1.0):
                r.append((step32(lit, k), 4, m, 1.25, 0.5))
    r += [(1.0, 2, 1.0, 1.0, 0.0), (1.0, 2, 0.3, 1.5, -0.75), (1.0, 2, 0.0, 0.5, 3.0), (0.5, 0, 0.7, 1.0, 0.5)]
    return r


def s1_pixels(W, H, seed):
    """Inputs of r3dg_stage1_loss for a W x H image.  Random rows: opacity ~ U(0,1), n_contrib = 0 on 10 %, rendered normal ~ N(0,1),
    depth D ~ U(0.5, 2) with var = +-U(1e-4, 0.5) (either sign: a naive D2 = D^2 + s^2 flips the variance clamp on 0.2 % of the
    pixels), image / gt ~ U(0,1), pseudo normal ~ unit vectors, soft mask ~ U(0,1).  Where the image has room behind the edge rows (64 x 33 and larger) the
    rendered normals of its last 4 x 4 pixels are constant (opacity 0.5, so the division is exact): sign(G normal) = 0 over a
    3 x 3 neighbourhood at a corner, on two edges and in the interior, for the stencil adjoint."""
    HW = W * H
    g = torch.Generator().manual_seed(seed)
    U = lambda *s: torch.rand(*s, generator=g)
    N = lambda *s: torch.randn(*s, generator=g)
    op = U(HW)
    nc = torch.where(U(HW) < 0.1, torch.zeros(HW, dtype=torch.int32), (1 + (U(HW) * 40)).to(torch.int32))
    mask = U(HW)
    D = 0.5 + 1.5 * U(HW)
    var = (1e-4 + 0.5 * U(HW)) * torch.where(U(HW) < 0.5, -1.0, 1.0)
    normal = N(3, HW)
    edge = s1_edge_pixels()[:HW]
    for i, (o, n, m, d, v) in enumerate(edge):
        op[i], nc[i], mask[i], D[i], var[i] = o, n, m, d, v
    ne = len(edge)
    for _ in range(100):
        bad = near(op.double(), (gr.OP_MIN, gr.ENT_LO, gr.ENT_HI), op.double())
        bad[:ne] = False
        if not bad.any():
            break
        op[bad] = U(int(bad.sum()))
    opc = op.clamp_min(gr.OP_MIN)
    feature = torch.cat([normal * opc, (D * opc)[None], ((var + D * D) * opc)[None]], 0)
    if W >= 4 and (H - 4) * W >= ne:                  # (behind the edge rows)
        blk = torch.zeros(H, W, dtype=torch.bool)
        blk[H - 4:, W - 4:] = True
        blk = blk.reshape(-1)
        op[blk], nc[blk] = 0.5, 7
        feature[:3, blk] = torch.tensor([0.125, -0.25, 0.375])[:, None]
        feature[3, blk], feature[4, blk] = 0.5, 1.0
    for _ in range(100):                              # the variance as the kernel forms it from the float32 feature maps
        feat, _, _ = gr.divided(op.double(), feature.double(), nc)
        v64 = feat[4] - feat[3] * feat[3]
        bad = near(v64, (gr.VAR_MIN,), feat[4].abs() + feat[3] * feat[3])
        bad[:ne] = False
        if not bad.any():
            break
        feature[4, bad] = feature[4, bad] + (2e-4 * opc[bad])
    else:
        raise AssertionError("s1_pixels: could not clear the variance clamp")
    gt, image = U(3, HW), U(3, HW)
    if HW > 1:
        image[:, 1] = gt[:, 1]                        # sign(0)
    pn = torch.nn.functional.normalize(N(3, HW), dim=0)
    return dict(W=W, H=H, n_edge=ne, image=image, opacity=op, feature=feature, pseudo=pn, n_contrib=nc, gt=gt, mask=mask,
                extra_dimage=N(3, HW) / HW)


def s1_var_offenders(c):
    feat, _, _ = gr.divided(c["opacity"].double(), c["feature"].double(), c["n_contrib"])
    bad = near(feat[4] - feat[3] * feat[3], (gr.VAR_MIN,), feat[4].abs() + feat[3] * feat[3])
    bad[:c["n_edge"]] = False
    return bad


# ---- per Gaussian ------------------------------------------------------------------------------------------------------------------
SIG_RAW = [0.0, 1e-3, -1e-3, 10.0, -10.0, 17.0, -17.0, 30.0, -30.0, 90.0, -90.0, 105.0, -105.0]
SCALING_RAW = [-20.0, -10.0, -3.0, 0.0, 3.0, 10.0]
CAMPOS = (0.7, -1.1, 2.3)


def _unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v)


def gaussians(P, seed):
    """Raw parameters of P Gaussians + a camera.  Edge rows (first min(P, 13)): opacity / base / roughness raw through SIG_RAW,
    scaling raw through SCALING_RAW, the zero quaternion and quaternions of length 1e-13, 1e-6, 1e3 and with one non-zero component,
    normals of length 0, 5e-4, 2e-3, 1e3, xyz == campos and at 1e-3 from it.  Random rows: xyz ~ N(0,1), scaling raw ~ N(-3,1),
    quaternion ~ N(0,1), opacity / base / roughness raw ~ N(0,2), normal raw ~ N(0,1)."""
    g = torch.Generator().manual_seed(seed)
    N = lambda *s: torch.randn(*s, generator=g)
    a = dict(xyz=N(P, 3), scaling_raw=N(P, 3) - 3.0, rotation_raw=N(P, 4), opacity_raw=2.0 * N(P), normal_raw=N(P, 3),
             base_raw=2.0 * N(P, 3), rough_raw=2.0 * N(P))
    quats = [np.zeros(4), 1e-13 * _unit([1, -2, 3, 0.5]), 1e-6 * _unit([0.3, 1, -1, 2]), 1e3 * _unit([1, 1, -1, 0.2]), [0, 0, -0.75, 0]]
    normals = [np.zeros(3), 5e-4 * _unit([1, 2, -2]), 2e-3 * _unit([-1, 0.5, 2]), 1e3 * _unit([0.2, -1, 1])]
    ne = min(P, len(SIG_RAW))
    for i in range(ne):
        a["opacity_raw"][i] = SIG_RAW[i]
        a["rough_raw"][i] = SIG_RAW[(i + 3) % len(SIG_RAW)]
        a["base_raw"][i] = torch.tensor([SIG_RAW[(i + k) % len(SIG_RAW)] for k in (5, 6, 8)])
        a["scaling_raw"][i] = torch.tensor([SCALING_RAW[(i + k) % len(SCALING_RAW)] for k in (0, 1, 3)])
        a["rotation_raw"][i] = torch.tensor(np.asarray(quats[i % len(quats)], np.float32))
        a["normal_raw"][i] = torch.tensor(np.asarray(normals[i % len(normals)], np.float32))
    campos = torch.tensor(CAMPOS)
    a["xyz"][0] = campos
    if P > 1:
        a["xyz"][1] = campos + torch.tensor([6e-4, -6e-4, 5e-4])
    # keep the random rows' vector lengths clear of their eps
    for k, eps in (("normal_raw", gr.N_EPS), ("rotation_raw", gr.Q_EPS)):
        n = a[k].double().norm(dim=-1)
        bad = near(n, (eps,), n)
        bad[:ne] = False
        assert not bad.any()
    rot = np.asarray([[0.36, 0.48, -0.8], [-0.8, 0.6, 0.0], [0.48, 0.64, 0.6]], np.float32)
    vm = np.eye(4, dtype=np.float32)
    vm[:3, :3] = rot
    vm[3, :3] = (0.3, -0.2, 4.0)
    a.update(campos=campos, viewmatrix=torch.tensor(vm).reshape(-1), P=P, n_edge=ne)
    return a


def shade_rows(P, seed):
    """shade_out [P,19] ~ U(0,2); row 0 has three equal diffuse channels, row 1 all zeros (sign(0) of the light-smoothness L1)."""
    g = torch.Generator().manual_seed(seed)
    so = 2.0 * torch.rand(P, 19, generator=g)
    so[0, 3:6] = 0.1
    if P > 1:
        so[1, 3:6] = 0.0
    return so


def upstream(P, seed, stage2=True):
    """Upstream gradients of the activation chain rule, ~ N(0,1)."""
    g = torch.Generator().manual_seed(seed)
    N = lambda *s: torch.randn(*s, generator=g)
    up = dict(dL_dfeatures=N(P, 16 if stage2 else 5), dL_dscales=N(P, 3), dL_drot=N(P, 4), dL_dopacity=N(P), dL_dmeans3D=N(P, 3))
    if stage2:
        up.update(dL_dbase=N(P, 3), dL_drough=N(P), dL_dviewdirs=N(P, 3))
    return up


ENV_RAW_EDGE = [-30.0, 0.0, 19.999, 20.0, step32(20.0, 1), 50.0]


def env_texture(n, seed):
    """n raw texture floats ~ N(0,3), the first ones through ENV_RAW_EDGE; random ones keep clear of the softplus threshold 20."""
    g = torch.Generator().manual_seed(seed)
    raw = 3.0 * torch.randn(n, generator=g)
    ne = min(n, len(ENV_RAW_EDGE))
    raw[:ne] = torch.tensor(ENV_RAW_EDGE[:ne])
    bad = near(raw.double(), (gr.SOFT_T,), raw.double().abs())
    bad[:ne] = False
    raw[bad] = 0.25
    return raw
