"""r3dg_adam_step (csrc/adam.hip, csrc/adam_update.hpp) on its own: ONE step from a given float32 state, so nothing accumulates,
against the float64 restatement of torch.optim.Adam (tests/glue_reference.adam_step, pinned to torch's in
tests/test_glue_reference_cpu.py) -- parameter, exp_avg AND exp_avg_sq, every element.

Tolerance: the rule of tests/test_glue_kernels_gpu.py (|kernel - ref64| <= max(2 d, n 2^-24) scale per element, d from the float32
evaluation of the same restatement, scale = the sum of the absolute addends as adam_update forms them).  n, from adam_update:
  exp_avg     fma(1 - beta1, fma(grad_scale, g, -m), m): two fused operations, 1 - beta1 exact                       -> 4 (rounded up)
  exp_avg_sq  gk * ((1 - beta2) * gk) two products, one fma                                                          -> 4 (rounded up)
  param       v's 4 halved by the square root 2, sqrt 1, inv_sqrt_bias2 (a rounded float) and its fma 2 -> denom 5; m's 4, the
              quotient 1, lr / bias1 (bias1 a rounded float) 2, the fma 1                                            -> 14 (rounded up)

Sixteen groups (the maximum) in one launch: n = 0 first, in the middle and last; 1, 3, 4, 5 (the ragged tail of the float4 loop alone),
1023, 1024, 1025 (either side of one workgroup's 1024 floats), 4097; two groups with two rates (period 48, split 3, n no multiple of 48)
and period 0 elsewhere; one group with lr = 0.  Every array is a view 256 bytes into a canary-filled buffer of its own.
Random state: p ~ N(0,1), g ~ N(0,1), m ~ 0.1 N(0,1), v ~ 0.01 U(0,1) + 1e-6; crafted rows at the head of the 4097 group:
g = 0 with v = 0 (and m = 0), g = 1e-20, g = 1e18, m and g of opposite sign, v large with g small."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import glue_reference as gr
from tests.helpers import report_elementwise

pytestmark = pytest.mark.gpu
DEV = "cuda"
CANARY = -7.5
PAD = 64
BETA1, BETA2, EPS = gr.f32(0.9), gr.f32(0.999), gr.f32(1e-15)
SIZES = [0, 1, 3, 4, 5, 1023, 1024, 0, 1025, 4097, 50, 1, 5, 1023, 100, 0]
TWO_RATE = (10, 14)
LR_ZERO = 8
N_OUT = {"param": 14, "exp_avg": 4, "exp_avg_sq": 4}
_STATE = {}


def _state():
    """The sixteen groups' float32 state (numpy), computed once and never modified."""
    if not _STATE:
        rng = np.random.RandomState(7)
        groups = []
        for i, n in enumerate(SIZES):
            g = dict(n=n, p=rng.randn(n), g=rng.randn(n), m=0.1 * rng.randn(n), v=0.01 * rng.rand(n) + 1e-6,
                     lr=np.float32(0.0 if i == LR_ZERO else 1e-3 * (1 + i)), period=48 if i in TWO_RATE else 0, split=3 if i in TWO_RATE else 0)
            g["lr_tail"] = np.float32(g["lr"] / 20) if i in TWO_RATE else np.float32(123.0)       # (period 0: the tail rate is ignored)
            if n == 4097:
                g["g"][:5] = [0.0, 1e-20, 1e18, -0.7, 1e-6]
                g["m"][:5] = [0.0, 0.05, 0.05, 0.4, 0.05]
                g["v"][:5] = [0.0, 0.01, 0.01, 0.01, 1e6]
            for k in "pgmv":
                g[k] = g[k].astype(np.float32)
            groups.append(g)
        _STATE["groups"] = groups
    return _STATE["groups"]


class Buf:
    def __init__(self, a):
        self.n = a.size
        self.big = torch.full((self.n + 2 * PAD,), CANARY, device=DEV)
        self.t = self.big[PAD:PAD + self.n]
        self.t.copy_(torch.from_numpy(a))
        assert self.t.data_ptr() % 16 == 0 and self.t.data_ptr() != self.big.data_ptr()

    def cpu(self):
        torch.cuda.synchronize()
        big = self.big.cpu()
        assert bool((big[:PAD] == CANARY).all()) and bool((big[-PAD:] == CANARY).all()), "canary overwritten"
        return big[PAD:PAD + self.n].numpy()


def _launch(groups, step, grad_scale, skip=None):
    from relightable3dgaussian_amd import _lib
    from relightable3dgaussian_amd.fused_adam import AdamGroup
    bufs = [{k: Buf(g[k]) for k in "pgmv"} for g in groups]
    table = (AdamGroup * len(groups))()
    for j, (g, b) in enumerate(zip(groups, bufs)):
        table[j] = AdamGroup(b["p"].t.data_ptr(), b["g"].t.data_ptr(), b["m"].t.data_ptr(), b["v"].t.data_ptr(), g["n"], float(g["lr"]),
                             float(g["lr_tail"]), g["period"], g["split"])
    flag = None if skip is None else torch.tensor([skip], device=DEV)
    _lib.check(_lib.lib().r3dg_adam_step(_lib.current_stream(), len(groups), C.cast(table, C.c_void_p), BETA1, BETA2, EPS, step,
                                         float(grad_scale), None if flag is None else flag.data_ptr()), "adam_step")
    return [{k: b[k].cpu().copy() for k in "pgmv"} for b in bufs]


def _reference(g, step, grad_scale, dtype):
    lr = gr.adam_rates(g["n"], np.float64(g["lr"]), np.float64(g["lr_tail"]), g["period"], g["split"])
    return gr.adam_step(*(g[k].astype(dtype) for k in "pgmv"), lr.astype(dtype), BETA1, BETA2, EPS, step, grad_scale)


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


@pytest.mark.parametrize("grad_scale", [1.0, 0.5])
@pytest.mark.parametrize("step", [1, 2, 7, 1000, 100000])
def test_adam_step_matches_float64_adam(step, grad_scale):
    groups = _state()
    got = _launch(groups, step, grad_scale)
    for i, (g, out) in enumerate(zip(groups, got)):
        assert np.array_equal(_bits(out["g"]), _bits(g["g"])), "group %d: the gradient was written" % i
        if g["n"] == 0:
            continue
        r64, r32 = _reference(g, step, grad_scale, np.float64), _reference(g, step, grad_scale, np.float32)
        for name, key in (("param", "p"), ("exp_avg", "m"), ("exp_avg_sq", "v")):
            d, bound = gr.tolerance(r64[name][0], r32[name][0], r64[name][1], N_OUT[name])
            tag = "adam step=%d gs=%g group %d (n=%d) %s" % (step, grad_scale, i, g["n"], name)
            ok, msg = report_elementwise(tag, out[key], r64[name][0], bound)
            print("%s  d %.2e  n %d  %s" % (tag, d, N_OUT[name], msg.split("max err/bound", 1)[-1].strip()))
            assert d < 1e-5, "%s: badly conditioned case, d = %.3e" % (tag, d)
            assert ok, msg
        if i == LR_ZERO:
            assert np.array_equal(_bits(out["p"]), _bits(g["p"])), "lr = 0: the parameter must stay bit for bit"
            assert not np.array_equal(out["m"], g["m"]) and not np.array_equal(out["v"], g["v"]), "lr = 0: the moments still advance"
        if g["n"] == 4097:
            assert out["p"][0] == g["p"][0] and out["m"][0] == 0.0 and out["v"][0] == 0.0, "g = 0, m = 0, v = 0 must stay put"


def test_adam_step_with_only_empty_groups_is_a_no_op():
    got = _launch([g for g in _state() if g["n"] == 0] * 5 + [_state()[0]], 3, 1.0)
    assert len(got) == 16 and all(o["p"].size == 0 for o in got)


@pytest.mark.parametrize("flag", [0.0, 1.0, float("nan")])
def test_adam_step_skip_flag(flag):
    """*d_skip_flag == 0 updates exactly as without a flag; 1.0 and NaN leave all three arrays bit for bit."""
    groups = _state()
    got = _launch(groups, 7, 1.0, skip=flag)
    want = _launch(groups, 7, 1.0) if flag == 0.0 else groups
    for g, out, w in zip(groups, got, want):
        for k in "pmv":
            assert np.array_equal(_bits(out[k]), _bits(w[k])), (flag, g["n"], k)
