"""The one-launch Adam of the fused iterations (r3dg_adam_step, csrc/adam.hip): torch.optim.Adam's arithmetic over a
fixed set of tensors, every group -- or a chosen subset of them -- in ONE kernel launch."""
import ctypes as C

import torch

from . import _abi, _lib

AdamGroup = _abi.structs["r3dg_adam_group"]


class FusedAdam:
    """torch.optim.Adam semantics (no weight decay / amsgrad) over a fixed set of tensors, one kernel launch per step.
    `groups`: list of dicts {param, lr, lr_tail=None, period=0, split=0}; elements whose index modulo `period` is >= `split`
    train with `lr_tail`, resolved HERE (None -> lr).  A group with period 0 has one rate: the kernel never reads its `lr_tail`."""
    MAX_GROUPS = _abi.constants["R3DG_ADAM_MAX_GROUPS"]

    def __init__(self, groups, betas=(0.9, 0.999), eps=1e-15):
        if len(groups) > self.MAX_GROUPS:
            raise RuntimeError("FusedAdam supports at most %d groups" % self.MAX_GROUPS)
        self.groups = groups
        self.betas, self.eps = betas, eps
        self.step_count = 0
        for g in groups:
            p = g["param"]
            if not p.is_contiguous() or p.dtype != torch.float32:
                raise RuntimeError("FusedAdam needs contiguous float32 parameters")
            if g.get("lr_tail") is None:
                g["lr_tail"] = g["lr"]
            g["exp_avg"] = torch.zeros_like(p)
            g["exp_avg_sq"] = torch.zeros_like(p)

    def step(self, grads, grad_scale=1.0, skip_flag=None):
        """grads: list of gradient tensors, one per group (same order).  One launch for all groups."""
        self.begin_step()
        self.step_groups(range(len(self.groups)), grads, grad_scale, skip_flag)

    def begin_step(self):
        self.step_count += 1

    def fused_step_of(self, i, step, grad_scale=1.0, skip_flag=None):
        """The trailing arguments of an entry point whose kernel applies group i's update as step `step` itself, where the
        gradient is produced (r3dg_rasterize_backward_split's sh_adam): (group descriptor, betas, eps, step, grad_scale, skip flag).
        The descriptor names no gradient buffer; it lives until the next call."""
        g = self.groups[i]
        p = g["param"]
        self._fused_desc = AdamGroup(p.data_ptr(), None, g["exp_avg"].data_ptr(), g["exp_avg_sq"].data_ptr(), p.numel(),
                                     g["lr"], g["lr_tail"], g.get("period", 0), g.get("split", 0))
        return (C.addressof(self._fused_desc), self.betas[0], self.betas[1], self.eps, int(step), float(grad_scale),
                skip_flag.data_ptr() if skip_flag is not None else None)

    def step_groups(self, indices, grads, grad_scale=1.0, skip_flag=None):
        """Adam update of a subset of the groups for the current step (begin_step() first); `grads[i]` belongs to group i.
        Lets a data-parallel caller update each gradient bucket as soon as its all-reduce has landed.  `skip_flag`: float32
        device tensor; a non-zero first element (read on the device) turns the launch into a no-op."""
        L = _lib.lib()
        indices = list(indices)
        table = (AdamGroup * len(indices))()
        for j, i in enumerate(indices):
            g, gr = self.groups[i], grads[i]
            p = g["param"]
            if gr.shape != p.shape or not gr.is_contiguous() or gr.dtype != torch.float32:
                raise RuntimeError("FusedAdam: gradient %d does not match its parameter" % i)
            table[j] = AdamGroup(p.data_ptr(), gr.data_ptr(), g["exp_avg"].data_ptr(), g["exp_avg_sq"].data_ptr(),
                                 p.numel(), g["lr"], g["lr_tail"], g.get("period", 0), g.get("split", 0))
        with torch.cuda.device(self.groups[0]["param"].device):
            st = L.r3dg_adam_step(_lib.current_stream(), len(indices), C.cast(table, C.c_void_p), self.betas[0],
                                  self.betas[1], self.eps, self.step_count, float(grad_scale),
                                  skip_flag.data_ptr() if skip_flag is not None else None)
        _lib.check(st, "adam_step")
