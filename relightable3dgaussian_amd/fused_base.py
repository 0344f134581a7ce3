"""What the two fused iterations (fused_step.FusedStage2Step, fused_stage1.FusedStage1Step) share: the option context their
library calls run in, the process-wide side streams, the raw parameters and their padded gradient slab, and the host side of
the bounded rasterizer forward."""
import functools
import os

import torch

from . import _abi, _lib, rasterizer_ops

SUM_SLOTS = _abi.constants["R3DG_SUM_SLOTS"]           # floats per scalar accumulator of the glue kernels


def _in_context(method):
    """Run a step object's method inside its option context (`self._ctx`, _lib.OptionContext): the library calls it issues see
    THIS object's tuning options (CUs reserved for a collective, ...), not whatever another object of the process set last."""
    @functools.wraps(method)
    def wrapped(self, *a, **k):
        # (... and with the step's device current: the library's pooled join events belong to the CURRENT device, so a step on
        # cuda:N in a process that never called torch.cuda.set_device(N) must not record them from device 0)
        with self._ctx, torch.cuda.device(self.dev):
            return method(self, *a, **k)
    return wrapped


def _world_of(process_group):
    """-> (world size, run the data-parallel path?).  The data-parallel path (bucketed async all-reduces, reduced skip
    flag, deferred incident-light update) runs whenever the group has more than one rank -- and, for a smoke test of the
    RCCL calls on a box with ONE GPU (RCCL refuses two ranks on one device), also on a one-rank group when
    R3DG_DP_SINGLE_RANK=1: the collectives are then identities and the result must equal the plain single-GPU iteration
    up to the order of the float atomics (tests/test_fused_dp_gpu.py)."""
    td = torch.distributed
    if not (td.is_available() and td.is_initialized()):
        return 1, False
    world = td.get_world_size(process_group)
    return world, world > 1 or os.environ.get("R3DG_DP_SINGLE_RANK") == "1"


_STREAMS = {}


def shared_stream(dev, role):
    """The process's ONE side stream of `role` ("order", "early", "geometry") on `dev`, created at first use and shared by every
    step object.  torch hands out pool streams round robin and HIP maps them onto GPU_MAX_HW_QUEUES hardware queues round robin,
    so every NEW stream lands on another queue -- sooner or later on the one the main stream uses, and two streams on one queue run
    their kernels in turn (measured: a later step object in the same process 15 % slower than the first).  Step objects never run
    concurrently inside a process, so they can share the three streams the first one got."""
    dev = torch.device(dev)
    key = (dev.type, dev.index if dev.index is not None else (torch.cuda.current_device() if dev.type == "cuda" else 0), role)
    if key not in _STREAMS:
        _STREAMS[key] = torch.cuda.Stream(device=dev)
    return _STREAMS[key]


def learning_rates(lr, lrs, lr_rest_scale):
    """-> (rate, tail): the learning rate of a group / of the non-dc columns of an SH group, from the optional per-group `lrs`
    (`<group>_rest`: the non-dc columns); missing names use `lr` (`rate * lr_rest_scale` for the non-dc columns)."""
    lrs = dict(lrs or {})
    rate = lambda k: float(lrs.get(k, lr))
    tail = lambda k: float(lrs.get(k + "_rest", rate(k) * lr_rest_scale))
    return rate, tail


def grad_slab(order, tensors, dev):
    """One flat float32 gradient slab for the groups of `order`: group k holds `tensors[k].numel()` floats ("flag": the bounded
    forward's 4-float overflow flag) and starts on a 16-byte boundary (float4 accesses in the Adam kernel).
    -> (flat, {k: the group's view, shaped like tensors[k]}, {k: start offset in floats})."""
    pad4 = lambda n: (n + 3) // 4 * 4
    sizes = {k: 4 if k == "flag" else tensors[k].numel() for k in order}
    flat = torch.zeros(sum(pad4(sizes[k]) for k in order), dtype=torch.float32, device=dev)
    views, start, o = {}, {}, 0
    for k in order:
        start[k] = o
        views[k] = flat[o:o + sizes[k]] if k == "flag" else flat[o:o + sizes[k]].view_as(tensors[k])
        o += pad4(sizes[k])
    return flat, views, start


class FusedStepBase:
    """Initialised FIRST by both step classes: device, process group, option context, the raw parameters (cloned from a
    bench_core.GaussianParams-like holder) and the host side of the bounded rasterizer forward
    (r3dg_rasterize_forward_begin_bounded) -- capacity bookkeeping, the pinned ring the counts go to, and the poll that notices
    dropped views.  The subclass lays out its gradient slab (`grad_flat`, `grads`, `_flag`) and creates `opt` (a FusedAdam)."""

    _SKIP_RING = 1024

    def __init__(self, params, names, process_group, world, dp, bounded, order_stream):
        """`names`: the parameters cloned as they are (the SH colour coefficients always: `shs`, dc and rest joined).
        `world`, `dp`: what _world_of(process_group) answered.
        `order_stream`: the side stream that wrote the bounded forward's count (None: the current stream)."""
        self.dev = dev = params.xyz.device
        self.group = process_group
        self.world, self.dp = world, dp
        # tuning options of THIS object (include/r3dg_hip.h "option contexts"): every library call of the step runs inside it
        self._ctx = _lib.OptionContext()
        self._order_stream = order_stream
        for k in names:
            setattr(self, k, getattr(params, k).detach().clone().contiguous())
        self.shs = torch.cat([params.features_dc.detach(), params.features_rest.detach()], 1).contiguous()
        self.P = self.xyz.shape[0]
        self.M = self.shs.shape[1]
        self.opt = self.grad_flat = self.grads = None                            # (the subclass's)
        self.viewspace_grad = self.last_outs = self._N = None
        self.bounded = bool(bounded)
        self._flag = None                          # 4 floats inside the gradient slab (summed by the first all-reduce)
        self._capacity = None                      # instance slots of the bounded forward (None: not known yet)
        self._overflow_count = torch.zeros(1, dtype=torch.int32, device=dev)
        self._overflow_seen = 0
        self.dropped_steps = 0
        # data parallel: a step is dropped on EVERY rank when any rank's view did not fit; each rank counts those steps from
        # the reduced flag (identical everywhere), so Adam's step counts stay in lockstep
        self._skip = torch.zeros(self._SKIP_RING, 4, dtype=torch.float32, device=dev)   # snapshots of the reduced flag
        self._skip_polled = 0                      # iterations [1, _skip_polled] are accounted for
        # single GPU: iteration i's overflow flag lives in slot i mod _SKIP_RING of a ring of its own -- a launch that reads it late
        # (the incident-light group's Adam on the early stream) cannot see the NEXT iteration's tile scan overwrite it, and
        # poll_overflow can tell WHICH iterations were dropped (`dropped_iterations`: what a loop replays, see replay_dropped)
        self._flag_ring = torch.zeros(self._SKIP_RING, 4, dtype=torch.float32, device=dev)
        self._drop_polled = 0
        self.dropped_iterations = []
        self._iter = 0
        self._geom = None
        self._count_ring = torch.zeros(4096, dtype=torch.int64)                 # num_rendered of the last iterations
        if dev.type == "cuda":
            self._count_ring = self._count_ring.pin_memory()

    features_dc = property(lambda self: self.shs[:, :1])
    features_rest = property(lambda self: self.shs[:, 1:])

    def flush(self):
        """Complete deferred work of the iteration (none here)."""

    def _use_bounded(self, W, H):
        """Bounded forward for this frame?  Only once a capacity is known, and only where the library can run it (direct
        tile binning, at most 16384 tiles -- r3dg_bounded_forward_supported; a 2560x1664 view takes the exact two-phase
        forward every time instead of raising on its second iteration)."""
        if not (self.bounded and self._capacity is not None):
            return False
        # (asked every iteration: trivial host code, and the answer depends on the TILE_BINNING option, which an experiment or
        # a test may change between two frames -- a cached answer then raised instead of falling back to the two-phase forward)
        return bool(_lib.lib().r3dg_bounded_forward_supported(int(W), int(H)))

    @staticmethod
    def _capacity_for(R):
        return int(min(2 ** 31 - 1, max(2 * int(R), int(R) + (1 << 20))))

    def _end_forward_backward(self, fw, viewspace_grad, used_bounded, N):
        """The common end of forward_backward.  `fw`: what the rasterizer forward returned -- its 10 public outputs (a bounded
        forward: its CAPACITY as R, the backward's layout), then the state buffers.  -> the public outputs."""
        self.viewspace_grad, self.last_outs, self._N = viewspace_grad, tuple(fw[:10]), N
        self._note_count(fw[10], fw[0], used_bounded)
        return self.last_outs

    def _note_count(self, geom, R, used_bounded):
        """Remember the state buffer and send the count to the pinned ring without anybody waiting for it (rendered_counts)."""
        self._geom = geom
        slot = self._count_ring[(self._iter - 1) % self._count_ring.numel()]
        if used_bounded:
            count = rasterizer_ops.num_rendered_of(geom, self.P)
            if self.dev.type == "cuda":
                # (a one-thread kernel storing into the pinned slot: the runtime's 8-byte copy ran as __amd_rocclr_copyBuffer and
                # held a hardware queue for up to 128 us of the step.  On the ordering stream, which wrote the count and is idle
                # by now: 5 us that would sit between the backward and Adam)
                side = self._order_stream
                stream = side if side is not None else torch.cuda.current_stream(self.dev)
                _lib.check(_lib.lib().r3dg_store_u64_to_host(stream.cuda_stream, count.data_ptr(), slot.data_ptr()), "store_u64_to_host")
            else:
                slot.copy_(count, non_blocking=True)
        else:
            slot.fill_(int(R))
            if self.bounded:
                self._capacity = self._capacity_for(R)

    def _snapshot_flag(self):
        """(world > 1, after the all-reduce that carries the flag) this iteration's REDUCED flag, kept in a ring: what the
        iteration's Adam launches read (the slab's slot is rewritten by the next forward while a deferred update may still
        be pending) and what poll_overflow counts the dropped steps from -- one 16-byte copy, nothing else per step."""
        slot = self._skip[self._iter % self._SKIP_RING]
        slot.copy_(self._flag)
        return slot

    @_in_context
    def poll_overflow(self):
        """Did the device drop a view since the last call?  (One 4-byte read-back; synchronises.)  If THIS rank's view did
        not fit, its capacity is doubled -- at least to twice the count that did not fit; every dropped iteration (under
        data parallelism: dropped on all ranks together) is counted in `dropped_steps` and taken back from Adam's step
        count.  Returns the number of newly dropped iterations."""
        if not self.bounded or self._capacity is None:
            return 0
        count = int(self._overflow_count.item())
        new_local = count - self._overflow_seen
        if new_local > 0:
            self._overflow_seen = count
            needed = int(rasterizer_ops.num_rendered_of(self._geom, self.P).item())
            self._capacity = self._capacity_for(max(needed, self._capacity))
        new = new_local
        if new_local > 0 and not self.dp:
            # which iterations: their slots of the flag ring (older ones than the ring holds were overwritten)
            lo = max(self._drop_polled, self._iter - self._SKIP_RING)
            its = torch.arange(lo + 1, self._iter + 1, device=self.dev)
            hit = self._flag_ring[its % self._SKIP_RING, 0] != 0
            self.dropped_iterations.extend(int(i) for i in its[hit].tolist())
        self._drop_polled = self._iter
        if self.dp:
            lo = max(self._skip_polled, self._iter - self._SKIP_RING)          # (older snapshots were overwritten)
            idx = torch.arange(lo + 1, self._iter + 1, device=self.dev) % self._SKIP_RING
            new = int((self._skip[idx, 0] != 0).sum().item()) if idx.numel() else 0
            self._skip_polled = self._iter
        if new > 0:
            self.dropped_steps += new
            self.opt.step_count = max(0, self.opt.step_count - new)
        return new

    def _flag_of_iteration(self):
        """The overflow flag slot of the CURRENT iteration (call after `_iter` was advanced): the slab's slot under data
        parallelism (it is reduced with the gradients), the iteration's slot of the ring otherwise."""
        return self._flag if self.dp else self._flag_ring[self._iter % self._SKIP_RING]

    def replay_dropped(self, inputs_of):
        """Train again on the views the bounded forward dropped (VERDICT r4 missing 5: the reference sizes its binning state from
        the count it reads back and trains on EVERY view, rasterizer_impl.cu:291, train.py:114-127).  `inputs_of(iteration)` ->
        the arguments of that iteration's __call__ (iteration numbers count this object's forward_backward calls from 1).
        Every iteration poll_overflow() found dropped since the last replay runs once more through the exact two-phase forward
        (the capacity is forgotten for it: the count is read back, the state sized from it, the capacity re-learned), with its
        optimizer step.  Returns the iteration numbers replayed.  Single GPU only (under data parallelism a dropped step is
        dropped on every rank and the ranks would have to agree on the replay: poll_overflow keeps counting them)."""
        if self.dp:
            return []
        self.poll_overflow()
        todo, self.dropped_iterations = self.dropped_iterations, []
        for it in todo:
            self._capacity = None                      # two-phase forward for this view
            self(*inputs_of(it))
        if todo:
            self.dropped_steps -= len(todo)            # they are trained on after all
        return todo

    def rendered_counts(self, n=1):
        """num_rendered of the last `n` iterations (python ints, oldest first).  Synchronises: a bounded forward never
        hands the count to the host on its own; last_outs[0] is then the CAPACITY the state buffers were laid out for."""
        torch.cuda.synchronize(self.dev)
        n = max(0, min(int(n), self._iter, self._count_ring.numel()))
        return [int(self._count_ring[(self._iter - 1 - k) % self._count_ring.numel()]) for k in range(n - 1, -1, -1)]
