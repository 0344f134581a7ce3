"""Fused stage-2 training iteration: the same computation as train_step.Stage2Step + loss.backward()
+ Adam, but with the ~250 elementwise PyTorch launches around the hot ops replaced by the streaming HIP kernels of
csrc/stage2_glue.hip and without an autograd graph: forward, loss, backward and optimizer are explicit calls in order.

    GaussianModel activations + viewdirs,     r3dg_stage2_activate_with        (scene/gaussian_model.py:183-232, neilf.py:74-76,
      softplus of the env texture, sum reset                                      direct_light_map.py:18-27)
    shading integral                          r3dg_shade_frs_forward (fixed ray set) / r3dg_shade_forward_cached (neilf.py:339-371)
    S=16 feature row + light-smoothness sum   written by the two launches above; r3dg_stage2_pack_features behind the general
                                              shading kernel                   (neilf.py:115-122, 286-292)
    rasterize                                 r3dg_rasterize_forward_*         (r3dg_rasterization.py:75-113)
    pseudo normals + sRGB-mapped PBR image    r3dg_stage2_normals_srgb
    SSIM of the image and the PBR image       r3dg_ssim_forward_pair / r3dg_ssim_backward_pair
    image-space loss terms + their gradients  r3dg_stage2_loss (+ r3dg_stage2_smooth_fused)  (neilf.py:212-318)
    rasterize backward                        r3dg_rasterize_backward_*
    feature grads -> shading upstream grads   r3dg_stage2_unpack_gradients
    shading backward                          r3dg_shade_frs_backward / r3dg_shade_backward_cached
    activation chain rule -> parameter grads, r3dg_stage2_activate_backward_with  (neilf.py:294-300)
      env texture: softplus' + TV term
    Adam, all groups in one launch            r3dg_adam_step                   (gaussian_model.py:465-497); the incident-light
                                              group on the fixed ray set: r3dg_shade_frs_incident_chain

The SH colour coefficients and the incident-light coefficients are each held as ONE [P,16,3] tensor (the reference
concatenates features_dc / features_rest and incidents_dc / incidents_rest every iteration, gaussian_model.py:199-203);
`features_dc` etc. are exposed as views, and the Adam kernel applies the dc / rest learning rates by column.
The parity target is the unfused path (tests/test_fused_step_gpu.py compares loss and every gradient)."""
import ctypes as C
import os

import torch
import torch.nn.functional as F

from . import _lib, rasterizer_ops, shading_ops
from .train_step import FROZEN_GEOMETRY_GROUPS, LAMBDA_DSSIM, STAGE2_WEIGHTS, update_visibility

SUM_SLOTS = 32           # R3DG_SUM_SLOTS (include/r3dg_hip.h): floats per scalar accumulator of the glue kernels


class AdamGroup(C.Structure):
    _fields_ = [("param", C.c_void_p), ("grad", C.c_void_p), ("exp_avg", C.c_void_p), ("exp_avg_sq", C.c_void_p),
                ("n", C.c_uint64), ("lr", C.c_float), ("lr_tail", C.c_float), ("period", C.c_uint32),
                ("split", C.c_uint32)]


def _in_context(method):
    """Run a step object's method inside its option context (`self._ctx`, _lib.OptionContext): the library calls it issues see
    THIS object's tuning options (CUs reserved for a collective, ...), not whatever another object of the process set last."""
    import functools

    @functools.wraps(method)
    def wrapped(self, *a, **k):
        ctx = getattr(self, "_ctx", None)
        if ctx is None:
            return method(self, *a, **k)
        # (... and with the step's device current: the library's pooled join events belong to the CURRENT device, so a step on
        # cuda:N in a process that never called torch.cuda.set_device(N) must not record them from device 0)
        with ctx, torch.cuda.device(self.dev):
            return method(self, *a, **k)
    return wrapped


def _fake_comm_gbs():
    v = os.environ.get("R3DG_DP_FAKE_COMM_GBS")
    return float(v) if v else None


class _FakeCommHandle:
    """What torch.distributed's Work is to the callers of _allreduce_async: wait() orders the current stream behind the
    (priced) end of the collective."""

    def __init__(self, event, begin=None):
        self.event, self.begin = event, begin

    def wait(self):
        torch.cuda.current_stream().wait_event(self.event)

    def _get_duration(self):
        """ms the priced collective held the communication stream (same name as torch.distributed.Work's)."""
        if self.begin is None:
            raise RuntimeError("the priced collective was not timed")
        return self.begin.elapsed_time(self.event)


class FusedAdam:
    """torch.optim.Adam semantics (no weight decay / amsgrad) over a fixed set of tensors, one kernel launch per step.
    `groups`: list of dicts {param, grad (callable or tensor), lr, lr_tail=None, period=0, split=0}."""
    MAX_GROUPS = 16

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
            g["exp_avg"] = torch.zeros_like(p)
            g["exp_avg_sq"] = torch.zeros_like(p)

    def step(self, grads, grad_scale=1.0, skip_flag=None):
        """grads: list of gradient tensors, one per group (same order).  One launch for all groups."""
        self.begin_step()
        self.step_groups(range(len(self.groups)), grads, grad_scale, skip_flag)

    def begin_step(self):
        self.step_count += 1

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
                                 p.numel(), g["lr"], g.get("lr_tail") if g.get("lr_tail") is not None else g["lr"],
                                 g.get("period", 0), g.get("split", 0))
        with torch.cuda.device(self.groups[0]["param"].device):
            st = L.r3dg_adam_step(_lib.current_stream(), len(indices), C.cast(table, C.c_void_p), self.betas[0],
                                  self.betas[1], self.eps, self.step_count, float(grad_scale),
                                  skip_flag.data_ptr() if skip_flag is not None else None)
        _lib.check(st, "adam_step")


PARAM_NAMES = ("xyz", "normal", "scaling", "rotation", "opacity", "shs", "base_color", "roughness", "incidents", "env")


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


class _BoundedForward:
    """Host side of the bounded rasterizer forward (r3dg_rasterize_forward_begin_bounded), shared by the fused iterations:
    capacity bookkeeping, the pinned ring the counts go to, and the poll that notices dropped views."""

    def _init_bounded(self, bounded, flag):
        self.bounded = bool(bounded)
        self._flag = flag                          # 4 floats inside the gradient slab (summed by the first all-reduce)
        self._capacity = None                      # instance slots of the bounded forward (None: not known yet)
        self._bounded_ok = {}                      # (W, H) -> the library can run the bounded forward at this size
        self._overflow_count = torch.zeros(1, dtype=torch.int32, device=self.dev)
        self._overflow_seen = 0
        self.dropped_steps = 0
        # data parallel: a step is dropped on EVERY rank when any rank's view did not fit; each rank counts those steps from
        # the reduced flag (identical everywhere), so Adam's step counts stay in lockstep
        self._skip = torch.zeros(self._SKIP_RING, 4, dtype=torch.float32, device=self.dev)   # snapshots of the reduced flag
        self._skip_polled = 0                      # iterations [1, _skip_polled] are accounted for
        # single GPU: iteration i's overflow flag lives in slot i mod _SKIP_RING of a ring of its own -- a launch that reads it late
        # (the incident-light group's Adam on the early stream) cannot see the NEXT iteration's tile scan overwrite it, and
        # poll_overflow can tell WHICH iterations were dropped (`dropped_iterations`: what a loop replays, see replay_dropped)
        self._flag_ring = torch.zeros(self._SKIP_RING, 4, dtype=torch.float32, device=self.dev)
        self._drop_polled = 0
        self.dropped_iterations = []
        self._flag_cur = flag
        self._iter = 0
        self._geom = None
        self._count_ring = torch.zeros(4096, dtype=torch.int64)                 # num_rendered of the last iterations
        if self.dev.type == "cuda":
            self._count_ring = self._count_ring.pin_memory()

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

    def _note_count(self, geom, R, used_bounded):
        """After a forward: remember the state buffer and send the count to the ring without waiting for it."""
        self._geom = geom
        slot = self._count_ring[(self._iter - 1) % self._count_ring.numel()]
        if used_bounded:
            # (on the ordering stream, which wrote the count and is idle by now: 5 us that would sit between the backward and Adam)
            side = getattr(self, "_order_stream", None)
            count = rasterizer_ops.num_rendered_of(geom, self.P)
            if self.dev.type == "cuda":
                # (a one-thread kernel storing into the pinned slot: the runtime's 8-byte copy ran as __amd_rocclr_copyBuffer and
                # held a hardware queue for up to 128 us of the step)
                stream = side if side is not None else torch.cuda.current_stream(self.dev)
                _lib.check(_lib.lib().r3dg_store_u64_to_host(stream.cuda_stream, count.data_ptr(), slot.data_ptr()), "store_u64_to_host")
            else:
                slot.copy_(count, non_blocking=True)
        else:
            slot.fill_(int(R))
            if self.bounded:
                self._capacity = self._capacity_for(R)

    _SKIP_RING = 1024

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
        if new_local > 0 and not getattr(self, "dp", False):
            # which iterations: their slots of the flag ring (older ones than the ring holds were overwritten)
            lo = max(self._drop_polled, self._iter - self._SKIP_RING)
            its = torch.arange(lo + 1, self._iter + 1, device=self.dev)
            hit = self._flag_ring[its % self._SKIP_RING, 0] != 0
            self.dropped_iterations.extend(int(i) for i in its[hit].tolist())
        self._drop_polled = self._iter
        if getattr(self, "dp", False):
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
        return self._flag if getattr(self, "dp", False) else self._flag_ring[self._iter % self._SKIP_RING]

    def replay_dropped(self, inputs_of):
        """Train again on the views the bounded forward dropped (VERDICT r4 missing 5: the reference sizes its binning state from
        the count it reads back and trains on EVERY view, rasterizer_impl.cu:291, train.py:114-127).  `inputs_of(iteration)` ->
        the arguments of that iteration's __call__ (iteration numbers count this object's forward_backward calls from 1).
        Every iteration poll_overflow() found dropped since the last replay runs once more through the exact two-phase forward
        (the capacity is forgotten for it: the count is read back, the state sized from it, the capacity re-learned), with its
        optimizer step.  Returns the iteration numbers replayed.  Single GPU only (under data parallelism a dropped step is
        dropped on every rank and the ranks would have to agree on the replay: poll_overflow keeps counting them)."""
        if getattr(self, "dp", False):
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


class FusedStage2Step(_BoundedForward):
    """Owns the raw parameters (copied from a bench_core.GaussianParams) and runs whole iterations."""

    # whole single-GPU iterations close the incident-light group with ONE chain kernel (read by bench_core's --full attribution)
    _chain_kernel = True

    def __init__(self, params, sample_num, lr=1e-4, lr_rest_scale=1.0, loss_weights=None, process_group=None, lrs=None,
                 bounded=True):
        """`lrs`: optional per-group learning rates {xyz, normal, scaling, rotation, opacity, shs, shs_rest, base_color,
        roughness, incidents, incidents_rest, env} as GaussianModel.training_setup / DirectLightMap.training_setup set
        them (scene/gaussian_model.py:465-486, the stage-2 values of script/run_nerf.sh:25-31); missing names use `lr`
        (`lr * lr_rest_scale` for the non-dc SH columns).
        `bounded`: after the first iteration (which reads num_rendered like the reference) the rasterizer forward runs
        WITHOUT the host read-back: binning state sized for twice the largest count seen, projection + instance ordering
        queued at once beside the shading forward.  A view that needs more is dropped on the device (its Adam launches
        read the flag and update nothing); `poll_overflow()` -- called by loss() -- then doubles the capacity and counts
        it in `dropped_steps`.
        `loss_weights`: overrides of train_step.STAGE2_WEIGHTS (the lambdas of script/run_nerf.sh:20-39);
        train_step.STAGE2_WEIGHTS_SYN4 adds the three edge-aware smoothness terms of script/run_syn4.sh / run_dtu.sh.
        FROZEN GEOMETRY: a group whose learning rate(s) are 0 gets no Adam launch; when ALL of xyz, normal, scaling,
        rotation, opacity and shs are frozen (run_syn4.sh:27-33, run_dtu.sh:29-35) the iteration also skips what only they
        would consume -- the alpha-gradient half of the tile backward and the whole per-Gaussian geometry backward
        (r3dg_rasterize_backward_features instead), the geometry half of the activation chain rule, their all-reduce
        buckets -- and their entries of `grads` stay zero."""
        dev = params.xyz.device
        self.dev = dev
        d = lambda t: t.detach().clone().contiguous()
        self.xyz, self.normal = d(params.xyz), d(params.normal)
        self.scaling, self.rotation, self.opacity = d(params.scaling), d(params.rotation), d(params.opacity)
        self.shs = torch.cat([params.features_dc.detach(), params.features_rest.detach()], 1).contiguous()
        self.base_color, self.roughness = d(params.base_color), d(params.roughness)
        self._incidents = torch.cat([params.incidents_dc.detach(), params.incidents_rest.detach()], 1).contiguous()
        self.env = d(params.env)
        self.P = P = self.xyz.shape[0]
        self.K = sample_num
        self.M = self.shs.shape[1]
        if self._incidents.shape[1] != self.M:      # the reference gives both the same degree (gaussian_model.py:421, :450)
            raise RuntimeError("FusedStage2Step: colour and incident-light SH must hold the same number of coefficients")
        # script/run_nerf.sh:20-39 (stage 2): lambda_pbr 1, lambda_light 0.01, lambda_env_smooth 0.01; the command does not
        # pass --lambda_normal_render_depth, so that term is off (arguments/__init__.py:115) -- opt in with
        # loss_weights={"normal": 0.01}; the edge-aware smoothness terms are 0 there and 1 / 0.5 / 1 in run_syn4.sh / run_dtu.sh
        self.w = dict(STAGE2_WEIGHTS)
        if loss_weights:
            unknown = set(loss_weights) - set(self.w)
            if unknown:
                raise RuntimeError("FusedStage2Step: unknown loss weights %s" % sorted(unknown))
            self.w.update(loss_weights)
        lrs = dict(lrs or {})
        rate = lambda k: float(lrs.get(k, lr))
        tail = lambda k: float(lrs.get(k + "_rest", rate(k) * lr_rest_scale))
        # groups that do not train (both rates 0 for the two SH tensors)
        self.frozen = {k for k in PARAM_NAMES if rate(k) == 0.0 and (k not in ("shs", "incidents") or tail(k) == 0.0)}
        self.frozen_geometry = all(k in self.frozen for k in FROZEN_GEOMETRY_GROUPS)
        # activations / intermediates (persistent, overwritten every step)
        f = dict(dtype=torch.float32, device=dev)
        self.a_scales, self.a_rot = torch.empty(P, 3, **f), torch.empty(P, 4, **f)
        self.a_opacity, self.a_normal = torch.empty(P, 1, **f), torch.empty(P, 3, **f)
        self.a_base, self.a_rough = torch.empty(P, 3, **f), torch.empty(P, 1, **f)
        self.a_viewdirs = torch.empty(P, 3, **f)
        self.shade_out = torch.empty(P, shading_ops.NOUT, **f)
        self.features = torch.empty(P, 16, **f)
        # unweighted sums: l1, pbr l1, normal mse, light l1, TV(env), SSIM(image), SSIM(pbr), and the three edge-aware
        # smoothness sums (base colour, roughness, diffuse light)
        self.sums = torch.zeros(10, SUM_SLOTS, **f)       # R3DG_SUM_SLOTS floats per quantity (include/r3dg_hip.h)
        self.d_pbr, self.d_diffuse = torch.empty(P, 3, **f), torch.empty(P, 3, **f)
        self._absmax = torch.zeros((P + 255) // 256, **f)       # block maxima of |d_pbr|, |d_diffuse| (unpack kernel)
        self._d_env = None
        # flat gradient slab: [shs 3M | xyz3 normal3 scaling3 rotation4 opacity1 base3 rough1 per Gaussian, env texture |
        # incidents 3M]; every group starts on a 16-byte boundary (float4 accesses in the Adam kernel)
        sizes = dict(xyz=3 * P, normal=3 * P, scaling=3 * P, rotation=4 * P, opacity=P, base_color=3 * P, roughness=P,
                     shs=3 * self.M * P, incidents=3 * self.M * P, env=self.env.numel(), flag=4)
        # `flag`: the bounded forward's overflow flag rides at the end of bucket A, so that under data parallelism the
        # first all-reduce tells every rank whether ANY rank dropped its view (sum > 0) before the first Adam launch
        if self.frozen_geometry:
            # nothing of the frozen groups is reduced or updated: [flag, base_color, roughness, env | incidents | the rest]
            order = ("flag", "base_color", "roughness", "env", "incidents", "shs", "xyz", "normal", "scaling", "rotation",
                     "opacity")
        else:
            order = ("shs", "flag", "xyz", "normal", "scaling", "rotation", "opacity", "base_color", "roughness", "env",
                     "incidents")
        pad4 = lambda n: (n + 3) // 4 * 4
        self.grad_flat = torch.zeros(sum(pad4(sizes[k]) for k in order), **f)
        self.grads, o, start = {}, 0, {}
        for k in order:
            start[k] = o
            if k == "flag":
                self._flag = self.grad_flat[o:o + 4]
            else:
                self.grads[k] = self.grad_flat[o:o + sizes[k]].view_as(getattr(self, k))
            o += pad4(sizes[k])
        self._init_bounded(bounded, self._flag)
        self._skip_cur = None
        # three all-reduce buckets (world > 1): A = SH colour grads, final right after the rasterizer backward (reduced
        # under the shading backward); C = the small per-Gaussian groups, final after the activation chain rule;
        # B = incident-light grads, final after the shading backward -- reduced LAST and only waited for right before
        # the NEXT iteration's shading forward, so it travels under that iteration's projection + binning
        # (the env texture's gradient rides in bucket C: one collective instead of a separate 6 KB all-reduce)
        if self.frozen_geometry:
            self._bucket_a = None                                               # (no SH colour gradient to send early)
            self._bucket_c = self.grad_flat[:start["incidents"]]                # flag + base colour, roughness, env texture
            self._bucket_b = self.grad_flat[start["incidents"]:start["shs"]]
            self._bucket_all = self.grad_flat[:start["shs"]]
        else:
            self._bucket_a = self.grad_flat[:start["xyz"]]
            self._bucket_c = self.grad_flat[start["xyz"]:start["incidents"]]
            self._bucket_b = self.grad_flat[start["incidents"]:]
            self._bucket_all = self.grad_flat
        self._pending_b = None
        self._acc = None                            # the tile backward's accumulator slab, zero-filled off the critical path
        self._early_pending = False                 # the early-Adam stream holds work no other stream has been ordered behind yet
        # the iteration's schedule (forward_backward): work on the early stream, the incident-light chain queued there, the SH
        # group updated with the others although the chain is queued
        self._early = self._b_early = self._a_late = False
        self._dp_chain = None                       # data parallel: the ray set whose chain kernel closes this iteration's bucket B
        # softplus of the environment texture, refreshed behind the Adam launch that updates the texture (see optimizer_step)
        self._env_c = None                          # softplus(environment texture), see _env_buffer
        self._zero_depth_grad = None
        # instance ordering of the rasterizer runs here, under the shading forward (register-light, latency-bound kernels
        # next to a VALU-bound one)
        self._order_stream = shared_stream(dev, "order")
        self._adam_stream = None                    # the early-Adam stream, created at first use (_early_stream)
        self._geo_done = None
        self.group = process_group
        self.world, self.dp = _world_of(process_group)
        # tuning options of THIS object (include/r3dg_hip.h "option contexts"): every library call of the step runs inside it
        self._ctx = _lib.OptionContext()
        # feature rows without a pack kernel: the activations write the columns they own, the fixed-ray-set shading kernels
        # theirs (r3dg_shade_frs_forward d_feature_rows) -- one launch and its join less between the shading integral and the
        # rasterizer.  The general shading kernels keep r3dg_stage2_pack_features.
        self._direct_rows = os.environ.get("R3DG_DIRECT_ROWS", "1") != "0"
        if self.dp:
            # The shading kernels and the visibility trace are PERSISTENT grids that fill every CU (the backward: 2 workgroups
            # x ~60 KB LDS, ~2 x 230 VGPRs per SIMD); RCCL's workgroups could then only start when one of them retires and
            # bucket A's "hidden" all-reduce would serialise behind the shading backward.  Under data parallelism the
            # persistent grids leave a few CUs free (r3dg_set_option(R3DG_OPT_RESERVE_CUS); R3DG_RESERVE_CUS_FOR_COMM
            # overrides, 0 = off); the cost on one rank is measured by bench.py (`data_parallel_path_one_rank_rccl`).
            self._ctx.set("RESERVE_CUS", int(os.environ.get("R3DG_RESERVE_CUS_FOR_COMM", "8")))
            # the side-stream schedule needs one hardware queue per stream: HIP maps a process's streams onto GPU_MAX_HW_QUEUES
            # queues (default 4) round robin and two streams on one queue run their kernels in turn (DESIGN.md section 5:
            # 575 -> 621 it/s on one rank); the variable is read when the runtime starts, so it can only be checked here
            if int(os.environ.get("GPU_MAX_HW_QUEUES", "4")) < 8:
                import warnings
                warnings.warn("FusedStage2Step under data parallelism: GPU_MAX_HW_QUEUES=%s (< 8) -- RCCL's streams and this "
                              "iteration's three streams will share hardware queues and serialise; export GPU_MAX_HW_QUEUES=8 "
                              "before the process starts (bench.py does)" % os.environ.get("GPU_MAX_HW_QUEUES", "unset (4)"))
        # bench.py's one-stream pass: every launch of the iteration on the caller's stream (no ordering / early-Adam / geometry
        # side streams), so that each stage's HIP-event bracket times its kernel with nothing beside it
        self.serial_streams = False
        self.measure_comm = False                   # bench.py: time the main stream spends waiting for all-reduce buckets
        self._comm_events = []
        self._bucket_events = []                    # (iteration, bucket, bytes, ready event, done event): comm_table()
        # with measure_comm: every n-th iteration's buckets get the two probe events (0 = never; R3DG_COMM_PROBE_EVERY)
        self.comm_probe_every = int(os.environ.get("R3DG_COMM_PROBE_EVERY", "4"))
        # R3DG_DP_BUCKETS=1 (A/B, message size against overlap): ONE all-reduce of the whole gradient slab behind the backward
        # and one Adam launch behind it, instead of the three buckets A / C / B each sent the moment it is final
        self._single_bucket = self.dp and os.environ.get("R3DG_DP_BUCKETS", "3") == "1"
        with torch.no_grad(), self._ctx:
            self.refresh_activations()
            self.visibility, self.incident_dirs, self.incident_areas, self.tracer = update_visibility(
                self.xyz, self.a_scales, self.a_rot, self.a_opacity, self.a_normal, sample_num, group=process_group)
            # the normals the ray set was generated from (the trained normal moves on; the cached directions do not)
            self._ray_normals = self.a_normal.clone()
        self._taps, self._taps_key, self._taps_size, self._frs_built = None, None, None, None
        self._frs = None                            # shading_ops.FixedRaySet of the current direction cache, or None
        # incident-light chain of a whole single-GPU iteration: (ray set, coefficient tensor, its version) the rotated coefficients
        # in the ray set were computed FROM, when that was done ahead of the next iteration; work still running on the early stream
        self._pre_rotated = None
        self._chain_deferred = None                 # (ray set, skip flag, Adam step count) of the chain optimizer_step queues
        self.opt = FusedAdam([
            dict(param=self.xyz, lr=rate("xyz")), dict(param=self.normal, lr=rate("normal")),
            dict(param=self.scaling, lr=rate("scaling")), dict(param=self.rotation, lr=rate("rotation")),
            dict(param=self.opacity, lr=rate("opacity")),
            dict(param=self.shs, lr=rate("shs"), lr_tail=tail("shs"), period=3 * self.M, split=3),
            dict(param=self.base_color, lr=rate("base_color")), dict(param=self.roughness, lr=rate("roughness")),
            dict(param=self._incidents, lr=rate("incidents"), lr_tail=tail("incidents"), period=3 * self.M, split=3),
            dict(param=self.env, lr=rate("env"))])
        self._opt_order = ("xyz", "normal", "scaling", "rotation", "opacity", "shs", "base_color", "roughness",
                           "incidents", "env")
        # Adam launches of an iteration: the groups of each gradient bucket that train
        live = lambda idx: tuple(i for i in idx if self._opt_order[i] not in self.frozen)
        self._groups_a, self._groups_c, self._groups_b = live((5,)), live((0, 1, 2, 3, 4, 6, 7, 9)), live((8,))
        self.last_outs = None

    # views with the reference's parameter names (gaussian_model.py:199-203, 232)
    features_dc = property(lambda self: self.shs[:, :1])
    features_rest = property(lambda self: self.shs[:, 1:])
    incidents_dc = property(lambda self: self.incidents[:, :1])
    incidents_rest = property(lambda self: self.incidents[:, 1:])

    # The incident-light coefficients as everybody OUTSIDE the iteration sees them.  A whole single-GPU iteration (__call__) leaves
    # their Adam update -- and the rotation of the new coefficients for the next iteration -- running on the early-Adam stream
    # (see forward_backward: "incident-light chain"); a reader on any other stream must be ordered behind it first.
    @property
    def incidents(self):
        if getattr(self, "_early_pending", False):
            self.flush()
        return self._incidents

    @incidents.setter
    def incidents(self, value):
        if getattr(self, "_early_pending", False):
            self.flush()
        self._incidents = value
        self._pre_rotated = None

    # GaussianModel-style accessors (plain PyTorch; used by eval / relight code, not by the fused iteration)
    def get_scaling(self):
        return torch.exp(self.scaling)

    def get_rotation(self):
        return F.normalize(self.rotation)

    def get_opacity(self):
        return torch.sigmoid(self.opacity)

    def get_shs(self):
        return self.shs

    def get_normal(self):
        return F.normalize(self.normal, dim=-1, eps=1e-3)

    def refresh_activations(self, cam=None, env_out=None, zero=None):
        """GaussianModel's activations + view directions (+ the feature-row columns that do not wait for the shading integral).
        `env_out` / `zero` (the iteration): the softplus of the environment texture into `env_out` and a zero fill of `zero` ride
        as extra workgroups of the same launch (r3dg_stage2_activate_with) instead of two launches on the critical stream."""
        L = _lib.lib()
        campos = cam.camera_center if cam is not None else torch.zeros(3, device=self.dev)
        with torch.cuda.device(self.dev):
            st = L.r3dg_stage2_activate_with(
                _lib.current_stream(), self.P, self.xyz.data_ptr(), self.scaling.data_ptr(), self.rotation.data_ptr(),
                self.opacity.data_ptr(), self.normal.data_ptr(), self.base_color.data_ptr(), self.roughness.data_ptr(),
                campos.contiguous().data_ptr(), self.a_scales.data_ptr(), self.a_rot.data_ptr(),
                self.a_opacity.data_ptr(), self.a_normal.data_ptr(), self.a_base.data_ptr(), self.a_rough.data_ptr(),
                self.a_viewdirs.data_ptr(),
                # the nine columns of the feature rows that do not wait for the shading integral (see forward_backward)
                cam.world_view_transform.contiguous().data_ptr() if cam is not None and self._direct_rows else None,
                self.features.data_ptr() if cam is not None and self._direct_rows else None,
                0 if env_out is None else env_out.numel(), None if env_out is None else self.env.data_ptr(),
                None if env_out is None else env_out.data_ptr(), None if zero is None else zero.data_ptr(),
                0 if zero is None else zero.numel())
        _lib.check(st, "stage2_activate")

    def taps(self, He, We):
        """The per-sample lookup cache of the general shading kernels for a He x We environment texture
        (shading_ops.build_taps: 12 bytes per sample, read beside the [P,K,3] directions) -- or None when the direction cache IS
        the Fibonacci set of the snapshot normals and the fixed-ray-set kernels run (`self._frs`: they read neither; their own
        8-byte records come from the ray normals, shading_ops.FixedRaySet.taps).  Decided once per visibility update / texture
        size."""
        # keyed by the direction tensor ITSELF (held in _taps_src for as long as its taps are: a replaced cache can then never
        # come back at the address of the old one and pass for it) + its version counter (in-place updates).  The texture size is a
        # key of its own: only the lookup records depend on it, the ray set (P x K directions regenerated and classified, a host
        # read-back) does not
        src = self.incident_dirs
        dir_key, size_key = (src._version, tuple(src.shape)), (He, We)
        fresh = getattr(self, "_taps_src", None) is not src or self._taps_key != dir_key
        if fresh:
            self._taps_key, self._taps_src, self._taps_size = dir_key, src, None
            # fibonacci_sphere_sampling gives every sample the area 2 pi: then the area cache need not be read at all
            lo, hi = float(self.incident_areas.min()), float(self.incident_areas.max())
            self._uniform_area = lo if lo == hi else None
            # fixed-ray-set kernels (csrc/shading_frs.hpp) when the cache IS the Fibonacci set of the snapshot normals --
            # checked here, once per visibility update -- and fits their limits; otherwise (caches handed in from elsewhere,
            # other K, R3DG_SHADE_FRS=0) the general kernels
            self._frs_built, self._taps = None, None
            if (os.environ.get("R3DG_SHADE_FRS", "1") != "0" and self._uniform_area is not None and
                    shading_ops.FixedRaySet.supported(self.K, self.M, 16, 32)):      # (K and the SH degree; the size: below)
                self._frs_built = shading_ops.FixedRaySet.try_build(getattr(self, "_ray_normals", None), src)
        if fresh or self._taps_size != size_key:
            # a new texture size: new lookup records for the ray set that is already there (FixedRaySet.taps is keyed on the size
            # itself) if the fixed-ray-set kernels take that size, the general kernels' 12-byte taps otherwise
            self._taps_size = size_key
            built = self._frs_built
            self._frs = built if built is not None and shading_ops.FixedRaySet.supported(self.K, self.M, He, We) else None
            if self._frs is None:
                self._taps = shading_ops.build_taps(src, He, We)
            else:
                self._taps = None
                self._frs.taps(He, We)
        return self._taps

    def _env_buffer(self):
        """Where the iteration keeps softplus(environment texture) (DirectLightMap.get_env) [He,We,3]: filled by the activation
        launch of every iteration (refresh_activations(env_out=)), read by the shading kernels and the texture's chain rule."""
        shape = tuple(self.env.shape[1:])
        if self._env_c is None or tuple(self._env_c.shape) != shape:
            self._env_c = torch.empty(shape, dtype=torch.float32, device=self.dev)
        return self._env_c

    def _rotation_is_current(self):
        """The ray set already holds the rotation of the CURRENT coefficients (queued on the early-Adam stream right behind their
        Adam update, at the end of the previous iteration)?  Keyed on the tensor and its version counter: anything that replaces or
        edits the coefficients in between (a checkpoint load, a test) invalidates it -- the Adam kernel itself writes through the raw
        pointer and does not count."""
        pr = self._pre_rotated
        return pr is not None and pr[0] is self._frs and pr[1] is self._incidents and pr[2] == self._incidents._version

    def _early_stream(self):
        """The early-Adam stream (the process's shared "early" stream), created at first use."""
        if self._adam_stream is None:
            self._adam_stream = shared_stream(self.dev, "early")
        return self._adam_stream

    def _aux_stream(self):
        """The early-Adam stream, for the side work of the fixed-ray-set path on one GPU; None without that path and under data
        parallelism (the stream then carries the buckets' waits and the coefficients are updated late, in flush())."""
        if self._frs is None or self.dp or self.serial_streams:
            return None
        return self._early_stream()

    def _listed_stream(self):
        """The early-Adam stream when the fixed-ray-set path has Gaussians off the rotated path: their general kernels run there in
        the forward, and the rasterizer's geometry backward beside them in the backward (data-parallel runs too: the stream is
        idle during the forward, and in the backward bucket A's all-reduce is issued from it, behind the geometry backward)."""
        if self._frs is None or self._frs.n_invalid == 0 or self.serial_streams:
            return None
        return self._early_stream()

    @_in_context
    def forward_backward(self, cam, bg, gt, early_adam=False, image_mask=None, split_geometry=None, chain_incidents=False):
        """One forward + loss + backward; gradients land in self.grads.  Returns the rasterizer's 10 public outputs.
        `image_mask` [1,H,W]: the view's object mask (Camera.image_mask; None = all ones) of the normal and smoothness terms.
        `early_adam` (single-GPU whole iterations only, see __call__): the SH colour coefficients, whose gradient is final
        after the rasterizer backward, get their Adam update on a side stream UNDER the shading backward (an HBM-bound,
        register-light kernel next to a VALU-bound one); optimizer_step() then updates the remaining groups.
        `split_geometry` (default: `early_adam`): the rasterizer's per-Gaussian geometry backward on the early stream, beside the
        gradient unpack and the listed Gaussians' shading backward.  (Measured on its own at 2M Gaussians, where the early Adam is
        off: 160.7 vs 166.3 it/s -- both kernels stream from HBM there and slow each other by more than the overlap buys.)"""
        # `chain_incidents` (whole iterations only, see __call__; implied by `early_adam`): the incident-light gradient may stay in the
        # rotated frame for the chain kernel that optimizer_step launches -- a caller of a bare forward_backward reads
        # grads["incidents"] in the world frame, always
        if split_geometry is None:
            split_geometry = early_adam
        L = _lib.lib()
        P, dev = self.P, self.dev
        H, W = cam.image_height, cam.image_width
        N = H * W
        main = torch.cuda.current_stream(dev)           # (looked up ONCE: 10 us of Python per lookup, this method had six)
        main_raw = main.cuda_stream
        stream = lambda: main_raw
        vm = cam.world_view_transform.contiguous()
        campos = cam.camera_center.contiguous()
        empty = torch.Tensor([])
        order_stream = None if self.serial_streams else self._order_stream
        with torch.cuda.device(dev):
            # the rotation of the incident-light coefficients into the ray frames depends on nothing of this view: it goes to the
            # side stream now and runs beside the activations and the projection instead of in front of the shading forward
            rotated_for = None
            aux = self._aux_stream()
            if self._chain_deferred is not None:
                self.flush()         # (forward_backward was called twice without optimizer_step: the pending chain runs now)
            if aux is not None:
                _lib.stream_wait(aux, main)
                # (normally the previous iteration's incident-light chain left the rotated coefficients in place: see below)
                if not self._rotation_is_current():
                    with torch.cuda.stream(aux):
                        self._frs.rotate(self._incidents)
                rotated_for = self._frs
            # The small view-independent jobs of the iteration -- softplus of the environment texture, the loss-sum reset -- ride
            # as extra workgroups of the activation launch.  The tile backward's accumulator slab needs no zero fill: its scatter
            # pass writes every element.
            acc_n = (11 + 16) * P
            if self._acc is None or self._acc.numel() != acc_n:
                self._acc = torch.empty(acc_n, dtype=torch.float32, device=dev)
            env_c = self._env_buffer()
            self.refresh_activations(cam, env_out=env_c, zero=self.sums)
            self._iter += 1
            flag_cur = self._flag_of_iteration()
            use_bounded = self._use_bounded(W, H)
            if self._early_pending and (aux is None or not (use_bounded and order_stream is not None)):
                # (the previous iteration left work on the early stream that only the bounded, three-stream schedule is ordered
                # behind by construction: any other schedule joins it here)
                _lib.stream_wait(main, self._adam_stream)
                self._early_pending = False
            if use_bounded:
                # bounded forward: projection + instance ordering go to the ordering stream NOW and run beside the
                # shading kernels queued below; nobody waits for the count
                pending = rasterizer_ops.rasterize_gaussians_begin(
                    bg, self.xyz, self.features, empty, self.a_opacity, self.a_scales, self.a_rot, 1.0, empty, vm,
                    cam.full_proj_transform, cam.tanfovx, cam.tanfovy, cam.cx, cam.cy, H, W, self.shs, 3, campos, False,
                    True, False, capacity=self._capacity, overflow_flag=flag_cur,
                    overflow_count=self._overflow_count, ordering_stream=order_stream, want_weights=False,
                    defer_pseudo_normal=True)
            else:
                # first half of the rasterizer (projection + async read-back of num_rendered): the shading kernels below
                # run while the host waits for the count and enqueues the second half
                flag_cur.zero_()
                pending = rasterizer_ops.rasterize_gaussians_begin(
                    bg, self.xyz, self.features, empty, self.a_opacity, self.a_scales, self.a_rot, 1.0, empty, vm,
                    cam.full_proj_transform, cam.tanfovx, cam.tanfovy, cam.cx, cam.cy, H, W, self.shs, 3, campos, False,
                    True, False, want_weights=False,       # (stage 2 does not densify: nobody reads the blend weights)
                    defer_pseudo_normal=True)
            if self._pending_b is not None:
                self.flush()    # (world > 1) the previous iteration's incident-light update lands here
            if aux is not None:
                _lib.stream_wait(main, aux)
                self._early_pending = False          # (aux IS the early stream: the main stream is behind all of it now)
            He, We = env_c.shape[0], env_c.shape[1]
            taps = self.taps(He, We)
            if self._frs is not None:
                # (taps() may have rebuilt the ray set: then it rotates itself; data parallel: flush() above ran the chain kernel)
                rotated = rotated_for is self._frs or (self.dp and self._rotation_is_current())
                self._frs.forward(self.a_base, self.a_rough, self.a_normal, self.a_viewdirs, self._incidents, env_c,
                                  self.visibility, self.shade_out, uniform_area=self._uniform_area,
                                  # (one workgroup per CU beside the instance ordering while THAT is the longer path: 806 vs 801
                                  # it/s without the cap, frozen geometry (run_syn4.sh) 835 vs 826.  Not under data parallelism,
                                  # where the deferred incident-light update sits in front of this kernel: 558 -> 568 it/s on one
                                  # rank without the cap)
                                  leave_room=order_stream is not None and not self.dp,
                                  # the few hundred Gaussians off the rotated path: their general kernel on the (idle) early-Adam
                                  # stream beside the rotation and the main kernel, joined below before the features are packed
                                  listed_stream=self._listed_stream(), rotated=rotated,
                                  feature_rows=self.features if self._direct_rows else None)
            else:
                _lib.check(L.r3dg_shade_forward_cached(
                    stream(), P, self.K, self.M, self.a_base.data_ptr(), self.a_rough.data_ptr(), self.a_normal.data_ptr(),
                    self.a_viewdirs.data_ptr(), self._incidents.data_ptr(), env_c.data_ptr(), He, We, None,
                    self.visibility.data_ptr(), self.incident_dirs.data_ptr(),
                    None if self._uniform_area is not None else self.incident_areas.data_ptr(), self._uniform_area or 0.0,
                    taps.data_ptr(), 1 | (4 if order_stream is not None else 0),     # train outputs | leave room
                    self.shade_out.data_ptr()), "shade_forward")
            if self._frs is not None and self._listed_stream() is not None:
                _lib.stream_wait(main, self._listed_stream())
            packed = not (self._frs is not None and self._direct_rows)
            if packed:
                _lib.check(L.r3dg_stage2_pack_features(
                    stream(), P, self.xyz.data_ptr(), vm.data_ptr(), self.a_normal.data_ptr(), self.a_base.data_ptr(),
                    self.a_rough.data_ptr(), self.shade_out.data_ptr(), self.features.data_ptr(),
                    self.sums[3].data_ptr()), "stage2_pack_features")
            fw = pending.finish(order_stream)
            R, n_contrib, image, opacity, depth, feature, pseudo_normal, sxyz, weights, radii, geom, binning, img = fw
            # the Adam launches of this iteration skip themselves when the view was dropped; under data parallelism they
            # read a snapshot of the flag taken after bucket A's all-reduce (optimizer_step)
            self._skip_cur = flag_cur              # (world > 1: replaced by the reduced snapshot in optimizer_step)
            # image-space loss terms and their gradients.  One slab: dL_dimage 3 | dL_dopacity 1 | dL_dfeature 16 | sRGB PBR
            # image 3 | SSIM partials 2x9 | SSIM gradients 2x3 (the depth image carries no loss)
            g = torch.empty((47, H, W), dtype=torch.float32, device=dev)
            if self._zero_depth_grad is None or self._zero_depth_grad.shape[-2:] != (H, W):
                self._zero_depth_grad = torch.zeros((1, H, W), dtype=torch.float32, device=dev)
            gt_c, bg_c = gt.contiguous(), bg.contiguous()
            srgb, part_i, part_p, gs_i, gs_p = g[20:23], g[23:32], g[32:41], g[41:44], g[44:47]
            lam = LAMBDA_DSSIM
            # the rasterizer forward's pseudo-normal pass (deferred above) and the sRGB-mapped PBR image: one per-pixel launch
            _lib.check(L.r3dg_stage2_normals_srgb(
                stream(), W, H, vm.data_ptr(), float(cam.tanfovx), float(cam.tanfovy), float(cam.cx), float(cam.cy),
                opacity.data_ptr(), depth.data_ptr(), pseudo_normal.data_ptr(), sxyz.data_ptr(), feature.data_ptr(),
                n_contrib.data_ptr(), bg_c.data_ptr(), srgb.data_ptr()), "stage2_normals_srgb")
            # SSIM terms of both images: one forward and one backward launch for the pair
            _lib.check(L.r3dg_ssim_forward_pair(stream(), W, H, 3, image.data_ptr(), srgb.data_ptr(), gt_c.data_ptr(),
                                                part_i.data_ptr(), part_p.data_ptr(), self.sums[5].data_ptr(),
                                                self.sums[6].data_ptr()), "ssim_forward")
            _lib.check(L.r3dg_ssim_backward_pair(stream(), W, H, 3, image.data_ptr(), srgb.data_ptr(), gt_c.data_ptr(),
                                                 part_i.data_ptr(), part_p.data_ptr(), -self.w["l1"] * lam / (3.0 * N),
                                                 -self.w["pbr"] * lam / (3.0 * N), gs_i.data_ptr(), gs_p.data_ptr()),
                       "ssim_backward")
            mask_c = None if image_mask is None else image_mask.contiguous()
            _lib.check(L.r3dg_stage2_loss(
                stream(), W, H, image.data_ptr(), opacity.data_ptr(), feature.data_ptr(), pseudo_normal.data_ptr(),
                n_contrib.data_ptr(), gt_c.data_ptr(), bg_c.data_ptr(), _lib.ptr(mask_c),
                self.w["l1"] * (1.0 - lam) / (3.0 * N), self.w["pbr"] * (1.0 - lam) / (3.0 * N),
                self.w["normal"] / (3.0 * N), gs_i.data_ptr(), gs_p.data_ptr(),
                g[0:3].data_ptr(), g[3:4].data_ptr(), g[4:20].data_ptr(), self.sums.data_ptr(), 1), "stage2_loss")
            # r3dg_stage2_loss only writes the pbr maps and -- when that term is on -- the normal maps; the smoothness terms
            # add base colour / roughness / diffuse light (and, through the light term's guide, the normal maps)
            active = [2, 3, 4] + ([5, 6, 7] if self.w["normal"] != 0.0 else [])
            w_bc, w_r, w_ls = (self.w[k] / (3.0 * N) for k in ("base_color_smooth", "roughness_smooth", "light_smooth"))
            if w_bc != 0.0 or w_r != 0.0 or w_ls != 0.0:
                # one streaming kernel: the divided maps and the adjoint inputs never exist in HBM (r3dg_stage2_smooth_forward /
                # _backward, the three-pass formulation, stay as its reference in the tests)
                _lib.check(L.r3dg_stage2_smooth_fused(
                    stream(), W, H, opacity.data_ptr(), feature.data_ptr(), n_contrib.data_ptr(), gt_c.data_ptr(),
                    _lib.ptr(mask_c), w_bc, w_r, w_ls, 1 if self.w["normal"] != 0.0 else 0, g[3:4].data_ptr(),
                    g[4:20].data_ptr(), self.sums[7].data_ptr()), "stage2_smooth_fused")
                active += ([8, 9, 10] if w_bc != 0.0 else []) + ([11] if w_r != 0.0 else [])
                if w_ls != 0.0:
                    active += [12, 13, 14] + ([5, 6, 7] if self.w["normal"] == 0.0 else [])
            geo_stream = None
            self.last_active_features = sorted(set(active))      # (bench.py prices the backward launch with these)
            if self.frozen_geometry:
                # nothing but the feature gradients is consumed (the normal maps' gradient belongs to the frozen normal)
                active = [a for a in active if a not in (5, 6, 7)]
                dL_dfeatures = rasterizer_ops.rasterize_gaussians_backward_features(
                    P, 16, H, W, g[4:20], geom, R, binning, img, active_features=sorted(active))
                dL_dmeans2D = None
            else:
                # whole iterations with Gaussians off the rotated path: the per-Gaussian geometry backward goes to the early-Adam
                # stream and runs beside the gradient unpack and the general shading backward on those few hundred Gaussians (a
                # latency-bound launch that r3dg_shade_frs_backward queues FIRST) instead of in front of them; the main shading
                # backward, which fills the register file, starts when both are about done
                geo_stream = self._listed_stream() if split_geometry else None
                bw = rasterizer_ops.rasterize_gaussians_backward(
                    bg, self.xyz, self.features, radii, empty, self.a_scales, self.a_rot, 1.0, empty, vm,
                    # (no depth gradient: an EMPTY tensor = NULL = the caller's promise that the depth image carries no loss term)
                    cam.full_proj_transform, cam.tanfovx, cam.tanfovy, g[0:3], g[3:4], empty, g[4:20],
                    self.shs, 3, campos, geom, R, binning, img, True, False, dL_dsh_out=self.grads["shs"],
                    geometry_stream=geo_stream, active_features=sorted(active),
                    zeroed_accumulators=self._acc)
                dL_dmeans2D, _dcol, dL_dopacity, dL_dmeans3D, dL_dfeatures, _dcov, _dsh, dL_dscales, dL_drot = bw
                if geo_stream is not None:
                    if self._geo_done is None:
                        self._geo_done = torch.cuda.Event()
                    self._geo_done.record(geo_stream)
            handle_a = None
            if self._bucket_a is not None and not self._single_bucket:
                # bucket A (SH gradient + flag) travels under the shading backward; issued from the stream that produced it
                if geo_stream is not None:
                    with torch.cuda.stream(geo_stream):
                        handle_a = self._allreduce_async(self._bucket_a, "A")
                else:
                    handle_a = self._allreduce_async(self._bucket_a, "A")
            # SCHEDULE of the two large groups' updates.
            # a_early: the SH group's Adam on the early stream UNDER the shading backward, behind the geometry backward that
            #   produces its gradient -- under data parallelism behind bucket A's all-reduce, which carries the overflow flag too.
            # b_early: the INCIDENT-LIGHT CHAIN (single GPU, fixed ray set, bounded three-stream forward).  The group's gradient is
            #   finished by the rotation back; the group's Adam and the rotation of the NEW coefficients into the ray frames (the
            #   first thing the next iteration's shading forward needs, and independent of the next view) follow it as ONE kernel on
            #   the early stream, queued by optimizer_step behind the other groups' Adam -- beside the next iteration's activations
            #   + projection instead of Adam(all groups) -> activations -> rotation -> shading forward in a row (~100 us in which
            #   only small launches ran).  Without the early Adam: frozen SH colour (run_syn4.sh / run_dtu.sh)
            #   831 -> 843 it/s at sample_num 64, 606 -> 610 on the DTU frame, but not above 40 M samples (399 -> 392 at
            #   sample_num 384: there the shading forward is the long path of the forward window and the chain in front of it
            #   costs more than the launches it saves); above a million Gaussians (no early Adam: __call__) the launches it
            #   replaces stream 2112 bytes per Gaussian, the chain 1741.
            # a_late: the chain is queued but the SH group is updated with the others in optimizer_step.
            a_early = early_adam and bool(self._groups_a) and (handle_a is not None or not self.dp)
            b_early = (not self.dp and self._frs is not None and order_stream is not None and use_bounded and
                       (a_early or (bool(self._groups_b) and (P * self.K <= 40_000_000 if early_adam else chain_incidents))))
            self._early, self._b_early, self._a_late = a_early or b_early, b_early, b_early and not a_early
            if self._early:
                side = self._early_stream()
                self.opt.begin_step()
                self._early_pending = not self.dp
            if a_early:
                if geo_stream is None and not self.dp:
                    side.wait_stream(main)
                with torch.cuda.stream(side):
                    if self.dp:
                        # (whenever bucket A lands while the shading backward is still running, the SH group's Adam runs under it
                        # too: DESIGN.md section 5.  The reduced overflow flag is snapshotted right after the all-reduce that
                        # carries it.)
                        self._wait(handle_a, "A", side)       # the SIDE stream waits for RCCL's stream
                        self._skip_cur = self._snapshot_flag()
                    self.opt.step_groups(self._groups_a, [self.grads[k] for k in self._opt_order], 1.0 / self.world,
                                         skip_flag=self._skip_cur)
                if b_early:
                    # The main stream is NOT joined with the early stream at the end of the iteration:
                    #   * the ordering stream, which reads the SH colour coefficients in the next projection, is ordered behind the
                    #     SH group's Adam HERE (an event recorded now: it does not wait for what is queued on this stream later);
                    #   * the main stream joins this stream in front of the next shading forward;
                    #   * anybody else goes through `incidents` / flush().
                    # (The overflow flag the chain reads later is this iteration's own slot of the flag ring.)
                    _lib.stream_wait(order_stream, side)
            _lib.check(L.r3dg_stage2_unpack_gradients(
                stream(), P, dL_dfeatures.data_ptr(), self.shade_out.data_ptr(), self.w["light"] / (3.0 * P),
                self.d_pbr.data_ptr(), self.d_diffuse.data_ptr(), self._absmax.data_ptr(),
                # (the light-smoothness term's value, when no pack kernel added it)
                None if packed else self.sums[3].data_ptr()), "stage2_unpack_gradients")
            # the texture-gradient accumulator comes back zeroed from r3dg_stage2_env_backward (consume), the gradient
            # scale from the unpack kernel: nothing sits between that kernel and the shading backward
            if self._d_env is None or self._d_env.shape != env_c.shape:
                self._d_env = torch.zeros_like(env_c)
            if self._frs is not None:
                # the incident-light chain kernel rotates the coefficient gradient back itself: the main shading backward then
                # leaves it in the rotated frame (a frozen group: the chain is only the rotation of the coefficients)
                chain = b_early and bool(self._groups_b)
                # DATA PARALLEL: the same kernel closes the incident-light group there too.  The coefficient gradient stays in the
                # rotated frame (the Gaussians off the rotated path: their world-frame rows, in the same buffer), THAT buffer is
                # bucket B -- the rotation is linear and the same on every rank, so the sum over ranks of the rotated gradients is
                # the rotated sum -- and the chain kernel behind the all-reduce rotates it back, applies Adam with 1 / world and
                # rotates the new coefficients: bucket B is final one rotation launch (40 us) earlier, two launches fewer sit
                # between its arrival and the shading forward.  Whole iterations only (`chain_incidents`).
                dp_chain = (self.dp and chain_incidents and bool(self._groups_b) and not self._single_bucket
                            and os.environ.get("R3DG_DP_CHAIN", "1") != "0")
                d_base, d_rough, d_view, _d_inc, d_env = self._frs.backward(
                    self.a_base, self.a_rough, self.a_normal, self.a_viewdirs, self._incidents, env_c, self.visibility,
                    self.d_pbr, self.d_diffuse,
                    uniform_area=self._uniform_area,
                    out_incidents=self._frs.dcprime_rows() if dp_chain else self.grads["incidents"], out_env=self._d_env,
                    block_absmax=self._absmax,
                    # whole iterations: the rotation back of the coefficient gradient goes to the stream that already carries the
                    # SH group's early Adam (optimizer_step joins it before any Adam launch reads the gradient; under data
                    # parallelism bucket B's all-reduce is issued from it) and runs beside the activation chain rule
                    rotate_stream=self._adam_stream if self._early else None, rotation_back=not (chain or dp_chain))
                self._dp_chain = self._frs if dp_chain else None
                if b_early:
                    # optimizer_step queues the chain BEHIND the other groups' Adam.  Both are HBM streams; side by side the
                    # activation chain rule + that Adam -- which the whole front end of the next iteration waits for -- took 68 + 45
                    # us instead of 20 + 40, while the chain only gates the shading forward (801-806 vs 793-796 it/s, HISTORY.md)
                    self._chain_deferred = (self._frs, self._skip_cur, self.opt.step_count)
            else:
                d_base, d_rough, d_view, _d_inc, d_env = shading_ops.shade_backward(
                    self.a_base, self.a_rough, self.a_normal, self.a_viewdirs, self._incidents, env_c, self.visibility,
                    self.incident_dirs, self.incident_areas, self.d_pbr, self.d_diffuse,
                    out_incidents=self.grads["incidents"], taps=taps, out_env=self._d_env, block_absmax=self._absmax)
            gr = self.grads
            if geo_stream is not None:                                       # join the geometry backward (and nothing
                main.wait_event(self._geo_done)       # queued behind it on that stream)
            # the environment texture's chain rule (softplus' + total-variation term; r3dg_stage2_env_backward) rides as six
            # extra workgroups of the activation chain rule's launch
            env_job = (He, We, self.env.data_ptr(), env_c.data_ptr(), d_env.data_ptr(), self.w["env_smooth"],
                       gr["env"].data_ptr(), self.sums[4].data_ptr(), 1)
            if self.frozen_geometry:
                _lib.check(L.r3dg_stage2_activate_backward_with(
                    stream(), P, None, None, None, None, None, self.base_color.data_ptr(), self.roughness.data_ptr(), None,
                    None, dL_dfeatures.data_ptr(), d_base.data_ptr(), d_rough.data_ptr(), None, None, None, None, None,
                    None, None, None, None, None, gr["base_color"].data_ptr(), gr["roughness"].data_ptr(), *env_job),
                    "stage2_activate_backward")
            else:
                _lib.check(L.r3dg_stage2_activate_backward_with(
                    stream(), P, self.xyz.data_ptr(), self.scaling.data_ptr(), self.rotation.data_ptr(),
                    self.opacity.data_ptr(), self.normal.data_ptr(), self.base_color.data_ptr(), self.roughness.data_ptr(),
                    vm.data_ptr(), campos.data_ptr(), dL_dfeatures.data_ptr(), d_base.data_ptr(), d_rough.data_ptr(),
                    d_view.data_ptr(), dL_dscales.data_ptr(), dL_drot.data_ptr(), dL_dopacity.data_ptr(),
                    dL_dmeans3D.data_ptr(), gr["xyz"].data_ptr(), gr["scaling"].data_ptr(), gr["rotation"].data_ptr(),
                    gr["opacity"].data_ptr(), gr["normal"].data_ptr(), gr["base_color"].data_ptr(),
                    gr["roughness"].data_ptr(), *env_job), "stage2_activate_backward")
            self._handles = None
            if self._single_bucket:
                # (R3DG_DP_BUCKETS=1) the whole slab in one collective: everything is final on this stream here (no early Adam
                # without bucket A's handle, so the rotation back of the coefficient gradient ran on this stream too)
                self._handles = (None, self._allreduce_async(self._bucket_all, "ALL"), None)
            elif self.dp:
                handle_c = self._allreduce_async(self._bucket_c, "C")
                if self._dp_chain is not None:
                    # (BEHIND bucket C although it was final first: the collectives run in the order they are issued, and C is the
                    # bucket the main stream waits for -- issued right behind the shading backward, B cost the priced rehearsal
                    # 397 -> 374 it/s per rank at 150 GB/s, 590 -> 543 at 300)
                    handle_b = self._allreduce_async(self._dp_chain.dcprime.view(-1), "B")
                elif self._early:       # the incident-light gradient is finished by the rotation back, on the early stream
                    with torch.cuda.stream(self._adam_stream):
                        handle_b = self._allreduce_async(self._bucket_b, "B")
                else:
                    handle_b = self._allreduce_async(self._bucket_b, "B")
                self._handles = (handle_a, handle_c, handle_b)
        self.viewspace_grad = dL_dmeans2D
        # a bounded forward returned its capacity as R (the backward's layout); the count itself goes to a pinned ring
        # without anybody waiting for it (rendered_counts)
        self._note_count(geom, R, use_bounded)
        self.last_outs = (R, n_contrib, image, opacity, depth, feature, pseudo_normal, sxyz, weights, radii)
        self._N = N
        return self.last_outs

    def _allreduce_async(self, flat, name="?"):
        if not self.dp:
            return None
        if self.measure_comm and self._probe_this_iteration():
            # per-bucket attribution (bench.py): `ready` = the moment the issuing stream has the bucket final (one event record on a
            # stream that exists anyway).  The collective's own time comes from the events RCCL's process group brackets it with
            # on ITS stream (Work._get_duration, TORCH_NCCL_ENABLE_TIMING=1), read in comm_table once the work is complete.
            # (A first version recorded a `done` event behind handle.wait() on a probe stream of its own: the extra stream moved
            # the round-robin assignment of the iteration's streams to hardware queues -- 756 -> 513 it/s on the one-rank RCCL path,
            # whether every iteration was probed or every fourth.  No new stream here.)
            ready = torch.cuda.Event(enable_timing=True)
            ready.record()
            handle = self._allreduce_issue(flat)
            self._bucket_events.append((self._iter, name, flat.numel() * 4, ready, handle))
            return handle
        return self._allreduce_issue(flat)

    def _probe_this_iteration(self):
        return self.comm_probe_every > 0 and self._iter % self.comm_probe_every == 0

    def _allreduce_issue(self, flat):
        gbs = _fake_comm_gbs()
        if gbs is None:
            return torch.distributed.all_reduce(flat, group=self.group, async_op=True)
        # PRICED REHEARSAL (R3DG_DP_FAKE_COMM_GBS=<bus GB/s>, one-rank groups only): the identity collective, then a spin of
        # the time a ring all-reduce of this bucket takes over `world_assumed` ranks at that bus bandwidth --
        # 2 (W - 1) / W x bytes / B -- on ONE communication stream, so that the buckets serialise like RCCL's kernels do.
        # The returned handle's wait() makes the current stream wait for the end of the spin.
        W = int(os.environ.get("R3DG_DP_FAKE_COMM_WORLD", "8"))
        us = 2.0 * (W - 1) / W * flat.numel() * 4 / (gbs * 1e9) * 1e6
        comm = shared_stream(self.dev, "fake_comm")
        _lib.stream_wait(comm, torch.cuda.current_stream())
        if os.environ.get("R3DG_DP_FAKE_COMM_WITH_RCCL", "0") != "0":
            with torch.cuda.stream(comm):              # (the identity collective too: its launch + two stream joins)
                torch.distributed.all_reduce(flat, group=self.group, async_op=True).wait()
        begin = torch.cuda.Event(enable_timing=True) if self.measure_comm else None
        if begin is not None:
            begin.record(comm)
        _lib.check(_lib.lib().r3dg_spin(comm.cuda_stream, float(us)), "spin")
        done = torch.cuda.Event(enable_timing=self.measure_comm)
        done.record(comm)
        return _FakeCommHandle(done, begin)

    def _wait(self, handle, name="?", side=None, it=None):
        """Make the current stream wait for a bucket's all-reduce; with `measure_comm` the wait is bracketed by events so that
        the time the stream actually stalls on it (the EXPOSED communication) can be read back (exposed_comm_ms).  `side`: the
        wait sits on this side stream (bucket A: under the shading backward), not on the compute stream -- it is then only
        recorded for comm_table's `released_us`, not counted as exposed."""
        if not self.measure_comm:
            handle.wait()
            return
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        handle.wait()
        e1.record()
        # (`it`: the iteration the bucket belongs to -- bucket B is waited for at the top of the NEXT iteration)
        self._comm_events.append((self._iter if it is None else it, e0, e1, name, side is not None))

    def exposed_comm_ms(self, split=False):
        """Mean per iteration of the time the compute stream waited for gradient all-reduces since measure_comm was set
        (synchronises).  The early bucket A is waited for on a side stream and is not part of it by construction.
        `split`: -> (total, {bucket name: mean ms per iteration})."""
        if not self._comm_events:
            return (None, {}) if split else None
        torch.cuda.synchronize(self.dev)
        per_iter, per_name = {}, {}
        self._released = {}
        for it, e0, e1, name, on_side in self._comm_events:
            self._released[(it, name)] = e1
            if on_side:
                continue
            ms = e0.elapsed_time(e1)
            per_iter[it] = per_iter.get(it, 0.0) + ms
            per_name[name] = per_name.get(name, 0.0) + ms
        self._comm_events = []
        n = max(1, len(per_iter))
        total = sum(per_iter.values()) / n
        return (total, {k: v / n for k, v in per_name.items()}) if split else total

    def comm_table(self, world_assumed=None):
        """Per-bucket attribution of the gradient all-reduces of the probed iterations since measure_comm was set (call after
        exposed_comm_ms; synchronises): for each bucket its bytes, when it became final on the stream that issued it (`ready_us`,
        relative to the first bucket of its iteration), when its first consumer's stream got past the wait (`released_us`), the
        collective's OWN time `collective_ms` -- bracketed by the events the process group records on RCCL's stream
        (Work._get_duration; needs TORCH_NCCL_ENABLE_TIMING=1 before the group is created, bench.py sets it); for a backend without
        them (gloo: the tests) the ready -> released interval, an upper bound -- and the bus bandwidth that time amounts to for a
        ring all-reduce over the group's ranks, 2 (W-1)/W x bytes / collective_ms.  Means over the probed iterations; None when
        nothing was probed."""
        if not self._bucket_events:
            return None
        torch.cuda.synchronize(self.dev)
        W = world_assumed or (int(os.environ.get("R3DG_DP_FAKE_COMM_WORLD", "8")) if _fake_comm_gbs() is not None else self.world)
        released = getattr(self, "_released", {})
        base_of, acc = {}, {}
        for it, name, nbytes, ready, handle in self._bucket_events:
            base = base_of.setdefault(it, ready)
            a = acc.setdefault(name, dict(bytes=nbytes, n=0, ready=0.0, released=0.0, n_rel=0, coll=0.0, timed_by=None))
            a["n"] += 1
            a["ready"] += base.elapsed_time(ready)
            rel = released.get((it, name))
            if rel is not None:
                a["released"] += base.elapsed_time(rel)
                a["n_rel"] += 1
            try:
                ms, by = float(handle._get_duration()), "collective's own events"
            except Exception:
                ms, by = (ready.elapsed_time(rel) if rel is not None else 0.0), "ready -> released (upper bound)"
            a["coll"] += ms
            a["timed_by"] = by
        self._bucket_events = []
        self._released = {}
        out = {}
        for name, a in acc.items():
            n = a["n"]
            coll = a["coll"] / n
            out[name] = dict(MB=round(a["bytes"] / 1e6, 2), ready_us=round(1e3 * a["ready"] / n, 1),
                             released_us=None if not a["n_rel"] else round(1e3 * a["released"] / a["n_rel"], 1),
                             collective_ms=round(coll, 4), timed_by=a["timed_by"],
                             bus_GBs=None if coll <= 0 or W < 2 else round(2.0 * (W - 1) / W * a["bytes"] / (coll * 1e-3) / 1e9, 1),
                             alg_GBs=None if coll <= 0 else round(a["bytes"] / (coll * 1e-3) / 1e9, 1), probed_iterations=n)
        return out

    def loss(self):
        """Loss value of the last forward_backward (a 0-d tensor; costs a few tiny kernels, so it is on demand)."""
        self.poll_overflow()
        N, P = self._N, self.P
        lam = LAMBDA_DSSIM
        w = torch.tensor([self.w["l1"] * (1 - lam) / (3.0 * N), self.w["pbr"] * (1 - lam) / (3.0 * N),
                          self.w["normal"] / (3.0 * N), self.w["light"] / (3.0 * P), self.w["env_smooth"],
                          -self.w["l1"] * lam / (3.0 * N), -self.w["pbr"] * lam / (3.0 * N),
                          self.w["base_color_smooth"] / (3.0 * N), self.w["roughness_smooth"] / (3.0 * N),
                          self.w["light_smooth"] / (3.0 * N)], device=self.dev)
        return (self.sums.sum(1) * w).sum() + lam * (self.w["l1"] + self.w["pbr"])

    @_in_context
    def optimizer_step(self):
        """Adam on every group that trains (groups with learning rate 0 get no launch): _groups_a = shs, _groups_c = the small
        per-Gaussian groups + env, _groups_b = incidents -- indices into self.opt.groups, one tuple per gradient bucket."""
        grads = [self.grads[k] for k in self._opt_order]
        if not self.dp:
            if self._b_early:
                # the incident-light group is updated by the chain queued below, on the early stream (forward_backward,
                # "SCHEDULE"): no join here
                todo = (self._groups_a if self._a_late else ()) + self._groups_c
            elif self._early:            # the SH group was updated under the shading backward (forward_backward)
                _lib.stream_wait(torch.cuda.current_stream(), self._adam_stream)
                self._early_pending = False
                todo = self._groups_c + self._groups_b
            else:
                self.opt.begin_step()
                todo = self._groups_a + self._groups_c + self._groups_b
            self._early = self._b_early = self._a_late = False
            if todo:                     # ONE launch for every remaining group
                self.opt.step_groups(todo, grads, skip_flag=self._skip_cur)
                if set(todo) & set(self._groups_b):
                    # the coefficients change under a rotation some earlier iteration's chain may have left behind (the kernel writes
                    # through the raw pointer: the version counter _rotation_is_current() looks at does not move)
                    self._pre_rotated = None
            if self._chain_deferred is not None:
                self._run_chain()
            return
        # data parallel: update each bucket when its (sum) all-reduce has landed; 1/world is applied inside the kernel
        scale = 1.0 / self.world
        handle_a, handle_c, handle_b = self._handles
        if self._single_bucket:
            self.opt.begin_step()
            self._wait(handle_c, "ALL")
            self._skip_cur = self._snapshot_flag()
            todo = self._groups_a + self._groups_c + self._groups_b
            if todo:
                self.opt.step_groups(todo, grads, scale, skip_flag=self._skip_cur)
                self._pre_rotated = None
            return
        if self._early:                  # bucket A was waited for and applied on the side stream (forward_backward)
            torch.cuda.current_stream().wait_stream(self._adam_stream)
            self._early = False
            self._wait(handle_c, "C")
        else:
            self.opt.begin_step()
            # the overflow flag rides in the first bucket that is reduced: A, or C when the geometry is frozen
            self._wait(handle_a if handle_a is not None else handle_c, "A" if handle_a is not None else "C")
            self._skip_cur = self._snapshot_flag()      # > 0 on every rank when any rank dropped its view
            if handle_a is not None:
                if self._groups_a:
                    self.opt.step_groups(self._groups_a, grads, scale, skip_flag=self._skip_cur)
                self._wait(handle_c, "C")
        if self._groups_c:
            self.opt.step_groups(self._groups_c, grads, scale, skip_flag=self._skip_cur)
        self._pending_b = (handle_b, grads, scale, self._skip_cur, self._iter)

    def _run_chain(self):
        """Queue the incident-light chain forward_backward deferred (`_chain_deferred`) on the early stream, behind what the
        current stream holds now: rotation back of the group's gradient + its Adam update with the iteration's own step count
        + rotation of the new coefficients, one kernel; a frozen group only gets its coefficients rotated."""
        frs, skip, count = self._chain_deferred
        self._chain_deferred = None
        early = self._adam_stream
        _lib.stream_wait(early, torch.cuda.current_stream(self.dev))
        with torch.cuda.stream(early):
            if self._groups_b:
                grp = self.opt.groups[self._groups_b[0]]
                frs.incident_chain(self._incidents, self.grads["incidents"], grp["exp_avg"], grp["exp_avg_sq"], grp["lr"],
                                   grp.get("lr_tail") if grp.get("lr_tail") is not None else grp["lr"], self.opt.betas,
                                   self.opt.eps, count, 1.0, skip_flag=skip)
            else:
                frs.rotate(self._incidents)
        self._pre_rotated = (frs, self._incidents, self._incidents._version)

    @_in_context
    def flush(self):
        """Complete a deferred incident-light update: data-parallel runs apply it here; a single-GPU iteration that left it running
        on the early-Adam stream gets the CURRENT stream ordered behind it (no host wait).  A no-op otherwise."""
        if self._chain_deferred is not None:          # (somebody asks for the coefficients between forward_backward and optimizer_step)
            self._run_chain()
        if self._early_pending:
            _lib.stream_wait(torch.cuda.current_stream(self.dev), self._adam_stream)
            self._early_pending = False
        if self._pending_b is not None:
            handle_b, grads, scale, skip, it_b = self._pending_b
            self._pending_b = None
            self._wait(handle_b, "B", it=it_b)
            frs, self._dp_chain = self._dp_chain, None
            if frs is not None:
                # rotation back of the REDUCED gradient (into grads["incidents"]) + Adam with 1 / world + rotation of the new
                # coefficients, one kernel; the next shading forward finds its rotated coefficients in place
                grp = self.opt.groups[self._groups_b[0]]
                frs.incident_chain(self._incidents, self.grads["incidents"], grp["exp_avg"], grp["exp_avg_sq"], grp["lr"],
                                   grp.get("lr_tail") if grp.get("lr_tail") is not None else grp["lr"], self.opt.betas,
                                   self.opt.eps, self.opt.step_count, scale, skip_flag=skip, listed_in_dcprime=True)
                self._pre_rotated = (frs, self._incidents, self._incidents._version)
            elif self._groups_b:
                self.opt.step_groups(self._groups_b, grads, scale, skip_flag=skip)
                self._pre_rotated = None           # (see optimizer_step)

    @_in_context
    def __call__(self, cam, bg, gt, image_mask=None):
        # the SH group's Adam under the shading backward: pays while the group's 64 bytes x 48 per Gaussian mostly live in the
        # 256 MB last-level cache (300k Gaussians: 58 us of Adam for 31 us of slower shading backward); streamed from HBM it
        # costs the latency-sensitive shading kernel nearly its whole duration (2M: 0.99 ms of Adam for +0.85 ms, 159 vs 163 it/s)
        early = os.environ.get("R3DG_EARLY_ADAM", "1" if self.P <= 1_000_000 else "0") != "0" and not self.serial_streams
        outs = self.forward_backward(cam, bg, gt, early_adam=early, image_mask=image_mask, chain_incidents=True)
        self.optimizer_step()
        return outs


class FusedStage1Step(_BoundedForward):
    """Stage-1 (plain 3DGS + normals) iteration without an autograd graph: activations -> S=5 feature row -> rasterize ->
    image-space loss + gradients -> rasterize backward -> activation chain rule -> one-launch Adam.  Same computation as
    bench_core.render_stage1 + loss_stage1 + torch.optim.Adam (the parity target, tests/test_fused_step_gpu.py);
    single-bucket gradient all-reduce under data parallelism."""

    def __init__(self, params, lr=1e-4, lr_rest_scale=1.0, process_group=None, lrs=None, loss_weights=None, bounded=True):
        """`bounded`: as FusedStage2Step -- after the first iteration (and again after every densify / prune, which changes
        the count) the rasterizer forward runs without the host read-back of num_rendered; a dropped view updates nothing
        and adds nothing to the densification statistics.
        `lrs`: optional per-group learning rates {xyz, normal, scaling, rotation, opacity, shs, shs_rest} as in
        GaussianModel.training_setup (gaussian_model.py:465-472); missing names use `lr` (`lr * lr_rest_scale` for the
        non-dc SH columns).  `loss_weights`: overrides of train_step.STAGE1_WEIGHTS (the lambdas of script/run_nerf.sh:7-14).
        `self.iteration` (the reference's 1-based iteration, advanced by __call__) drives the depth-variance schedule
        (render.py:202)."""
        from .train_step import STAGE1_WEIGHTS
        dev = params.xyz.device
        self.dev = dev
        self.w = dict(STAGE1_WEIGHTS)
        if loss_weights:
            self.w.update(loss_weights)
        self.iteration = 0
        d = lambda t: t.detach().clone().contiguous()
        self.xyz, self.normal = d(params.xyz), d(params.normal)
        self.scaling, self.rotation, self.opacity = d(params.scaling), d(params.rotation), d(params.opacity)
        self.shs = torch.cat([params.features_dc.detach(), params.features_rest.detach()], 1).contiguous()
        self.M = self.shs.shape[1]
        self._zero_depth_grad = None
        self.group = process_group
        self.world, self.dp = _world_of(process_group)
        self._ctx = _lib.OptionContext()
        lrs = dict(lrs or {})
        rate = lambda k: float(lrs.get(k, lr))
        rest = float(lrs.get("shs_rest", rate("shs") * lr_rest_scale))
        self._opt_order = ("xyz", "normal", "scaling", "rotation", "opacity", "shs")
        self.opt = FusedAdam([dict(param=self.xyz, lr=rate("xyz")), dict(param=self.normal, lr=rate("normal")),
                              dict(param=self.scaling, lr=rate("scaling")), dict(param=self.rotation, lr=rate("rotation")),
                              dict(param=self.opacity, lr=rate("opacity")),
                              dict(param=self.shs, lr=rate("shs"), lr_tail=rest, period=3 * self.M, split=3)])
        self.stats = None                  # densification statistics (enable_densification)
        self.last_outs = None
        self._allocate()
        self._init_bounded(bounded, self._flag)

    def _allocate(self):
        """Per-Gaussian work buffers for the current number of Gaussians (again after every densify / prune)."""
        dev = self.dev
        self.P = P = self.xyz.shape[0]
        f = dict(dtype=torch.float32, device=dev)
        self.a_scales, self.a_rot = torch.empty(P, 3, **f), torch.empty(P, 4, **f)
        self.a_opacity, self.a_normal = torch.empty(P, 1, **f), torch.empty(P, 3, **f)
        self.features = torch.empty(P, 5, **f)
        self.sums = torch.zeros(6, SUM_SLOTS, **f)          # (R3DG_SUM_SLOTS floats each) l1, normal mse, mask entropy, SSIM(image), edge-aware normal, sqrt depth var
        names = ("shs", "xyz", "normal", "scaling", "rotation", "opacity")
        sizes = {k: getattr(self, k).numel() for k in names}
        pad4 = lambda n: (n + 3) // 4 * 4         # every group starts on a 16-byte boundary (float4 accesses in the Adam kernel)
        self.grad_flat = torch.zeros(sum(pad4(v) for v in sizes.values()) + 4, **f)
        self.grads, o = {}, 0
        for k in names:
            self.grads[k] = self.grad_flat[o:o + sizes[k]].view_as(getattr(self, k))
            o += pad4(sizes[k])
        self._flag = self.grad_flat[o:o + 4]       # overflow flag of the bounded forward: reduced with the gradients
        self._capacity = None                      # (a new Gaussian count means a new instance count: learn it again)
        self.last_outs = None

    # ---- densification (train.py:158-175; kernels in csrc/densify.hip, host mirror densify.py) ----------------------
    def enable_densification(self):
        """Start collecting the densification statistics: every forward_backward adds its view (add_densification_stats +
        max radii, train.py:160-165), from this rank's own gradients, before the gradient all-reduce is launched."""
        from . import densify
        self.stats = densify.DensificationStats(self.P, self.dev)

    def _groups(self):
        import collections
        return collections.OrderedDict(
            (k, dict(param=getattr(self, k), exp_avg=self.opt.groups[i]["exp_avg"],
                     exp_avg_sq=self.opt.groups[i]["exp_avg_sq"])) for i, k in enumerate(self._opt_order))

    def _drain(self):
        """Complete a gradient all-reduce that is still in flight (data parallel) before its buffers are replaced."""
        h = getattr(self, "_handle", None)
        if h is not None:
            h.wait()
            self._handle = None

    def _rebind(self, new, new_stats):
        self._drain()
        for i, k in enumerate(self._opt_order):
            setattr(self, k, new[k]["param"])
            g = self.opt.groups[i]
            g["param"], g["exp_avg"], g["exp_avg_sq"] = new[k]["param"], new[k]["exp_avg"], new[k]["exp_avg_sq"]
        self.stats = new_stats
        self._allocate()

    @_in_context
    def densify_and_prune(self, max_grad, min_opacity, extent, max_screen_size, max_grad_normal, percent_dense=0.01,
                          generator=None):
        """GaussianModel.densify_and_prune on the raw parameters and their Adam moments.  Under data parallelism the
        statistics are summed over ranks first (max for the radii) and every rank must pass a generator in the same state,
        so the replicas stay identical."""
        from . import densify
        if self.stats is None:
            raise RuntimeError("densify_and_prune: call enable_densification() first")
        self.stats.all_reduce(self.group)
        new, new_stats, info = densify.densify_and_prune(self._groups(), self.stats, max_grad, min_opacity, extent,
                                                         max_screen_size, max_grad_normal, percent_dense,
                                                         generator=generator)
        self._rebind(new, new_stats)
        return info

    @_in_context
    def prune(self, min_opacity, extent, max_screen_size):
        from . import densify
        if self.stats is None:
            raise RuntimeError("prune: call enable_densification() first")
        self.stats.all_reduce(self.group)
        new, new_stats, info = densify.prune(self._groups(), self.stats, min_opacity, extent, max_screen_size)
        self._rebind(new, new_stats)
        return info

    @_in_context
    def reset_opacity(self):
        """GaussianModel.reset_opacity.  The reference swaps in a fresh parameter object, so the optimizer step of the same
        iteration leaves the opacity alone (its .grad is None): the pending opacity gradient is cleared here, which with
        zeroed moments makes that Adam update exactly zero."""
        from . import densify
        g = self.opt.groups[self._opt_order.index("opacity")]
        densify.reset_opacity(self.opacity, g["exp_avg"], g["exp_avg_sq"])
        self._drain()
        self.grads["opacity"].zero_()

    features_dc = property(lambda self: self.shs[:, :1])
    features_rest = property(lambda self: self.shs[:, 1:])

    def _weights(self, N):
        """The five weights of r3dg_stage1_loss / loss(), each already divided by the element count of its mean."""
        from .train_step import depth_var_weight
        w = self.w
        return ((1.0 - LAMBDA_DSSIM) * w["l1"] / (3.0 * N), w["mask_entropy"] / N, w["normal_render_depth"] / (3.0 * N),
                w["normal_smooth"] / (3.0 * N), depth_var_weight(w["depth_var"], self.iteration) / N)

    @_in_context
    def forward_backward(self, cam, bg, gt, image_mask=None):
        """`image_mask` [1,H,W] (the view's object mask, scene/cameras.py image_mask; None = all ones)."""
        L = _lib.lib()
        P, dev = self.P, self.dev
        H, W = cam.image_height, cam.image_width
        N = H * W
        stream = _lib.current_stream
        vm = cam.world_view_transform.contiguous()
        campos = cam.camera_center.contiguous()
        empty = torch.Tensor([])
        with torch.cuda.device(dev):
            _lib.check(L.r3dg_stage2_activate(
                stream(), P, self.xyz.data_ptr(), self.scaling.data_ptr(), self.rotation.data_ptr(),
                self.opacity.data_ptr(), self.normal.data_ptr(), None, None, None, self.a_scales.data_ptr(),
                self.a_rot.data_ptr(), self.a_opacity.data_ptr(), self.a_normal.data_ptr(), None, None, None, None, None),
                "stage2_activate")
            self._iter += 1
            flag_cur = self._flag_cur = self._flag_of_iteration()
            use_bounded = self._use_bounded(W, H)
            if not use_bounded:
                flag_cur.zero_()
            pending = rasterizer_ops.rasterize_gaussians_begin(
                bg, self.xyz, self.features, empty, self.a_opacity, self.a_scales, self.a_rot, 1.0, empty, vm,
                cam.full_proj_transform, cam.tanfovx, cam.tanfovy, cam.cx, cam.cy, H, W, self.shs, 3, campos, False,
                True, False, **(dict(capacity=self._capacity, overflow_flag=flag_cur,
                                     overflow_count=self._overflow_count) if use_bounded else {}))
            _lib.check(L.r3dg_stage1_pack_features(stream(), P, self.xyz.data_ptr(), vm.data_ptr(),
                                                   self.a_normal.data_ptr(), self.features.data_ptr()),
                       "stage1_pack_features")
            self.sums.zero_()
            fw = pending.finish()
            R, n_contrib, image, opacity, depth, feature, pseudo_normal, sxyz, weights, radii, geom, binning, img = fw
            # dL_dimage 3 | dL_dopacity 1 | dL_dfeature 5 | SSIM partials 9 | SSIM gradient 3 | edge-aware scratch 6
            g = torch.empty((27, H, W), dtype=torch.float32, device=dev)
            if self._zero_depth_grad is None or self._zero_depth_grad.shape[-2:] != (H, W):
                self._zero_depth_grad = torch.zeros((1, H, W), dtype=torch.float32, device=dev)
            gt_c = gt.contiguous()
            lam = LAMBDA_DSSIM
            _lib.check(L.r3dg_ssim_forward(stream(), W, H, 3, image.data_ptr(), gt_c.data_ptr(), g[9:18].data_ptr(),
                                           self.sums[3].data_ptr()), "ssim_forward")
            _lib.check(L.r3dg_ssim_backward(stream(), W, H, 3, image.data_ptr(), gt_c.data_ptr(), g[9:18].data_ptr(),
                                            -lam * self.w["l1"] / (3.0 * N), g[18:21].data_ptr()), "ssim_backward")
            w_l1, w_ent, w_nrm, w_smooth, w_var = self._weights(N)
            mask_c = None if image_mask is None else image_mask.contiguous()
            _lib.check(L.r3dg_stage1_loss(
                stream(), W, H, image.data_ptr(), opacity.data_ptr(), feature.data_ptr(), pseudo_normal.data_ptr(),
                n_contrib.data_ptr(), gt_c.data_ptr(), _lib.ptr(mask_c), w_l1, w_ent, w_nrm, w_smooth, w_var,
                g[18:21].data_ptr(), g[21:27].data_ptr(), g[0:3].data_ptr(), g[3:4].data_ptr(), g[4:9].data_ptr(),
                self.sums.data_ptr()), "stage1_loss")
            bw = rasterizer_ops.rasterize_gaussians_backward(
                bg, self.xyz, self.features, radii, empty, self.a_scales, self.a_rot, 1.0, empty, vm,
                cam.full_proj_transform, cam.tanfovx, cam.tanfovy, g[0:3], g[3:4], empty, g[4:9],        # (empty: no depth gradient)
                self.shs, 3, campos, geom, R, binning, img, True, False, dL_dsh_out=self.grads["shs"],
                # the normal maps carry the two normal terms, depth / depth^2 the variance term
                active_features=(0, 1, 2, 3, 4) if w_var != 0.0 else (0, 1, 2))
            dL_dmeans2D, _dcol, dL_dopacity, dL_dmeans3D, dL_dfeatures, _dcov, _dsh, dL_dscales, dL_drot = bw
            gr = self.grads
            _lib.check(L.r3dg_stage1_activate_backward(
                stream(), P, self.xyz.data_ptr(), self.scaling.data_ptr(), self.rotation.data_ptr(),
                self.opacity.data_ptr(), self.normal.data_ptr(), vm.data_ptr(), dL_dfeatures.data_ptr(),
                dL_dscales.data_ptr(), dL_drot.data_ptr(), dL_dopacity.data_ptr(), dL_dmeans3D.data_ptr(),
                gr["xyz"].data_ptr(), gr["scaling"].data_ptr(), gr["rotation"].data_ptr(), gr["opacity"].data_ptr(),
                gr["normal"].data_ptr()), "stage1_activate_backward")
            if self.stats is not None:           # this view's densification statistics, from the LOCAL gradients
                self.stats.add(dL_dmeans2D, gr["normal"], radii, weights, skip_flag=flag_cur)
            self._handle = None
            if self.dp:
                self._handle = torch.distributed.all_reduce(self.grad_flat, group=self.group, async_op=True)
        self.viewspace_grad = dL_dmeans2D
        self._note_count(geom, R, use_bounded)
        self.last_outs = (R, n_contrib, image, opacity, depth, feature, pseudo_normal, sxyz, weights, radii)
        self._N = N
        return self.last_outs

    def loss(self):
        self.poll_overflow()
        N = self._N
        lam = LAMBDA_DSSIM
        w_l1, w_ent, w_nrm, w_smooth, w_var = self._weights(N)
        w = torch.tensor([w_l1, w_nrm, w_ent, -lam * self.w["l1"] / (3.0 * N), w_smooth, w_var], device=self.dev)
        return (self.sums.sum(1) * w).sum() + lam * self.w["l1"]

    @_in_context
    def optimizer_step(self):
        self._drain()
        skip = self._snapshot_flag() if (self.dp and self.bounded) else self._flag_cur
        self.opt.step([self.grads[k] for k in self._opt_order], 1.0 / self.world, skip_flag=skip)

    @_in_context
    def flush(self):
        pass

    @_in_context
    def __call__(self, cam, bg, gt, image_mask=None):
        self.iteration += 1
        outs = self.forward_backward(cam, bg, gt, image_mask)
        self.optimizer_step()
        return outs
