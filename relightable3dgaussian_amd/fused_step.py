"""Fused stage-2 training iteration: the same computation as train_step.Stage2Step + loss.backward()
+ Adam, but with the ~250 elementwise PyTorch launches around the hot ops replaced by the streaming HIP kernels of
csrc/stage2_glue.hip, smooth.hip and adam.hip and without an autograd graph: forward, loss, backward and optimizer are explicit calls in order.

    GaussianModel activations + viewdirs,     r3dg_stage2_activate_with        (scene/gaussian_model.py:183-232, neilf.py:74-76,
      softplus of the env texture, sum reset                                      direct_light_map.py:18-27)
    shading integral                          r3dg_shade_frs_forward (fixed ray set) / r3dg_shade_forward_cached (neilf.py:339-371)
    S=16 feature row + light-smoothness sum   written by the two launches above; r3dg_stage2_pack_features behind the general
                                              shading kernel                   (neilf.py:115-122, 286-292)
    rasterize                                 r3dg_rasterize_forward_*         (r3dg_rasterization.py:75-113)
    the image tail, one launch                r3dg_stage2_image_tail (where the library has it; otherwise, and with
                                              R3DG_IMAGE_TAIL=0, the three rows below)
    pseudo normals + sRGB-mapped PBR image    r3dg_stage2_normals_srgb
    SSIM of the image and the PBR image       r3dg_ssim_forward_pair / r3dg_ssim_backward_pair
    image-space loss terms + their gradients  r3dg_stage2_loss (+ r3dg_stage2_smooth_fused, + r3dg_stage2_supervision when the
                                              MVS depth / normal terms are on)  (neilf.py:212-318)
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
The parity target is the unfused path (tests/test_fused_step_gpu.py compares loss and every gradient).

Beside this module: fused_adam (the one-launch Adam), fused_base (what the two iterations share), grad_comm (the data-parallel
bucket all-reduces and their measurement), fused_samples (the owner of the traced visibility, the ray set and the lookup cache
of the P x K samples), fused_stage1 (the stage-1 iteration with densification)."""
import collections
import contextlib
import os

import torch
import torch.nn.functional as F

from . import _lib, rasterizer_ops, shading_ops
from .fused_adam import AdamGroup, FusedAdam                                              # noqa: F401  (re-exported)
from .fused_base import _STREAMS, SUM_SLOTS, FusedStepBase, _in_context, _world_of, grad_slab, learning_rates, shared_stream  # noqa: F401
from .fused_samples import SampleSet, of_samples
from .fused_stage1 import FusedStage1Step                                                 # noqa: F401  (re-exported)
from .grad_comm import BucketComm
from .shading_ops import LEAVE_ROOM, TRAIN_OUTPUTS
from .train_step import FROZEN_GEOMETRY_GROUPS, LAMBDA_DSSIM, STAGE2_WEIGHTS, update_visibility, update_visibility_device

PARAM_NAMES = ("xyz", "normal", "scaling", "rotation", "opacity", "shs", "base_color", "roughness", "incidents", "env")

# what the phases of forward_backward see of the view (`main` / `raw`: the caller's stream, looked up ONCE: 10 us of Python each)
_View = collections.namedtuple("_View", "cam bg gt mask H W N vm campos main raw order_stream gt_depth mvs_normal")


class FusedStage2Step(FusedStepBase):
    """Owns the raw parameters (copied from a bench_core.GaussianParams) and runs whole iterations."""

    # whole single-GPU iterations close the incident-light group with ONE chain kernel (read by bench_core's --full attribution)
    _chain_kernel = True
    _opt_order = PARAM_NAMES

    def __init__(self, params, sample_num, lr=1e-4, lr_rest_scale=1.0, loss_weights=None, process_group=None, lrs=None,
                 bounded=True, device_visibility=False):
        """`lrs`: optional per-group learning rates {xyz, normal, scaling, rotation, opacity, shs, shs_rest, base_color,
        roughness, incidents, incidents_rest, env} as GaussianModel.training_setup / DirectLightMap.training_setup set
        them (scene/gaussian_model.py:465-486, the stage-2 values of script/run_nerf.sh:25-31; fused_base.learning_rates).
        `bounded`: after the first iteration (which reads num_rendered like the reference) the rasterizer forward runs
        WITHOUT the host read-back: binning state sized for twice the largest count seen, projection + instance ordering
        queued at once beside the shading forward.  A view that needs more is dropped on the device (its Adam launches
        read the flag and update nothing); `poll_overflow()` -- called by loss() -- then doubles the capacity and counts
        it in `dropped_steps`.
        `loss_weights`: overrides of train_step.STAGE2_WEIGHTS (the lambdas of script/run_nerf.sh:20-39);
        train_step.STAGE2_WEIGHTS_SYN4 adds the three edge-aware smoothness terms of script/run_syn4.sh / run_dtu.sh.
        `depth` / `normal_mvs_depth` (lambda_depth / lambda_normal_mvs_depth, neilf.py:241-249, :266-273; 0 by default) switch on
        the supervision by the view's MVS depth map and normals, which forward_backward / __call__ then take as `gt_depth` /
        `mvs_normal` (csrc/supervision.hip); with both at 0 nothing of it is allocated or launched.
        FROZEN GEOMETRY: a group whose learning rate(s) are 0 gets no Adam launch; when ALL of xyz, normal, scaling,
        rotation, opacity and shs are frozen (run_syn4.sh:27-33, run_dtu.sh:29-35) the iteration also skips what only they
        would consume -- the alpha-gradient half of the tile backward and the whole per-Gaussian geometry backward
        (r3dg_rasterize_backward_features instead), the geometry half of the activation chain rule, their all-reduce
        buckets -- and their entries of `grads` stay zero.
        `device_visibility`: the visibility is traced by train_step.update_visibility_device (the rays are generated inside the
        trace kernel) instead of update_visibility; while the fixed-ray-set shading kernels apply, `incident_dirs` and
        `incident_areas` stay None -- no [P,K,3] tensor exists.  `refresh_visibility()` re-traces with the current parameters in
        either mode."""
        unknown = set(loss_weights or ()) - set(STAGE2_WEIGHTS)
        if unknown:                                  # (before anything is created)
            raise RuntimeError("FusedStage2Step: unknown loss weights %s" % sorted(unknown))
        dev = params.xyz.device
        # instance ordering of the rasterizer runs on the ordering stream, under the shading forward (register-light,
        # latency-bound kernels next to a VALU-bound one)
        super().__init__(params, [k for k in PARAM_NAMES if k not in ("shs", "incidents")], process_group,
                         *_world_of(process_group), bounded, order_stream=shared_stream(dev, "order"))
        P, self.K = self.P, sample_num
        self._incidents = torch.cat([params.incidents_dc.detach(), params.incidents_rest.detach()], 1).contiguous()
        if self._incidents.shape[1] != self.M:      # the reference gives both the same degree (gaussian_model.py:421, :450)
            raise RuntimeError("FusedStage2Step: colour and incident-light SH must hold the same number of coefficients")
        # the baked-visibility SH groups (visibility_bake.bake_visibility): carried for checkpoint.capture, read by no kernel here
        for k in ("visibility_dc", "visibility_rest"):
            t = getattr(params, k, None)
            setattr(self, k, None if t is None else t.detach().clone().contiguous())
        # script/run_nerf.sh:20-39 (stage 2): lambda_pbr 1, lambda_light 0.01, lambda_env_smooth 0.01; the command does not
        # pass --lambda_normal_render_depth, so that term is off (arguments/__init__.py:115) -- opt in with
        # loss_weights={"normal": 0.01}; the edge-aware smoothness terms are 0 there and 1 / 0.5 / 1 in run_syn4.sh / run_dtu.sh
        self.w = dict(STAGE2_WEIGHTS, **(loss_weights or {}))
        rate, tail = learning_rates(lr, lrs, lr_rest_scale)
        # groups that do not train (both rates 0 for the two SH tensors)
        self.frozen = {k for k in PARAM_NAMES if rate(k) == 0.0 and (k not in ("shs", "incidents") or tail(k) == 0.0)}
        self.frozen_geometry = all(k in self.frozen for k in FROZEN_GEOMETRY_GROUPS)
        f = dict(dtype=torch.float32, device=dev)
        self.a_scales, self.a_rot = torch.empty(P, 3, **f), torch.empty(P, 4, **f)
        self.a_opacity, self.a_normal = torch.empty(P, 1, **f), torch.empty(P, 3, **f)
        self.a_base, self.a_rough = torch.empty(P, 3, **f), torch.empty(P, 1, **f)
        self.a_viewdirs = torch.empty(P, 3, **f)
        self.shade_out = torch.empty(P, shading_ops.NOUT, **f)
        self.features = torch.zeros(P, 16, **f)     # (zero-filled once: the pack kernels write the active channels only)
        # unweighted sums: l1, pbr l1, normal mse, light l1, TV(env), SSIM(image), SSIM(pbr), and the three edge-aware
        # smoothness sums (base colour, roughness, diffuse light)
        # (+ with an MVS term on: the depth L1 sum over the selected pixels, the squared MVS-normal difference sum)
        self._supervised = self.w["depth"] != 0.0 or self.w["normal_mvs_depth"] != 0.0
        self.sums = torch.zeros(12 if self._supervised else 10, SUM_SLOTS, **f)   # R3DG_SUM_SLOTS floats per quantity (include/r3dg_hip.h)
        self._sup_counts = {}                       # id(gt_depth) -> (gt_depth, image mask, their versions, the device count)
        self._sup_count_cur = None                  # the count the last forward_backward's depth term divided by
        self.d_pbr, self.d_diffuse = torch.empty(P, 3, **f), torch.empty(P, 3, **f)
        self._absmax = torch.zeros((P + 255) // 256, **f)       # block maxima of |d_pbr|, |d_diffuse| (unpack kernel)
        # flat gradient slab: [shs 3M | xyz3 normal3 scaling3 rotation4 opacity1 base3 rough1 per Gaussian, env texture |
        # incidents 3M].  `flag`: the bounded forward's overflow flag rides at the end of bucket A, so that under data
        # parallelism the first all-reduce tells every rank whether ANY rank dropped its view (sum > 0) before the first Adam launch
        geo = ("xyz", "normal", "scaling", "rotation", "opacity")
        if self.frozen_geometry:
            # nothing of the frozen groups is reduced or updated: [flag, base_color, roughness, env | incidents | the rest]
            order = ("flag", "base_color", "roughness", "env", "incidents", "shs") + geo
        else:
            order = ("shs", "flag") + geo + ("base_color", "roughness", "env", "incidents")
        raw = {k: self._incidents if k == "incidents" else getattr(self, k) for k in PARAM_NAMES}
        self.grad_flat, self.grads, start = grad_slab(order, raw, dev)
        self._flag = self.grads.pop("flag")
        self._skip_cur = None
        # three all-reduce buckets (world > 1): A = SH colour grads, final right after the rasterizer backward (reduced
        # under the shading backward); C = the small per-Gaussian groups, final after the activation chain rule;
        # B = incident-light grads, final after the shading backward -- reduced LAST and only waited for right before
        # the NEXT iteration's shading forward, so it travels under that iteration's projection + binning
        # (the env texture's gradient rides in bucket C: one collective instead of a separate 6 KB all-reduce)
        flat, s_inc = self.grad_flat, start["incidents"]
        if self.frozen_geometry:    # (no SH colour gradient to send early; C = flag + base colour, roughness, env texture)
            self._bucket_a, self._bucket_c, self._bucket_b = None, flat[:s_inc], flat[s_inc:start["shs"]]
            self._bucket_all = flat[:start["shs"]]
        else:
            self._bucket_a, self._bucket_c, self._bucket_b = flat[:start["xyz"]], flat[start["xyz"]:s_inc], flat[s_inc:]
            self._bucket_all = flat
        self._comm = BucketComm(dev, process_group, self.world, self.dp)
        self.exposed_comm_ms, self.comm_table = self._comm.exposed_comm_ms, self._comm.comm_table
        self._handles = self._pending_b = None      # (world > 1) the work handles of buckets A, C, B; the deferred incident-light update
        # the tile backward's accumulator slab (no zero fill: its scatter pass writes every element)
        self._acc = torch.empty((11 + 16) * P, **f)
        self._early_pending = False                 # the early-Adam stream holds work no other stream has been ordered behind yet
        # the iteration's schedule (forward_backward): work on the early stream, the incident-light chain queued there, the SH
        # group updated with the others although the chain is queued
        self._early = self._b_early = self._a_late = False
        self._dp_chain = None                       # data parallel: the ray set whose chain kernel closes this iteration's bucket B
        self._env_c = self._d_env = None            # softplus(environment texture) (_front_end), its gradient accumulator
        self._records = None                        # the tile backward's gradient records, while they are left in place
        self._adam_stream = self._geo_done = None   # the early-Adam stream, created at first use (_early_stream); the geometry backward's event
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
        self.last_active_features = None            # feature maps the last backward consumed (bench.py prices the launch with these)
        # R3DG_DP_BUCKETS=1 (A/B, message size against overlap): ONE all-reduce of the whole gradient slab behind the backward
        # and one Adam launch behind it, instead of the three buckets A / C / B each sent the moment it is final
        self._single_bucket = self.dp and os.environ.get("R3DG_DP_BUCKETS", "3") == "1"
        # the P x K samples: traced visibility, direction caches, snapshot normals, ray set and lookup cache (fused_samples)
        # (the two traces by THIS module's names: what tests replace here reaches the owner)
        self._samples = SampleSet(sample_num, self.M, (update_visibility, update_visibility_device), process_group, device_visibility)
        with torch.no_grad(), self._ctx:
            self.refresh_activations()
            self._samples.acquire(self.xyz, self.a_scales, self.a_rot, self.a_opacity, self.a_normal)
        # incident-light chain of a whole single-GPU iteration: (ray set, coefficient tensor, its version) the rotated coefficients
        # in the ray set were computed FROM, when that was done ahead of the next iteration; work still running on the early stream
        self._pre_rotated = None
        self._chain_deferred = None                 # (ray set, skip flag, Adam step count) of the chain optimizer_step queues
        two_rates = lambda k: dict(lr_tail=tail(k), period=3 * self.M, split=3) if k in ("shs", "incidents") else {}
        self.opt = FusedAdam([dict(param=raw[k], lr=rate(k), **two_rates(k)) for k in self._opt_order])
        # Adam launches of an iteration: the groups of each gradient bucket that train
        live = lambda idx: tuple(i for i in idx if self._opt_order[i] not in self.frozen)
        self._groups_a, self._groups_c, self._groups_b = live((5,)), live((0, 1, 2, 3, 4, 6, 7, 9)), live((8,))

    # what tests, tools, the training loop and the benchmark read, swap and drop on the step (SampleSet.select notices)
    visibility, incident_dirs, incident_areas, tracer, device_visibility = map(of_samples, (
        "visibility", "incident_dirs", "incident_areas", "tracer", "device_visibility"))
    visibility_refreshes, _ray_normals, _frs, _taps, _taps_src, _uniform_area = map(of_samples, (
        "refreshes", "ray_normals", "frs", "taps", "src", "uniform_area"))

    incidents_dc = property(lambda self: self.incidents[:, :1])
    incidents_rest = property(lambda self: self.incidents[:, 1:])

    # The incident-light coefficients as everybody OUTSIDE the iteration sees them.  A whole single-GPU iteration (__call__) leaves
    # their Adam update -- and the rotation of the new coefficients for the next iteration -- running on the early-Adam stream
    # (see _schedule_early: "incident-light chain"); a reader on any other stream must be ordered behind it first.
    @property
    def incidents(self):
        if self._early_pending:
            self.flush()
        return self._incidents

    @incidents.setter
    def incidents(self, value):
        if self._early_pending:
            self.flush()
        self._incidents = value
        self._pre_rotated = None

    measure_comm = property(lambda self: self._comm.measure_comm, lambda self, v: setattr(self._comm, "measure_comm", v))
    comm_probe_every = property(lambda self: self._comm.comm_probe_every,
                                lambda self, v: setattr(self._comm, "comm_probe_every", v))

    # GaussianModel-style accessors (plain PyTorch; used by eval / relight code, not by the fused iteration)
    get_scaling = lambda self: torch.exp(self.scaling)                           # noqa: E731
    get_rotation = lambda self: F.normalize(self.rotation)                       # noqa: E731
    get_opacity = lambda self: torch.sigmoid(self.opacity)                       # noqa: E731
    get_shs = lambda self: self.shs                                              # noqa: E731
    get_normal = lambda self: F.normalize(self.normal, dim=-1, eps=1e-3)         # noqa: E731

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
                # the nine columns of the feature rows that do not wait for the shading integral (see _shade_forward)
                cam.world_view_transform.contiguous().data_ptr() if cam is not None and self._direct_rows else None,
                self.features.data_ptr() if cam is not None and self._direct_rows else None,
                0 if env_out is None else env_out.numel(), None if env_out is None else self.env.data_ptr(),
                None if env_out is None else env_out.data_ptr(), None if zero is None else zero.data_ptr(),
                0 if zero is None else zero.numel())
        _lib.check(st, "stage2_activate")

    @_in_context
    def refresh_visibility(self):
        """Re-trace the visibility with the CURRENT parameters (the reference's commented-out "Every 1000 update visibility",
        train.py:110-112), on the device path whichever way the step was constructed: deferred work is completed, the activations
        are recomputed, the P x K rays are generated from the current normals and traced, the snapshot normals are replaced and
        the ray set / lookup cache is rebuilt for the texture size in use (SampleSet.refresh).  Parameters, gradients, Adam moments
        and step counts are untouched.  Data parallel: every rank calls it at the same iteration (one all-gather inside)."""
        self.flush()
        self.refresh_activations()
        self._samples.refresh(self.xyz, self.a_scales, self.a_rot, self.a_opacity, self.a_normal)
        self._pre_rotated = None                    # (the rotated coefficients belonged to the old ray set)

    def taps(self, He, We):
        """SampleSet.select: the general shading kernels' lookup cache for a He x We environment texture, or None when the
        fixed-ray-set kernels run (`_samples.frs`)."""
        return self._samples.select(He, We)

    def _rotation_is_current(self):
        """The ray set already holds the rotation of the CURRENT coefficients (queued on the early-Adam stream right behind their
        Adam update, at the end of the previous iteration)?  Keyed on the tensor and its version counter: anything that replaces or
        edits the coefficients in between (a checkpoint load, a test) invalidates it -- the Adam kernel itself writes through the raw
        pointer and does not count."""
        pr = self._pre_rotated
        return pr is not None and pr[0] is self._samples.frs and pr[1] is self._incidents and pr[2] == self._incidents._version

    def _early_stream(self):
        """The early-Adam stream (the process's shared "early" stream), created at first use."""
        if self._adam_stream is None:
            self._adam_stream = shared_stream(self.dev, "early")
        return self._adam_stream

    def _aux_stream(self):
        """The early-Adam stream, for the side work of the fixed-ray-set path on one GPU; None without that path and under data
        parallelism (the stream then carries the buckets' waits and the coefficients are updated late, in flush())."""
        if self._samples.frs is None or self.dp or self.serial_streams:
            return None
        return self._early_stream()

    def _listed_stream(self):
        """The early-Adam stream when the fixed-ray-set path has Gaussians off the rotated path: their general kernels run there in
        the forward, and the rasterizer's geometry backward beside them in the backward (data-parallel runs too: the stream is
        idle during the forward, and in the backward bucket A's all-reduce is issued from it, behind the geometry backward)."""
        frs = self._samples.frs
        if frs is None or frs.n_invalid == 0 or self.serial_streams:
            return None
        return self._early_stream()

    @_in_context
    def forward_backward(self, cam, bg, gt, early_adam=False, image_mask=None, split_geometry=None, chain_incidents=False,
                         gt_depth=None, mvs_normal=None, sh_adam_in_backward=False, gradient_records=False):
        """One forward + loss + backward; gradients land in self.grads.  Returns the rasterizer's 10 public outputs.
        A bare call leaves EVERY entry of `grads` holding this view's gradient.  As part of a whole iteration (__call__) two
        entries do not: grads["shs"] and grads["incidents"] are then not written at all (see `sh_adam_in_backward` and
        optimizer_step) -- they keep whatever an earlier bare call or schedule left in them.
        `image_mask` [1,H,W]: the view's object mask (Camera.image_mask; None = all ones) of the normal and smoothness terms.
        `gt_depth` [1,H,W], `mvs_normal` [3,H,W]: the view's MVS depth map and the normals derived from it (Camera.depth /
        Camera.normal); required by the `depth` / `normal_mvs_depth` terms (both need the depth map), ignored without them.
        `early_adam` (single-GPU whole iterations only, see __call__): the SH colour coefficients, whose gradient is final
        after the rasterizer backward, get their Adam update on a side stream UNDER the shading backward (an HBM-bound,
        register-light kernel next to a VALU-bound one); optimizer_step() then updates the remaining groups.
        `split_geometry` (default: `early_adam`): the rasterizer's per-Gaussian geometry backward on the early stream, beside the
        gradient unpack and the listed Gaussians' shading backward.  (Measured on its own at 2M Gaussians, where the early Adam is
        off: 160.7 vs 166.3 it/s -- both kernels stream from HBM there and slow each other by more than the overlap buys.)
        `chain_incidents` (whole iterations only, see __call__; implied by `early_adam`): the incident-light gradient may stay in
        the rotated frame for the chain kernel that optimizer_step launches -- a caller of a bare forward_backward reads
        grads["incidents"] in the world frame, always.
        `sh_adam_in_backward` (whole iterations only, see __call__ and _fuses_sh_adam): the rasterizer's per-Gaussian geometry
        backward applies the SH colour group's Adam itself, from the gradient rows it holds on chip; there is no Adam launch for
        the group and grads["shs"] is not written.
        `gradient_records` (whole iterations only, see __call__ and _reads_gradient_records): the tile backward's per-Gaussian
        gradient records are not scattered into arrays; the geometry backward, the gradient unpack and the activation chain rule
        read their Gaussian's record row themselves, and the last of them zeroes it.  Same gradients, one launch and 71 MB (300k
        Gaussians) less on the serial stretch behind the tile backward.  A bare call fills every array, as ever."""
        H, W = cam.image_height, cam.image_width
        if self._supervised and (gt_depth is None or (self.w["normal_mvs_depth"] != 0.0 and mvs_normal is None)):
            raise RuntimeError("FusedStage2Step: the depth / normal_mvs_depth terms need gt_depth%s" % (
                "" if self.w["normal_mvs_depth"] == 0.0 else " and mvs_normal"))
        main = torch.cuda.current_stream(self.dev)
        v = _View(cam, bg, gt, image_mask, H, W, H * W, cam.world_view_transform.contiguous(), cam.camera_center.contiguous(),
                  main, main.cuda_stream, None if self.serial_streams else self._order_stream, gt_depth, mvs_normal)
        with torch.cuda.device(self.dev):
            pending, env_c, flag_cur, use_bounded, rotated_for = self._front_end(v)
            taps, packed = self._shade_forward(v, env_c, rotated_for)
            fw = pending.finish(v.order_stream)
            # the Adam launches of this iteration skip themselves when the view was dropped; under data parallelism they
            # read a snapshot of the flag taken after bucket A's all-reduce (_schedule_early / optimizer_step)
            self._skip_cur = flag_cur
            g, active = self._image_loss(v, fw)
            fused_a = sh_adam_in_backward and self._fuses_sh_adam()
            dL_dfeatures, bw, geo_stream, handle_a = self._raster_backward(
                v, fw, g, active, early_adam if split_geometry is None else split_geometry, fused_a,
                gradient_records and self._reads_gradient_records())
            b_early = self._schedule_early(v, handle_a, geo_stream, use_bounded, early_adam, chain_incidents, fused_a)
            self._shade_backward(v, env_c, taps, packed, dL_dfeatures, bw, geo_stream, b_early, chain_incidents)
            self._remaining_buckets(handle_a)
        return self._end_forward_backward(fw, None if bw is None else bw[0], use_bounded, v.N)

    def _front_end(self, v):
        """-> (the pending rasterizer forward, softplus(env texture), this iteration's overflow flag slot, bounded forward?, the ray
        set whose rotated coefficients are in place or queued).  The rotation of the incident-light coefficients into the ray
        frames depends on nothing of this view: it goes to the side stream now and runs beside the activations and the
        projection instead of in front of the shading forward."""
        rotated_for = None
        aux = self._aux_stream()
        if self._chain_deferred is not None:
            self.flush()         # (forward_backward was called twice without optimizer_step: the pending chain runs now)
        if aux is not None:
            _lib.stream_wait(aux, v.main)
            # (normally the previous iteration's incident-light chain left the rotated coefficients in place: _run_chain)
            rotated_for = self._samples.frs      # (the PREVIOUS iteration's choice: this one's texture size is asked in _shade_forward)
            if not self._rotation_is_current():
                with torch.cuda.stream(aux):
                    rotated_for.rotate(self._incidents)
        # softplus(environment texture) (DirectLightMap.get_env) [He,We,3]: filled by the activation launch below, read by the
        # shading kernels and the texture's chain rule
        if self._env_c is None or self._env_c.shape != self.env.shape[1:]:
            self._env_c = torch.empty(tuple(self.env.shape[1:]), dtype=torch.float32, device=self.dev)
        env_c = self._env_c
        self.refresh_activations(v.cam, env_out=env_c, zero=self.sums)
        self._iter += 1
        flag_cur = self._flag_of_iteration()
        use_bounded = self._use_bounded(v.W, v.H)
        if self._early_pending and (aux is None or not (use_bounded and v.order_stream is not None)):
            # (the previous iteration left work on the early stream that only the bounded, three-stream schedule is ordered
            # behind by construction: any other schedule joins it here)
            _lib.stream_wait(v.main, self._adam_stream)
            self._early_pending = False
        if use_bounded:
            # projection + instance ordering go to the ordering stream NOW, beside the shading kernels; nobody waits for the count
            bounded = dict(capacity=self._capacity, overflow_flag=flag_cur, overflow_count=self._overflow_count,
                           ordering_stream=v.order_stream)
        else:
            # projection + async read-back of num_rendered: the shading kernels run while the host waits for the count
            flag_cur.zero_()
            bounded = {}
        cam, empty = v.cam, torch.Tensor([])
        pending = rasterizer_ops.rasterize_gaussians_begin(
            v.bg, self.xyz, self.features, empty, self.a_opacity, self.a_scales, self.a_rot, 1.0, empty, v.vm,
            cam.full_proj_transform, cam.tanfovx, cam.tanfovy, cam.cx, cam.cy, v.H, v.W, self.shs, 3, v.campos, False,
            True, False, want_weights=False,       # (stage 2 does not densify: nobody reads the blend weights)
            defer_pseudo_normal=True, **bounded)
        if self._pending_b is not None:
            self.flush()    # (world > 1) the previous iteration's incident-light update lands here
        if aux is not None:
            _lib.stream_wait(v.main, aux)
            self._early_pending = False          # (aux IS the early stream: the main stream is behind all of it now)
        return pending, env_c, flag_cur, use_bounded, rotated_for

    def _shade_forward(self, v, env_c, rotated_for):
        """Shading integral + S=16 feature rows.  -> (the general kernels' lookup cache or None, a pack kernel wrote the rows?)."""
        L = _lib.lib()
        He, We = env_c.shape[0], env_c.shape[1]
        sm = self._samples
        taps = sm.select(He, We)
        frs, area = sm.frs, sm.uniform_area         # (this iteration's choice, from here on)
        if frs is not None:
            # (select() may have rebuilt the ray set: then it rotates itself; data parallel: flush() above ran the chain kernel)
            rotated = rotated_for is frs or (self.dp and self._rotation_is_current())
            frs.forward(self.a_base, self.a_rough, self.a_normal, self.a_viewdirs, self._incidents, env_c,
                        sm.visibility, self.shade_out, uniform_area=area,
                        # (one workgroup per CU beside the instance ordering while THAT is the longer path: 806 vs 801
                        # it/s without the cap, frozen geometry (run_syn4.sh) 835 vs 826.  Not under data parallelism,
                        # where the deferred incident-light update sits in front of this kernel: 558 -> 568 it/s on one
                        # rank without the cap)
                        leave_room=v.order_stream is not None and not self.dp,
                        # the few hundred Gaussians off the rotated path: their general kernel on the (idle) early-Adam
                        # stream beside the rotation and the main kernel, joined below before the features are packed
                        listed_stream=self._listed_stream(), rotated=rotated,
                        feature_rows=self.features if self._direct_rows else None)
        else:
            _lib.check(L.r3dg_shade_forward_cached(
                v.raw, self.P, self.K, self.M, self.a_base.data_ptr(), self.a_rough.data_ptr(), self.a_normal.data_ptr(),
                self.a_viewdirs.data_ptr(), self._incidents.data_ptr(), env_c.data_ptr(), He, We, None,
                sm.visibility.data_ptr(), sm.incident_dirs.data_ptr(),
                None if area is not None else sm.incident_areas.data_ptr(), area or 0.0,
                taps.data_ptr(), TRAIN_OUTPUTS | (LEAVE_ROOM if v.order_stream is not None else 0),
                self.shade_out.data_ptr()), "shade_forward")
        if frs is not None and self._listed_stream() is not None:
            _lib.stream_wait(v.main, self._listed_stream())
        packed = not (frs is not None and self._direct_rows)
        if packed:
            _lib.check(L.r3dg_stage2_pack_features(v.raw, self.P, self.xyz.data_ptr(), v.vm.data_ptr(), self.a_normal.data_ptr(),
                self.a_base.data_ptr(), self.a_rough.data_ptr(), self.shade_out.data_ptr(), self.features.data_ptr(),
                self.sums[3].data_ptr()), "stage2_pack_features")
        return taps, packed

    def _image_loss(self, v, fw):
        """Image-space loss terms and their gradients.  -> (the gradient slab `g`: dL_dimage 3 | dL_dopacity 1 | dL_dfeature 16
        (the depth image carries no loss) -- and behind them, on the four-launch path only, its scratch: sRGB PBR image 3 | SSIM
        partials 2x9 | SSIM gradients 2x3 --, the feature maps that carry a gradient)."""
        L = _lib.lib()
        cam, W, H, N = v.cam, v.W, v.H, v.N
        _R, n_contrib, image, opacity, depth, feature, pseudo_normal, sxyz = fw[:8]
        gt_c, bg_c = v.gt.contiguous(), v.bg.contiguous()
        mask_c = None if v.mask is None else v.mask.contiguous()
        lam = LAMBDA_DSSIM
        w_l1, w_pbr, w_n = (self.w["l1"] * (1.0 - lam) / (3.0 * N), self.w["pbr"] * (1.0 - lam) / (3.0 * N),
                            self.w["normal"] / (3.0 * N))
        ssim_i, ssim_p = -self.w["l1"] * lam / (3.0 * N), -self.w["pbr"] * lam / (3.0 * N)
        if self._fuses_image_tail(W, H):
            # the four launches below as one (r3dg_stage2_image_tail): the sRGB image, the SSIM partials and the SSIM gradients
            # stay on chip, so the slab ends behind the feature gradients
            g = torch.empty((20, H, W), dtype=torch.float32, device=self.dev)
            _lib.check(L.r3dg_stage2_image_tail(v.raw, W, H, v.vm.data_ptr(), float(cam.tanfovx), float(cam.tanfovy), float(cam.cx),
                float(cam.cy), image.data_ptr(), opacity.data_ptr(), depth.data_ptr(), feature.data_ptr(), n_contrib.data_ptr(),
                gt_c.data_ptr(), bg_c.data_ptr(), _lib.ptr(mask_c), w_l1, w_pbr, w_n, ssim_i, ssim_p, pseudo_normal.data_ptr(),
                sxyz.data_ptr(), g[0:3].data_ptr(), g[3:4].data_ptr(), g[4:20].data_ptr(), self.sums.data_ptr(),
                self.sums[5].data_ptr(), self.sums[6].data_ptr()), "stage2_image_tail")
        else:
            g = torch.empty((47, H, W), dtype=torch.float32, device=self.dev)
            srgb, part_i, part_p, gs_i, gs_p = g[20:23], g[23:32], g[32:41], g[41:44], g[44:47]
            # the rasterizer forward's pseudo-normal pass (deferred in _front_end) and the sRGB-mapped PBR image: one per-pixel launch
            _lib.check(L.r3dg_stage2_normals_srgb(v.raw, W, H, v.vm.data_ptr(), float(cam.tanfovx), float(cam.tanfovy),
                float(cam.cx), float(cam.cy), opacity.data_ptr(), depth.data_ptr(), pseudo_normal.data_ptr(), sxyz.data_ptr(),
                feature.data_ptr(), n_contrib.data_ptr(), bg_c.data_ptr(), srgb.data_ptr()), "stage2_normals_srgb")
            _lib.check(L.r3dg_ssim_forward_pair(v.raw, W, H, 3, image.data_ptr(), srgb.data_ptr(), gt_c.data_ptr(),
                part_i.data_ptr(), part_p.data_ptr(), self.sums[5].data_ptr(), self.sums[6].data_ptr()), "ssim_forward")
            _lib.check(L.r3dg_ssim_backward_pair(v.raw, W, H, 3, image.data_ptr(), srgb.data_ptr(), gt_c.data_ptr(),
                part_i.data_ptr(), part_p.data_ptr(), ssim_i, ssim_p, gs_i.data_ptr(), gs_p.data_ptr()), "ssim_backward")
            _lib.check(L.r3dg_stage2_loss(v.raw, W, H, image.data_ptr(), opacity.data_ptr(), feature.data_ptr(),
                pseudo_normal.data_ptr(), n_contrib.data_ptr(), gt_c.data_ptr(), bg_c.data_ptr(), _lib.ptr(mask_c), w_l1, w_pbr, w_n,
                gs_i.data_ptr(), gs_p.data_ptr(), g[0:3].data_ptr(), g[3:4].data_ptr(), g[4:20].data_ptr(), self.sums.data_ptr(), 1),
                "stage2_loss")
        # r3dg_stage2_loss only writes the pbr maps and -- when that term is on -- the normal maps; the smoothness terms
        # add base colour / roughness / diffuse light (and, through the light term's guide, the normal maps)
        active = [2, 3, 4] + ([5, 6, 7] if self.w["normal"] != 0.0 else [])
        w_bc, w_r, w_ls = (self.w[k] / (3.0 * N) for k in ("base_color_smooth", "roughness_smooth", "light_smooth"))
        if w_bc != 0.0 or w_r != 0.0 or w_ls != 0.0:
            # one streaming kernel: the divided maps and the adjoint inputs never exist in HBM (r3dg_stage2_smooth_forward /
            # _backward, the three-pass formulation, stay as its reference in the tests)
            _lib.check(L.r3dg_stage2_smooth_fused(v.raw, W, H, opacity.data_ptr(), feature.data_ptr(), n_contrib.data_ptr(),
                gt_c.data_ptr(), _lib.ptr(mask_c), w_bc, w_r, w_ls, 1 if self.w["normal"] != 0.0 else 0, g[3:4].data_ptr(),
                g[4:20].data_ptr(), self.sums[7].data_ptr()), "stage2_smooth_fused")
            active += ([8, 9, 10] if w_bc != 0.0 else []) + ([11] if w_r != 0.0 else [])
            if w_ls != 0.0:
                active += [12, 13, 14] + ([5, 6, 7] if self.w["normal"] == 0.0 else [])
        if self._supervised:
            # the MVS terms behind both: map 0 is theirs alone, the normal maps are added to when a kernel above wrote them
            w_d, w_nm = self.w["depth"], self.w["normal_mvs_depth"] / (3.0 * N)
            depth_c = v.gt_depth.contiguous()
            mvs_c = None if w_nm == 0.0 else v.mvs_normal.contiguous()
            self._sup_count_cur = self._supervision_count(v, depth_c, mask_c) if w_d != 0.0 else None
            _lib.check(L.r3dg_stage2_supervision(v.raw, W, H, opacity.data_ptr(), feature.data_ptr(), n_contrib.data_ptr(),
                depth_c.data_ptr(), _lib.ptr(mvs_c), _lib.ptr(mask_c), _lib.ptr(self._sup_count_cur), w_d, w_nm,
                1 if 5 in active else 0, g[3:4].data_ptr(), g[4:20].data_ptr(), self.sums[10].data_ptr()), "stage2_supervision")
            active += ([0] if w_d != 0.0 else []) + ([5, 6, 7] if w_nm != 0.0 and 5 not in active else [])
        self.last_active_features = sorted(set(active))
        return g, active

    @staticmethod
    def _fuses_image_tail(W, H):
        """The image tail runs as one launch (r3dg_stage2_image_tail)?  The forward in use says that the library has the kernel for
        this image size (rasterize_gaussians_begin.image_tail_supported: a stand-in without the attribute, or a library that
        answers 0, keeps the four launches), and R3DG_IMAGE_TAIL is not 0 (the A/B switch: 0 restores r3dg_stage2_normals_srgb,
        r3dg_ssim_forward_pair, r3dg_ssim_backward_pair, r3dg_stage2_loss)."""
        can = getattr(rasterizer_ops.rasterize_gaussians_begin, "image_tail_supported", None)
        return can is not None and os.environ.get("R3DG_IMAGE_TAIL", "1") != "0" and bool(can(W, H))

    def _supervision_count(self, v, depth_c, mask_c):
        """The number of pixels the depth term averages over (r3dg_supervision_count), on the device.  It depends on the view's
        depth map and object mask alone, so it is computed once per (depth map, mask) pair and kept for as long as both tensors
        are unchanged (held here, so a new tensor can never pass for a dropped one at the same address)."""
        key = id(v.gt_depth)
        hit = self._sup_counts.get(key)
        mv = None if v.mask is None else v.mask._version
        if hit is not None and hit[0] is v.gt_depth and hit[1] is v.mask and hit[2] == (v.gt_depth._version, mv):
            return hit[3]
        count = torch.empty(1, dtype=torch.int32, device=self.dev)
        _lib.check(_lib.lib().r3dg_supervision_count(v.raw, v.W, v.H, depth_c.data_ptr(), _lib.ptr(mask_c), count.data_ptr()),
                   "supervision_count")
        self._sup_counts[key] = (v.gt_depth, v.mask, (v.gt_depth._version, mv), count)
        return count

    def _fuses_sh_adam(self):
        """A whole iteration lets the geometry backward apply the SH colour group's Adam (r3dg_rasterize_backward_split's sh_adam:
        the gradient rows never reach device memory, the group gets no Adam launch)?  Single GPU (under data parallelism the
        gradient has to travel in bucket A, and replicas must stay bit-identical through ONE kernel), the group trains, the
        geometry backward runs at all, the backward in use has the kernel for this SH size (asked every iteration: it depends on
        an option), and R3DG_SH_ADAM_IN_BACKWARD is not 0 (the A/B switch: 0 restores the separate launch)."""
        can = getattr(rasterizer_ops.rasterize_gaussians_backward, "sh_adam_supported", None)
        return (not self.dp and bool(self._groups_a) and not self.frozen_geometry and can is not None
                and os.environ.get("R3DG_SH_ADAM_IN_BACKWARD", "1") != "0" and can(self.M))

    def _reads_gradient_records(self):
        """A whole iteration reads the tile backward's gradient records in place (r3dg_rasterize_backward_split with record outputs; no
        scatter pass)?  The geometry backward runs at all, the backward in use takes `gradient_records`, and
        R3DG_GRADIENT_RECORDS is not 0 (the A/B switch: 0 restores the scatter pass).  Whether the call's kernel instance has
        such records is the library's answer, call by call (_raster_backward)."""
        return (not self.frozen_geometry and os.environ.get("R3DG_GRADIENT_RECORDS", "1") != "0"
                and getattr(rasterizer_ops.rasterize_gaussians_backward, "gradient_records_supported", False))

    def _raster_backward(self, v, fw, g, active, split_geometry, fused_a=False, records=False):
        """-> (dL_dfeatures, ALL outputs of the geometry backward or None with frozen geometry, the stream the geometry backward
        went to or None, the work handle of bucket A's all-reduce or None).  The caller holds every output until that stream is
        joined: the allocator would hand the memory of a dropped one to the next launch of the main stream.
        `fused_a`: the geometry backward applies the SH group's Adam as the step _schedule_early is about to begin.
        `records` (_reads_gradient_records): `_records` holds the gradient records for _shade_backward when the library left them
        in place -- dL_dfeatures and the arrays only the scatter pass writes are then None -- and None otherwise."""
        cam, empty = v.cam, torch.Tensor([])
        self._records = None
        R, radii, geom, binning, img = fw[0], fw[9], fw[10], fw[11], fw[12]
        geo_stream = None
        if self.frozen_geometry:
            # nothing but the feature gradients is consumed (the normal maps' gradient belongs to the frozen normal, the depth
            # map's to the frozen positions: the MVS terms then only show in loss(), as in the reference)
            active = [a for a in active if a not in (0, 5, 6, 7)]
            dL_dfeatures = rasterizer_ops.rasterize_gaussians_backward_features(
                self.P, 16, v.H, v.W, g[4:20], geom, R, binning, img, active_features=sorted(active))
            bw = None
        else:
            # whole iterations with Gaussians off the rotated path: the per-Gaussian geometry backward goes to the early-Adam
            # stream and runs beside the gradient unpack and the general shading backward on those few hundred Gaussians (a
            # latency-bound launch that r3dg_shade_frs_backward queues FIRST) instead of in front of them; the main shading
            # backward, which fills the register file, starts when both are about done
            geo_stream = self._listed_stream() if split_geometry else None
            # (fused: the step count opt.begin_step() gives this iteration in _schedule_early, this iteration's own skip flag)
            fused = dict(sh_adam=self.opt.fused_step_of(self._groups_a[0], self.opt.step_count + 1, 1.0, self._skip_cur)) \
                if fused_a else {}
            rows = rasterizer_ops.GradientRecords() if records else None
            if rows is not None:
                fused["gradient_records"] = rows
            bw = rasterizer_ops.rasterize_gaussians_backward(
                v.bg, self.xyz, self.features, radii, empty, self.a_scales, self.a_rot, 1.0, empty, v.vm,
                # (no depth gradient: an EMPTY tensor = NULL = the caller's promise that the depth image carries no loss term)
                cam.full_proj_transform, cam.tanfovx, cam.tanfovy, g[0:3], g[3:4], empty, g[4:20],
                self.shs, 3, v.campos, geom, R, binning, img, True, False, dL_dsh_out=self.grads["shs"],
                geometry_stream=geo_stream, active_features=sorted(active), zeroed_accumulators=self._acc, **fused)
            dL_dfeatures = bw[4]
            self._records = rows if rows else None
            if geo_stream is not None:
                if self._geo_done is None:
                    self._geo_done = torch.cuda.Event()
                self._geo_done.record(geo_stream)
        handle_a = None
        if self._bucket_a is not None and not self._single_bucket:
            # bucket A (SH gradient + flag) travels under the shading backward; issued from the stream that produced it
            with torch.cuda.stream(geo_stream) if geo_stream is not None else contextlib.nullcontext():
                handle_a = self._comm.allreduce_async(self._bucket_a, "A", self._iter)
        return dL_dfeatures, bw, geo_stream, handle_a

    def _schedule_early(self, v, handle_a, geo_stream, use_bounded, early_adam, chain_incidents, fused_a=False):
        """SCHEDULE of the two large groups' updates (`_early`, `_b_early`, `_a_late`, read by optimizer_step), and the SH
        group's early Adam.  -> b_early.
        a_early: the SH group's Adam on the early stream UNDER the shading backward, behind the geometry backward that
          produces its gradient -- under data parallelism behind bucket A's all-reduce, which carries the overflow flag too.
        b_early: the INCIDENT-LIGHT CHAIN (single GPU, fixed ray set, bounded three-stream forward).  The group's gradient is
          finished by the rotation back; the group's Adam and the rotation of the NEW coefficients into the ray frames (the
          first thing the next iteration's shading forward needs, and independent of the next view) follow it as ONE kernel on
          the early stream, queued by optimizer_step behind the other groups' Adam -- beside the next iteration's activations
          + projection instead of Adam(all groups) -> activations -> rotation -> shading forward in a row (~100 us in which
          only small launches ran).  Without the early Adam: frozen SH colour (run_syn4.sh / run_dtu.sh)
          831 -> 843 it/s at sample_num 64, 606 -> 610 on the DTU frame, but not above 40 M samples (399 -> 392 at
          sample_num 384: there the shading forward is the long path of the forward window and the chain in front of it
          costs more than the launches it saves); above a million Gaussians (no early Adam: __call__) the launches it
          replaces stream 2112 bytes per Gaussian, the chain 1741.
        a_late: the chain is queued but the SH group is updated with the others in optimizer_step.
        fused_a (_fuses_sh_adam): the geometry backward has applied the SH group's Adam already, on `geo_stream` or the main
          stream, as the step begun here: a_early without the launch -- with or without `early_adam`, so also above a
          million Gaussians -- and the choice of b_early is what it would be without it."""
        a_launch = early_adam and bool(self._groups_a) and (handle_a is not None or not self.dp)
        b_early = (not self.dp and self._samples.frs is not None and v.order_stream is not None and use_bounded and
                   (a_launch or (bool(self._groups_b) and (self.P * self.K <= 40_000_000 if early_adam else chain_incidents))))
        a_early = a_launch or fused_a
        self._early, self._b_early, self._a_late = a_early or b_early, b_early, b_early and not a_early
        if self._early:
            side = self._early_stream()
            self.opt.begin_step()
            self._early_pending = not self.dp
        if fused_a:
            if b_early:
                # (as below: the next projection reads the SH colour coefficients; the kernel that wrote them is the geometry
                # backward, the last thing queued on its stream)
                _lib.stream_wait(v.order_stream, geo_stream if geo_stream is not None else v.main)
        elif a_early:
            if geo_stream is None and not self.dp:
                side.wait_stream(v.main)
            with torch.cuda.stream(side):
                if self.dp:
                    # (whenever bucket A lands while the shading backward is still running, the SH group's Adam runs under it
                    # too: DESIGN.md section 5.  The reduced overflow flag is snapshotted right after the all-reduce that
                    # carries it.)
                    self._comm.wait(handle_a, "A", self._iter, side)       # the SIDE stream waits for RCCL's stream
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
                _lib.stream_wait(v.order_stream, side)
        return b_early

    def _shade_backward(self, v, env_c, taps, packed, dL_dfeatures, bw, geo_stream, b_early, chain_incidents):
        """Feature gradients -> shading backward -> activation chain rule: every gradient but the SH colour group's."""
        L = _lib.lib()
        P, gr = self.P, self.grads
        rows = self._records
        # (gradient records left in place: both readers of the [P,16] feature-gradient array read the record rows instead)
        unpack, source = (L.r3dg_stage2_unpack_gradients, (dL_dfeatures.data_ptr(),)) if rows is None else \
            (L.r3dg_stage2_unpack_gradients_records, (rows.ptr, rows.layout))
        _lib.check(unpack(
            v.raw, P, *source, self.shade_out.data_ptr(), self.w["light"] / (3.0 * P),
            self.d_pbr.data_ptr(), self.d_diffuse.data_ptr(), self._absmax.data_ptr(),
            # (the light-smoothness term's value, when no pack kernel added it)
            None if packed else self.sums[3].data_ptr()), "stage2_unpack_gradients")
        # the texture-gradient accumulator comes back zeroed from r3dg_stage2_env_backward (consume), the gradient
        # scale from the unpack kernel: nothing sits between that kernel and the shading backward
        if self._d_env is None or self._d_env.shape != env_c.shape:
            self._d_env = torch.zeros_like(env_c)
        sm = self._samples
        frs = sm.frs
        if frs is not None:
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
            d_base, d_rough, d_view, _d_inc, d_env = frs.backward(
                self.a_base, self.a_rough, self.a_normal, self.a_viewdirs, self._incidents, env_c, sm.visibility,
                self.d_pbr, self.d_diffuse, uniform_area=sm.uniform_area,
                out_incidents=frs.dcprime_rows() if dp_chain else gr["incidents"], out_env=self._d_env,
                block_absmax=self._absmax,
                # whole iterations: the rotation back of the coefficient gradient goes to the stream that already carries the
                # SH group's early Adam (optimizer_step joins it before any Adam launch reads the gradient; under data
                # parallelism bucket B's all-reduce is issued from it) and runs beside the activation chain rule
                rotate_stream=self._adam_stream if self._early else None, rotation_back=not (chain or dp_chain))
            self._dp_chain = frs if dp_chain else None
            if b_early:
                # optimizer_step queues the chain BEHIND the other groups' Adam.  Both are HBM streams; side by side the
                # activation chain rule + that Adam -- which the whole front end of the next iteration waits for -- took 68 + 45
                # us instead of 20 + 40, while the chain only gates the shading forward (801-806 vs 793-796 it/s, HISTORY.md)
                self._chain_deferred = (frs, self._skip_cur, self.opt.step_count)
        else:
            d_base, d_rough, d_view, _d_inc, d_env = shading_ops.shade_backward(self.a_base, self.a_rough, self.a_normal,
                self.a_viewdirs, self._incidents, env_c, sm.visibility, sm.incident_dirs, sm.incident_areas, self.d_pbr,
                self.d_diffuse, out_incidents=gr["incidents"], taps=taps, out_env=self._d_env, block_absmax=self._absmax)
        if geo_stream is not None:                                       # join the geometry backward (and nothing
            v.main.wait_event(self._geo_done)       # queued behind it on that stream)
        # the environment texture's chain rule (softplus' + total-variation term; r3dg_stage2_env_backward) rides as six
        # extra workgroups of the activation chain rule's launch
        env_job = (env_c.shape[0], env_c.shape[1], self.env.data_ptr(), env_c.data_ptr(), d_env.data_ptr(),
                   self.w["env_smooth"], gr["env"].data_ptr(), self.sums[4].data_ptr(), 1)
        # (frozen geometry: NULL for everything its half of the chain rule would read or write)
        geo = (lambda t: None) if self.frozen_geometry else (lambda t: t.data_ptr())
        _means2D, _dcol, dL_dopacity, dL_dmeans3D, _dfeat, _dcov, _dsh, dL_dscales, dL_drot = bw or (None,) * 9
        if rows is not None:
            # the last reader of the record rows (the unpack ran on this stream, the geometry backward is joined): it zeroes them
            _lib.check(L.r3dg_stage2_activate_backward_with_records(v.raw, P, geo(self.xyz), geo(self.scaling), geo(self.rotation),
                geo(self.opacity), geo(self.normal), self.base_color.data_ptr(), self.roughness.data_ptr(), geo(v.vm),
                geo(v.campos), rows.ptr, rows.layout, d_base.data_ptr(), d_rough.data_ptr(), geo(d_view), geo(dL_dscales),
                geo(dL_drot), geo(dL_dmeans3D), geo(gr["xyz"]), geo(gr["scaling"]), geo(gr["rotation"]), geo(gr["opacity"]),
                geo(gr["normal"]), gr["base_color"].data_ptr(), gr["roughness"].data_ptr(), *env_job),
                "stage2_activate_backward")
            self._records = None
            return
        _lib.check(L.r3dg_stage2_activate_backward_with(v.raw, P, geo(self.xyz), geo(self.scaling), geo(self.rotation),
            geo(self.opacity), geo(self.normal), self.base_color.data_ptr(), self.roughness.data_ptr(), geo(v.vm), geo(v.campos),
            dL_dfeatures.data_ptr(), d_base.data_ptr(), d_rough.data_ptr(), geo(d_view), geo(dL_dscales), geo(dL_drot),
            geo(dL_dopacity), geo(dL_dmeans3D), geo(gr["xyz"]), geo(gr["scaling"]), geo(gr["rotation"]), geo(gr["opacity"]),
            geo(gr["normal"]), gr["base_color"].data_ptr(), gr["roughness"].data_ptr(), *env_job), "stage2_activate_backward")

    def _remaining_buckets(self, handle_a):
        """(world > 1) The all-reduces of everything but bucket A; `_handles` = the iteration's (A, C, B) for optimizer_step."""
        comm, it = self._comm, self._iter
        self._handles = None
        if self._single_bucket:
            # (R3DG_DP_BUCKETS=1) the whole slab in one collective: everything is final on this stream here (no early Adam
            # without bucket A's handle, so the rotation back of the coefficient gradient ran on this stream too)
            self._handles = (None, comm.allreduce_async(self._bucket_all, "ALL", it), None)
        elif self.dp:
            handle_c = comm.allreduce_async(self._bucket_c, "C", it)
            if self._dp_chain is not None:
                # (BEHIND bucket C although it was final first: the collectives run in the order they are issued, and C is the
                # bucket the main stream waits for -- issued right behind the shading backward, B cost the priced rehearsal
                # 397 -> 374 it/s per rank at 150 GB/s, 590 -> 543 at 300)
                handle_b = comm.allreduce_async(self._dp_chain.dcprime.view(-1), "B", it)
            else:                   # the incident-light gradient is finished by the rotation back: on the early stream, if any
                with torch.cuda.stream(self._adam_stream) if self._early else contextlib.nullcontext():
                    handle_b = comm.allreduce_async(self._bucket_b, "B", it)
            self._handles = (handle_a, handle_c, handle_b)

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
        if self._supervised:
            # the depth term is a mean over the pixels r3dg_supervision_count selected (none: the term is zero)
            count = 0 if self._sup_count_cur is None else int(self._sup_count_cur.item())
            w = torch.cat([w, torch.tensor([self.w["depth"] / count if count else 0.0, self.w["normal_mvs_depth"] / (3.0 * N)],
                                           device=self.dev)])
        return (self.sums.sum(1) * w).sum() + lam * (self.w["l1"] + self.w["pbr"])

    @_in_context
    def optimizer_step(self):
        """Adam on every group that trains (groups with learning rate 0 get no launch): _groups_a = shs, _groups_c = the small
        per-Gaussian groups + env, _groups_b = incidents -- indices into self.opt.groups, one tuple per gradient bucket.
        Behind a forward_backward that ran as part of a whole single-GPU iteration two groups are not updated from `grads`:
        the SH colour group was updated inside the geometry backward (`sh_adam_in_backward`), the incident-light group is
        updated by the chain kernel queued here, which keeps the rotated-back gradient on chip -- grads["shs"] and
        grads["incidents"] do NOT hold that iteration's gradient afterwards (data-parallel runs and a bare forward_backward
        write both)."""
        grads = [self.grads[k] for k in self._opt_order]
        if not self.dp:
            if self._b_early:
                # the incident-light group is updated by the chain queued below, on the early stream (_schedule_early): no join here
                todo = (self._groups_a if self._a_late else ()) + self._groups_c
            elif self._early:            # the SH group was updated under the shading backward (_schedule_early)
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
        scale, wait, it = 1.0 / self.world, self._comm.wait, self._iter
        handle_a, handle_c, handle_b = self._handles
        if self._single_bucket:
            self.opt.begin_step()
            wait(handle_c, "ALL", it)
            self._skip_cur = self._snapshot_flag()
            todo = self._groups_a + self._groups_c + self._groups_b
            if todo:
                self.opt.step_groups(todo, grads, scale, skip_flag=self._skip_cur)
                self._pre_rotated = None
            return
        if self._early:                  # bucket A was waited for and applied on the side stream (_schedule_early)
            torch.cuda.current_stream().wait_stream(self._adam_stream)
            self._early = False
            wait(handle_c, "C", it)
        else:
            self.opt.begin_step()
            # the overflow flag rides in the first bucket that is reduced: A, or C when the geometry is frozen
            wait(handle_a if handle_a is not None else handle_c, "A" if handle_a is not None else "C", it)
            self._skip_cur = self._snapshot_flag()      # > 0 on every rank when any rank dropped its view
            if handle_a is not None:
                if self._groups_a:
                    self.opt.step_groups(self._groups_a, grads, scale, skip_flag=self._skip_cur)
                wait(handle_c, "C", it)
        if self._groups_c:
            self.opt.step_groups(self._groups_c, grads, scale, skip_flag=self._skip_cur)
        self._pending_b = (handle_b, grads, scale, self._skip_cur, it)

    def _incident_chain(self, frs, count, scale, skip, **listed):
        """The incident-light chain on the current stream, ONE kernel: rotation back of the group's gradient (into
        grads["incidents"]) + its Adam update as step `count` + rotation of the new coefficients, where the next shading forward
        finds them.  `listed`: FixedRaySet.incident_chain's `listed_in_dcprime` (data parallel) / `write_gradient` (False in
        whole single-GPU iterations: grads["incidents"] is then not written)."""
        grp = self.opt.groups[self._groups_b[0]]
        frs.incident_chain(self._incidents, self.grads["incidents"], grp["exp_avg"], grp["exp_avg_sq"], grp["lr"],
                           grp["lr_tail"], self.opt.betas, self.opt.eps, count, scale, skip_flag=skip, **listed)
        self._pre_rotated = (frs, self._incidents, self._incidents._version)

    def _run_chain(self):
        """Queue the incident-light chain _shade_backward deferred (`_chain_deferred`) on the early stream, behind what the
        current stream holds now, with the iteration's own step count; a frozen group only gets its coefficients rotated."""
        frs, skip, count = self._chain_deferred
        self._chain_deferred = None
        early = self._adam_stream
        _lib.stream_wait(early, torch.cuda.current_stream(self.dev))
        with torch.cuda.stream(early):
            if self._groups_b:
                # (nobody reads the world-frame gradient of a whole single-GPU iteration behind the update: the kernel keeps the
                # row on chip, 192 of its 1728 bytes per Gaussian; R3DG_CHAIN_WRITES_GRADIENT=1 is the A/B switch)
                lean = (getattr(frs, "chain_gradient_optional", False)
                        and os.environ.get("R3DG_CHAIN_WRITES_GRADIENT", "0") == "0")
                self._incident_chain(frs, count, 1.0, skip, **(dict(write_gradient=False) if lean else {}))
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
            self._comm.wait(handle_b, "B", it_b)
            frs, self._dp_chain = self._dp_chain, None
            if frs is not None:
                # the REDUCED gradient, 1 / world inside; the Gaussians off the rotated path have their rows in the same buffer
                self._incident_chain(frs, self.opt.step_count, scale, skip, listed_in_dcprime=True)
            elif self._groups_b:
                self.opt.step_groups(self._groups_b, grads, scale, skip_flag=skip)
                self._pre_rotated = None           # (see optimizer_step)

    @_in_context
    def __call__(self, cam, bg, gt, image_mask=None, gt_depth=None, mvs_normal=None):
        """One whole training iteration: forward_backward + optimizer_step.  On one GPU, grads["shs"] and grads["incidents"] do
        NOT hold this iteration's gradient afterwards: the kernels that produce those two [P,48] gradients apply their groups'
        Adam themselves and never write them out (_fuses_sh_adam, _run_chain); every other entry of `grads` does."""
        # the SH group's Adam as a launch of its own (where the geometry backward does not apply it itself: _fuses_sh_adam) under the shading backward: pays while the group's 64 bytes x 48 per Gaussian mostly live in the
        # 256 MB last-level cache (300k Gaussians: 58 us of Adam for 31 us of slower shading backward); streamed from HBM it
        # costs the latency-sensitive shading kernel nearly its whole duration (2M: 0.99 ms of Adam for +0.85 ms, 159 vs 163 it/s)
        early = os.environ.get("R3DG_EARLY_ADAM", "1" if self.P <= 1_000_000 else "0") != "0" and not self.serial_streams
        outs = self.forward_backward(cam, bg, gt, early_adam=early, image_mask=image_mask, chain_incidents=True,
                                     gt_depth=gt_depth, mvs_normal=mvs_normal, sh_adam_in_backward=True,
                                     gradient_records=True)
        self.optimizer_step()
        return outs
