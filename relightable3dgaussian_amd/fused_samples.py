"""The P x K samples of the fused stage-2 iteration (fused_step.FusedStage2Step._samples): ONE owner for the traced visibility,
the direction / area caches, the snapshot normals they were generated from, the fixed ray set and the general shading kernels'
lookup cache -- acquired by a trace, selected per environment-texture size.  The step asks for `frs` / `uniform_area` / the taps
and never how they came about (relight._Samples is the renderer's counterpart: it answers other questions; the two share
sampling.fibonacci_directions)."""
import math
import os

import torch

from . import sampling, shading_ops


def of_samples(attr):
    """A step attribute that lives in the sample-set owner, as `attr`."""
    return property(lambda self: getattr(self._samples, attr), lambda self, value: setattr(self._samples, attr, value))


class SampleSet:
    """`K` samples per Gaussian, `M` SH coefficients; `traces`: (train_step.update_visibility, update_visibility_device) as the
    module of the step names them; `device_visibility`: acquire() traces on the device.  Two kinds, told apart
    HERE alone by whether a direction tensor is held (anybody may assign `incident_dirs`, a tensor or None: the next select()
    notices):
      stored      `incident_dirs` [P,K,3] and `incident_areas` [P,K,1] are resident; the cache is keyed on the direction tensor.
      generated   no direction or area tensor: the samples ARE the Fibonacci set of the snapshot normals; keyed on the number of
                  refreshes.  A texture size the fixed-ray-set kernels do not take (or R3DG_SHADE_FRS=0) materialises both tensors,
                  and from then on the set is of the stored kind.
    After select(He, We): `frs` is the shading_ops.FixedRaySet to shade with or None (the general kernels), `uniform_area` the
    area of all samples where there is one (the kernels then read no area tensor).
    Release: whoever needs the memory assigns None to `visibility` / `incident_dirs` / `incident_areas` and to `taps` / `src` /
    `frs` (the benchmark does, through the step's forwarding properties) -- no more than that, so there is no method for it."""

    def __init__(self, sample_num, sh_coeffs, traces, group=None, device_visibility=False):
        self.K, self.M, self.group, self.device_visibility = sample_num, sh_coeffs, group, bool(device_visibility)
        self._trace, self._trace_on_device = traces
        self.visibility = self.incident_dirs = self.incident_areas = self.tracer = None
        # the normals the samples were generated from (the trained normal moves on); refresh() calls so far (key of the generated kind)
        self.ray_normals, self.refreshes = None, 0
        # the selection (class docstring) and the general kernels' taps; then `src`: the direction tensor the cache was made for,
        # HELD for as long as the cache is (a replaced tensor can then never come back at the address of the old one and pass for it); `_key`: its (_version, shape), or ("device", refreshes); `_size`: the texture
        # size -- a key of its own: only the lookup records depend on it, the ray set (a host read-back) does not; `_built`: the ray
        # set of `_key`, selected (`frs`) for the sizes it takes
        self.frs = self.uniform_area = self.taps = self.src = self._key = self._size = self._built = None

    def _frs_wanted(self):
        """The fixed-ray-set kernels are switched on and take this K and SH degree (the texture size is asked per size: select)."""
        return os.environ.get("R3DG_SHADE_FRS", "1") != "0" and shading_ops.FixedRaySet.supported(self.K, self.M, 16, 32)

    def acquire(self, xyz, scales, rotations, opacity, normal, on_device=None):
        """Trace the visibility of these ACTIVATED parameters and snapshot the normals: train_step.update_visibility, or (device
        kind) update_visibility_device -- the rays are generated inside the trace kernel, and a direction cache only comes back
        where the general shading kernels will read it."""
        if self.device_visibility if on_device is None else on_device:
            self.visibility, self.incident_dirs, self.tracer = self._trace_on_device(
                xyz, scales, rotations, opacity, normal, self.K, group=self.group, want_dirs=not self._frs_wanted())
            self.incident_areas = None if self.incident_dirs is None else normal.new_full((normal.shape[0], self.K, 1), 2 * math.pi)
        else:
            self.visibility, self.incident_dirs, self.incident_areas, self.tracer = self._trace(
                xyz, scales, rotations, opacity, normal, self.K, group=self.group)
        self.ray_normals = normal.clone()

    def refresh(self, *activated):
        """Re-trace (always on the device), drop every cache and select again for the texture size that was in use, if any."""
        size = self._size
        self.acquire(*activated, on_device=True)
        self.refreshes += 1
        self.taps = self._key = self._size = self.src = self._built = self.frs = None
        if size is not None:
            self.select(*size)

    def select(self, He, We):
        """Decide, once per acquired set / texture size, what shades a He x We environment texture.  -> the general kernels'
        per-sample lookup cache (shading_ops.build_taps: 12 bytes per sample, read beside the directions), or None when the
        fixed-ray-set kernels run (`frs`: they read neither; their own 8-byte records come from the ray normals)."""
        ray_set, size = shading_ops.FixedRaySet, (He, We)
        takes = lambda: self._built is not None and ray_set.supported(self.K, self.M, He, We)
        if self.incident_dirs is None:
            # generated: nothing to regenerate and compare, and the set changes exactly when the visibility is re-traced
            key = ("device", self.refreshes)
            if self.src is not None or self._key != key:
                self._key, self.src, self._size, self.taps = key, None, None, None
                self.uniform_area = float(torch.tensor(2 * math.pi, dtype=torch.float32))
                self._built = ray_set(self.ray_normals, self.K) if self._frs_wanted() else None
            if not takes():                 # the general kernels after all: from here on as with stored tensors
                self.incident_dirs, self.incident_areas = sampling.fibonacci_directions(self.ray_normals, self.K, want_areas=True)
        src = self.incident_dirs
        if src is not None:
            key = (src._version, tuple(src.shape))
            if self.src is not src or self._key != key:
                self._key, self.src, self._size = key, src, None
                # fibonacci_sphere_sampling gives every sample the area 2 pi: then the area cache need not be read at all
                lo, hi = float(self.incident_areas.min()), float(self.incident_areas.max())
                self.uniform_area = lo if lo == hi else None
                # fixed-ray-set kernels (csrc/shading_frs.hip) when the cache IS the Fibonacci set of the snapshot normals --
                # checked here, once per direction tensor -- and fits their limits; otherwise (caches handed in from elsewhere,
                # other K, R3DG_SHADE_FRS=0) the general kernels
                wanted = self.uniform_area is not None and self._frs_wanted()
                self._built = ray_set.try_build(self.ray_normals, src) if wanted else None
        if self._size != size:
            # a new set or texture size: new lookup records for the ray set that is already there (FixedRaySet.taps is keyed on the
            # size itself) if the fixed-ray-set kernels take that size, the general kernels' 12-byte taps otherwise
            self._size, self.frs = size, self._built if takes() else None
            self.taps = None if self.frs is not None else shading_ops.build_taps(src, He, We)
            if self.frs is not None:
                self.frs.taps(He, We)
        return self.taps
