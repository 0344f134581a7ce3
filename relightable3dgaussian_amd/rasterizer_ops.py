"""Host-side mirror of the reference's `r3dg_rasterization._C` pybind module (r3dg-rasterization/ext.cpp:15-19):
same function names, argument order, return tuples and error behaviour (RuntimeError), implemented over the
C ABI in libr3dg_hip.so.  PyTorch is used only for device memory and the current HIP stream.

    rasterize_gaussians(...)          -> 13-tuple   (rasterize_points.h:18-42, rasterize_points.cu:36-141)
    rasterize_gaussians_backward(...) -> 9-tuple    (rasterize_points.h:44-71, rasterize_points.cu:143-235)
    mark_visible(means3D, viewmatrix, projmatrix) -> bool[P]   (rasterize_points.h:73-76)
"""
import ctypes as C

import torch

from . import _abi, _lib

NUM_CHANNELS = 3
RasterScene, RasterOutputs, RasterBackward = (_abi.structs["r3dg_raster_" + n] for n in ("scene", "outputs", "backward"))


def _f32c(t):
    """contiguous fp32 view on the device (the reference calls .contiguous().data_ptr<float>() on everything)."""
    if t is None or t.numel() == 0:
        return None
    if t.dtype != torch.float32:
        raise RuntimeError("expected a float32 tensor, got %s" % t.dtype)
    if not t.is_cuda:
        raise RuntimeError("expected a CUDA(HIP) tensor")
    return t.contiguous()


class _Resizer:
    """The reference's resizeFunctional (rasterize_points.cu:28-34): three byte buffers grown on request."""

    def __init__(self, device):
        self.device = device
        self.buffers = [torch.empty(0, dtype=torch.uint8, device=device) for _ in range(3)]
        self.callbacks = [_lib.ALLOC_FN(self._make(i)) for i in range(3)]

    # Large requests are rounded up to 16 MiB steps: the binning buffer's size follows num_rendered, which changes with
    # every view, and a caching allocator serves a handful of recurring sizes from its free lists where an ever-new size
    # sooner or later costs a hipMalloc (milliseconds, in the middle of an iteration).  The state buffers are opaque.
    _STEP = 16 << 20

    def _make(self, i):
        def cb(_user, nbytes):
            try:
                n = int(nbytes)
                if n > (4 << 20):
                    n = (n + self._STEP - 1) // self._STEP * self._STEP
                self.buffers[i] = torch.empty(n, dtype=torch.uint8, device=self.device)
                return self.buffers[i].data_ptr()
            except Exception:          # surfaces as R3DG_EALLOC -> RuntimeError
                return 0
        return cb


def _scene(P, S, degree, M, W, H, scale_modifier, tan_fovx, tan_fovy, cx=0.0, cy=0.0, **inputs):
    """The r3dg_raster_scene of a call, and {field name without d_: contiguous fp32 tensor or None} of the `inputs` its pointers
    name: the caller keeps those referenced for as long as kernels of the call may still be enqueued."""
    kept = {k: _f32c(v) for k, v in inputs.items()}
    return RasterScene(P=P, S=S, D=int(degree), M=M, width=W, height=H, scale_modifier=float(scale_modifier),
                       tan_fovx=float(tan_fovx), tan_fovy=float(tan_fovy), cx=float(cx), cy=float(cy),
                       **{"d_" + k: _lib.ptr(v) for k, v in kept.items()}), kept


def _offsets(fn, n, *args):
    arr = (C.c_size_t * n)()
    fn(*args, arr)
    return list(arr)


class _PendingForward:
    """Second half of a split forward (see rasterize_gaussians_begin): call .finish() exactly once."""

    def __init__(self, ticket, rs, outs, dev, H, W, capacity=None):
        self.ticket, self.rs, self.outs, self.dev, self.H, self.W = ticket, rs, outs, dev, H, W
        self.capacity = capacity

    def finish(self, ordering_stream=None):
        """`ordering_stream`: optional torch stream for the instance ordering (sort) part, which then overlaps whatever
        was queued on the forward's stream since begin; the binning buffer is allocated from that stream's pool.
        A bounded forward (rasterize_gaussians_begin(capacity=...)) has its ordering queued already: finish() renders on
        the current stream and returns `capacity` in the num_rendered slot (the value the backward's state layout needs)."""
        L = _lib.lib()
        rendered = C.c_int(0)
        with torch.cuda.device(self.dev):
            if self.capacity is not None:
                st = L.r3dg_rasterize_forward_finish_bounded(self.ticket, _lib.current_stream())
                rendered = C.c_int(int(self.capacity))
            elif ordering_stream is None:
                st = L.r3dg_rasterize_forward_finish(self.ticket, C.byref(rendered))
            else:
                with torch.cuda.stream(ordering_stream):        # resize callback allocates on that stream
                    st = L.r3dg_rasterize_forward_finish_on(self.ticket, C.c_void_p(ordering_stream.cuda_stream),
                                                            C.byref(rendered))
        self.ticket = None
        geomBuffer, binningBuffer, imgBuffer = self.rs.buffers
        # the resize callbacks are closures over the resizer, which holds them: a reference cycle around the frame's scratch
        # buffers that only the garbage collector would break (hundreds of MB of device memory per frame in the meantime).
        # The library does not call them after this point
        self.rs.callbacks = None
        self.rs = None
        _lib.check(st, "rasterize_gaussians")
        out_color, out_opacity, out_depth, out_feature, out_normal, out_surface_xyz, out_weights, radii = self.outs
        H, W = self.H, self.W
        if imgBuffer.numel() == 0:
            imgBuffer = torch.zeros(int(L.r3dg_image_state_bytes(W, H)), dtype=torch.uint8, device=self.dev)
        # n_contrib: int32 view into the image state (the reference returns a from_blob view, rasterize_points.cu:136-139)
        off = _offsets(L.r3dg_image_state_offsets, 3, W, H)
        n_contrib = imgBuffer[off[1]:off[1] + 4 * H * W].view(torch.int32).view(H, W)
        return (rendered.value, n_contrib, out_color, out_opacity, out_depth, out_feature, out_normal, out_surface_xyz,
                out_weights, radii, geomBuffer, binningBuffer, imgBuffer)


def rasterize_gaussians_begin(background, means3D, features, colors, opacity, scales, rotations, scale_modifier,
                              cov3D_precomp, viewmatrix, projmatrix, tan_fovx, tan_fovy, cx, cy, image_height,
                              image_width, sh, degree, campos, prefiltered, computer_pseudo_normal, debug,
                              capacity=None, overflow_flag=None, overflow_count=None, ordering_stream=None,
                              want_weights=True, defer_pseudo_normal=False):
    """First half of rasterize_gaussians (same arguments): projection + asynchronous read-back of num_rendered.  Returns
    an object whose .finish() completes the call and returns the 13-tuple.  Kernels launched on the current stream in
    between (e.g. the ones that fill `features`, whose CONTENTS are first read by .finish()'s kernels) overlap the wait.

    `capacity` (not in the reference): the BOUNDED forward (r3dg_rasterize_forward_begin_bounded) -- no host read-back;
    the projection is queued on the current stream and the instance ordering behind it on `ordering_stream` (default:
    the current stream) at once, with the binning state sized for `capacity` instances.
    `overflow_flag` (float32 tensor, >= 1 element) is set to 1 when the frame needed more and was dropped, else 0;
    `overflow_count` (int32 tensor) counts dropped frames.  All tensors are allocated on the current stream.
    `want_weights=False` (not in the reference): the per-Gaussian blend weights -- which only the densification statistics
    read -- are not computed; the `weights` slot of the result is None.
    `defer_pseudo_normal=True` (not in the reference): the pseudo-normal / surface-point maps are allocated and returned but NOT
    computed (and not zero-filled): the caller runs r3dg_stage2_normals_srgb on them, fused with its own per-pixel pass."""
    L = _lib.lib()
    if means3D.ndimension() != 2 or means3D.size(1) != 3:
        raise RuntimeError("means3D must have dimensions (num_points, 3)")
    if not means3D.is_cuda:
        raise RuntimeError("means3D must be a CUDA(HIP) tensor")
    P = means3D.size(0)
    S = features.size(1)
    H, W = int(image_height), int(image_width)
    dev = means3D.device
    fopt = dict(dtype=torch.float32, device=dev)

    # Every pixel of every image buffer is written by the kernels, so one uninitialised slab suffices (the reference
    # zero-fills eight tensors, rasterize_points.cu:72-79); only `weights` is accumulated with atomics and needs zeros.
    # P == 0 launches nothing, so that case keeps the reference's all-zero outputs.
    slab = (torch.zeros if P == 0 else torch.empty)((11 + S, H, W), **fopt)
    out_color, out_opacity, out_depth = slab[0:3], slab[3:4], slab[4:5]
    out_feature, out_normal, out_surface_xyz = slab[5:5 + S], slab[5 + S:8 + S], slab[8 + S:11 + S]
    if defer_pseudo_normal:
        computer_pseudo_normal = False
    elif not computer_pseudo_normal:
        slab[5 + S:].zero_()
    out_weights = torch.zeros((P, 1), **fopt) if want_weights else None
    radii = torch.empty((P,), dtype=torch.int32, device=dev)

    rs = _Resizer(dev)
    ticket = C.c_void_p(None)
    if P != 0:
        M = sh.size(1) if sh.size(0) != 0 else 0
        scene, kept = _scene(P, S, degree, M, W, H, scale_modifier, tan_fovx, tan_fovy, cx, cy, background=background,
                             means3D=means3D, shs=sh, colors_precomp=colors, features=features, opacities=opacity, scales=scales,
                             rotations=rotations, cov3D_precomp=cov3D_precomp, viewmatrix=viewmatrix, projmatrix=projmatrix,
                             campos=campos)
        if kept["features"] is not None and kept["features"].data_ptr() != features.data_ptr():
            raise RuntimeError("rasterize_gaussians_begin needs contiguous features (their contents are read later)")
        rs.keep = list(kept.values())                 # inputs stay alive until finish()
        outputs = RasterOutputs(
            prefiltered=int(bool(prefiltered)), compute_pseudo_normal=int(bool(computer_pseudo_normal)), debug=int(bool(debug)),
            d_out_color=out_color.data_ptr(), d_out_opacity=out_opacity.data_ptr(), d_out_depth=out_depth.data_ptr(),
            d_out_feature=_lib.ptr(out_feature), d_out_normal=out_normal.data_ptr(), d_out_surface_xyz=out_surface_xyz.data_ptr(),
            d_out_weights=_lib.ptr(out_weights), d_radii=radii.data_ptr())
        common = (rs.callbacks[0], rs.callbacks[1], rs.callbacks[2], None, C.byref(scene), C.byref(outputs))
        with torch.cuda.device(dev):
            if capacity is None:
                st = L.r3dg_rasterize_forward_begin(_lib.current_stream(), *common, C.byref(ticket))
            else:
                if overflow_flag is not None and (overflow_flag.dtype != torch.float32 or not overflow_flag.is_cuda):
                    raise RuntimeError("overflow_flag must be a float32 device tensor")
                if overflow_count is not None and (overflow_count.dtype != torch.int32 or not overflow_count.is_cuda):
                    raise RuntimeError("overflow_count must be an int32 device tensor")
                rs.keep.append((overflow_flag, overflow_count))
                st = L.r3dg_rasterize_forward_begin_bounded(
                    _lib.current_stream(), *common,
                    C.c_void_p(ordering_stream.cuda_stream) if ordering_stream is not None else None, int(capacity),
                    overflow_flag.data_ptr() if overflow_flag is not None else None,
                    overflow_count.data_ptr() if overflow_count is not None else None, C.byref(ticket))
        _lib.check(st, "rasterize_gaussians")
    elif capacity is not None and overflow_flag is not None:
        overflow_flag[:1].zero_()
    return _PendingForward(ticket, rs, (out_color, out_opacity, out_depth, out_feature, out_normal, out_surface_xyz,
                                        out_weights, radii), dev, H, W, capacity=capacity)


def rasterize_gaussians(background, means3D, features, colors, opacity, scales, rotations, scale_modifier,
                        cov3D_precomp, viewmatrix, projmatrix, tan_fovx, tan_fovy, cx, cy, image_height, image_width,
                        sh, degree, campos, prefiltered, computer_pseudo_normal, debug):
    return rasterize_gaussians_begin(background, means3D, features, colors, opacity, scales, rotations, scale_modifier,
                                     cov3D_precomp, viewmatrix, projmatrix, tan_fovx, tan_fovy, cx, cy, image_height,
                                     image_width, sh, degree, campos, prefiltered, computer_pseudo_normal,
                                     debug).finish()


class GradientRecords:
    """The tile backward's per-Gaussian gradient records, left in place (r3dg_rasterize_backward_split with record outputs): `ptr`
    is the first of P rows of 16 floats in the library's scratch of the stream the backward ran on, `layout` the
    R3DG_GRAD_RECORD_LAYOUT_INTS ints that say which channel holds what.  Handed EMPTY to rasterize_gaussians_backward
    (`gradient_records=`); it comes back filled -- true -- when the call's kernel instance has such rows, and then the caller
    runs r3dg_stage2_unpack_gradients_records and r3dg_stage2_activate_backward_with_records on them (the second zeroes the
    rows again), or r3dg_gradient_records_scatter.  Empty on return: the call was the classic one."""

    def __init__(self):
        self.ptr, self.layout, self.P, self.device = None, None, 0, None

    def __bool__(self):
        return self.ptr is not None

    def tensor(self):
        """The rows as a [P,16] float32 tensor that VIEWS the library's memory (tests, debugging)."""
        view = type("_RecordRows", (), {"__cuda_array_interface__": {
            "shape": (self.P, 16), "typestr": "<f4", "data": (int(self.ptr), False), "version": 2, "strides": None}})()
        return torch.as_tensor(view, device=self.device)


def rasterize_gaussians_backward(background, means3D, features, radii, colors, scales, rotations, scale_modifier,
                                 cov3D_precomp, viewmatrix, projmatrix, tan_fovx, tan_fovy, dL_dout_color,
                                 dL_dout_opacity, dL_dout_depth, dL_dout_feature, sh, degree, campos, geomBuffer, R,
                                 binningBuffer, imageBuffer, backward_geometry, debug, dL_dsh_out=None,
                                 geometry_stream=None, active_features=None, zeroed_accumulators=None, sh_adam=None,
                                 gradient_records=None):
    """`dL_dsh_out` (not in the reference signature): optional preallocated [P,M,3] buffer the SH gradient is written
    into (every element is written), e.g. a view of a flat gradient bucket.  `geometry_stream`: optional torch stream
    for the per-Gaussian geometry backward (dL_dmeans3D, dL_dcov3D, dL_dsh, dL_dscales, dL_drotations are then only
    valid after the caller joins that stream; see r3dg_rasterize_backward_split).  `active_features`: optional list of
    the feature channels whose upstream gradient can be non-zero -- the caller's promise that all other channels of
    dL_dout_feature are zero; they are then skipped by the tile kernel (same results).  `zeroed_accumulators`: optional float32
    tensor of (11 + S) * P floats (any contents since round 5 -- the name is from when it had to be zeros) that takes the place
    of the slab allocated here; dL_dmeans2D, dL_dconic, dL_dopacity, dL_dcolors and dL_dfeatures are views of it.
    `sh_adam` (FusedAdam.fused_step_of(group of `sh`, ...); r3dg_rasterize_backward_split's sh_adam): the per-Gaussian geometry
    backward applies the Adam step of the SH group itself -- `sh` and its two moment tensors are updated in place and the
    returned dL_dsh is NOT written (it keeps whatever it held).  Raises where the library has no such kernel
    (sh_adam_supported).
    `gradient_records` (an empty GradientRecords; whole stage-2 iterations): where the call's kernel instance keeps 16-float
    records -- up to 7 active feature channels without a depth gradient -- there is NO scatter pass: the geometry backward reads
    the records in place, `gradient_records` comes back filled, and dL_dcolors, dL_dopacity and dL_dfeatures are returned as
    None (dL_dmeans2D is written as ever).  The caller's kernels read the rest of the rows and zero them (GradientRecords).
    Otherwise `gradient_records` stays empty and the call is the classic one."""
    L = _lib.lib()
    P = means3D.size(0)
    S = features.size(1)
    H = dL_dout_color.size(1)
    W = dL_dout_color.size(2)
    M = sh.size(1) if sh.size(0) != 0 else 0
    dev = means3D.device
    fopt = dict(dtype=torch.float32, device=dev)

    # gradients accumulated with atomics share ONE zero-filled slab; the per-Gaussian outputs of the fused
    # preprocess-backward kernel are fully written (zeros for invisible Gaussians) and start uninitialised
    # (dL_dfeatures first: its rows stay 16-byte aligned for S % 4 == 0 whatever P is)
    if zeroed_accumulators is not None:
        acc = zeroed_accumulators
        if acc.numel() != (11 + S) * P or acc.dtype != torch.float32 or not acc.is_contiguous() or acc.device != dev:
            raise RuntimeError("zeroed_accumulators must be a contiguous float32 tensor of (11 + S) * P floats on the device")
    else:
        # (round 5: the tile backward accumulates into per-Gaussian records of the library and its scatter pass WRITES every
        # element of these five arrays -- zeros for Gaussians nothing touched, and for P == 0 / num_rendered == 0 the library
        # fills them -- so the slab starts uninitialised; rounds 1-4 zero-filled it here, the reference fills five tensors,
        # rasterize_points.cu:183-192)
        acc = torch.empty((11 + S) * P, **fopt)
    dL_dfeatures = acc[0:S * P].view(P, S)
    o = S * P
    dL_dconic = acc[o:o + 4 * P].view(P, 2, 2); o += 4 * P
    dL_dmeans2D = acc[o:o + 3 * P].view(P, 3); o += 3 * P
    dL_dopacity = acc[o:o + P].view(P, 1); o += P
    dL_dcolors = acc[o:o + 3 * P].view(P, NUM_CHANNELS)
    have_sh = sh.numel() != 0 and colors.numel() == 0
    have_scale = scales.numel() != 0 and cov3D_precomp.numel() == 0
    dL_dmeans3D = torch.empty((P, 3), **fopt)
    dL_dcov3D = torch.empty((P, 6), **fopt)
    if dL_dsh_out is not None and have_sh:
        if tuple(dL_dsh_out.shape) != (P, M, 3) or not dL_dsh_out.is_contiguous() or dL_dsh_out.dtype != torch.float32:
            raise RuntimeError("dL_dsh_out must be a contiguous float32 [P,M,3] tensor")
        dL_dsh = dL_dsh_out
    else:
        dL_dsh = (torch.empty if have_sh else torch.zeros)((P, M, 3), **fopt)
    dL_dscales = (torch.empty if have_scale else torch.zeros)((P, 3), **fopt)
    dL_drotations = (torch.empty if have_scale else torch.zeros)((P, 4), **fopt)

    if P != 0:
        scene, kept = _scene(P, S, degree, M, W, H, scale_modifier, tan_fovx, tan_fovy, background=background, means3D=means3D,
                             shs=sh, features=features, colors_precomp=colors, scales=scales, rotations=rotations,
                             cov3D_precomp=cov3D_precomp, viewmatrix=viewmatrix, projmatrix=projmatrix, campos=campos)
        gC, gO, gD, gF = [_f32c(x) for x in (dL_dout_color, dL_dout_opacity, dL_dout_depth, dL_dout_feature)]
        radii_ = radii.contiguous()
        if sh_adam is not None and (kept["shs"] is not sh or not have_sh):
            raise RuntimeError("sh_adam: needs the contiguous float32 SH tensor itself as `sh`")
        if active_features is None:
            n_act, act = -1, None
        else:
            n_act = len(active_features)
            act = (C.c_int * max(1, n_act))(*[int(a) for a in active_features])
        # (`kept`, the four gradients, radii_ and `act` are locals: referenced until both calls below have returned)
        call = RasterBackward(
            R=int(R), d_radii=radii_.data_ptr(), d_geom_buffer=_lib.ptr(geomBuffer), d_binning_buffer=_lib.ptr(binningBuffer),
            d_img_buffer=_lib.ptr(imageBuffer), d_dL_dpix=_lib.ptr(gC), d_dL_dpix_o=_lib.ptr(gO), d_dL_dpix_d=_lib.ptr(gD),
            d_dL_dpix_f=_lib.ptr(gF), d_dL_dmean2D=dL_dmeans2D.data_ptr(), d_dL_dconic=dL_dconic.data_ptr(),
            d_dL_dopacity=dL_dopacity.data_ptr(), d_dL_dcolor=dL_dcolors.data_ptr(), d_dL_dfeature=_lib.ptr(dL_dfeatures),
            d_dL_dmean3D=dL_dmeans3D.data_ptr(), d_dL_dcov3D=dL_dcov3D.data_ptr(), d_dL_dsh=_lib.ptr(dL_dsh),
            d_dL_dscale=dL_dscales.data_ptr(), d_dL_drot=dL_drotations.data_ptr(), backward_geometry=int(bool(backward_geometry)),
            debug=int(bool(debug)), n_active_features=n_act, active_features=C.addressof(act) if act is not None else None)
        with torch.cuda.device(dev):
            cur = _lib.current_stream()
            gs = cur if geometry_stream is None else C.c_void_p(geometry_stream.cuda_stream)
            head = (cur, gs, C.byref(scene), C.byref(call)) + \
                (tuple(sh_adam) if sh_adam is not None else (None, 0.0, 0.0, 0.0, 1, 1.0, None))
            if gradient_records is not None:
                rows, supported = C.c_void_p(), C.c_int(0)
                layout = (C.c_int * _abi.constants["R3DG_GRAD_RECORD_LAYOUT_INTS"])()
                st = L.r3dg_rasterize_backward_split(*head, C.byref(rows), layout, C.byref(supported))
                _lib.check(st, "rasterize_gaussians_backward")
                if supported.value:
                    gradient_records.ptr, gradient_records.layout = rows.value, layout
                    gradient_records.P, gradient_records.device = P, dev
                    return (dL_dmeans2D, None, None, dL_dmeans3D, None, dL_dcov3D, dL_dsh, dL_dscales, dL_drotations)
            st = L.r3dg_rasterize_backward_split(*head, None, None, None)
        _lib.check(st, "rasterize_gaussians_backward")
    return (dL_dmeans2D, dL_dcolors, dL_dopacity, dL_dmeans3D, dL_dfeatures, dL_dcov3D, dL_dsh, dL_dscales,
            dL_drotations)


def _sh_adam_supported(M):
    """rasterize_gaussians_backward(sh_adam=...) has a kernel for [P,M,3] SH coefficients
    (r3dg_rasterize_backward_sh_adam_supported: it depends on M and on the STAGE_SH_ROWS option)?"""
    return bool(_lib.lib().r3dg_rasterize_backward_sh_adam_supported(int(M)))


# (asked of the FUNCTION, so that whatever stands in its place -- a wrapper, a recorder -- answers for itself; one without the
# attribute takes no `sh_adam`)
rasterize_gaussians_backward.sh_adam_supported = _sh_adam_supported
# (likewise: the function takes `gradient_records`; a stand-in without the attribute is never handed one)
rasterize_gaussians_backward.gradient_records_supported = True


def _image_tail_supported(W, H):
    """The pseudo-normal pass that rasterize_gaussians_begin(defer_pseudo_normal=True) leaves to its caller can run inside the fused
    stage-2 image tail (r3dg_stage2_image_tail_supported: the library has the kernel for a W x H image)?"""
    return _lib.lib().r3dg_stage2_image_tail_supported(int(W), int(H)) == 1


# (asked of the FUNCTION that defers the pass, as sh_adam_supported above: a stand-in without the attribute keeps the four launches)
rasterize_gaussians_begin.image_tail_supported = _image_tail_supported


def rasterize_gaussians_backward_features(P, S, image_height, image_width, dL_dout_feature, geomBuffer, R, binningBuffer,
                                          imageBuffer, debug=False, active_features=None):
    """The backward for FROZEN geometry (not in the reference; r3dg_rasterize_backward_features): only dL_dfeatures [P,S]
    from dL_dout_feature [S,H,W] -- what is left of rasterize_gaussians_backward when positions, covariances, opacities and
    SH colour have learning rate 0 (script/run_syn4.sh:27-33, run_dtu.sh).  Same state buffers and `active_features`
    contract; equals that call's dL_dfeatures up to the order of the float atomics."""
    L = _lib.lib()
    dev = dL_dout_feature.device
    dL_dfeatures = torch.zeros((P, S), dtype=torch.float32, device=dev)
    if P != 0 and int(R) != 0:
        gF = _f32c(dL_dout_feature)
        if active_features is None:
            n_act, act = -1, None
        else:
            n_act = len(active_features)
            act = (C.c_int * max(1, n_act))(*[int(a) for a in active_features])
        with torch.cuda.device(dev):
            st = L.r3dg_rasterize_backward_features(
                _lib.current_stream(), int(P), int(S), int(R), int(image_width), int(image_height), _lib.ptr(geomBuffer),
                _lib.ptr(binningBuffer), _lib.ptr(imageBuffer), gF.data_ptr(), dL_dfeatures.data_ptr(), n_act, act,
                int(bool(debug)))
        _lib.check(st, "rasterize_gaussians_backward_features")
    return dL_dfeatures


def mark_visible(means3D, viewmatrix, projmatrix):
    L = _lib.lib()
    P = means3D.size(0)
    present = torch.zeros((P,), dtype=torch.bool, device=means3D.device)
    if P != 0:
        m, v, p = _f32c(means3D), _f32c(viewmatrix), _f32c(projmatrix)
        with torch.cuda.device(means3D.device):
            st = L.r3dg_mark_visible(_lib.current_stream(), P, m.data_ptr(), v.data_ptr(), p.data_ptr(),
                                     present.data_ptr())
        _lib.check(st, "mark_visible")
    return present


def num_rendered_of(geomBuffer, P):
    """0-d int64 DEVICE tensor viewing the instance count of the forward that wrote `geomBuffer` (what a bounded forward
    does not hand to the host)."""
    off = int(_lib.lib().r3dg_geometry_state_total_offset(int(P)))
    return geomBuffer[off:off + 8].view(torch.int64)[0]


# ---- helpers for tests / debugging: decode the opaque state buffers ---------------------------------------
def decode_state(geomBuffer, binningBuffer, imgBuffer, P, R, H, W):
    L = _lib.lib()
    T = ((W + 15) // 16) * ((H + 15) // 16)
    g = _offsets(L.r3dg_geometry_state_offsets, 9, P)
    i = _offsets(L.r3dg_image_state_offsets, 3, W, H)
    b = _offsets(L.r3dg_binning_state_offsets, 4, R)

    def view(buf, off, count, dtype, shape):
        nb = count * torch.empty((), dtype=dtype).element_size()
        return buf[off:off + nb].view(dtype).view(*shape)
    out = dict(
        depths=view(geomBuffer, g[0], P, torch.float32, (P,)),
        clamped=view(geomBuffer, g[1], 3 * P, torch.uint8, (P, 3)),
        means2D=view(geomBuffer, g[3], 2 * P, torch.float32, (P, 2)),
        cov3D=view(geomBuffer, g[4], 6 * P, torch.float32, (P, 6)),
        conic_opacity=view(geomBuffer, g[5], 4 * P, torch.float32, (P, 4)),
        rgb=view(geomBuffer, g[6], 3 * P, torch.float32, (P, 3)),
        tiles_touched=view(geomBuffer, g[7], P, torch.int32, (P,)),
        point_offsets=view(geomBuffer, g[8], P, torch.int32, (P,)),
        final_T=view(imgBuffer, i[0], H * W, torch.float32, (H, W)),
        n_contrib=view(imgBuffer, i[1], H * W, torch.int32, (H, W)),
        ranges=view(imgBuffer, i[2], 2 * T, torch.int32, (T, 2)),
    )
    if R > 0:
        out.update(
            keys_unsorted=view(binningBuffer, b[0], R, torch.int64, (R,)),
            keys=view(binningBuffer, b[1], R, torch.int64, (R,)),
            vals_unsorted=view(binningBuffer, b[2], R, torch.int32, (R,)),
            point_list=view(binningBuffer, b[3], R, torch.int32, (R,)),
        )
    return out
