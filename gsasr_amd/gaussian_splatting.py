"""Rasterizer host API -- mirror of the reference's utils/gaussian_splatting.py (same function names,
arguments, defaults and error behaviour), with the CUDA ops replaced by the HIP rasterizer.

    generate_2D_gaussian_splatting_step(sr_size, gs_parameters, scale, scale_modify, sample_coords=None,
        default_step_size=1.2, cuda_rendering=True, mode='scale_modify', if_dmax=True,
        dmax_mode='fix', dmax=25) -> [3,H,W]                      (reference :158-217)
    generate_2D_gaussian_splatting_step_buffer(..., buffer_size=4000000)   (reference :219-265)
    generate_2D_gaussian_splatting_query(sr_size, gs_parameters, scale, scale_modify, query_coords, ...) -> [3,S]
                                                                  (no reference counterpart: the splat evaluated at
                                                                   fractional pixel positions (r, c) of the sr_size grid)
    rendering_cuda / rendering_cuda_dmax / rendering_cuda_buffer / rendering_cuda_dmax_buffer
                                                                  (reference :86-155)
    rendering_python                                               (reference :11-84)

`gs_parameters[N,9]` columns are the decoder's raw `[sigma_x, sigma_y, rho, alpha, r, g, b, mu_x, mu_y]`
(reference utils/fea2gs.py:632-635).  Everything here is ordinary differentiable torch code on the
tensors' own device; the only custom op is `GSCUDA.apply` (gsasr_amd/gs_cuda*/gswrapper.py).
`cuda_rendering=False` selects the reference's pure-PyTorch *approximation* (`rendering_python`); it
is part of the API surface and is never used as a fallback for the HIP path.
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

from ._amp import fp32_boundary_bwd, fp32_boundary_fwd


def _capturing() -> bool:
    """is the current stream being captured into a graph (no caching of tensors created then, no deferred checks)"""
    return torch.cuda.is_available() and torch.cuda.is_current_stream_capturing()


def _hw(sr_size):
    # sr_size arrives as list, CPU tensor or GPU int tensor (gsasr_model.py:148,202); make ints once -- a GPU tensor
    # with ONE device-to-host copy (the reference's `int(sr_size[0])`, `int(sr_size[1])` are two synchronisations)
    if torch.is_tensor(sr_size):
        v = sr_size.tolist()
        return int(v[0]), int(v[1])
    return int(sr_size[0]), int(sr_size[1])


def _to_kernel_frame(sigma_x, sigma_y, rho, coords, colours_with_alpha, sr_size, step_size):
    """sigmas/coords in the kernels' align-corners frame (reference :121-124): note the x/y swap -- the
    network's sigma_x is the ROW std, the kernel's first sigma pairs with WIDTH."""
    H, W = _hw(sr_size)
    sigmas = torch.cat([sigma_y / step_size * 2 / (W - 1), sigma_x / step_size * 2 / (H - 1), rho],
                       dim=-1).contiguous()
    cx = (coords[:, 0:1] + 1 - 1 / W) * W / (W - 1) - 1.0
    cy = (coords[:, 1:2] + 1 - 1 / H) * H / (H - 1) - 1.0
    return sigmas, torch.cat([cx, cy], dim=-1).contiguous(), colours_with_alpha.contiguous(), H, W


class _Splat(torch.autograd.Function):
    """`GSCUDA.apply(sigmas, coords, colors, zeros(H,W,3)[, dmax])` without the zero image: the forward kernel
    stores into an uninitialised buffer (GSASR_FLAG_OVERWRITE_IMAGE) -- same values, one memset and one
    12 B/px read less.  Used only where this module itself owns the image (the non-chunked renderers)."""

    @staticmethod
    @fp32_boundary_fwd
    def forward(ctx, sigmas, coords, colors, H, W, dmax):
        from . import _cabi
        plan = _cabi.plan(sigmas, coords, colors, H, W, dmax)
        img = torch.empty(H, W, 3, device=sigmas.device, dtype=torch.float32)
        _cabi.forward(plan, img, overwrite=True)
        ctx.save_for_backward(sigmas, coords, colors)
        ctx.plan = plan
        return img

    @staticmethod
    @torch.autograd.function.once_differentiable
    @fp32_boundary_bwd
    def backward(ctx, grad_output):
        from . import _cabi
        sigmas, coords, colors = ctx.saved_tensors
        g = (torch.empty_like(sigmas), torch.empty_like(coords), torch.empty_like(colors))
        _cabi.backward(ctx.plan, sigmas, coords, colors, grad_output.contiguous(), *g, overwrite=True)
        return (*g, None, None, None)


class _SplatInto(torch.autograd.Function):
    """One chunk of a chunked render: `img += splat(chunk)` into the image this module owns, with the support cutoff of
    the WHOLE set (`cutoff`): the adaptive default is tau = ln(N/1e-5), and chunks planned on their own would each cull
    with their own smaller tau -- the skipped mass would grow with the number of chunks (tools/fuzz_host.py: 1e-4 of an
    image rendered in 1 700 chunks) instead of staying below 1e-5.  Unlike a chain of the reference-shaped
    `GSCUDA.apply` calls (whose backward returns None for `rendered_img`, so only the LAST chunk would see a gradient --
    the reference's chain has the same gap, utils/gaussian_splatting.py:146-151), the image's gradient is passed on: every
    chunk is differentiated."""

    @staticmethod
    @fp32_boundary_fwd
    def forward(ctx, sigmas, coords, colors, img, dmax, cutoff):
        from . import _cabi
        sigmas, coords, colors = sigmas.contiguous(), coords.contiguous(), colors.contiguous()
        plan = _cabi.plan(sigmas, coords, colors, img.shape[0], img.shape[1], dmax, cutoff=cutoff)
        _cabi.forward(plan, img, overwrite=False)
        ctx.mark_dirty(img)
        ctx.save_for_backward(sigmas, coords, colors)
        ctx.plan = plan
        return img

    @staticmethod
    @torch.autograd.function.once_differentiable
    @fp32_boundary_bwd
    def backward(ctx, grad_output):
        from . import _cabi
        sigmas, coords, colors = ctx.saved_tensors
        g = (torch.empty_like(sigmas), torch.empty_like(coords), torch.empty_like(colors))
        _cabi.backward(ctx.plan, sigmas, coords, colors, grad_output.contiguous(), *g, overwrite=True)
        return (*g, grad_output, None, None)


def _render_chunked(sigmas, xy, col, H, W, dmax, device, buffer_size):
    from . import _cabi
    final_image = torch.zeros(H, W, 3, device=device, dtype=torch.float32)
    tau = _cabi.resolve_cutoff(0.0, max(1, sigmas.shape[0]))
    for a, b in _chunks(sigmas.shape[0], buffer_size):
        if sigmas[a:b].shape[0] == 0:
            continue
        final_image = _SplatInto.apply(sigmas[a:b], xy[a:b], col[a:b], final_image, dmax, tau)   # kernels accumulate (+=)
    return final_image.permute(2, 0, 1).contiguous()


# Which backward kernel the fused entry points plan for: "gaussian" (one wave per Gaussian; needs the upstream gradient
# permuted to [H,W,3]), "tile" (one workgroup per 32x16-px tile; reads the planar gradient in place; deterministic), "home"
# (round 6: a workgroup finishes the Gaussians binned in its tile from a staged region; interleaved gradient; deterministic)
# or "auto" (the measured choice per shape).
BACKWARD_KERNEL = "auto"


def _backward_kernel(n_pixels: int, n_gaussians: int, shape=None) -> int:
    """the C flag of the backward kernel the fused entry points plan for (FLAG_BWD_TILE / _GAUSSIAN / _HOME): the forced one, a
    choice registered for `shape()`, or the rule.  Measured through this API on MI355X (tools/e2e_modes.py,
    profiles/history/r02_e2e_modes.txt): with >= 4 HR pixels per Gaussian (one Gaussian per LR pixel at x2 and up) the
    tile-stationary backward is level or ahead end to end -- it reads the planar gradient in place, where the
    Gaussian-stationary kernel needs it interleaved first -- and it is deterministic; at 16 Gaussians per LR pixel (the training
    crops: ~1 pixel per Gaussian) a tile holds thousands of Gaussians and the Gaussian-stationary kernel is 15-50% faster.  Small
    images have too few tiles to fill the chip."""
    from . import _cabi
    forced = {"tile": _cabi.FLAG_BWD_TILE, "gaussian": _cabi.FLAG_BWD_GAUSSIAN, "home": _cabi.FLAG_BWD_HOME}.get(BACKWARD_KERNEL)
    if forced is not None:
        return forced
    if shape is not None and _cabi.kernel_choices_registered():      # a choice measured and registered for this shape (gsasr_amd/tune.py)
        hit = _cabi.get_kernel_choice(shape())
        if hit is not None:
            for f in (_cabi.FLAG_BWD_TILE, _cabi.FLAG_BWD_GAUSSIAN, _cabi.FLAG_BWD_HOME):
                if hit[0] & f:
                    return f
    if n_pixels >= 4 * n_gaussians and n_pixels >= 128 * 1024:
        return _cabi.FLAG_BWD_TILE
    # round 6 (the library's own rule, splat_common.h:bwd_wants_home): denser than one Gaussian per two pixels on at least 1024 tiles
    # of 32 x 16 px -- through this API 1024^2 at 16 per LR pixel -5%, 1280^2 -7%, 1152^2 x3 -17%, a batch of 16 x 256^2 -4%
    # (profiles/r06_home_default.txt)
    if n_pixels < 2 * n_gaussians and n_pixels >= 1024 * 512:
        return _cabi.FLAG_BWD_HOME
    return _cabi.FLAG_BWD_GAUSSIAN


def _step_shape(n, H, W, dm):
    from . import _cabi
    return lambda: _cabi.make_dims(n, H, W, dm)


def _batch_shape(n_per, sizes, dm):
    from . import _cabi
    return lambda: _cabi.make_batch_dims(n_per, sizes, max(w for _, w in sizes), max(h for h, _ in sizes), dm)


def _step_kernel(n, H, W, dm, window=None) -> int:
    """`_backward_kernel` of a fused step: `n` Gaussians on the H x W grid, or on its `window` = (y0, x0, h, w) -- then for the
    Gaussians the window can expect, as the library judges a view (no registered choice).  The Python and the C++ node both
    plan with this flag."""
    if window is None:
        return _backward_kernel(H * W, n, _step_shape(n, H, W, dm))
    h, w = window[2], window[3]
    live = max(1, n * (h * w) // (H * W))
    return _backward_kernel(h * w, live)


def _canvas_kernel(n_per, B, sizes, dm, views=None) -> int:
    """`_step_kernel` of a canvas of B samples of `n_per` Gaussians, `sizes[b]` the slot's image or, with `views`, its window"""
    n_pixels = sum(h * w for h, w in sizes)
    if views is None:
        return _backward_kernel(n_pixels, B * n_per, _batch_shape(n_per, sizes, dm))
    live = max(1, sum(n_per * (h * w) // (v[0] * v[1]) for (h, w), v in zip(sizes, views)))
    return _backward_kernel(n_pixels, live)


# The caller's scale factor as a HINT for the forward kernel (never for the numbers).  The C library sees pixels per Gaussian, which
# says "x2-sized windows" for x8 at Fea2GS's 16 Gaussians per LR pixel (4 px per Gaussian) -- the windows there are x8's, and the
# wide forward (16 x 16-px sub-tiles) is 5..8% ahead (profiles/history/r05_inference_sweep.txt: x8d16_2048).  This module knows the scale.
SCALE_HINT = True


def _forward_flag(scale, H: int, W: int) -> int:
    """FLAG_FWD_WIDE from x5 up on images of 2 Mpx and more (the library's own line at one Gaussian per LR pixel), else 0"""
    if not SCALE_HINT or isinstance(scale, bool) or not isinstance(scale, (int, float)):
        return 0            # (a tensor would cost a synchronisation to read: the library's rule stays)
    from . import _cabi
    return _cabi.FLAG_FWD_WIDE if scale >= 5.0 and H * W >= 2 * 1024 * 1024 else 0


def _plan_flags(needs_grad: bool, kernel) -> int:
    """flags of a fused step's plan: the backward kernel is chosen HERE, explicitly (the library's own default would
    otherwise plan slots for large images that this module then never uses); planar gradient in, forward-only plans
    for inference.  `kernel`: the C flag from _backward_kernel"""
    from . import _cabi
    if not needs_grad:
        return _cabi.FLAG_FORWARD_ONLY
    return _cabi.FLAG_CHW_GRAD | int(kernel)


class _FusedStep(torch.autograd.Function):
    """raw decoder output `gs_parameters[N,9]` -> `[3,H,W]` image with ONE prologue kernel (activations +
    kernel-frame conversion, reference :174-180 and :121-123) in front of the splat, the splat writing the
    planar layout directly (no `permute(2,0,1).contiguous()` pass, reference :129), and the matching chain
    rule behind the splat's backward.  Replaces ~15 elementwise launches in forward
    and ~30 in backward; numerically the same expressions evaluated in fp32.  The step size is `step` (a `[1]`
    device tensor), or -- `step is None` -- `default_step / scale_modify[0]` formed on the device from the caller's
    `scale_modify` tensor (`_StepSource`)."""

    @staticmethod
    @fp32_boundary_fwd
    def forward(ctx, gs_parameters, step, H, W, dmax, scale_modify=None, default_step=1.2, extra_flags=0, window=None):
        from . import _cabi
        # `window`: the h x w window at (y0, x0) of the H x W grid (generate_2D_gaussian_splatting_view)
        h, w, view = (H, W, None) if window is None else (window[2], window[3], (H, W, window[0], window[1]))
        # the planar gradient autograd hands back goes to the C call as it is (GSASR_FLAG_CHW_GRAD): the
        # tile-stationary backward stages the planes directly, the Gaussian-stationary one behind one interleaving
        # kernel inside the same call -- no torch permute / allocation on the host path either way
        flags = _plan_flags(ctx.needs_input_grad[0], _step_kernel(gs_parameters.shape[0], H, W, dmax, window)) | int(extra_flags)
        img, plan = _cabi.step_forward(gs_parameters, step, h, w, dmax, flags, scale_modify, default_step, view=view)   # one C call: prologue + plan + splat
        ctx.save_for_backward(gs_parameters, step)
        ctx.plan = plan
        return img

    @staticmethod
    @torch.autograd.function.once_differentiable
    @fp32_boundary_bwd
    def backward(ctx, grad_output):
        from . import _cabi
        gs_parameters, step = ctx.saved_tensors
        g = _cabi.step_backward(ctx.plan, gs_parameters, step, grad_output.contiguous(), chw=True)
        return g, None, None, None, None, None, None, None, None


class _FusedStepSampled(torch.autograd.Function):
    """`_FusedStep` for `sample_coords`: only the requested pixels are evaluated (`[3,S]`), instead of rendering
    `[3,H,W]` and indexing it once per point as the reference does (:214-216).  The backward is
    the sampled one too: each Gaussian visits the points inside its window, not every pixel of it."""

    @staticmethod
    @fp32_boundary_fwd
    def forward(ctx, gs_parameters, step, H, W, dmax, points, scale_modify=None, default_step=1.2):
        from . import _cabi
        out, plan, state = _cabi.step_sample_forward(gs_parameters, step, H, W, dmax, points, scale_modify, default_step)
        ctx.save_for_backward(gs_parameters, step)
        ctx.plan, ctx.state = plan, state
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    @fp32_boundary_bwd
    def backward(ctx, grad_output):
        from . import _cabi
        gs_parameters, step = ctx.saved_tensors
        return (_cabi.step_sample_backward(ctx.plan, ctx.state, gs_parameters, step, grad_output.contiguous()),
                None, None, None, None, None, None, None)


class _FusedBatchSampled(torch.autograd.Function):
    """`_FusedBatch` for `sample_coords[B,S,2]` -> `[B,3,S]`."""

    @staticmethod
    @fp32_boundary_fwd
    def forward(ctx, gs_parameters, steps, sizes, dmax, points):
        from . import _cabi
        out, plan, state = _cabi.batch_sample_forward(gs_parameters, steps, sizes, dmax, points)
        ctx.save_for_backward(gs_parameters, steps)
        ctx.plan, ctx.state = plan, state
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    @fp32_boundary_bwd
    def backward(ctx, grad_output):
        from . import _cabi
        gs_parameters, steps = ctx.saved_tensors
        return (_cabi.step_sample_backward(ctx.plan, ctx.state, gs_parameters, steps, grad_output.contiguous()),
                None, None, None, None)


def _query_backward(ctx, grad_output, points_arg):
    """the two backward passes of a query, each only when its input needs a gradient: the Gaussians' (query backward + prologue
    backward) and the positions' (`gsasr_step_query_backward_points`: like `query_coords` in shape, dtype and device)"""
    from . import _cabi
    gs_parameters, step = ctx.saved_tensors
    go = grad_output.contiguous()
    g_par = _cabi.step_query_backward(ctx.plan, ctx.state, gs_parameters, step, go) if ctx.needs_input_grad[0] else None
    g_pts = None
    if ctx.needs_input_grad[points_arg]:
        dtype, device = ctx.points_like
        g_pts = _cabi.step_query_backward_points(ctx.plan, ctx.state, go).to(device=device, dtype=dtype)
    return g_par, g_pts


class _FusedStepQuery(torch.autograd.Function):
    """`_FusedStepSampled` at fractional pixel positions: float `(r, c)` points on a continuous plan (`[3,S]`).  The gradient goes
    to `gs_parameters` and, when `points` requires it (`coords_grad=True`), to the positions."""

    @staticmethod
    @fp32_boundary_fwd
    def forward(ctx, gs_parameters, step, H, W, dmax, points, scale_modify=None, default_step=1.2):
        from . import _cabi
        out, plan, state = _cabi.step_query_forward(gs_parameters, step, H, W, dmax, points, scale_modify, default_step)
        ctx.save_for_backward(gs_parameters, step)
        ctx.plan, ctx.state, ctx.points_like = plan, state, (points.dtype, points.device)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    @fp32_boundary_bwd
    def backward(ctx, grad_output):
        g_par, g_pts = _query_backward(ctx, grad_output, 5)
        return g_par, None, None, None, None, g_pts, None, None


class _FusedBatchQuery(torch.autograd.Function):
    """`_FusedBatchSampled` for `query_coords[B,S,2]` (float) -> `[B,3,S]`; the positions' gradient as in `_FusedStepQuery`."""

    @staticmethod
    @fp32_boundary_fwd
    def forward(ctx, gs_parameters, steps, sizes, dmax, points):
        from . import _cabi
        out, plan, state = _cabi.batch_query_forward(gs_parameters, steps, sizes, dmax, points)
        ctx.save_for_backward(gs_parameters, steps)
        ctx.plan, ctx.state, ctx.points_like = plan, state, (points.dtype, points.device)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    @fp32_boundary_bwd
    def backward(ctx, grad_output):
        g_par, g_pts = _query_backward(ctx, grad_output, 4)
        return g_par, None, None, None, g_pts


# Kernel time of the sampled path equals the full render's at about a quarter of the pixels, but the alternative ends
# in a torch advanced-indexing gather whose backward (index_put_ with accumulate) takes longer than either rasterizer
# (DESIGN.md 3b): the sampled kernels are used unless the points outnumber the pixels.
SAMPLED_MAX_FRACTION = 1.0


def _as_points(sample_coords):
    """`sample_coords` as an integer `[S,2]` tensor, or None if it is not a plain list/tensor of (row, column) pairs"""
    sc = sample_coords
    if not torch.is_tensor(sc):
        try:
            sc = torch.as_tensor(sc)
        except Exception:
            return None
    if sc.dim() != 2 or sc.shape[1] != 2 or sc.dtype.is_floating_point or sc.dtype == torch.bool:
        return None
    return sc


def _fused_ok(gs_parameters) -> bool:
    return gs_parameters.is_cuda and gs_parameters.dtype == torch.float32 and gs_parameters.dim() == 2 \
        and gs_parameters.shape[1] == 9


_STEP_TENSORS = {}      # (value(s), device, stream) -> float32 device tensor of python-number step sizes (read-only)


def _cached_constant(value, dev):
    """read-only float32 device tensor of python numbers -- a float: `[1]`, a tuple of floats: `[len]` -- made once per DISTINCT
    value, device and stream (the tensor is filled asynchronously on the stream that first asks for the value); made afresh,
    and not kept, while that stream is being captured"""
    capturing = _capturing()
    key = (value, dev, None if capturing else torch.cuda.current_stream(dev).cuda_stream)
    t = None if capturing else _STEP_TENSORS.get(key)
    if t is None:
        if value.__class__ is float:
            t = torch.full((1,), value, device=dev, dtype=torch.float32)
        else:
            t = torch.tensor(value, dtype=torch.float32, device=dev)
        if not capturing:
            if len(_STEP_TENSORS) > 256:
                _STEP_TENSORS.clear()
            _STEP_TENSORS[key] = t
    return t


def _step_tensor(step_size, dev):
    if torch.is_tensor(step_size):
        return step_size.detach().to(device=dev, dtype=torch.float32).reshape(1)   # stays on the device: no sync
    return _cached_constant(float(step_size), dev)


class _StepSource:
    """`default_step_size / scale_modify[0]`, not evaluated: the fused entry points hand the caller's `scale_modify`
    tensor to the plan's first kernel, which forms the step size and checks `[0] == [1]` itself (gsasr_step_forward_sm)"""
    __slots__ = ("scale_modify", "default_step")

    def __init__(self, scale_modify, default_step):
        self.scale_modify, self.default_step = scale_modify, default_step


def _fused_step_args(step_size, dev):
    """`(step, scale_modify, default_step, watch)` of a fused launch from what `_step_size(..., fused=True)` returned: the
    caller's device pair and nothing evaluated (`watch`: count the call with `deferred_asserts.watch` AFTER the launch -- a
    look covers this call's own pair), or the value (a python number or a tensor) as a `[1]` device tensor"""
    if step_size.__class__ is _StepSource:
        return None, step_size.scale_modify, step_size.default_step, True
    return _step_tensor(step_size, dev), None, 1.2, False


def _fused_step(gs_parameters, step, H, W, dm, scale_modify=None, default_step=1.2, extra_flags=0):
    """`_FusedStep.apply`, as a C++ autograd node when the extension is there (gsasr_amd/_cpp_node.py: the engine calls its
    backward without taking the GIL -- the reference's training loop makes sixteen of these nodes per step)"""
    from . import _cpp_node
    if _cpp_node.load() is None:
        return _FusedStep.apply(gs_parameters, step, H, W, dm, scale_modify, default_step, extra_flags)
    needs_grad = gs_parameters.requires_grad and torch.is_grad_enabled()
    flags = _plan_flags(needs_grad, _step_kernel(gs_parameters.shape[0], H, W, dm)) | int(extra_flags)
    return _cpp_node.fused_step_apply(gs_parameters, step, H, W, dm, flags, scale_modify, default_step)


def _fused_batch(gs_parameters, steps, sizes, dm, scale_modify=None, default_step=1.2):
    """`_FusedBatch.apply`, through the same C++ node when it is there"""
    from . import _cpp_node
    if _cpp_node.load() is None:
        return _FusedBatch.apply(gs_parameters, steps, sizes, dm, scale_modify, default_step)
    needs_grad = gs_parameters.requires_grad and torch.is_grad_enabled()
    flags = _plan_flags(needs_grad, _canvas_kernel(gs_parameters.shape[1], gs_parameters.shape[0], sizes, dm))
    return _cpp_node.fused_step_apply(gs_parameters, steps, 0, 0, dm, flags, scale_modify, default_step, sizes=sizes)


def rendering_cuda(sigma_x, sigma_y, rho, coords, colours_with_alpha, sr_size, step_size, device):
    sigmas, xy, col, H, W = _to_kernel_frame(sigma_x, sigma_y, rho, coords, colours_with_alpha, sr_size, step_size)
    final_image = _Splat.apply(sigmas, xy, col, H, W, None)
    return final_image.permute(2, 0, 1).contiguous()


def rendering_cuda_dmax(sigma_x, sigma_y, rho, coords, colours_with_alpha, sr_size, step_size, device, dmax=1):
    sigmas, xy, col, H, W = _to_kernel_frame(sigma_x, sigma_y, rho, coords, colours_with_alpha, sr_size, step_size)
    final_image = _Splat.apply(sigmas, xy, col, H, W, float(dmax))
    return final_image.permute(2, 0, 1).contiguous()


def _chunks(n, buffer_size):
    # the reference runs len//buffer_size + 1 slices, the last possibly empty (:146-151)
    for k in range(n // buffer_size + 1):
        yield k * buffer_size, (k + 1) * buffer_size


def rendering_cuda_buffer(sigma_x, sigma_y, rho, coords, colours_with_alpha, sr_size, step_size, device,
                          buffer_size=1000000):
    sigmas, xy, col, H, W = _to_kernel_frame(sigma_x, sigma_y, rho, coords, colours_with_alpha, sr_size, step_size)
    return _render_chunked(sigmas, xy, col, H, W, None, device, buffer_size)


def rendering_cuda_dmax_buffer(sigma_x, sigma_y, rho, coords, colours_with_alpha, sr_size, step_size, device,
                               dmax=1, buffer_size=1000000):
    sigmas, xy, col, H, W = _to_kernel_frame(sigma_x, sigma_y, rho, coords, colours_with_alpha, sr_size, step_size)
    return _render_chunked(sigmas, xy, col, H, W, float(dmax), device, buffer_size)


def rendering_python(sigma_x, sigma_y, rho, coords, colours_with_alpha, sr_size, step_size, device):
    """The reference's `cuda_rendering=False` path (:11-84): every Gaussian is sampled on a
    `num_step x num_step` grid in sigma units, normalised by its sampled peak (+1e-4) and bilinearly
    resampled onto the HR grid centred at its mean.  An approximation of the kernels, kept for API
    completeness (BASELINE.json config 1); plain torch ops on `device`."""
    H, W = _hw(sr_size)
    # `step_size` is used as it comes: in the reference's default mode it is the 0-dim fp32 tensor
    # `default_step_size / scale_modify[0]`, so `10 * 2 / step_size` and `i * step_size` are fp32 operations -- at scale 3.3
    # the grid has int(55.0) = 55 steps where the same expression on the Python float gives int(54.9999...) = 54
    # (tests/golden/tiled_frac_s3p3_30x16.npz)
    step = step_size
    n = sigma_x.shape[0]
    cxy = rho * sigma_x * sigma_y
    if ((sigma_x ** 2) * (sigma_y ** 2) - cxy ** 2 < 0).any():
        raise ValueError("Covariance matrix must be positive semi-definite")
    cov = torch.stack([torch.cat([sigma_x ** 2, cxy], -1), torch.cat([cxy, sigma_y ** 2], -1)], dim=-2)
    inv = torch.inverse(cov)
    num_step = int(10 * 2 / step)
    ax = torch.tensor([k * step for k in range(num_step)], device=device)
    ax = ax - ax.mean()
    xy = torch.stack([ax[:, None].expand(num_step, num_step), ax[None, :].expand(num_step, num_step)], dim=-1)
    final_image = torch.zeros((3, H, W), device=device)
    max_buffer = 2000
    for s0 in range(0, n, max_buffer):
        s1 = min(s0 + max_buffer, n)
        b = s1 - s0
        z = torch.einsum("xyi,bij,xyj->bxy", xy, -0.5 * inv[s0:s1], xy)
        kernel = torch.exp(z) / (2 * math.pi * torch.sqrt(torch.det(cov[s0:s1])).view(b, 1, 1))
        kernel = kernel / (kernel.amax(dim=(-1, -2), keepdim=True) + 1e-4)
        kernel = kernel[:, None].expand(b, 3, num_step, num_step)
        theta = torch.zeros(b, 2, 3, dtype=torch.float32, device=device)
        theta[:, 0, 0] = W / num_step
        theta[:, 1, 1] = H / num_step
        theta[:, 0, 2] = -coords[s0:s1, 0] * W / num_step
        theta[:, 1, 2] = -coords[s0:s1, 1] * H / num_step
        grid = F.affine_grid(theta, size=(b, 3, H, W), align_corners=False)
        moved = F.grid_sample(kernel, grid, align_corners=False)
        final_image = final_image + (colours_with_alpha[s0:s1, :, None, None] * moved).sum(0)
    return final_image


# The reference's `assert scale_modify[0] == scale_modify[1]` without a host synchronisation per call: gsasr_amd/_deferred.py
from ._deferred import _DeferredAsserts, deferred_asserts  # noqa: E402,F401


def _sm_source_ok(scale_modify) -> bool:
    """can the fused entry points read this `scale_modify` on the device themselves (a `[2]`-like float32 CUDA tensor)"""
    return (scale_modify.__class__ is torch.Tensor and scale_modify.is_cuda and scale_modify.dtype is torch.float32
            and scale_modify.dim() == 1 and scale_modify.shape[0] >= 2 and scale_modify.stride(0) == 1)


def _step_size(scale, scale_modify, default_step_size, mode, fused=False):
    """the reference's step size (:163-172).  `fused`: the caller is the fused path, which can take a `_StepSource`
    (scale_modify left on the device, nothing evaluated here) instead of a value"""
    if mode == 'scale':
        final_scale = scale
    elif mode == 'scale_modify':
        if fused and _sm_source_ok(scale_modify):
            return _StepSource(scale_modify, float(default_step_size))
        if torch.is_tensor(scale_modify) and scale_modify.is_cuda and not _capturing():
            deferred_asserts.add(scale_modify, "scale_modify is not the same")
        elif not (torch.is_tensor(scale_modify) and scale_modify.is_cuda):
            assert scale_modify[0] == scale_modify[1], f"scale_modify is not the same-{scale_modify}"
        final_scale = scale_modify[0]
    else:  # the reference leaves final_scale unbound here (UnboundLocalError, a NameError subclass)
        raise UnboundLocalError(f"mode-{mode} must be scale or scale_modify")
    return default_step_size / final_scale


def _activate(gs_parameters):
    # reference :174-180
    sigma_x = 0.99999 * torch.sigmoid(gs_parameters[:, 0:1]) + 1e-6
    sigma_y = 0.99999 * torch.sigmoid(gs_parameters[:, 1:2]) + 1e-6
    rho = 0.999999 * torch.tanh(gs_parameters[:, 2:3])
    alpha = torch.sigmoid(gs_parameters[:, 3:4])
    colours = torch.sigmoid(gs_parameters[:, 4:7])
    coords = gs_parameters[:, 7:9] * 2 - 1
    return sigma_x, sigma_y, rho, coords, colours * alpha


def _resolve_dmax(dmax, dmax_mode, sr_size):
    if dmax_mode == 'dynamic':
        H, W = _hw(sr_size)
        return (dmax + 2) / min(H, W)
    if dmax_mode == 'fix':
        return dmax
    raise ValueError(f"dmax_mode-{dmax_mode} must be fix or dynamic")


def _dmax_arg(dmax, dmax_mode, if_dmax, size):
    """the `dmax` of the C calls: `_resolve_dmax` on the `size` grid as a float, or None -- the unbounded op -- with `if_dmax` off"""
    if not if_dmax:
        return None
    d = _resolve_dmax(dmax, dmax_mode, size)
    return None if d is None else float(d)


def _sample(final_image, sample_coords):
    """reference :214-216: `stack([img[:, c[0], c[1]] for c in sample_coords], dim=1)` -> `[3, S]`.  An `[S,2]`
    integer tensor (what the datasets produce, continuous_bicubic_downsample_dataset.py:87-88) is gathered with
    ONE indexing op instead of S of them (same values, same gradient scatter); anything else takes the loop."""
    if sample_coords is None:
        return final_image
    if torch.is_tensor(sample_coords) and sample_coords.dim() == 2 and sample_coords.shape[1] == 2 \
            and not sample_coords.dtype.is_floating_point and sample_coords.dtype != torch.bool:
        sc = sample_coords.to(device=final_image.device, dtype=torch.long)
        return final_image[:, sc[:, 0], sc[:, 1]]
    return torch.stack([final_image[:, c[0], c[1]] for c in sample_coords], dim=1)


def generate_2D_gaussian_splatting_step(sr_size, gs_parameters, scale, scale_modify, sample_coords=None,
                                        default_step_size=1.2, cuda_rendering=True, mode='scale_modify',
                                        if_dmax=True, dmax_mode='fix', dmax=25):
    if gs_parameters.dtype != torch.float32:
        # under bf16 autocast the decoder happens to emit fp32; make that explicit
        gs_parameters = gs_parameters.float()
    fused = cuda_rendering and _fused_ok(gs_parameters)
    step_size = _step_size(scale, scale_modify, default_step_size, mode, fused=fused)
    if fused:
        # fused prologue + splat (same maths as the unfused branch below, one kernel instead of ~15)
        H, W = _hw(sr_size)
        dm = _dmax_arg(dmax, dmax_mode, if_dmax, (H, W))
        pts = _as_points(sample_coords) if sample_coords is not None else None
        sampled = pts is not None and 0 < pts.shape[0] <= SAMPLED_MAX_FRACTION * H * W
        step, sm, default_step, watch = _fused_step_args(step_size, gs_parameters.device)
        if sampled:
            out = _FusedStepSampled.apply(gs_parameters.contiguous(), step, H, W, dm, pts, sm, default_step)
        else:
            out = _fused_step(gs_parameters.contiguous(), step, H, W, dm, sm, default_step, _forward_flag(scale, H, W))
        if watch:
            deferred_asserts.watch(gs_parameters.device)
        return out if sampled else _sample(out, sample_coords)
    sigma_x, sigma_y, rho, coords, colours_with_alpha = _activate(gs_parameters)
    dev = sigma_x.device
    if cuda_rendering:
        if if_dmax:
            dmax = _resolve_dmax(dmax, dmax_mode, sr_size)
            final_image = rendering_cuda_dmax(sigma_x, sigma_y, rho, coords, colours_with_alpha, sr_size,
                                              step_size, dmax=dmax, device=dev)
        else:
            final_image = rendering_cuda(sigma_x, sigma_y, rho, coords, colours_with_alpha, sr_size, step_size,
                                         device=dev)
    else:
        final_image = rendering_python(sigma_x, sigma_y, rho, coords, colours_with_alpha, sr_size, step_size,
                                       device=dev)
    return _sample(final_image, sample_coords)


def _as_query(query_coords, batched=False, coords_grad=False):
    """`query_coords` as a floating-point `[S,2]` (`batched`: `[B,S,2]`) tensor of (r, c); the argument errors of the query API"""
    qc = query_coords if torch.is_tensor(query_coords) else torch.as_tensor(query_coords)
    if not qc.dtype.is_floating_point:
        raise ValueError("query_coords must be floating point (fractional pixel indices (r, c)); integer pixel indices go to sample_coords")
    if qc.dim() != (3 if batched else 2) or qc.shape[-1] != 2:
        raise ValueError("query_coords must be [B,S,2]" if batched else "query_coords must be [S,2]")
    if qc.requires_grad and not coords_grad:
        raise ValueError("query_coords.requires_grad: the gradient with respect to the positions is computed only on request "
                         "(pass coords_grad=True, or detach them)")
    return qc


def query_dense(sigmas, xy, col, H, W, dmax, query_coords):
    """The definition of a query, in plain differentiable torch (`[S,N]` terms): the point (r, c) sits at the pixel tables' own
    expression with a real index, px = float(2 c / (W - 1) - 1) formed in double, and is worth the op's sum there -- the
    reference kernels' exponent (gs_cuda/gs.cu:33-56) and, bounded op, their float32 box test |dx|, |dy| <= dmax per term.
    Outside 0 <= r <= H - 1, 0 <= c <= W - 1 (NaN and infinities included): 0, and no gradient.  `sigmas, xy, col`: the
    kernel-frame tensors (`_to_kernel_frame`).  The maths runs in float64; the result is `[3,S]` in the inputs' dtype."""
    qc = query_coords.to(device=sigmas.device, dtype=torch.float32)
    r, c = qc[:, 0], qc[:, 1]
    valid = (r >= 0) & (r <= H - 1) & (c >= 0) & (c <= W - 1)
    r, c = torch.where(valid, r, torch.zeros_like(r)), torch.where(valid, c, torch.zeros_like(c))
    px = (2.0 * c.double() / (W - 1) - 1.0).float()
    py = (2.0 * r.double() / (H - 1) - 1.0).float()
    inside = valid[:, None].expand(-1, sigmas.shape[0])
    if dmax is not None:   # the kernels' decision: float32 differences against the float32 dmax
        dm = torch.tensor(float(dmax), dtype=torch.float32, device=sigmas.device)
        dxf, dyf = px[:, None] - xy[:, 0].detach().float()[None, :], py[:, None] - xy[:, 1].detach().float()[None, :]
        inside = inside & (dxf.abs() <= dm) & (dyf.abs() <= dm)
    dx, dy = px.double()[:, None] - xy[:, 0].double()[None, :], py.double()[:, None] - xy[:, 1].double()[None, :]
    sx, sy, rho = sigmas[:, 0].double()[None, :], sigmas[:, 1].double()[None, :], sigmas[:, 2].double()[None, :]
    d = dx * dx / (sx * sx) - 2 * rho * dx * dy / (sx * sy) + dy * dy / (sy * sy)
    v = torch.where(inside, torch.exp(-0.5 / (1 - rho * rho) * d), torch.zeros((), dtype=torch.float64, device=sigmas.device))
    return (v @ col.double()).t().to(col.dtype)


def generate_2D_gaussian_splatting_query(sr_size, gs_parameters, scale, scale_modify, query_coords, default_step_size=1.2,
                                         cuda_rendering=True, mode='scale_modify', if_dmax=True, dmax_mode='fix', dmax=25,
                                         coords_grad=False):
    """The splatted image at fractional pixel positions: `query_coords` float `[S,2]` (tensor or nested list) of (r, c) on the
    `sr_size` grid -> `[3,S]`, differentiable in `gs_parameters`.  The Gaussians are a continuous image; pixel (i, j) of
    `generate_2D_gaussian_splatting_step` is the query (i, j), and (i + 0.5, j) lies halfway to the next row.  Domain:
    0 <= r <= H - 1, 0 <= c <= W - 1, ends included; a point outside it, or with a NaN / infinite component, gives 0 and no
    gradient.  Repeated points are independent outputs whose gradients add.  `coords_grad=True`: differentiable in the
    positions too -- `query_coords.grad` has `query_coords`' shape, dtype and device (host or float64 positions included); it is
    the derivative almost everywhere (neither the dmax box test nor the float32 rounding of the position is differentiated), the
    analytic value on the edge of the domain and (0, 0) for a point outside it.  Each of the two backward passes runs only
    when its input needs a gradient.  Without the keyword `query_coords.requires_grad` raises.  CUDA tensors: the HIP query
    kernels (fused prologue, fp32 under autocast); CPU tensors or `cuda_rendering=False`: the dense torch evaluation
    `query_dense`, never a fallback for the kernels."""
    qc = _as_query(query_coords, coords_grad=coords_grad)
    if gs_parameters.dtype != torch.float32:
        gs_parameters = gs_parameters.float()
    if gs_parameters.dim() != 2 or gs_parameters.shape[1] != 9:
        raise ValueError("gs_parameters must be [N,9]")
    H, W = _hw(sr_size)
    dm = _dmax_arg(dmax, dmax_mode, if_dmax, (H, W))
    fused = cuda_rendering and gs_parameters.is_cuda
    step_size = _step_size(scale, scale_modify, default_step_size, mode, fused=fused)
    if fused:
        if qc.shape[0] == 0:
            empty = gs_parameters.new_zeros((3, 0)) + 0.0 * gs_parameters.sum()
            return empty + (0.0 * qc.sum()).to(empty) if qc.requires_grad else empty      # (a graph to both inputs)
        step, sm, default_step, watch = _fused_step_args(step_size, gs_parameters.device)
        out = _FusedStepQuery.apply(gs_parameters.contiguous(), step, H, W, dm, qc, sm, default_step)
        if watch:
            deferred_asserts.watch(gs_parameters.device)
        return out
    sigma_x, sigma_y, rho, coords, colours_with_alpha = _activate(gs_parameters)
    sigmas, xy, col, H, W = _to_kernel_frame(sigma_x, sigma_y, rho, coords, colours_with_alpha, (H, W), step_size)
    return query_dense(sigmas, xy, col, H, W, dm, qc)


def quantise_uint8(image, crop=None, bgr=False):
    """The reference's inference epilogue (inference_paper.py:134-140, basicsr/utils/img_util.py:73-96) with torch ops: planar
    float `[3,H,W]` -> uint8 `[crop_h, crop_w, 3]` = `(clamp(x[:, :crop_h, :crop_w], 0, 1) * 255).round()` (half to even, like
    numpy), channels reversed with `bgr`; NaN -> 0.  What the 8-bit forward kernels store, for images that exist as floats."""
    x = image.detach()
    if crop is not None:
        x = x[:, : crop[0], : crop[1]]
    x = torch.nan_to_num(x.float(), nan=0.0).clamp(0, 1)
    if bgr:
        x = x.flip(0)
    return (x.permute(1, 2, 0) * 255.0).round().to(torch.uint8).contiguous()


def generate_2D_gaussian_splatting_step_uint8(sr_size, gs_parameters, scale, scale_modify, default_step_size=1.2,
                                              mode='scale_modify', if_dmax=True, dmax_mode='fix', dmax=25, crop=None, bgr=False,
                                              window=None):
    """`generate_2D_gaussian_splatting_step` for inference, handing over the picture instead of the tensor: uint8
    `[crop_h, crop_w, 3]` = `quantise_uint8` of the `[3,H,W]` image, i.e. the reference's
    `x[:, :, :gt_h, :gt_w] -> clamp_(0, 1) -> HWC -> (x * 255.0).round().astype(uint8)` in the call itself.  On CUDA tensors
    the forward kernels store the bytes directly (gsasr_step_forward_u8: no float image, a forward-only plan, no autograd
    graph) and there is no other path: anything the fused call cannot take raises.  On CPU tensors the image of
    `rendering_python` is quantised with torch ops.  `crop` = (rows, cols) of the top-left corner (default: everything),
    `bgr`: b, g, r byte order (cv2.imwrite).  `window` = (y0, x0, h, w): that window of the `sr_size` grid only
    (`generate_2D_gaussian_splatting_view`); `crop` and `bgr` then apply to the window."""
    if gs_parameters.dtype != torch.float32:
        gs_parameters = gs_parameters.float()
    H, W = _hw(sr_size)
    y0, x0, h, w = (0, 0, H, W) if window is None else _window(window, H, W)
    view = None if window is None else (H, W, y0, x0)
    crop = (h, w) if crop is None else (int(crop[0]), int(crop[1]))
    if not (1 <= crop[0] <= h and 1 <= crop[1] <= w):
        raise ValueError(f"crop-{crop} must lie inside " + (f"sr_size-{(H, W)}" if window is None else f"window-{(y0, x0, h, w)}"))
    if gs_parameters.is_cuda:
        if not _fused_ok(gs_parameters):
            raise RuntimeError("generate_2D_gaussian_splatting_step_uint8 needs gs_parameters [N,9] on the GPU (no fallback)")
        from . import _cabi
        step_size = _step_size(scale, scale_modify, default_step_size, mode, fused=True)
        dm = _dmax_arg(dmax, dmax_mode, if_dmax, (H, W))
        gp, flags = gs_parameters.detach().contiguous(), _forward_flag(scale, h, w)
        step, sm, default_step, watch = _fused_step_args(step_size, gp.device)
        out, _ = _cabi.step_forward_u8(gp, step, h, w, dm, crop, bgr, None, flags, sm, default_step, view)
        if watch:
            deferred_asserts.watch(gp.device)
        return out
    step_size = _step_size(scale, scale_modify, default_step_size, mode)
    sigma_x, sigma_y, rho, coords, colours_with_alpha = _activate(gs_parameters)
    image = rendering_python(sigma_x, sigma_y, rho, coords, colours_with_alpha, sr_size, step_size, device=sigma_x.device)
    return quantise_uint8(image[:, y0:y0 + h, x0:x0 + w], crop, bgr)


def generate_2D_gaussian_splatting_step_uint8_metrics(sr_size, gs_parameters, scale, scale_modify, gt, crop_border=0,
                                                      test_y_channel=False, default_step_size=1.2, mode='scale_modify', if_dmax=True,
                                                      dmax_mode='fix', dmax=25, crop=None, bgr=False, window=None):
    """`generate_2D_gaussian_splatting_step_uint8` and the validation metrics of its picture in one call: returns
    `(picture, metrics)`, the picture being bit for bit what `..._step_uint8` returns with the same arguments and `metrics`
    float64 `[2]` = {psnr, ssim} of it against `gt` (`gsasr_amd.metrics.image_metrics`: the reference's `calculate_psnr` /
    `calculate_ssim` with `crop_border` and `test_y_channel`).  `gt`: uint8 `[gt_h, gt_w, 3]` in the byte order `bgr` says, on the
    parameters' device; it defines `crop` when that is not given (the reference's `[:, :, :gt_h, :gt_w]`) and must have the
    crop's extent otherwise.  On CUDA tensors the 8-bit forward and gsasr_image_metrics run on the current stream, back to
    back, and nothing is read on the host: the picture need not leave the device for its metrics to exist."""
    from .metrics import image_metrics
    if not (torch.is_tensor(gt) and gt.dtype == torch.uint8 and gt.dim() == 3 and gt.shape[-1] == 3):
        raise ValueError("gt must be a uint8 tensor [gt_h, gt_w, 3]")
    if gt.device != gs_parameters.device:
        raise ValueError(f"gt is on {gt.device}, gs_parameters on {gs_parameters.device}")
    crop = (int(gt.shape[0]), int(gt.shape[1])) if crop is None else (int(crop[0]), int(crop[1]))
    if crop != (int(gt.shape[0]), int(gt.shape[1])):
        raise ValueError(f"Image shapes are different: {crop + (3,)}, {tuple(gt.shape)}.")
    picture = generate_2D_gaussian_splatting_step_uint8(sr_size, gs_parameters, scale, scale_modify, default_step_size, mode, if_dmax,
                                                        dmax_mode, dmax, crop, bgr, window)
    return picture, image_metrics(picture, gt, crop_border, test_y_channel, bgr)


def _window(window, H: int, W: int):
    """`window` = (y0, x0, h, w) on the H x W grid, checked: at least 2 x 2 pixels, inside the grid"""
    try:
        y0, x0, h, w = (int(v) for v in window)
    except (TypeError, ValueError):
        raise ValueError(f"window-{window} must be (y0, x0, h, w)") from None
    if not (h >= 2 and w >= 2 and 0 <= y0 and y0 + h <= H and 0 <= x0 and x0 + w <= W):
        raise ValueError(f"window-{(y0, x0, h, w)} must be at least 2 x 2 pixels and lie inside sr_size-{(H, W)}")
    return y0, x0, h, w


def generate_2D_gaussian_splatting_view(sr_size, gs_parameters, scale, scale_modify, window, default_step_size=1.2,
                                        cuda_rendering=True, mode='scale_modify', if_dmax=True, dmax_mode='fix', dmax=25):
    """`generate_2D_gaussian_splatting_step(...)[:, y0:y0+h, x0:x0+w]` for `window` = (y0, x0, h, w) on the `sr_size` grid,
    without the rest of the image: `[3, h, w]`, differentiable.  GSASR is arbitrary-scale -- a 1024 x 1024 look into a x30
    grid should cost what the window costs.  On CUDA tensors the fused step plans, renders and differentiates the window only
    (gsasr_step_forward_view: every pixel sits at its full-grid coordinate, same box test and cutoff rules; the plan still
    classifies all the Gaussians) and there is no other path; `dmax_mode` resolves against `sr_size`, not the window.  On CPU
    tensors, or with `cuda_rendering=False`, the slice of `rendering_python`'s image is returned."""
    if gs_parameters.dtype != torch.float32:
        gs_parameters = gs_parameters.float()
    H, W = _hw(sr_size)
    y0, x0, h, w = _window(window, H, W)
    fused = cuda_rendering and gs_parameters.is_cuda
    if fused and not _fused_ok(gs_parameters):
        raise RuntimeError("generate_2D_gaussian_splatting_view needs gs_parameters [N,9] on the GPU (no fallback)")
    step_size = _step_size(scale, scale_modify, default_step_size, mode, fused=fused)
    if not fused:
        sigma_x, sigma_y, rho, coords, colours_with_alpha = _activate(gs_parameters)
        image = rendering_python(sigma_x, sigma_y, rho, coords, colours_with_alpha, sr_size, step_size, device=sigma_x.device)
        return image[:, y0:y0 + h, x0:x0 + w]
    dm = _dmax_arg(dmax, dmax_mode, if_dmax, (H, W))
    gp = gs_parameters.contiguous()
    step, sm, default_step, watch = _fused_step_args(step_size, gp.device)
    # (the scale hint of the forward kernel reads the window's size: that is the image the kernels render)
    out = _FusedStep.apply(gp, step, H, W, dm, sm, default_step, _forward_flag(scale, h, w), (y0, x0, h, w))
    if watch:
        deferred_asserts.watch(gp.device)
    return out


class _FusedBatch(torch.autograd.Function):
    """A whole training batch in one set of launches: `gs_parameters[B,N,9]` ->
    `[B,3,Hmax,Wmax]`, sample b rendered on its own `sizes[b]` pixel grid in the top-left corner of its slot
    and zero elsewhere.  Replaces the reference's per-sample Python loop of `generate_2D_gaussian_splatting_step`
    + `F.pad` (basicsr/models/gsasr_model.py:191-233): B x (prologue, plan, splat) launches and B autograd nodes
    become one of each.  `views` = [(H_b, W_b, y0_b, x0_b)]: `sizes[b]` is then the window at (y0_b, x0_b) of sample b's own
    H_b x W_b grid (`generate_2D_gaussian_splatting_batch(windows=...)`)."""

    @staticmethod
    @fp32_boundary_fwd
    def forward(ctx, gs_parameters, steps, sizes, dmax, scale_modify=None, default_step=1.2, views=None):
        from . import _cabi
        flags = _plan_flags(ctx.needs_input_grad[0], _canvas_kernel(gs_parameters.shape[1], gs_parameters.shape[0], sizes, dmax, views))
        img, plan = _cabi.batch_forward(gs_parameters, steps, sizes, dmax, flags, scale_modify, default_step, views=views)
        ctx.save_for_backward(gs_parameters, steps)
        ctx.plan = plan
        ctx.h_max = max(h for h, _ in sizes)
        return img[:, :, : ctx.h_max]          # the slot is h_max rounded up to whole 16-row tiles

    @staticmethod
    @torch.autograd.function.once_differentiable
    @fp32_boundary_bwd
    def backward(ctx, grad_output):
        from . import _cabi
        gs_parameters, steps = ctx.saved_tensors
        # [B,3,Hmax,Wmax] read in place (rows per plane = Hmax <= slot): pixels outside a sample's own grid are never read
        return _cabi.batch_backward(ctx.plan, gs_parameters, steps, grad_output.contiguous(), chw=True), None, None, None, None, None, None


def _batch_step_sizes(scales, scale_modifies, default_step_size, mode, dev):
    """`[B]` float32 device tensor of `_step_size(...)` per sample with ONE stack / division / check for the batch
    (the per-sample form costs a kernel and, through the reference's `assert scale_modify[0] == scale_modify[1]`,
    a host synchronisation per sample)."""
    def col(vals):
        if all(torch.is_tensor(v) for v in vals):
            return torch.stack([v.reshape(()) for v in vals]).to(device=dev, dtype=torch.float32)
        # python numbers: one host-to-device copy per DISTINCT tuple of values, not per call
        return _cached_constant(tuple(float(v) for v in vals), dev)
    if mode == 'scale':
        final = col(list(scales))
    elif mode == 'scale_modify':
        if all(torch.is_tensor(sm) and sm.is_cuda for sm in scale_modifies):
            both = torch.stack([sm.reshape(-1)[:2] for sm in scale_modifies]).to(device=dev, dtype=torch.float32)   # [B,2], one kernel
            a, b = both[:, 0], both[:, 1]
            if not _capturing():      # the reference's assert, without draining the pipeline
                bad = (a != b).to(torch.float32)
                deferred_asserts.add(torch.stack([bad.sum(), bad.new_zeros(())]), "scale_modify is not the same (batched step): differing pairs, 0")
        else:
            a, b = col([sm[0] for sm in scale_modifies]), col([sm[1] for sm in scale_modifies])
            assert bool((a == b).all()), f"scale_modify is not the same-{scale_modifies}"
        final = a
    else:
        raise UnboundLocalError(f"mode-{mode} must be scale or scale_modify")
    return default_step_size / final


def max_canvas_batch(h_max: int) -> int:
    """samples of up to `h_max` rows that fit ONE batched canvas: 64 slots (GSASR_MAX_BATCH) of h_max rounded up to
    whole 16-row tiles, 32 767 canvas rows in all (the plan packs pixel indices in 15 bits)"""
    slot = (int(h_max) + 15) // 16 * 16
    return max(1, min(64, 32767 // slot))


def _batch_sizes(sr_sizes):
    """`sr_sizes` as [(H_b, W_b)] ints; the [B,2] GPU tensor of gsasr_model.py:147 with ONE copy to the host"""
    if torch.is_tensor(sr_sizes) and sr_sizes.dim() == 2:
        return [(int(r[0]), int(r[1])) for r in sr_sizes.tolist()]
    return [_hw(s) for s in sr_sizes]


def _one_canvas(gs_parameters, cap, uniform_dmax) -> bool:
    """does ONE batched canvas of at most `cap` slots apply: 2 or more samples `[B,N,9]` on the GPU, one dmax for all of them"""
    return 1 < gs_parameters.shape[0] <= cap and gs_parameters.is_cuda and gs_parameters.dim() == 3 and gs_parameters.shape[2] == 9 \
        and uniform_dmax


def _batch_sm_source(scale_modifies, dev):
    """the `[B,2]` device tensor of scale_modify pairs the plan's first kernel can read itself, or None.  A [B,2] tensor is read
    in place as rows of stride >= 2 on the Gaussians' device: an `.expand(B, 2)` view -- row stride 0 -- or a tensor on another
    GPU is evaluated instead"""
    if torch.is_tensor(scale_modifies) and scale_modifies.dim() == 2 and _sm_source_ok(scale_modifies[0]) \
            and scale_modifies.stride(0) >= 2 and scale_modifies.device == dev:
        return scale_modifies
    if not torch.is_tensor(scale_modifies) and all(_sm_source_ok(v) and v.device == dev for v in scale_modifies):
        return torch.stack([v[:2] for v in scale_modifies])
    return None


def _canvas_step_args(scales, scale_modifies, default_step_size, mode, dev, source=True):
    """`_fused_step_args` of a canvas, `(steps, scale_modify, default_step, watch)`: scale_modify pairs that are already on the
    device go to the plan's first kernel as they are (one [B,2] tensor: no kernel at all; a list of [2] tensors: one
    torch.stack) -- no division, comparison or copy here --, anything else as the `[B]` tensor of `_batch_step_sizes`.
    `source=False`: the launch takes no `scale_modify` (the sampled and query canvases), the steps are evaluated"""
    sm = _batch_sm_source(scale_modifies, dev) if source and mode == 'scale_modify' else None
    if sm is not None:
        return None, sm, float(default_step_size), True
    return _batch_step_sizes(scales, scale_modifies, default_step_size, mode, dev), None, 1.2, False


def _batch_windows(sizes, gs_parameters, scales, scale_modifies, windows, default_step_size, mode, if_dmax, dmax_mode, dmax,
                   uniform_dmax):
    """`generate_2D_gaussian_splatting_batch(windows=...)`: one canvas whose slots are the windows, each on its own full grid
    (gsasr_view per sample), or the loop over `generate_2D_gaussian_splatting_view` where a canvas does not apply"""
    B = gs_parameters.shape[0]
    if len(windows) != B:
        raise ValueError("one window per sample")
    wins = [_window(windows[b], *sizes[b]) for b in range(B)]
    h_max, w_max = max(w[2] for w in wins), max(w[3] for w in wins)
    if _one_canvas(gs_parameters, max_canvas_batch(h_max), uniform_dmax):
        dev = gs_parameters.device
        dm = _dmax_arg(dmax, dmax_mode, if_dmax, sizes[0])
        wsizes = tuple((w[2], w[3]) for w in wins)
        views = tuple((H, W, w[0], w[1]) for (H, W), w in zip(sizes, wins))
        steps, sm, default_step, watch = _canvas_step_args(scales, scale_modifies, default_step_size, mode, dev)
        out = _FusedBatch.apply(gs_parameters.contiguous(), steps, wsizes, dm, sm, default_step, views)
        if watch:
            deferred_asserts.watch(dev)
        return out
    # per-sample path (a single sample, more samples than a canvas holds, a per-sample dmax, CPU tensors)
    outs = []
    for b in range(B):
        o = generate_2D_gaussian_splatting_view(sizes[b], gs_parameters[b], scales[b], scale_modifies[b], wins[b],
                                                default_step_size=default_step_size, mode=mode, if_dmax=if_dmax, dmax_mode=dmax_mode,
                                                dmax=dmax)
        outs.append(torch.nn.functional.pad(o, (0, w_max - wins[b][3], 0, h_max - wins[b][2])))
    return torch.stack(outs)


def generate_2D_gaussian_splatting_batch(sr_sizes, gs_parameters, scales, scale_modifies, default_step_size=1.2,
                                         mode='scale_modify', if_dmax=True, dmax_mode='fix', dmax=25, sample_coords=None,
                                         query_coords=None, coords_grad=False, windows=None):
    """Batched `generate_2D_gaussian_splatting_step`: `gs_parameters` `[B,N,9]`, per-sample
    `sr_sizes[b]`, `scales[b]`, `scale_modifies[b]`; returns `[B,3,Hmax,Wmax]` with every sample zero-padded to
    the largest size -- exactly `torch.stack([F.pad(step(...), ...)])` of the reference's loop.  With
    `sample_coords` `[B,S,2]` (row, column on each sample's own grid; gsasr_model.py:196-197) it returns the
    `[B,3,S]` stack of the per-sample `[3,S]` results instead.  With `query_coords` float `[B,S,2]` (fractional (r, c) on each
    sample's own grid: `generate_2D_gaussian_splatting_query`) likewise `[B,3,S]`; passing both is a ValueError.
    `coords_grad=True` (with `query_coords` only): differentiable in the positions as well.
    `windows` = [(y0, x0, h, w)] * B: sample b's window of its own `sr_sizes[b]` grid only
    (`generate_2D_gaussian_splatting_view` per sample) -- `[B,3,hmax,wmax]` with hmax, wmax the largest window height and width,
    window b in the top-left corner of its slot and zero elsewhere: one patch shape whatever the scales are, for the losses
    that need neighbouring pixels.  One set of launches and one autograd node on CUDA tensors; `dmax_mode` resolves against
    `sr_sizes`, not the windows; not combinable with `sample_coords` / `query_coords` (ValueError)."""
    B = gs_parameters.shape[0]
    if windows is not None and (sample_coords is not None or query_coords is not None):
        raise ValueError("windows render image patches: not combinable with sample_coords / query_coords")
    if coords_grad and query_coords is None:
        raise ValueError("coords_grad=True has a meaning with query_coords only")
    if query_coords is not None:
        if sample_coords is not None:
            raise ValueError("pass sample_coords (integer pixels) or query_coords (fractional positions), not both")
        query_coords = _as_query(query_coords, batched=True, coords_grad=coords_grad)
        if query_coords.shape[0] != B:
            raise ValueError("query_coords must be [B,S,2]")
    sizes = _batch_sizes(sr_sizes)
    if not (len(sizes) == B == len(scales) == len(scale_modifies)):
        raise ValueError("one sr_size, scale and scale_modify per sample")
    if gs_parameters.dtype != torch.float32:
        gs_parameters = gs_parameters.float()
    uniform_dmax = (not if_dmax) or dmax_mode == 'fix' or len(set(sizes)) == 1
    if windows is not None:
        return _batch_windows(sizes, gs_parameters, scales, scale_modifies, windows, default_step_size, mode, if_dmax,
                              dmax_mode, dmax, uniform_dmax)
    cap = max_canvas_batch(max(h for h, _ in sizes))
    if B > cap >= 2 and gs_parameters.is_cuda and gs_parameters.dim() == 3 and uniform_dmax:
        # more samples than one canvas holds (64 slots, 32 767 rows): several canvases of `cap` samples, the last
        # one possibly a single sample (which takes the per-sample path below)
        parts = [generate_2D_gaussian_splatting_batch(sr_sizes[a: a + cap], gs_parameters[a: a + cap], scales[a: a + cap],
                                                      scale_modifies[a: a + cap], default_step_size, mode, if_dmax, dmax_mode,
                                                      dmax, None if sample_coords is None else sample_coords[a: a + cap],
                                                      None if query_coords is None else query_coords[a: a + cap], coords_grad)
                 for a in range(0, B, cap)]
        if sample_coords is None and query_coords is None:
            h_max, w_max = max(h for h, _ in sizes), max(w for _, w in sizes)
            parts = [F.pad(o, (0, w_max - o.shape[3], 0, h_max - o.shape[2])) for o in parts]
        return torch.cat(parts)
    if _one_canvas(gs_parameters, cap, uniform_dmax):
        dev = gs_parameters.device
        dm = _dmax_arg(dmax, dmax_mode, if_dmax, sizes[0])
        # (only the plain image launch takes the device pairs: the sampled and query canvases evaluate the steps)
        plain = sample_coords is None and query_coords is None
        steps, sm, default_step, watch = _canvas_step_args(scales, scale_modifies, default_step_size, mode, dev, source=plain)
        if plain:
            out = _fused_batch(gs_parameters.contiguous(), steps, tuple(sizes), dm, sm, default_step)
            if watch:
                deferred_asserts.watch(dev)
            return out
        if query_coords is not None and query_coords.shape[1] > 0:
            return _FusedBatchQuery.apply(gs_parameters.contiguous(), steps, tuple(sizes), dm, query_coords)
        pts = None if sample_coords is None else sample_coords if torch.is_tensor(sample_coords) else torch.as_tensor(sample_coords)
        if pts is not None and pts.dim() == 3 and pts.shape[0] == B and pts.shape[2] == 2 and not pts.dtype.is_floating_point \
                and 0 < pts.shape[1] <= SAMPLED_MAX_FRACTION * min(h * w for h, w in sizes):
            return _FusedBatchSampled.apply(gs_parameters.contiguous(), steps, tuple(sizes), dm, pts)
    # per-sample path (single sample, > 64 samples, or a per-sample dmax): same kernels, one sample at a time
    h_max, w_max = max(h for h, _ in sizes), max(w for _, w in sizes)
    outs = []
    for b in range(B):
        if query_coords is not None:
            outs.append(generate_2D_gaussian_splatting_query(sr_sizes[b], gs_parameters[b], scales[b], scale_modifies[b], query_coords[b],
                                                             default_step_size=default_step_size, mode=mode, if_dmax=if_dmax,
                                                             dmax_mode=dmax_mode, dmax=dmax, coords_grad=coords_grad))
            continue
        o = generate_2D_gaussian_splatting_step(sr_sizes[b], gs_parameters[b], scales[b], scale_modifies[b],
                                                sample_coords=None if sample_coords is None else sample_coords[b],
                                                default_step_size=default_step_size, mode=mode, if_dmax=if_dmax,
                                                dmax_mode=dmax_mode, dmax=dmax)
        if sample_coords is None:
            o = torch.nn.functional.pad(o, (0, w_max - sizes[b][1], 0, h_max - sizes[b][0]))
        outs.append(o)
    return torch.stack(outs)


# ---- pixel loss fused into the forward's store (include/gsasr_splat.h: gsasr_loss) ---------------------------------------
# What GSASR does with a rendered batch during training (basicsr/models/gsasr_model.py:191-237): per sample slice output and ground
# truth to gt_size[i], cri_pix(b_output, b_gt) -- L1Loss / MSELoss / CharbonnierLoss of basicsr/losses/basic_loss.py:14-25,
# reduction='mean', times loss_weight --, summed over the samples and divided by b.  The forward kernels do it at the store: no image
# is written or read back, no torch loss kernels run, one autograd node.
from . import ssim as _ssim  # noqa: E402  (the torch expression of the SSIM term and its size rule)


def _loss_names(loss, reduction):
    from . import _cabi
    if loss not in _cabi.LOSS_KINDS:
        raise ValueError(f"loss-{loss} must be one of {sorted(_cabi.LOSS_KINDS)}")
    if reduction not in _cabi.LOSS_NORMS:
        raise ValueError(f"reduction-{reduction} must be mean or sum (weight maps and reduction='none' need the image: return_image=True)")
    return _cabi.LOSS_KINDS[loss], _cabi.LOSS_NORMS[reduction]


def _pixel_loss(image, target, loss, loss_weight, eps, reduction):
    """the torch expression of one sample's pixel loss (basic_loss.py:14-25): what the fused call computes, for CPU tensors"""
    d = image - target
    phi = d.abs() if loss == 'l1' else d * d if loss == 'mse' else torch.sqrt(d * d + eps)
    return loss_weight * (phi.mean() if reduction == 'mean' else phi.sum())


def _ssim_weight(ssim_weight, reduction) -> float:
    ssim_weight = float(ssim_weight)
    if ssim_weight != 0.0 and reduction != 'mean':
        raise ValueError(f"reduction-{reduction}: the SSIM term exists as a mean only (ssim_weight != 0 needs reduction='mean')")
    return ssim_weight


def _loss_returns(value, *extras):
    """the loss, or the tuple of it and whichever extras were asked for (not None)"""
    ret = (value,) + tuple(e for e in extras if e is not None)
    return ret[0] if len(ret) == 1 else ret


def _fused_loss_backward(ctx, g_loss, batched):
    """the existing step backward on the gradient buffer the forward wrote, times the upstream scalar -- one multiply of
    g_parameters by the 0-dim device tensor, never read on the host"""
    from . import _cabi
    gs_parameters, step = ctx.saved_tensors
    if ctx.grad is None:
        raise RuntimeError("the fused loss was computed on a forward-only plan (gs_parameters did not require grad)")
    chw = bool(ctx.plan.dims.flags & _cabi.FLAG_CHW_GRAD)
    g = (_cabi.batch_backward if batched else _cabi.step_backward)(ctx.plan, gs_parameters, step, ctx.grad, chw=chw)
    return g.mul_(g_loss.to(torch.float32))


def _loss_plan_flags(needs_grad: bool, kernel: int) -> int:
    """`_plan_flags` for the fused loss: the forward writes the image gradient in the layout the chosen backward reads --
    planar for the tile-stationary kernel, interleaved for the Gaussian-stationary and home-tile kernels (no k_chw_to_hwc pass)"""
    from . import _cabi
    if not needs_grad:
        return _cabi.FLAG_FORWARD_ONLY
    return int(kernel) | (_cabi.FLAG_CHW_GRAD if kernel == _cabi.FLAG_BWD_TILE else 0)


def _add_ssim(loss, grad, img, plan, target, sizes, ssim_weight):
    """the SSIM term behind a fused pixel loss that stored its image: gsasr_ssim_loss on `img` against the same `target`, its
    gradient ADDED to the one the forward wrote (in the layout the plan's backward reads) -- or, on a forward-only plan, the
    value alone.  Returns (total, per-sample totals, l_pix, l_ssim)."""
    from . import _cabi
    hwc = not (plan.dims.flags & _cabi.FLAG_CHW_GRAD)
    sl, _ = _cabi.ssim_loss(img, target, sizes, ssim_weight, want_grad=False, grad=grad, hwc=hwc and grad is not None,
                            accumulate=grad is not None)
    return loss[0] + sl[0], loss[1:] + sl[1:], loss[0], sl[0]


def _loss_outputs(ctx, loss, grad, img, plan, target, sizes, ssim_weight, want_image):
    """the outputs of the two loss Functions, always `(total, per-sample totals, l_pix, l_ssim, img)`: the two terms are None
    without the SSIM term and `img` is None unless `want_image`; all but the total are non-differentiable"""
    if ssim_weight != 0.0:
        total, per, l_pix, l_ssim = _add_ssim(loss, grad, img, plan, target, sizes, ssim_weight)
    else:
        total, per, l_pix, l_ssim = loss[0], loss[1:], None, None
    if not want_image:
        img = None
    elif sizes is not None:
        img = img[:, :, : max(h for h, _ in sizes)]          # the slot is h_max rounded up to whole 16-row tiles
    ctx.mark_non_differentiable(*(t for t in (per, l_pix, l_ssim, img) if t is not None))
    return total, per, l_pix, l_ssim, img


class _FusedStepLoss(torch.autograd.Function):
    """`_FusedStep` ending in the fused pixel loss: raw `gs_parameters[N,9]` and `target[3,h,w]` -> `_loss_outputs` (`[1]`
    per-sample loss), the image gradient kept in `ctx` for the existing backward."""

    @staticmethod
    @fp32_boundary_fwd
    def forward(ctx, gs_parameters, step, target, H, W, dmax, scale_modify, default_step, extra_flags, window, kind, norm, weight, eps,
                want_image, needs_grad, ssim_weight):
        from . import _cabi
        # (needs_grad: requires_grad AND grad mode, from the caller -- a Function's forward always runs with grad mode off)
        h, w, view = (H, W, None) if window is None else (window[2], window[3], (H, W, window[0], window[1]))
        flags = _loss_plan_flags(needs_grad, _step_kernel(gs_parameters.shape[0], H, W, dmax, window)) | int(extra_flags)
        loss, grad, img, plan = _cabi.step_forward_loss(gs_parameters, step, h, w, dmax, target, kind, norm, weight, eps, flags,
                                                        scale_modify, default_step, view, want_image or ssim_weight != 0.0)
        ctx.save_for_backward(gs_parameters, step)
        ctx.plan, ctx.grad = plan, grad
        return _loss_outputs(ctx, loss, grad, img, plan, target, None, ssim_weight, want_image)

    @staticmethod
    @torch.autograd.function.once_differentiable
    @fp32_boundary_bwd
    def backward(ctx, g_loss, *_):
        return (_fused_loss_backward(ctx, g_loss, False),) + (None,) * 16


class _FusedBatchLoss(torch.autograd.Function):
    """`_FusedBatch` ending in the fused pixel loss: `gs_parameters[B,N,9]` and `target[B,3,rows,w_max]` (read in place) ->
    `_loss_outputs` (`[B]` per-sample losses, with `want_image` the images `[B,3,h_max,w_max]`)."""

    @staticmethod
    @fp32_boundary_fwd
    def forward(ctx, gs_parameters, steps, target, sizes, dmax, scale_modify, default_step, views, kind, norm, weight, eps, want_image,
                needs_grad, ssim_weight):
        from . import _cabi
        flags = _loss_plan_flags(needs_grad, _canvas_kernel(gs_parameters.shape[1], gs_parameters.shape[0], sizes, dmax, views))
        loss, grad, img, plan = _cabi.batch_forward_loss(gs_parameters, steps, sizes, dmax, target, kind, norm, weight, eps, flags,
                                                         scale_modify, default_step, views, want_image or ssim_weight != 0.0)
        ctx.save_for_backward(gs_parameters, steps)
        ctx.plan, ctx.grad = plan, grad
        return _loss_outputs(ctx, loss, grad, img, plan, target, sizes, ssim_weight, want_image)

    @staticmethod
    @torch.autograd.function.once_differentiable
    @fp32_boundary_bwd
    def backward(ctx, g_loss, *_):
        return (_fused_loss_backward(ctx, g_loss, True),) + (None,) * 14


def _loss_target_tensor(target, shape, dev, what="target"):
    """`target` as a contiguous fp32 tensor on `dev` (half / bf16 targets are cast once, here); `shape`: what it must be, with
    None for a free extent"""
    if not torch.is_tensor(target) or not target.dtype.is_floating_point:
        raise ValueError(f"{what} must be a floating-point tensor")
    if target.dim() != len(shape) or any(s is not None and int(t) != s for t, s in zip(target.shape, shape)):
        raise ValueError(f"{what} has shape {tuple(target.shape)}, expected {['*' if s is None else s for s in shape]}")
    return target.detach().to(device=dev, dtype=torch.float32).contiguous()


def generate_2D_gaussian_splatting_loss(sr_size, gs_parameters, scale, scale_modify, target, loss='l1', loss_weight=1.0, eps=1e-12,
                                        reduction='mean', window=None, return_image=False, default_step_size=1.2,
                                        mode='scale_modify', if_dmax=True, dmax_mode='fix', dmax=25, sample_coords=None,
                                        query_coords=None, ssim_weight=0.0, return_terms=False):
    """`loss_weight * cri_pix(generate_2D_gaussian_splatting_step(...), target)` for `loss` in 'l1' | 'mse' | 'charbonnier'
    (basicsr/losses/basic_loss.py:14-25; `reduction` 'mean' | 'sum') as ONE differentiable call that never materialises the
    image: the forward kernels load `target[3,H,W]` at the store, write d loss / d image for the backward and reduce the loss
    (gsasr_step_forward_loss).  Returns the 0-dim loss, or `(loss, image)` with `return_image=True` (the image is not
    differentiable: perceptual terms that need gradients through it take the plain call).  `ssim_weight` != 0 adds GSASR's other
    training term, `ssim_weight * (1 - ssim(image, target))` (`cri_ssim`, basic_loss.py:256-264; 'mean' only): the forward stores
    the image, gsasr_ssim_loss adds its gradient to the one the forward wrote, and the whole `l_pix + l_ssim` is still one autograd
    node with one backward.  `return_terms` appends the pair `(l_pix, l_ssim)` of detached 0-dim tensors.  `window` =
    (y0, x0, h, w): the loss over that window of the grid only, `target[3,h,w]` (`generate_2D_gaussian_splatting_view`).
    Under `torch.no_grad()` the plan is forward-only (a validation loss).  CPU tensors: the torch expression on
    `rendering_python`'s image.  `sample_coords` / `query_coords` are not covered (ValueError)."""
    kind, norm = _loss_names(loss, reduction)
    if sample_coords is not None or query_coords is not None:
        raise ValueError("the fused pixel loss covers whole images and windows, not sample_coords / query_coords")
    if not (float(eps) >= 0.0):
        raise ValueError(f"eps-{eps} must be >= 0")
    ssim_weight = _ssim_weight(ssim_weight, reduction)
    if gs_parameters.dtype != torch.float32:
        gs_parameters = gs_parameters.float()
    H, W = _hw(sr_size)
    win = None if window is None else _window(window, H, W)
    h, w = (H, W) if win is None else (win[2], win[3])
    if ssim_weight != 0.0:
        _ssim.check_sizes([(h, w)], "sample or window")
    target = _loss_target_tensor(target, (3, h, w), gs_parameters.device)
    if not gs_parameters.is_cuda:
        step_size = _step_size(scale, scale_modify, default_step_size, mode)
        image = rendering_python(*_activate(gs_parameters), sr_size, step_size, device=gs_parameters.device)
        if win is not None:
            image = image[:, win[0]:win[0] + h, win[1]:win[1] + w]
        value = l_pix = _pixel_loss(image, target, loss, loss_weight, eps, reduction)
        l_ssim = torch.zeros((), dtype=value.dtype)
        if ssim_weight != 0.0:
            l_ssim = _ssim.ssim_torch(image, target, ssim_weight)
            value = l_pix + l_ssim
        return _loss_returns(value, image.detach() if return_image else None, (l_pix.detach(), l_ssim.detach()) if return_terms else None)
    if not _fused_ok(gs_parameters):
        raise RuntimeError("generate_2D_gaussian_splatting_loss needs gs_parameters [N,9] on the GPU (no fallback)")
    step_size = _step_size(scale, scale_modify, default_step_size, mode, fused=True)
    dm = _dmax_arg(dmax, dmax_mode, if_dmax, (H, W))
    gp = gs_parameters.contiguous()
    step, sm, default_step, watch = _fused_step_args(step_size, gp.device)
    total, _, l_pix, l_ssim, image = _FusedStepLoss.apply(
        gp, step, target, H, W, dm, sm, default_step, _forward_flag(scale, h, w), win, kind, norm, float(loss_weight), float(eps),
        bool(return_image), gp.requires_grad and torch.is_grad_enabled(), ssim_weight)
    if watch:
        deferred_asserts.watch(gp.device)
    if return_terms and ssim_weight == 0.0:
        l_pix, l_ssim = total.detach(), torch.zeros_like(total)
    return _loss_returns(total, image, (l_pix, l_ssim) if return_terms else None)


def generate_2D_gaussian_splatting_batch_loss(sr_sizes, gs_parameters, scales, scale_modifies, targets, loss='l1', loss_weight=1.0,
                                              eps=1e-12, reduction='mean', default_step_size=1.2, mode='scale_modify', if_dmax=True,
                                              dmax_mode='fix', dmax=25, windows=None, return_per_sample=False, return_images=False,
                                              sample_coords=None, query_coords=None, ssim_weight=0.0, return_terms=False):
    """The pixel loss of a training batch (the loop of basicsr/models/gsasr_model.py:191-237) as ONE differentiable call:
    sample b of `generate_2D_gaussian_splatting_batch(...)` against `targets[b][:, :h_b, :w_b]` with `cri_pix` = `loss`
    ('l1' | 'mse' | 'charbonnier', `reduction` 'mean' | 'sum', times `loss_weight`), summed over the samples and -- 'mean' --
    divided by B.  `targets`: `[B,3,rows,Wmax]` with any `rows` >= the tallest sample (the padded `self.gt`: read in place), or
    a list of `[3,h_b,w_b]` (stacked once); with `windows` the patches `[B,3,hmax,wmax]`.  Returns the 0-dim loss; with
    `return_per_sample` / `return_images` a tuple (loss, `[B]` per-sample losses L_b, `[B,3,Hmax,Wmax]` images) of what was asked
    for -- both non-differentiable.  On CUDA tensors the image is never written unless asked for, and there is one autograd node;
    where the batch function takes its per-sample path the same value is computed sample by sample.  `ssim_weight` != 0 adds
    `ssim_weight * (1 - ssim)` of every sample (`cri_ssim`; reduction 'mean' only) inside the same node -- the loop's
    `l_total = l_pix + l_ssim` --, the per-sample losses are then the totals, and `return_terms` appends the pair
    `(l_pix, l_ssim)` of detached 0-dim tensors (the reference's `loss_dict`)."""
    kind, norm = _loss_names(loss, reduction)
    if sample_coords is not None or query_coords is not None:
        raise ValueError("the fused pixel loss covers whole images and windows, not sample_coords / query_coords")
    if not (float(eps) >= 0.0):
        raise ValueError(f"eps-{eps} must be >= 0")
    ssim_weight = _ssim_weight(ssim_weight, reduction)
    B = gs_parameters.shape[0]
    sizes = _batch_sizes(sr_sizes)
    if not (len(sizes) == B == len(scales) == len(scale_modifies)):
        raise ValueError("one sr_size, scale and scale_modify per sample")
    if windows is not None and len(windows) != B:
        raise ValueError("one window per sample")
    if gs_parameters.dtype != torch.float32:
        gs_parameters = gs_parameters.float()
    wins = None if windows is None else [_window(windows[b], *sizes[b]) for b in range(B)]
    wsizes = tuple(sizes) if wins is None else tuple((w[2], w[3]) for w in wins)
    h_max, w_max = max(h for h, _ in wsizes), max(w for _, w in wsizes)
    if ssim_weight != 0.0:
        _ssim.check_sizes(wsizes, "sample or window")
    dev = gs_parameters.device
    if torch.is_tensor(targets):
        targets = _loss_target_tensor(targets, (B, 3, None, w_max), dev, "targets")
        if targets.shape[2] < h_max:
            raise ValueError(f"targets has {targets.shape[2]} rows, the tallest sample {h_max}")
    else:
        if len(targets) != B:
            raise ValueError("one target per sample")
        parts = [_loss_target_tensor(t, (3,) + wsizes[b], dev, f"targets[{b}]") for b, t in enumerate(targets)]
        targets = torch.stack([F.pad(t, (0, w_max - t.shape[2], 0, h_max - t.shape[1])) for t in parts])
    uniform_dmax = (not if_dmax) or dmax_mode == 'fix' or len(set(sizes)) == 1
    cap = max_canvas_batch(h_max)
    if _one_canvas(gs_parameters, cap, uniform_dmax):
        dm = _dmax_arg(dmax, dmax_mode, if_dmax, sizes[0])
        views = None if wins is None else tuple((H, W, w[0], w[1]) for (H, W), w in zip(sizes, wins))
        gp = gs_parameters.contiguous()
        steps, sm, default_step, watch = _canvas_step_args(scales, scale_modifies, default_step_size, mode, dev)
        total, per, l_pix, l_ssim, images = _FusedBatchLoss.apply(
            gp, steps, targets, wsizes, dm, sm, default_step, views, kind, norm, float(loss_weight), float(eps), bool(return_images),
            gp.requires_grad and torch.is_grad_enabled(), ssim_weight)
        if watch:
            deferred_asserts.watch(dev)
        if return_terms and ssim_weight == 0.0:
            l_pix, l_ssim = total.detach(), torch.zeros_like(total)
        terms = (l_pix, l_ssim)
    else:
        # per-sample path (a single sample, more samples than a canvas holds, a per-sample dmax, CPU tensors): the same value
        vals, imgs, pix, ssm = [], [], [], []
        for b in range(B):
            hb, wb = wsizes[b]
            o = generate_2D_gaussian_splatting_loss(sizes[b], gs_parameters[b], scales[b], scale_modifies[b], targets[b, :, :hb, :wb],
                                                    loss, loss_weight, eps, reduction, None if wins is None else wins[b], return_images,
                                                    default_step_size, mode, if_dmax, dmax_mode, dmax, ssim_weight=ssim_weight,
                                                    return_terms=True)
            if return_images:
                imgs.append(F.pad(o[1], (0, w_max - wb, 0, h_max - hb)))
            vals.append(o[0])
            pix.append(o[-1][0])
            ssm.append(o[-1][1])
        stacked = torch.stack(vals)
        div = B if reduction == 'mean' else 1
        total = stacked.sum() / div
        per, images = stacked.detach(), (torch.stack(imgs) if return_images else None)
        terms = (torch.stack(pix).sum() / div, torch.stack(ssm).sum() / div)
    return _loss_returns(total, per if return_per_sample else None, images if return_images else None, terms if return_terms else None)


def generate_2D_gaussian_splatting_step_buffer(sr_size, gs_parameters, scale, scale_modify, sample_coords=None,
                                               default_step_size=1.2, cuda_rendering=True, mode='scale_modify',
                                               if_dmax=True, dmax_mode='fix', dmax=25, buffer_size=4000000):
    step_size = _step_size(scale, scale_modify, default_step_size, mode)
    if gs_parameters.dtype != torch.float32:
        gs_parameters = gs_parameters.float()
    sigma_x, sigma_y, rho, coords, colours_with_alpha = _activate(gs_parameters)
    dev = sigma_x.device
    if cuda_rendering:
        if if_dmax:
            dmax = _resolve_dmax(dmax, dmax_mode, sr_size)
            final_image = rendering_cuda_dmax_buffer(sigma_x, sigma_y, rho, coords, colours_with_alpha, sr_size,
                                                     step_size, dmax=dmax, device=dev, buffer_size=buffer_size)
        else:
            final_image = rendering_cuda_buffer(sigma_x, sigma_y, rho, coords, colours_with_alpha, sr_size,
                                                step_size, device=dev, buffer_size=buffer_size)
    else:
        final_image = rendering_python(sigma_x, sigma_y, rho, coords, colours_with_alpha, sr_size, step_size,
                                       device=dev)
    return _sample(final_image, sample_coords)
