"""ctypes binding of libgsasr_splat.so (include/gsasr_splat.h) for torch tensors.

PyTorch is plumbing here: it owns device memory and the stream; every call below passes raw
`data_ptr()`s, sizes and `torch.cuda.current_stream().cuda_stream` through the C ABI.  There is NO
fallback: if the library is missing or a tensor is not a contiguous fp32 CUDA tensor this raises.
"""
from __future__ import annotations

import ctypes
import os
import threading
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np
import torch

_PKG = os.path.dirname(os.path.abspath(__file__))
# (GSASR_SPLAT_LIB: development override, e.g. to A/B two builds of the library on the same GPU box)
LIB_PATH = os.environ.get("GSASR_SPLAT_LIB") or os.path.join(_PKG, "lib", "libgsasr_splat.so")

FLAG_OVERWRITE_IMAGE = 2   # GSASR_FLAG_OVERWRITE_IMAGE
FLAG_OVERWRITE_GRADS = 4   # GSASR_FLAG_OVERWRITE_GRADS
FLAG_CHW_IMAGE = 8         # GSASR_FLAG_CHW_IMAGE
FLAG_STRIDE8 = 16          # GSASR_FLAG_STRIDE8
FLAG_CHW_GRAD = 32         # GSASR_FLAG_CHW_GRAD
FLAG_FORWARD_ONLY = 64     # GSASR_FLAG_FORWARD_ONLY
FLAG_BWD_GAUSSIAN = 128    # GSASR_FLAG_BWD_GAUSSIAN
FLAG_BWD_TILE = 256        # GSASR_FLAG_BWD_TILE
FLAG_BWD_ATOMIC = 512      # GSASR_FLAG_BWD_ATOMIC
FLAG_BWD_HOME = 32768      # GSASR_FLAG_BWD_HOME (home-tile backward, ABI 7)
FLAG_COUNTERS_CLEAN = 1024 # GSASR_FLAG_COUNTERS_CLEAN
FLAG_PARITY = 2048         # GSASR_FLAG_PARITY
FLAG_CUTOFF_CAP = 4096     # GSASR_FLAG_CUTOFF_CAP
FLAG_FWD_WIDE, FLAG_FWD_NARROW = 8192, 16384      # forward kernel choice (development A/B, tests): 16x16 / 8x16 sub-tiles
FLAG_CONTINUOUS = 65536    # GSASR_FLAG_CONTINUOUS: a plan for queries between the pixel centres (query_forward / query_backward[_points])
U8_SWAP_RB = 1             # GSASR_U8_SWAP_RB (u8_flags of the 8-bit forwards)
EXACT_CUTOFF = 104.0    # GSASR_SPLAT_EXACT_CUTOFF
NO_CUTOFF = -1.0


class Dims(ctypes.Structure):
    """struct gsasr_dims"""
    _fields_ = [("s", ctypes.c_int), ("h", ctypes.c_int), ("w", ctypes.c_int), ("c", ctypes.c_int),
                ("dmax", ctypes.c_float), ("row0", ctypes.c_int), ("row1", ctypes.c_int),
                ("cutoff", ctypes.c_float), ("flags", ctypes.c_uint),
                ("batch", ctypes.c_int), ("slot", ctypes.c_int), ("sample_hw", ctypes.POINTER(ctypes.c_int)),
                ("grad_rows", ctypes.c_int), ("list_cap", ctypes.c_int)]


class View(ctypes.Structure):
    """struct gsasr_view: the grid a window is cut from and the window's first row / column on it"""
    _fields_ = [("full_h", ctypes.c_int), ("full_w", ctypes.c_int), ("y0", ctypes.c_int), ("x0", ctypes.c_int)]


class Loss(ctypes.Structure):
    """struct gsasr_loss: the fused pixel loss of gsasr_splat_forward_loss / gsasr_step_forward_loss"""
    _fields_ = [("kind", ctypes.c_int), ("normalisation", ctypes.c_int), ("weight", ctypes.c_float), ("eps", ctypes.c_float),
                ("target", ctypes.c_void_p), ("target_rows", ctypes.c_int), ("grad_img", ctypes.c_void_p),
                ("loss", ctypes.c_void_p), ("img", ctypes.c_void_p), ("scratch", ctypes.c_void_p)]


class Ssim(ctypes.Structure):
    """struct gsasr_ssim: the SSIM loss of a stored image (gsasr_ssim_loss)"""
    _fields_ = [("batch", ctypes.c_int), ("rows", ctypes.c_int), ("w", ctypes.c_int), ("target_rows", ctypes.c_int),
                ("grad_rows", ctypes.c_int), ("sample_hw", ctypes.POINTER(ctypes.c_int)), ("weight", ctypes.c_float),
                ("flags", ctypes.c_uint), ("img", ctypes.c_void_p), ("target", ctypes.c_void_p), ("grad_img", ctypes.c_void_p),
                ("loss", ctypes.c_void_p), ("scratch", ctypes.c_void_p)]


class Metrics(ctypes.Structure):
    """struct gsasr_metrics: PSNR and SSIM of an 8-bit picture against its ground truth (gsasr_image_metrics)"""
    _fields_ = [("batch", ctypes.c_int), ("h", ctypes.c_int), ("w", ctypes.c_int), ("sample_hw", ctypes.POINTER(ctypes.c_int)),
                ("img", ctypes.c_void_p), ("img_pitch", ctypes.c_size_t), ("img_stride", ctypes.c_size_t),
                ("ref", ctypes.c_void_p), ("ref_pitch", ctypes.c_size_t), ("ref_stride", ctypes.c_size_t),
                ("crop_border", ctypes.c_int), ("flags", ctypes.c_uint), ("out", ctypes.c_void_p), ("scratch", ctypes.c_void_p)]


class Resize(ctypes.Structure):
    """struct gsasr_resize: MATLAB-compatible bicubic imresize of planar fp32 images and its adjoint (gsasr_imresize[_backward])"""
    _fields_ = [("batch", ctypes.c_int), ("channels", ctypes.c_int), ("in_h", ctypes.c_int), ("in_w", ctypes.c_int),
                ("sample_hw", ctypes.POINTER(ctypes.c_int)), ("scales", ctypes.POINTER(ctypes.c_double)),
                ("out_h", ctypes.c_int), ("out_w", ctypes.c_int),
                ("inp", ctypes.c_void_p), ("in_pitch", ctypes.c_size_t), ("in_plane", ctypes.c_size_t), ("in_stride", ctypes.c_size_t),
                ("out", ctypes.c_void_p), ("out_pitch", ctypes.c_size_t), ("out_plane", ctypes.c_size_t), ("out_stride", ctypes.c_size_t),
                ("flags", ctypes.c_uint), ("scratch", ctypes.c_void_p)]


class Batch(ctypes.Structure):
    """struct gsasr_batch: training batches from decoded 8-bit images (gsasr_batch_make / gsasr_batch_pick)"""
    _fields_ = [("batch", ctypes.c_int), ("src", ctypes.POINTER(ctypes.c_void_p)), ("src_hw", ctypes.POINTER(ctypes.c_int)),
                ("window", ctypes.POINTER(ctypes.c_int)), ("aug", ctypes.POINTER(ctypes.c_ubyte)),
                ("gt_h", ctypes.c_int), ("gt_w", ctypes.c_int), ("gt", ctypes.c_void_p),
                ("lr_h", ctypes.c_int), ("lr_w", ctypes.c_int), ("lq", ctypes.c_void_p),
                ("flags", ctypes.c_uint), ("scratch", ctypes.c_void_p)]


class WindowAttn(ctypes.Structure):
    """struct gsasr_window_attn: the decoder's window attention with its relative-position bias (gsasr_window_attn_forward / _backward)"""
    _fields_ = [("windows", ctypes.c_int), ("heads", ctypes.c_int), ("nq", ctypes.c_int), ("nk", ctypes.c_int),
                ("head_dim", ctypes.c_int), ("table_rows", ctypes.c_int), ("scale", ctypes.c_float), ("flags", ctypes.c_uint),
                ("q", ctypes.c_void_p), ("k", ctypes.c_void_p), ("v", ctypes.c_void_p), ("table", ctypes.c_void_p),
                ("index", ctypes.c_void_p), ("out", ctypes.c_void_p), ("stats", ctypes.c_void_p), ("grad_out", ctypes.c_void_p),
                ("g_q", ctypes.c_void_p), ("g_k", ctypes.c_void_p), ("g_v", ctypes.c_void_p), ("g_table", ctypes.c_void_p),
                ("scratch", ctypes.c_void_p)]


class WindowAttnRope(ctypes.Structure):
    """struct gsasr_window_attn_rope: the decoder's window attention with a 2-D rotary embedding (gsasr_window_attn_rope_forward / _backward)"""
    _fields_ = [("windows", ctypes.c_int), ("heads", ctypes.c_int), ("nq", ctypes.c_int), ("nk", ctypes.c_int),
                ("head_dim", ctypes.c_int), ("angle_rows", ctypes.c_int), ("scale", ctypes.c_float), ("flags", ctypes.c_uint),
                ("q", ctypes.c_void_p), ("k", ctypes.c_void_p), ("v", ctypes.c_void_p), ("angles", ctypes.c_void_p),
                ("out", ctypes.c_void_p), ("stats", ctypes.c_void_p), ("grad_out", ctypes.c_void_p),
                ("g_q", ctypes.c_void_p), ("g_k", ctypes.c_void_p), ("g_v", ctypes.c_void_p), ("g_angles", ctypes.c_void_p),
                ("cossin", ctypes.c_void_p), ("scratch", ctypes.c_void_p)]


class WindowAttnBf16(ctypes.Structure):
    """struct gsasr_window_attn_bf16: gsasr_window_attn with bf16 activations (same fields, same layout)"""
    _fields_ = list(WindowAttn._fields_)


class WindowAttnRopeBf16(ctypes.Structure):
    """struct gsasr_window_attn_rope_bf16: gsasr_window_attn_rope with bf16 activations (same fields, same layout)"""
    _fields_ = list(WindowAttnRope._fields_)


class WindowAttnMasked(ctypes.Structure):
    """struct gsasr_window_attn_masked: gsasr_window_attn with a mask per window and row pitches for q, k, v and their gradients"""
    _fields_ = list(WindowAttn._fields_) + [("mask", ctypes.c_void_p), ("mask_windows", ctypes.c_int)] + \
        [(p, ctypes.c_int) for p in ("pitch_q", "pitch_k", "pitch_v", "pitch_gq", "pitch_gk", "pitch_gv")]


class WindowAttnMaskedBf16(ctypes.Structure):
    """struct gsasr_window_attn_masked_bf16: gsasr_window_attn_masked with bf16 activations (same fields, same layout)"""
    _fields_ = list(WindowAttnMasked._fields_)


RESIZE_NO_ANTIALIAS, RESIZE_ACCUMULATE, RESIZE_SHARED_SCALE = 1, 2, 4     # GSASR_RESIZE_*
BATCH_HFLIP, BATCH_VFLIP, BATCH_TRANSPOSE = 1, 2, 4     # GSASR_BATCH_* (aug bits)
BATCH_BGR, BATCH_NO_ANTIALIAS = 1, 2                    # GSASR_BATCH_* (flags)
SSIM_GRAD_HWC, SSIM_ACCUMULATE = 1, 2                   # GSASR_SSIM_GRAD_HWC / _ACCUMULATE
METRIC_PSNR, METRIC_SSIM, METRIC_Y, METRIC_BGR = 1, 2, 4, 8     # GSASR_METRIC_*
LOSS_KINDS = {"l1": 0, "mse": 1, "charbonnier": 2}      # GSASR_LOSS_L1 / _MSE / _CHARBONNIER
LOSS_NORMS = {"mean": 0, "sum": 1}                      # GSASR_LOSS_MEAN / _SUM

_vp, _f, _i, _u, _sz, _dp = ctypes.c_void_p, ctypes.c_float, ctypes.c_int, ctypes.c_uint, ctypes.c_size_t, ctypes.POINTER(Dims)
_vwp, _lp, _ssp, _mp = ctypes.POINTER(View), ctypes.POINTER(Loss), ctypes.POINTER(Ssim), ctypes.POINTER(Metrics)
_rzp, _btp, _wap = ctypes.POINTER(Resize), ctypes.POINTER(Batch), ctypes.POINTER(WindowAttn)
_wrp, _wabp, _wrbp = ctypes.POINTER(WindowAttnRope), ctypes.POINTER(WindowAttnBf16), ctypes.POINTER(WindowAttnRopeBf16)
_wmp, _wmbp = ctypes.POINTER(WindowAttnMasked), ctypes.POINTER(WindowAttnMaskedBf16)
_step_tail, _sample_tail, _u8_tail = [_dp, _vp, _sz, _vp, _vp], [_dp, _vp, _sz, _vp, _i, _vp, _vp, _sz, _vp], [_dp, _vp, _sz, _vp, _i, _i, _sz, _u, _vp]
_SIGNATURES = {     # every symbol include/gsasr_splat.h declares: name -> (restype, argtypes)
    "gsasr_abi_version": (_i, []),
    "gsasr_last_error": (ctypes.c_char_p, []),
    "gsasr_splat_workspace_bytes": (_sz, [_dp]),
    "gsasr_splat_counter_bytes": (_sz, [_dp]),
    "gsasr_splat_plan": (_i, [_vp, _vp, _vp, _dp, _vp, _sz, _vp]),
    "gsasr_splat_forward": (_i, [_dp, _vp, _sz, _vp, _vp]),
    "gsasr_splat_forward_u8": (_i, _u8_tail),
    "gsasr_splat_backward": (_i, [_vp] * 7 + [_dp, _vp, _sz, _vp]),
    "gsasr_gs_render": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "gsasr_gs_render_backward": (_i, [_vp] * 7 + [_i, _i, _i, _i, _vp]),
    "gsasr_gs_render_dmax": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _f, _vp]),
    "gsasr_gs_render_backward_dmax": (_i, [_vp] * 7 + [_i, _i, _i, _i, _f, _vp]),
    "gsasr_release_launcher_scratch": (_i, []),
    "gsasr_prologue_forward": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp]),
    "gsasr_prologue_backward": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp]),
    "gsasr_step_workspace_bytes": (_sz, [_dp]),
    "gsasr_step_forward": (_i, [_vp, _vp] + _step_tail),
    "gsasr_step_forward_sm": (_i, [_vp, _vp, _i, _f, _vp] + _step_tail),
    "gsasr_step_forward_u8": (_i, [_vp, _vp] + _u8_tail),
    "gsasr_step_forward_sm_u8": (_i, [_vp, _vp, _i, _f, _vp] + _u8_tail),
    "gsasr_step_backward": (_i, [_vp, _vp, _vp, _vp, _dp, _vp, _sz, _vp]),
    "gsasr_band_select": (_i, [_vp, _dp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "gsasr_band_merge": (_i, [_vp, _i, _vp, _vp, _vp, _vp, _vp, _i, _vp]),
    "gsasr_sample_workspace_bytes": (_sz, [_dp, _i]),
    "gsasr_splat_sample_forward": (_i, _sample_tail),
    "gsasr_splat_sample_backward": (_i, [_vp] * 7 + [_dp, _vp, _sz, _vp, _i, _vp, _sz, _vp]),
    "gsasr_step_sample_forward": (_i, [_vp, _vp] + _sample_tail),
    "gsasr_step_sample_forward_sm": (_i, [_vp, _vp, _i, _f, _vp] + _sample_tail),
    "gsasr_step_sample_backward": (_i, [_vp, _vp, _vp, _vp, _dp, _vp, _sz, _vp, _i, _vp, _sz, _vp]),
    "gsasr_splat_query_forward": (_i, _sample_tail),
    "gsasr_splat_query_backward": (_i, [_vp] * 7 + [_dp, _vp, _sz, _vp, _i, _vp, _sz, _vp]),
    "gsasr_step_query_forward": (_i, [_vp, _vp] + _sample_tail),
    "gsasr_step_query_forward_sm": (_i, [_vp, _vp, _i, _f, _vp] + _sample_tail),
    "gsasr_step_query_backward": (_i, [_vp, _vp, _vp, _vp, _dp, _vp, _sz, _vp, _i, _vp, _sz, _vp]),
    "gsasr_splat_query_backward_points": (_i, [_dp, _vp, _sz, _vp, _vp, _i, _vp, _vp, _sz, _vp]),
    "gsasr_step_query_backward_points": (_i, [_dp, _vp, _sz, _vp, _vp, _i, _vp, _vp, _sz, _vp]),
    "gsasr_set_default_cutoff": (None, [_f]),
    "gsasr_get_default_cutoff": (_f, []),
    "gsasr_resolve_cutoff": (_f, [_f, _i]),
    "gsasr_forward_subtile_width": (_i, [_dp]),
    "gsasr_plan_cutoff": (_i, [_dp, _vp, _sz, _vp, ctypes.POINTER(_f), ctypes.POINTER(_u)]),
    "gsasr_set_kernel_choice": (_i, [_dp, _u, _i]),
    "gsasr_get_kernel_choice": (_i, [_dp, ctypes.POINTER(_u), ctypes.POINTER(_i)]),
    "gsasr_clear_kernel_choices": (None, []),
    # a window of the grid (gsasr_view): the view follows the dims in every argument list
    "gsasr_splat_workspace_bytes_view": (_sz, [_dp, _vwp]),
    "gsasr_step_workspace_bytes_view": (_sz, [_dp, _vwp]),
    "gsasr_splat_plan_view": (_i, [_vp, _vp, _vp, _dp, _vwp, _vp, _sz, _vp]),
    "gsasr_splat_forward_view": (_i, [_dp, _vwp, _vp, _sz, _vp, _vp]),
    "gsasr_splat_forward_u8_view": (_i, [_dp, _vwp] + _u8_tail[1:]),
    "gsasr_splat_backward_view": (_i, [_vp] * 7 + [_dp, _vwp, _vp, _sz, _vp]),
    "gsasr_step_forward_view": (_i, [_vp, _vp, _dp, _vwp] + _step_tail[1:]),
    "gsasr_step_forward_sm_view": (_i, [_vp, _vp, _i, _f, _vp, _dp, _vwp] + _step_tail[1:]),
    "gsasr_step_forward_u8_view": (_i, [_vp, _vp, _dp, _vwp] + _u8_tail[1:]),
    "gsasr_step_forward_sm_u8_view": (_i, [_vp, _vp, _i, _f, _vp, _dp, _vwp] + _u8_tail[1:]),
    "gsasr_step_backward_view": (_i, [_vp, _vp, _vp, _vp, _dp, _vwp, _vp, _sz, _vp]),
    # the pixel loss fused into the forward's store (gsasr_loss); the view is nullable
    "gsasr_loss_scratch_bytes": (_sz, [_dp]),
    "gsasr_splat_forward_loss": (_i, [_dp, _vwp, _vp, _sz, _lp, _vp]),
    "gsasr_step_forward_loss": (_i, [_vp, _vp, _vp, _i, _f, _vp, _dp, _vwp, _vp, _sz, _lp, _vp]),
    # the SSIM loss of a stored image (gsasr_ssim)
    "gsasr_ssim_scratch_bytes": (_sz, [_ssp]),
    "gsasr_ssim_loss": (_i, [_ssp, _vp]),
    # PSNR / SSIM of an 8-bit picture (gsasr_metrics)
    "gsasr_metrics_scratch_bytes": (_sz, [_mp]),
    "gsasr_image_metrics": (_i, [_mp, _vp]),
    # bicubic imresize of planar fp32 images and its adjoint (gsasr_resize)
    "gsasr_resize_scratch_bytes": (_sz, [_rzp]),
    "gsasr_imresize": (_i, [_rzp, _vp]),
    "gsasr_imresize_backward": (_i, [_rzp, _vp]),
    # training batches from decoded 8-bit images (gsasr_batch)
    "gsasr_batch_scratch_bytes": (_sz, [_btp]),
    "gsasr_batch_make": (_i, [_btp, _vp]),
    "gsasr_batch_pick": (_i, [_btp, _vp, _i, _vp, _vp]),
    # the decoder's window attention (gsasr_window_attn)
    "gsasr_window_attn_scratch_bytes": (_sz, [_wap]),
    "gsasr_window_attn_forward": (_i, [_wap, _vp]),
    "gsasr_window_attn_backward": (_i, [_wap, _vp]),
    # ... with a rotary embedding instead of the bias (gsasr_window_attn_rope)
    "gsasr_window_attn_rope_scratch_bytes": (_sz, [_wrp]),
    "gsasr_window_attn_rope_forward": (_i, [_wrp, _vp]),
    "gsasr_window_attn_rope_backward": (_i, [_wrp, _vp]),
    # ... both with bf16 activations (gsasr_window_attn_bf16, gsasr_window_attn_rope_bf16)
    "gsasr_window_attn_bf16_scratch_bytes": (_sz, [_wabp]),
    "gsasr_window_attn_bf16_forward": (_i, [_wabp, _vp]),
    "gsasr_window_attn_bf16_backward": (_i, [_wabp, _vp]),
    "gsasr_window_attn_rope_bf16_scratch_bytes": (_sz, [_wrbp]),
    "gsasr_window_attn_rope_bf16_forward": (_i, [_wrbp, _vp]),
    "gsasr_window_attn_rope_bf16_backward": (_i, [_wrbp, _vp]),
    # ... the biased one with a mask per window and packed q, k, v (gsasr_window_attn_masked, gsasr_window_attn_masked_bf16)
    "gsasr_window_attn_masked_scratch_bytes": (_sz, [_wmp]),
    "gsasr_window_attn_masked_forward": (_i, [_wmp, _vp]),
    "gsasr_window_attn_masked_backward": (_i, [_wmp, _vp]),
    "gsasr_window_attn_masked_bf16_scratch_bytes": (_sz, [_wmbp]),
    "gsasr_window_attn_masked_bf16_forward": (_i, [_wmbp, _vp]),
    "gsasr_window_attn_masked_bf16_backward": (_i, [_wmbp, _vp]),
}
EXPORTS = tuple(_SIGNATURES)

_lib = None


def lib():
    """Load the shared library (once). Raises if it has not been built -- there is no CPU path."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} not found: the HIP rasterizer is not built. Run `python -m gsasr_amd.build` "
                "(or __graft_entry__.build()). gsasr_amd has no CPU/eager fallback by design.")
        L = ctypes.CDLL(LIB_PATH)
        for name, (restype, argtypes) in _SIGNATURES.items():
            fn = getattr(L, name)
            fn.restype, fn.argtypes = restype, argtypes
        if L.gsasr_abi_version() != 7:
            raise RuntimeError("libgsasr_splat.so ABI version mismatch")
        _lib = L
    return _lib


def check(rc: int, what: str) -> None:
    if rc != 0:
        msg = lib().gsasr_last_error().decode(errors="replace")
        raise RuntimeError(f"{what} failed (status {rc}): {msg}")


def _chk(t: torch.Tensor, name: str, shape_tail: Optional[Tuple[int, ...]] = None) -> int:
    # same failure mode as the reference's CHECK_INPUT (gswrapper.cpp:5-7): RuntimeError
    if not isinstance(t, torch.Tensor):
        raise RuntimeError(f"{name} must be a torch.Tensor")
    if not t.is_cuda:
        raise RuntimeError(f"{name} must be a CUDA tensor")
    if not t.is_contiguous():
        raise RuntimeError(f"{name} must be contiguous")
    if t.dtype != torch.float32:
        raise RuntimeError(f"{name} must be float32 (got {t.dtype}); the kernels read raw fp32")
    if shape_tail is not None and tuple(t.shape[-len(shape_tail):]) != shape_tail:
        raise RuntimeError(f"{name} has shape {tuple(t.shape)}, expected [..., {shape_tail}]")
    return t.data_ptr()


def _stream(device: torch.device) -> int:
    return torch.cuda.current_stream(device).cuda_stream


def _ptr3(t: torch.Tensor, name: str, last: int) -> int:
    """`_chk(t, name, (last,))` for the hot path: one combined test first, the explanatory ones only when it fails"""
    if t.__class__ is torch.Tensor and t.is_cuda and t.dtype is torch.float32 and t.is_contiguous() and t.shape[-1] == last:
        return t.data_ptr()
    return _chk(t, name, (last,))


class _Nop:
    def __enter__(self):
        return None

    def __exit__(self, *a):
        return False


_NOP = _Nop()


def _on(device: torch.device):
    """`torch.cuda.device(device)` only when it is not the current device already (the context manager costs ~10 us,
    a third of a call's host time on the single-GPU-per-process layout this package is meant for)"""
    idx = device.index if device.index is not None else torch.cuda.current_device()
    return _NOP if idx == torch.cuda.current_device() else torch.cuda.device(device)


class _WorkspacePool:
    """Workspaces of the step entry points, kept between calls so that a plan can skip its counter memset: every plan
    zeroes the per-cell counters of the OTHER parity on the side (GSASR_FLAG_COUNTERS_CLEAN / GSASR_FLAG_PARITY), so a
    workspace that comes back from a finished step is clean for the flipped parity.  Keyed by (device, stream, size):
    reuse is ordered by the stream, exactly like the caching allocator's own reuse.  Bounded: a few workspaces per
    key, MAX_BYTES in all (least recently used keys go first -- training on ragged sizes meets many sizes).  Thread-safe:
    `Plan.__del__` gives workspaces back from whichever thread drops the last reference (the autograd engine's among them)
    while another thread takes one for its next plan."""
    KEEP = 4                    # free workspaces kept per key (forward and backward of a few steps in flight)
    MAX_BYTES = 2 << 30

    def __init__(self):
        self.free = {}          # key -> [(tensor, parity)]; dict order = least recently used first
        self.bytes = 0
        self.lock = threading.Lock()

    def take(self, key, nbytes, dev):
        with self.lock:
            lst = self.free.get(key)
            if lst:
                ws, parity = lst.pop()
                self.bytes -= ws.numel()
                if lst:
                    self.free[key] = self.free.pop(key)     # most recently used
                else:
                    del self.free[key]
                return ws, parity, True
        return torch.empty(nbytes, dtype=torch.uint8, device=dev), 0, False

    def give(self, key, ws, parity):
        dropped = []            # (freed outside the lock: a tensor's destructor may run arbitrary code)
        with self.lock:
            lst = self.free.pop(key, [])
            if len(lst) < self.KEEP and ws.numel() <= self.MAX_BYTES:
                lst.append((ws, parity))
                self.bytes += ws.numel()
            if lst:
                self.free[key] = lst
            while self.bytes > self.MAX_BYTES and self.free:
                old = next(iter(self.free))
                for t, _ in self.free.pop(old):
                    self.bytes -= t.numel()
                    dropped.append(t)
        del dropped

    def clear(self):
        with self.lock:
            dropped = list(self.free.values())
            self.free.clear()
            self.bytes = 0
        del dropped


_POOL = _WorkspacePool()


def clear_workspace_pool() -> None:
    """Drop the pooled plan workspaces (up to `_WorkspacePool.MAX_BYTES` of device memory that `torch.cuda.empty_cache()`
    cannot see as free while the pool holds it): call it next to `empty_cache()` when memory is tight.  Also frees the
    scratch the reference-shaped C launchers (module `gscuda`) keep per stream."""
    _POOL.clear()
    if _lib is not None:
        _lib.gsasr_release_launcher_scratch()
    from . import _cpp_node
    _cpp_node.clear_pool()


@dataclass
class Plan:
    """Binning workspace of one (sigmas, coords, colors, dims): shared by forward and backward."""
    dims: Dims
    workspace: torch.Tensor
    device: torch.device
    pool_key: Optional[tuple] = None      # set for pooled workspaces: returned (with the parity flipped) when the plan dies.
    #                                       A caller that re-plans on `workspace` itself (C entry points with its own flags)
    #                                       must set this to None: the pool's "counters clean" bookkeeping no longer holds
    parity: int = 0
    view: Optional[View] = None           # the window this plan renders (the view of its dims, `make_view`), None for a whole image /
    #                                       band / canvas: every call on the plan passes it on.  A canvas with one window per
    #                                       sample: the ctypes array of its B views

    def __post_init__(self):
        if self.view is None:
            self.view = self.dims.__dict__.get("_view")

    def __del__(self):
        if self.pool_key is not None:
            try:
                _POOL.give(self.pool_key, self.workspace, self.parity ^ 1)
            except Exception:      # interpreter shutdown
                pass


def make_dims(s: int, h: int, w: int, dmax: Optional[float], rows: Optional[Tuple[int, int]] = None,
              cutoff: float = 0.0, flags: int = 0, list_cap: int = 0) -> Dims:
    r0, r1 = (0, h) if rows is None else rows
    d = Dims(int(s), int(h), int(w), 3, -1.0 if dmax is None else float(dmax), int(r0), int(r1),
             float(cutoff), int(flags))
    d.list_cap = int(list_cap)      # tile lists: 0 = the library's capacity estimate, > 0 entries per tile, < 0 none
    return d


# ---- a window of the grid (include/gsasr_splat.h: gsasr_view) ------------------------------------------------
def make_view(d: Dims, view) -> Dims:
    """attach `view` = (full_h, full_w, y0, x0) to the dims of the window (`make_dims(s, h, w, ...)` with the WINDOW's h, w):
    the calls below then go to the `_view` entry points.  Dims of a batched canvas (`make_batch_dims`, whose sizes are then
    the windows'): `view` = one such tuple per sample"""
    if view is not None:
        if d.batch > 1:
            if len(view) != d.batch:
                raise RuntimeError("views must hold one (full_h, full_w, y0, x0) per sample")
            d._view = (View * d.batch)(*[View(*[int(v) for v in one]) for one in view])
        else:
            d._view = View(*[int(v) for v in view])
    return d


def _view_of(d: Dims) -> Optional[View]:
    return d.__dict__.get("_view")


def _vref(v):
    """a view as the `const gsasr_view *` argument: the struct by reference, a canvas' array of views as it is"""
    return v if isinstance(v, ctypes.Array) else ctypes.byref(v)


def _view_key(v) -> tuple:
    return tuple(x for one in (v if isinstance(v, ctypes.Array) else (v,)) for x in (one.full_h, one.full_w, one.y0, one.x0))


def _vcall(name: str, d: Dims):
    """(export, its leading dims arguments) for dims `d`: `name` with the dims, or `name_view` with the dims and their view"""
    v = d.__dict__.get("_view")
    if v is None:
        return getattr(lib(), name), name, (ctypes.byref(d),)
    name += "_view"
    return getattr(lib(), name), name, (ctypes.byref(d), _vref(v))


# ---- batched canvas: its dims -------------------------------------------------------
MAX_BATCH = 64   # GSASR_MAX_BATCH


def _canvas_slot(h_max: int) -> int:
    """rows of one slot of a canvas: the tallest sample, in whole 16-row tiles"""
    return (int(h_max) + 15) // 16 * 16


def make_batch_dims(n_per: int, sizes, w_max: int, h_max: int, dmax: Optional[float], cutoff: float = 0.0,
                    flags: int = 0) -> Dims:
    """dims of a canvas of len(sizes) slots; `sizes` = [(h_b, w_b)].  The returned struct owns the host array."""
    B = len(sizes)
    if not (1 < B <= MAX_BATCH):
        raise RuntimeError(f"batch size must be in 2..{MAX_BATCH}")
    slot = _canvas_slot(h_max)
    hw = (ctypes.c_int * (2 * B))(*[int(v) for hw_ in sizes for v in hw_])
    d = Dims(int(n_per) * B, slot * B, int(w_max), 3, -1.0 if dmax is None else float(dmax), 0, slot * B,
             float(cutoff), int(flags), B, slot, ctypes.cast(hw, ctypes.POINTER(ctypes.c_int)))
    d._keepalive = hw
    return d


# ---- what every planning entry point does first: the shape's dims and workspace size (cached), then a workspace ----
def _check_dmax(dmax: Optional[float]) -> None:
    if dmax is not None and not (float(dmax) >= 0.0):
        raise RuntimeError("dmax must be >= 0")


# Per shape, built once and not per call: what a plan's dims are made from -> ([Dims fresh, pooled parity 0, pooled parity 1],
# workspace bytes).  The Dims are shared by all plans of the shape: nobody edits them (`_dims_with`, and whoever needs other
# flags, copies first).  Workspace sizes follow a registered kernel choice: set_kernel_choice / clear_kernel_choices empty this.
_SHAPES = {}
_SPLAT_BYTES, _STEP_BYTES = "gsasr_splat_workspace_bytes", "gsasr_step_workspace_bytes"


def _new_shape(key, dmax, make, bytes_fn: str):
    """a cache miss of `_image_shape` / `_canvas_shape`: `make(extra_flags)` builds one Dims, the export `bytes_fn` sizes it"""
    _check_dmax(dmax)
    variants = [make(f) for f in (0, FLAG_COUNTERS_CLEAN, FLAG_COUNTERS_CLEAN | FLAG_PARITY)]
    fn, bytes_fn, dargs = _vcall(bytes_fn, variants[0])
    nbytes = fn(*dargs)
    if nbytes == 0:
        check(-1, bytes_fn)
    if len(_SHAPES) > 512:
        _SHAPES.clear()
    hit = _SHAPES[key] = (variants, nbytes)
    return hit


def _image_shape(bytes_fn: str, s: int, h: int, w: int, dmax, flags: int, rows=None, cutoff: float = 0.0, list_cap: int = 0, view=None):
    """`view` = (full_h, full_w, y0, x0): h, w are a window of that grid (`make_view`)"""
    if view is None:
        key = (bytes_fn, s, h, w, dmax, flags, rows, cutoff, list_cap)
    else:
        view = tuple(int(v) for v in view)
        if len(view) != 4:
            raise RuntimeError("view must be (full_h, full_w, y0, x0)")
        key = (bytes_fn, s, h, w, dmax, flags, rows, cutoff, list_cap, view)
    return _SHAPES.get(key) or _new_shape(key, dmax, lambda f: make_view(make_dims(s, h, w, dmax, rows, cutoff, int(flags) | f, list_cap), view), bytes_fn)


def _views(views, batch: int):
    """`views` = [(full_h, full_w, y0, x0)] * B of a canvas, as a tuple of int tuples"""
    views = tuple(tuple(int(v) for v in one) for one in views)
    if len(views) != batch or any(len(one) != 4 for one in views):
        raise RuntimeError("views must hold one (full_h, full_w, y0, x0) per sample")
    return views


def _canvas_shape(n_per: int, sizes, dmax, flags: int, views=None, bytes_fn: str = _STEP_BYTES, cutoff: float = 0.0, list_cap: int = 0):
    """the canvas of `sizes` = [(h_b, w_b)] with `n_per` Gaussians per sample, sized by gsasr_step_workspace_bytes.
    `views` = [(full_h, full_w, y0, x0)]: sample b is the h_b x w_b window at (y0, x0) of its own full grid (`make_view`)"""
    sizes = tuple(map(tuple, sizes))
    key = (n_per, sizes, dmax, flags)
    if views is not None:
        views = _views(views, len(sizes))
        key += (views,)
    if bytes_fn != _STEP_BYTES or cutoff != 0.0 or list_cap != 0:
        key += (bytes_fn, cutoff, list_cap)

    def make(f):
        d = make_batch_dims(n_per, sizes, max(w for _, w in sizes), max(h for h, _ in sizes), dmax, cutoff, flags=int(flags) | f)
        d.list_cap = int(list_cap)
        return make_view(d, views)
    return _SHAPES.get(key) or _new_shape(key, dmax, make, bytes_fn)


_LAYOUT_FLAGS = FLAG_FORWARD_ONLY | FLAG_BWD_TILE | FLAG_BWD_GAUSSIAN | FLAG_BWD_ATOMIC | FLAG_BWD_HOME | FLAG_CHW_GRAD | FLAG_STRIDE8


def _pool_key(d: Dims, nbytes: int, dev, stream: int):
    """Workspaces are interchangeable only between plans of the SAME layout: "the counters of parity p are zero" is a
    statement about where the counter arrays lie and how long they are (grid size), so the key carries everything the
    layout depends on, not just the byte count (two small shapes easily round to the same size)."""
    key = (dev.index, stream, nbytes, d.s, d.h, d.w, d.batch, d.slot, d.flags & _LAYOUT_FLAGS)
    v = d.__dict__.get("_view")     # (a window's layout also follows the grid it is cut from: the kernel-choice rules read it)
    return key if v is None else key + _view_key(v)


def _acquire(shape, dev, stream: int):
    """The workspace of a new plan of `shape` (an entry of `_SHAPES`), inside `with _on(dev)`: from the pool, with the Dims
    variant that tells the plan which counters are clean, or fresh.  Returns (dims to plan with, workspace, pool key or
    None, parity)."""
    variants, nbytes = shape
    if torch.cuda.is_current_stream_capturing():
        # a captured plan is replayed on the same workspace with the same parity: it must zero its own counters
        return variants[0], torch.empty(nbytes, dtype=torch.uint8, device=dev), None, 0
    pool_key = _pool_key(variants[0], nbytes, dev, stream)
    ws, parity, clean = _POOL.take(pool_key, nbytes, dev)
    return (variants[1 + parity] if clean else variants[0]), ws, pool_key, parity


def plan(sigmas: torch.Tensor, coords: torch.Tensor, colors: torch.Tensor, h: int, w: int,
         dmax: Optional[float], rows: Optional[Tuple[int, int]] = None, cutoff: float = 0.0,
         flags: int = 0, list_cap: int = 0, view=None, sizes=None, views=None) -> Plan:
    """`view` = (full_h, full_w, y0, x0): plan the h x w window of that grid whose first pixel is its (y0, x0); `forward`,
    `forward_u8` and `backward` on the plan then render / differentiate the window only.
    `sizes` = [(h_b, w_b)] * B: a batched canvas of kernel-frame Gaussians in sample-major order (`h`, `w`, `rows` are not
    read: `make_batch_dims`); with `views` = [(full_h, full_w, y0, x0)] * B sample b is that window of its own grid."""
    ps = _ptr3(sigmas, "sigmas", 3)
    pc = _ptr3(coords, "coords", 2)
    pk = _ptr3(colors, "colors", 3)
    s = sigmas.shape[0]
    if coords.shape[0] != s or colors.shape[0] != s:
        raise RuntimeError("sigmas, coords, colors disagree on the number of Gaussians")
    if sizes is not None:
        if view is not None or s % len(sizes) != 0:
            raise RuntimeError("a canvas takes `views`, one per sample, and the same number of Gaussians for every sample")
        shape = _canvas_shape(s // len(sizes), sizes, dmax, flags, views, _SPLAT_BYTES, cutoff, list_cap)
    elif views is not None:
        raise RuntimeError("`views` go with the `sizes` of a canvas (one image: `view`)")
    else:
        shape = _image_shape(_SPLAT_BYTES, s, int(h), int(w), dmax, flags, rows, cutoff, list_cap, view)
    dev = sigmas.device
    with _on(dev):
        stream = _stream(dev)
        d, ws, pool_key, parity = _acquire(shape, dev, stream)
        if _view_of(d) is None:
            check(lib().gsasr_splat_plan(ps, pc, pk, ctypes.byref(d), ws.data_ptr(), shape[1], stream), "gsasr_splat_plan")
        else:
            check(lib().gsasr_splat_plan_view(ps, pc, pk, ctypes.byref(d), _vref(_view_of(d)), ws.data_ptr(), shape[1], stream),
                  "gsasr_splat_plan_view")
    return Plan(d, ws, dev, pool_key, parity)


def _dims_with(p: Plan, extra_flags: int) -> Dims:
    """the plan's dims with `extra_flags` added (copies are cached on the Dims object, which plans of one shape share)"""
    d0 = p.dims
    if not extra_flags or (d0.flags & extra_flags) == extra_flags:
        return d0
    cache = d0.__dict__.get("_with")
    if cache is None:
        cache = d0.__dict__["_with"] = {}
    d = cache.get(extra_flags)
    if d is None or d.flags != (d0.flags | extra_flags):
        d = Dims.from_buffer_copy(d0)
        d.flags |= extra_flags
        if hasattr(d0, "_keepalive"):
            d._keepalive = d0._keepalive
        if "_view" in d0.__dict__:
            d._view = d0._view
        cache[extra_flags] = d
    return d


def forward(p: Plan, img: torch.Tensor, overwrite: bool = False, chw: bool = False, flags: int = 0) -> torch.Tensor:
    """img += splat (reference contract), or img = splat when `overwrite` (img may be torch.empty).
    `chw`: img is planar [3, rows, W] instead of [rows, W, 3].  `flags`: FLAG_FWD_WIDE / FLAG_FWD_NARROW (kernel choice)."""
    d0 = p.dims
    rows = d0.row1 - d0.row0
    if chw:
        pi = _chk(img, "rendered_img", (rows, d0.w))
        if img.shape[0] != 3 or img.dim() != 3 or img.device != p.device:
            raise RuntimeError("rendered_img does not match the plan (shape / device)")
    else:
        pi = _ptr3(img, "rendered_img", 3)
        if img.dim() != 3 or img.shape[0] != rows or img.shape[1] != d0.w or img.device != p.device:
            raise RuntimeError("rendered_img does not match the plan (shape / device)")
    d = _dims_with(p, (FLAG_OVERWRITE_IMAGE if overwrite else 0) | (FLAG_CHW_IMAGE if chw else 0) |
                   (flags & (FLAG_FWD_WIDE | FLAG_FWD_NARROW)))
    with _on(p.device):
        if p.view is None:
            check(lib().gsasr_splat_forward(ctypes.byref(d), p.workspace.data_ptr(), p.workspace.numel(), pi,
                                            _stream(p.device)), "gsasr_splat_forward")
        else:
            check(lib().gsasr_splat_forward_view(ctypes.byref(d), _vref(p.view), p.workspace.data_ptr(), p.workspace.numel(), pi,
                                                 _stream(p.device)), "gsasr_splat_forward_view")
    return img


def forward_subtile_width(p: Plan, flags: int = 0) -> int:
    """16 when `forward(p, ..., flags=flags)` runs the wide forward (16 x 16 sub-tiles), 8 for the 8 x 16 kernels"""
    return int(lib().gsasr_forward_subtile_width(ctypes.byref(_dims_with(p, flags & (FLAG_FWD_WIDE | FLAG_FWD_NARROW)))))


# ---- 8-bit image output (include/gsasr_splat.h: gsasr_splat_forward_u8) ---------------------------------------------
def _u8_target(d: Dims, crop, out: Optional[torch.Tensor], dev):
    """(crop rows, crop columns, output tensor, pitch in bytes) of an 8-bit forward with dims `d`.  `crop` = (rows, columns) of
    the grid's top-left corner (None: all of it).  The tensor is `[rows of the band inside the crop, columns, 3]` (batched
    canvas: `[B, rows, columns, 3]`), fresh or the caller's `out`, whose row stride is the pitch."""
    B = int(d.batch) if d.batch > 1 else 0
    full_h, full_w = (d.slot if B else d.h), d.w
    if B and crop is None:
        full_h = max(d.sample_hw[2 * b] for b in range(B))
    rows, cols = (full_h, full_w) if crop is None else (int(crop[0]), int(crop[1]))
    if not (1 <= rows <= (d.slot if B else d.h) and 1 <= cols <= d.w):
        raise RuntimeError(f"crop {(rows, cols)} must be at least 1 x 1 and at most the grid, {(d.slot if B else d.h, d.w)}")
    n_rows = rows if B else min(d.row1, rows) - d.row0
    if n_rows <= 0:
        raise RuntimeError("the plan's row band lies outside the crop")
    shape = (B, n_rows, cols, 3) if B else (n_rows, cols, 3)
    if out is None:
        return rows, cols, torch.empty(shape, dtype=torch.uint8, device=dev), 3 * cols
    if not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.uint8 and out.device == dev):
        raise RuntimeError("out must be a uint8 CUDA tensor on the plan's device")
    pitch = out.stride(-3)
    if tuple(out.shape) != shape or out.stride(-1) != 1 or out.stride(-2) != 3 or pitch < 3 * cols or \
            (B and out.stride(0) != n_rows * pitch):
        raise RuntimeError(f"out must be {shape} with interleaved pixels (strides [pitch >= {3 * cols}, 3, 1]"
                           + (", samples rows * pitch apart)" if B else ")") + f", got {tuple(out.shape)} / {out.stride()}")
    return rows, cols, out, int(pitch)


def forward_u8(p: Plan, crop=None, bgr: bool = False, out: Optional[torch.Tensor] = None, flags: int = 0) -> torch.Tensor:
    """The splat of plan `p` as an 8-bit image `[rows, cols, 3]` (batched canvas `[B, rows, cols, 3]`): per channel value
    `rint(clamp(v, 0, 1) * 255)`, stored by the forward kernels themselves -- no float image exists.  `crop` = (rows, cols):
    the top-left corner of the grid (the reference's `[:gt_h, :gt_w]`); `bgr`: bytes in b, g, r order; `out`: write into
    the caller's uint8 tensor (its row stride is the pitch; bytes outside the pixels are left alone).  `flags`:
    FLAG_FWD_WIDE / FLAG_FWD_NARROW, as for `forward`, which runs the same kernel for the same plan and flags."""
    d = _dims_with(p, flags & (FLAG_FWD_WIDE | FLAG_FWD_NARROW))
    with _on(p.device):
        rows, cols, out, pitch = _u8_target(d, crop, out, p.device)
        if p.view is None:
            check(lib().gsasr_splat_forward_u8(ctypes.byref(d), p.workspace.data_ptr(), p.workspace.numel(), out.data_ptr(), rows, cols,
                                               pitch, U8_SWAP_RB if bgr else 0, _stream(p.device)), "gsasr_splat_forward_u8")
        else:
            check(lib().gsasr_splat_forward_u8_view(ctypes.byref(d), _vref(p.view), p.workspace.data_ptr(), p.workspace.numel(),
                                                    out.data_ptr(), rows, cols, pitch, U8_SWAP_RB if bgr else 0, _stream(p.device)),
                  "gsasr_splat_forward_u8_view")
    return out


def backward(p: Plan, sigmas, coords, colors, grad_img, g_sigmas, g_coords, g_colors, overwrite: bool = False) -> None:
    """g_* += gradients (reference contract: caller zero-fills), or g_* = gradients when `overwrite`."""
    d0 = p.dims
    pg = _ptr3(grad_img, "grads", 3)
    if grad_img.dim() != 3 or grad_img.shape[1] != d0.w:
        raise RuntimeError(f"grads has shape {tuple(grad_img.shape)}, expected [rows, {d0.w}, 3]")
    if grad_img.shape[0] != d0.row1 - d0.row0:
        raise RuntimeError("grads does not match the plan's row band")
    _splat_backward(p, (_ptr3(sigmas, "sigmas", 3), _ptr3(coords, "coords", 2), _ptr3(colors, "colors", 3), pg,
                        _ptr3(g_sigmas, "grads_sigmas", 3), _ptr3(g_coords, "grads_coords", 2), _ptr3(g_colors, "grads_colors", 3)),
                    FLAG_OVERWRITE_GRADS if overwrite else 0)


def _splat_backward(p: Plan, ptrs, extra_flags: int) -> None:
    """gsasr_splat_backward on plan `p`; `ptrs` = the three inputs, the image gradient and the three gradient outputs"""
    d = _dims_with(p, extra_flags)
    with _on(p.device):
        if p.view is None:
            check(lib().gsasr_splat_backward(*ptrs, ctypes.byref(d), p.workspace.data_ptr(), p.workspace.numel(), _stream(p.device)),
                  "gsasr_splat_backward")
        else:
            check(lib().gsasr_splat_backward_view(*ptrs, ctypes.byref(d), _vref(p.view), p.workspace.data_ptr(),
                                                  p.workspace.numel(), _stream(p.device)), "gsasr_splat_backward_view")


_AUTOTUNE = os.environ.get("GSASR_AMD_AUTOTUNE", "0") not in ("", "0")


def _tune_on() -> bool:
    return _AUTOTUNE


def plan_forward(sigmas: torch.Tensor, coords: torch.Tensor, colors: torch.Tensor, img: torch.Tensor,
                 dmax: Optional[float]) -> Plan:
    """`plan` + `forward` (accumulating into `img[H,W,3]`) as one host call: what `GSCUDA.forward` does, with one device /
    stream lookup and one set of argument checks for both C calls"""
    ps = _ptr3(sigmas, "sigmas", 3)
    pc = _ptr3(coords, "coords", 2)
    pk = _ptr3(colors, "colors", 3)
    pi = _ptr3(img, "rendered_img", 3)
    if img.dim() != 3:
        raise RuntimeError("rendered_img must be [H,W,3]")
    s, h, w = sigmas.shape[0], img.shape[0], img.shape[1]
    dev = sigmas.device
    if coords.shape[0] != s or colors.shape[0] != s:
        raise RuntimeError("sigmas, coords, colors disagree on the number of Gaussians")
    if img.device != dev:
        raise RuntimeError("rendered_img does not match the plan (shape / device)")
    if _tune_on():      # GSASR_AMD_AUTOTUNE=1: a shape's first call measures the kernel combinations (gsasr_amd/tune.py)
        from . import tune
        tune.autotune_hook(sigmas, coords, colors, h, w, dmax,
                           torch.is_grad_enabled() and (sigmas.requires_grad or coords.requires_grad or colors.requires_grad))
    shape = _image_shape(_SPLAT_BYTES, s, h, w, dmax, 0)
    L, nbytes = lib(), shape[1]
    with _on(dev):
        stream = _stream(dev)
        d, ws, pool_key, parity = _acquire(shape, dev, stream)
        pw = ws.data_ptr()
        check(L.gsasr_splat_plan(ps, pc, pk, ctypes.byref(d), pw, nbytes, stream), "gsasr_splat_plan")
        check(L.gsasr_splat_forward(ctypes.byref(d), pw, nbytes, pi, stream), "gsasr_splat_forward")
    return Plan(d, ws, dev, pool_key, parity)


def backward_new(p: Plan, sigmas: torch.Tensor, coords: torch.Tensor, colors: torch.Tensor, grad_img: torch.Tensor):
    """`backward` into three fresh gradient tensors (stored, not accumulated): what `GSCUDA.backward` returns"""
    g_sigmas, g_coords, g_colors = torch.empty_like(sigmas), torch.empty_like(coords), torch.empty_like(colors)
    backward(p, sigmas, coords, colors, grad_img if grad_img.is_contiguous() else grad_img.contiguous(), g_sigmas, g_coords,
             g_colors, overwrite=True)
    return g_sigmas, g_coords, g_colors


# ---- packed [N,8] records (GSASR_FLAG_STRIDE8): the wire format of the multi-GPU exchange --------------
def _cols(packed: torch.Tensor, name: str):
    base = _chk(packed, name, (8,))
    if packed.dim() != 2:
        raise RuntimeError(f"{name} must be [N,8]")
    return base, base + 12, base + 20      # sigmas, coords, colors columns of the same records


def plan_packed(packed: torch.Tensor, h: int, w: int, dmax: Optional[float],
                rows: Optional[Tuple[int, int]] = None, cutoff: float = 0.0, workspace: Optional[torch.Tensor] = None,
                flags: int = 0) -> Plan:
    """`plan` for Gaussians held as one `[N,8]` tensor {sx,sy,rho,x,y,r,g,b}; no unpacking copies."""
    ps, pc, pk = _cols(packed, "packed")
    shape = _image_shape(_SPLAT_BYTES, packed.shape[0], int(h), int(w), dmax, FLAG_STRIDE8 | int(flags),
                         rows if rows is None else tuple(rows), cutoff)
    dev = packed.device
    with _on(dev):
        stream = _stream(dev)
        if workspace is None:
            d, ws, pool_key, parity = _acquire(shape, dev, stream)
        else:       # the caller's own workspace: nothing is known about its counters
            d, ws, pool_key, parity = shape[0][0], workspace, None, 0
            if ws.numel() < shape[1]:
                raise RuntimeError("workspace smaller than gsasr_splat_workspace_bytes()")
        check(lib().gsasr_splat_plan(ps, pc, pk, ctypes.byref(d), ws.data_ptr(), ws.numel(), stream), "gsasr_splat_plan")
    return Plan(d, ws, dev, pool_key, parity)


def backward_packed(p: Plan, packed: torch.Tensor, grad_img: torch.Tensor, g_packed: torch.Tensor,
                    overwrite: bool = False) -> None:
    """`backward` with inputs and gradients as `[N,8]` records (the plan must come from `plan_packed`)."""
    if not (p.dims.flags & FLAG_STRIDE8):
        raise RuntimeError("backward_packed needs a plan made by plan_packed")
    ps, pc, pk = _cols(packed, "packed")
    gs, gc, gk = _cols(g_packed, "g_packed")
    pg = _chk(grad_img, "grads", (p.dims.w, 3))
    if grad_img.shape[0] != p.dims.row1 - p.dims.row0 or g_packed.shape[0] != p.dims.s or packed.shape[0] != p.dims.s:
        raise RuntimeError("grads / g_packed do not match the plan")
    _splat_backward(p, (ps, pc, pk, pg, gs, gc, gk), FLAG_OVERWRITE_GRADS if overwrite else 0)


def backward_to_packed(p: Plan, sigmas: torch.Tensor, coords: torch.Tensor, colors: torch.Tensor, grad_img: torch.Tensor,
                       g_packed: torch.Tensor, overwrite: bool = True) -> None:
    """`backward` of a plan made from three separate arrays, with the gradient written as ONE `[N,8]` array
    {d sx, d sy, d rho, d x, d y, d r, d g, d b} -- the buffer a collective then runs on in place (gsasr_amd/shard.py).
    The backward reads the plan, not the input arrays, so only the OUTPUT stride changes (GSASR_FLAG_STRIDE8 at backward time)."""
    if p.dims.flags & FLAG_STRIDE8:
        raise RuntimeError("the plan is packed already: use backward_packed")
    ps, pc, pk = _ptr3(sigmas, "sigmas", 3), _ptr3(coords, "coords", 2), _ptr3(colors, "colors", 3)
    gs, gc, gk = _cols(g_packed, "g_packed")
    pg = _chk(grad_img, "grads", (p.dims.w, 3))
    if grad_img.shape[0] != p.dims.row1 - p.dims.row0 or g_packed.shape[0] != p.dims.s or sigmas.shape[0] != p.dims.s:
        raise RuntimeError("grads / g_packed do not match the plan")
    _splat_backward(p, (ps, pc, pk, pg, gs, gc, gk), FLAG_STRIDE8 | (FLAG_OVERWRITE_GRADS if overwrite else 0))


def _chk_i32(t: torch.Tensor, name: str, n: int) -> int:
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.is_contiguous() and t.dtype == torch.int32 and t.numel() >= n):
        raise RuntimeError(f"{name} must be a contiguous int32 CUDA tensor with >= {n} elements")
    return t.data_ptr()


def band_select(packed: torch.Tensor, h: int, w: int, dmax: Optional[float], rows: Tuple[int, int],
                rows_above: int, rows_below: int, up: torch.Tensor, down: torch.Tensor, up_index: torch.Tensor,
                down_index: torch.Tensor, counts: torch.Tensor, cutoff: float = 0.0) -> None:
    """gsasr_band_select: fill `up`/`down` `[cap,8]` with this band's Gaussians that reach the neighbour bands."""
    base = _chk(packed, "packed", (8,))
    cap = up.shape[0]
    if down.shape[0] != cap:
        raise RuntimeError("up and down must have the same capacity")
    d = make_dims(packed.shape[0], h, w, dmax, rows, cutoff, FLAG_STRIDE8)
    with _on(packed.device):
        check(lib().gsasr_band_select(base, ctypes.byref(d), int(rows_above), int(rows_below), cap,
                                      _chk(up, "up", (8,)), _chk(down, "down", (8,)), _chk_i32(up_index, "up_index", cap),
                                      _chk_i32(down_index, "down_index", cap), _chk_i32(counts, "counts", 4),
                                      _stream(packed.device)), "gsasr_band_select")


def band_merge(g_packed: torch.Tensor, g_up: torch.Tensor, g_down: torch.Tensor, up_index: torch.Tensor,
               down_index: torch.Tensor, counts: torch.Tensor) -> None:
    """gsasr_band_merge: g_packed[index] += the gradients the neighbours returned for the selected records."""
    cap = g_up.shape[0]
    with _on(g_packed.device):
        check(lib().gsasr_band_merge(_chk(g_packed, "g_packed", (8,)), g_packed.shape[0], _chk(g_up, "g_up", (8,)),
                                     _chk(g_down, "g_down", (8,)), _chk_i32(up_index, "up_index", cap),
                                     _chk_i32(down_index, "down_index", cap), _chk_i32(counts, "counts", 4), cap,
                                     _stream(g_packed.device)), "gsasr_band_merge")


def prologue_forward(gs_parameters: torch.Tensor, step: torch.Tensor, h: int, w: int):
    """gs_parameters[N,9] (raw decoder output) -> kernel-frame (sigmas[N,3], coords[N,2], colors[N,3])."""
    pp = _chk(gs_parameters, "gs_parameters", (9,))
    ps = _chk(step, "step_size")
    n, dev = gs_parameters.shape[0], gs_parameters.device
    out = (torch.empty(n, 3, device=dev), torch.empty(n, 2, device=dev), torch.empty(n, 3, device=dev))
    with _on(dev):
        check(lib().gsasr_prologue_forward(pp, ps, n, int(h), int(w), out[0].data_ptr(), out[1].data_ptr(),
                                           out[2].data_ptr(), _stream(dev)), "gsasr_prologue_forward")
    return out


def prologue_backward(gs_parameters, step, h: int, w: int, g_sigmas, g_coords, g_colors) -> torch.Tensor:
    pp = _chk(gs_parameters, "gs_parameters", (9,))
    ps = _chk(step, "step_size")
    ptrs = [_chk(g_sigmas, "g_sigmas", (3,)), _chk(g_coords, "g_coords", (2,)), _chk(g_colors, "g_colors", (3,))]
    n, dev = gs_parameters.shape[0], gs_parameters.device
    gp = torch.empty(n, 9, device=dev)
    with _on(dev):
        check(lib().gsasr_prologue_backward(pp, ps, n, int(h), int(w), *ptrs, gp.data_ptr(), _stream(dev)),
              "gsasr_prologue_backward")
    return gp


_MISMATCH = {}      # device index -> int32[2] device tensor: the sticky "scale_modify pair differs" word of the _sm entry points


def mismatch_flag(dev: torch.device) -> torch.Tensor:
    t = _MISMATCH.get(dev.index)
    if t is None:
        t = _MISMATCH[dev.index] = torch.zeros(2, dtype=torch.int32, device=dev)
    return t


def _sm_ptr(sm: torch.Tensor, batch: int):
    """pointer + element stride of `scale_modify` pairs: a float32 CUDA tensor `[2]` (or longer) for one image, `[B, >=2]`
    rows for a batched canvas"""
    if not (sm.__class__ is torch.Tensor and sm.is_cuda and sm.dtype is torch.float32):
        raise RuntimeError("scale_modify must be a float32 CUDA tensor")
    if batch <= 1:
        if sm.dim() != 1 or sm.shape[0] < 2 or sm.stride(0) != 1:
            raise RuntimeError("scale_modify must be a contiguous [2] tensor")
        return sm.data_ptr(), 2
    if sm.dim() != 2 or sm.shape[0] != batch or sm.shape[1] < 2 or sm.stride(1) != 1 or sm.stride(0) < 2:
        raise RuntimeError(f"scale_modify must be [{batch}, 2] with unit inner stride")
    return sm.data_ptr(), int(sm.stride(0))


_BATCH_ARGS = "gs_parameters must be [B,N,9] with one step size and one (h,w) per sample"


def _step_args(gs_parameters: torch.Tensor, step, scale_modify, default_step_size: float, sizes=None):
    """The argument checks of the step-shaped entry points (`sizes` given: a batched canvas, `gs_parameters` [B,N,9]).  Returns
    the pointer of `gs_parameters` and the step-size source, as the C arguments that follow that pointer: `(step sizes,)`, or for
    the `_sm` twins `(scale_modify, its stride, default step size, mismatch word)`."""
    pp = _ptr3(gs_parameters, "gs_parameters", 9)
    if sizes is None:
        B = 1
        if gs_parameters.dim() != 2:
            raise RuntimeError("gs_parameters must be [N,9]")
    else:
        B = gs_parameters.shape[0]
        if gs_parameters.dim() != 3 or len(sizes) != B:
            raise RuntimeError(_BATCH_ARGS)
    if scale_modify is not None:
        psm, stride = _sm_ptr(scale_modify, B)
        return pp, (psm, stride, float(default_step_size), mismatch_flag(gs_parameters.device).data_ptr())
    ps = _chk(step, "step_size" if sizes is None else "step_sizes")
    if sizes is not None and step.numel() != B:
        raise RuntimeError(_BATCH_ARGS)
    return pp, (ps,)


_STEP_FWD = ("gsasr_step_forward", "gsasr_step_forward_sm")
_STEP_FWD_U8 = ("gsasr_step_forward_u8", "gsasr_step_forward_sm_u8")
_STEP_SAMPLE = ("gsasr_step_sample_forward", "gsasr_step_sample_forward_sm")
_STEP_QUERY = ("gsasr_step_query_forward", "gsasr_step_query_forward_sm")


def _step_call(names, pp: int, src, d: Dims, ws: torch.Tensor, nbytes: int, *tail) -> None:
    """prologue + plan + forward with dims `d` on workspace `ws`: the export `names[0]`, or for a scale_modify source
    (`_step_args`) its `_sm` twin `names[1]`; `tail` = the arguments behind the workspace"""
    name = names[len(src) > 1]
    v = d.__dict__.get("_view")
    if v is None:
        check(getattr(lib(), name)(pp, *src, ctypes.byref(d), ws.data_ptr(), nbytes, *tail), name)
    else:
        name += "_view"
        check(getattr(lib(), name)(pp, *src, ctypes.byref(d), _vref(v), ws.data_ptr(), nbytes, *tail), name)


def _step_planar(shape, pp: int, src, dev):
    """prologue + plan + forward into a fresh planar image, for an image or a canvas `shape` (an entry of `_SHAPES`)"""
    with _on(dev):
        stream = _stream(dev)
        d, ws, pool_key, parity = _acquire(shape, dev, stream)
        img = torch.empty((d.batch, 3, d.slot, d.w) if d.batch > 1 else (3, d.h, d.w), dtype=torch.float32, device=dev)
        _step_call(_STEP_FWD, pp, src, d, ws, shape[1], img.data_ptr(), stream)
    return img, Plan(d, ws, dev, pool_key, parity)


def _step_u8(shape, pp: int, src, crop, bgr: bool, out, dev):
    """prologue + plan + 8-bit forward, likewise"""
    with _on(dev):
        stream = _stream(dev)
        rows, cols, out, pitch = _u8_target(shape[0][0], crop, out, dev)
        d, ws, pool_key, parity = _acquire(shape, dev, stream)
        _step_call(_STEP_FWD_U8, pp, src, d, ws, shape[1], out.data_ptr(), rows, cols, pitch, U8_SWAP_RB if bgr else 0, stream)
    return out, Plan(d, ws, dev, pool_key, parity)


def step_forward(gs_parameters: torch.Tensor, step: Optional[torch.Tensor], h: int, w: int, dmax: Optional[float],
                 extra_flags: int = 0, scale_modify: Optional[torch.Tensor] = None, default_step_size: float = 1.2, view=None):
    """prologue + plan + forward in ONE call: raw `gs_parameters[N,9]` -> planar image `[3,h,w]` (fresh).
    `extra_flags`: FLAG_FORWARD_ONLY (no backward will follow), FLAG_BWD_TILE (plan for the tile-stationary backward).
    The step size is `step` (a `[1]` device tensor), or with `scale_modify` (a `[2]` float32 CUDA tensor) the reference's
    `default_step_size / scale_modify[0]` formed on the device, its `[0] == [1]` assert reported through `mismatch_flag`.
    `view` = (full_h, full_w, y0, x0): the h x w window of that grid at (y0, x0) -- the prologue runs for the full grid."""
    pp, src = _step_args(gs_parameters, step, scale_modify, default_step_size)
    shape = _image_shape(_STEP_BYTES, gs_parameters.shape[0], int(h), int(w), dmax,
                         FLAG_OVERWRITE_IMAGE | FLAG_CHW_IMAGE | int(extra_flags), view=view)
    return _step_planar(shape, pp, src, gs_parameters.device)


def step_forward_u8(gs_parameters: torch.Tensor, step: Optional[torch.Tensor], h: int, w: int, dmax: Optional[float],
                    crop=None, bgr: bool = False, out: Optional[torch.Tensor] = None, extra_flags: int = 0,
                    scale_modify: Optional[torch.Tensor] = None, default_step_size: float = 1.2, view=None):
    """`step_forward` ending in the 8-bit store: raw `gs_parameters[N,9]` -> uint8 `[rows, cols, 3]` (see `forward_u8`) and
    the plan, always FLAG_FORWARD_ONLY (an 8-bit image has no backward).  `extra_flags`: FLAG_FWD_WIDE / FLAG_FWD_NARROW.
    `view`: as for `step_forward`; `crop` is then of the window."""
    pp, src = _step_args(gs_parameters, step, scale_modify, default_step_size)
    shape = _image_shape(_STEP_BYTES, gs_parameters.shape[0], int(h), int(w), dmax, FLAG_FORWARD_ONLY | int(extra_flags), view=view)
    return _step_u8(shape, pp, src, crop, bgr, out, gs_parameters.device)


def step_backward(p: Plan, gs_parameters: torch.Tensor, step: Optional[torch.Tensor], grad: torch.Tensor, chw: bool = False) -> torch.Tensor:
    """splat backward + prologue backward in ONE call; `grad` is `[h,w,3]`, or with `chw` the planar `[3,h,w]` autograd
    hands back (tile-stationary backward, GSASR_FLAG_CHW_GRAD); returns d/d gs_parameters `[N,9]`.  `step=None`: the step
    size the forward's prologue used (kept in the workspace)."""
    pp = _ptr3(gs_parameters, "gs_parameters", 9)
    ps = None if step is None else _chk(step, "step_size")
    pg = _chk(grad, "grads", (3, p.dims.h, p.dims.w) if chw else (p.dims.h, p.dims.w, 3))
    d = _dims_with(p, FLAG_CHW_GRAD if chw else 0)
    with _on(p.device):
        gp = torch.empty_like(gs_parameters)
        if p.view is None:
            check(lib().gsasr_step_backward(pp, ps, pg, gp.data_ptr(), ctypes.byref(d), p.workspace.data_ptr(),
                                            p.workspace.numel(), _stream(p.device)), "gsasr_step_backward")
        else:
            check(lib().gsasr_step_backward_view(pp, ps, pg, gp.data_ptr(), ctypes.byref(d), _vref(p.view), p.workspace.data_ptr(),
                                                 p.workspace.numel(), _stream(p.device)), "gsasr_step_backward_view")
    return gp


# ---- batched canvas: the step entry points on `make_batch_dims`' dims ----------------------------------------
def batch_forward(gs_parameters: torch.Tensor, steps: Optional[torch.Tensor], sizes, dmax: Optional[float], extra_flags: int = 0,
                  scale_modify: Optional[torch.Tensor] = None, default_step_size: float = 1.2, views=None):
    """prologue + plan + forward of a whole batch in ONE set of launches.
    `gs_parameters` [B,N,9], `steps` [B] (device), `sizes` [(h_b, w_b)] -> planar images `[B,3,slot,w_max]`
    (sample b in `[:, :, :h_b, :w_b]`, zero elsewhere) and the plan for `batch_backward`.
    `views` = [(full_h, full_w, y0, x0)] * B: sample b is the h_b x w_b window at (y0, x0) of its own full_h x full_w grid --
    step sizes and the prologue are the full grid's (gsasr_view)."""
    pp, src = _step_args(gs_parameters, steps, scale_modify, default_step_size, sizes)
    shape = _canvas_shape(gs_parameters.shape[1], sizes, dmax, FLAG_OVERWRITE_IMAGE | FLAG_CHW_IMAGE | int(extra_flags), views)
    return _step_planar(shape, pp, src, gs_parameters.device)


def batch_forward_u8(gs_parameters: torch.Tensor, steps: Optional[torch.Tensor], sizes, dmax: Optional[float], crop=None,
                     bgr: bool = False, out: Optional[torch.Tensor] = None, extra_flags: int = 0,
                     scale_modify: Optional[torch.Tensor] = None, default_step_size: float = 1.2, views=None):
    """`batch_forward` ending in the 8-bit store: `gs_parameters` [B,N,9] -> uint8 `[B, rows, cols, 3]` (`crop`, default the
    largest sample's size; sample b in `[b, :h_b, :w_b]`, zero elsewhere) and the plan (FLAG_FORWARD_ONLY).  `views`: as for
    `batch_forward`; `crop` is then of the windows."""
    pp, src = _step_args(gs_parameters, steps, scale_modify, default_step_size, sizes)
    shape = _canvas_shape(gs_parameters.shape[1], sizes, dmax, FLAG_FORWARD_ONLY | int(extra_flags), views)
    return _step_u8(shape, pp, src, crop, bgr, out, gs_parameters.device)


def batch_backward(p: Plan, gs_parameters: torch.Tensor, steps: Optional[torch.Tensor], grad: torch.Tensor, chw: bool = False) -> torch.Tensor:
    """`grad` is `[B, slot, w_max, 3]`, or with `chw` the planar `[B, 3, rows, w_max]` autograd hands back (any
    `rows` >= every sample's height; tile-stationary backward); returns d/d gs_parameters `[B,N,9]`.  `steps=None`: the
    step sizes the forward's prologue used."""
    pp = _chk(gs_parameters, "gs_parameters", (9,))
    ps = None if steps is None else _chk(steps, "step_sizes")
    d = p.dims
    if chw:
        if grad.dim() != 4 or grad.shape[0] != d.batch or grad.shape[1] != 3 or grad.shape[3] != d.w:
            raise RuntimeError(f"grads has shape {tuple(grad.shape)}, expected [{d.batch}, 3, rows, {d.w}]")
        hmax = max(d.sample_hw[2 * b] for b in range(d.batch))
        if not (hmax <= grad.shape[2]):
            raise RuntimeError(f"grads has {grad.shape[2]} rows per plane, a sample has {hmax}")
        pg = _chk(grad, "grads")
        d = Dims.from_buffer_copy(p.dims)
        d.flags |= FLAG_CHW_GRAD
        d.grad_rows = int(grad.shape[2])
    else:
        pg = _chk(grad, "grads", (p.dims.batch, p.dims.slot, p.dims.w, 3))
    with _on(p.device):
        gp = torch.empty_like(gs_parameters)
        if p.view is None:
            check(lib().gsasr_step_backward(pp, ps, pg, gp.data_ptr(), ctypes.byref(d), p.workspace.data_ptr(),
                                            p.workspace.numel(), _stream(p.device)), "gsasr_step_backward")
        else:
            check(lib().gsasr_step_backward_view(pp, ps, pg, gp.data_ptr(), ctypes.byref(d), _vref(p.view), p.workspace.data_ptr(),
                                                 p.workspace.numel(), _stream(p.device)), "gsasr_step_backward_view")
    return gp


# ---- pixel loss fused into the forward's store (include/gsasr_splat.h: gsasr_loss) ---------------------------
def _loss_target(target: torch.Tensor, d: Dims) -> int:
    """rows per plane of a planar fp32 target for dims `d`: `[3, h, w]`, or for a canvas `[B, 3, rows >= every h_b, w_max]`"""
    _chk(target, "target")
    if d.batch > 1:
        h_max = max(d.sample_hw[2 * b] for b in range(d.batch))
        if target.dim() != 4 or target.shape[0] != d.batch or target.shape[1] != 3 or target.shape[3] != d.w or target.shape[2] < h_max:
            raise RuntimeError(f"target has shape {tuple(target.shape)}, expected [{d.batch}, 3, >= {h_max}, {d.w}]")
        return int(target.shape[2])
    if tuple(target.shape) != (3, d.h, d.w):
        raise RuntimeError(f"target has shape {tuple(target.shape)}, expected [3, {d.h}, {d.w}]")
    return int(d.h)


def _loss_scratch(d: Dims, dev) -> torch.Tensor:
    n = int(lib().gsasr_loss_scratch_bytes(ctypes.byref(d)))
    if n == 0:
        check(-1, "gsasr_loss_scratch_bytes")
    return _loss_scratch_of(n, dev)


def _loss_scratch_of(nbytes: int, dev) -> torch.Tensor:
    """the partial sums of a fused loss: fp32, `nbytes` = gsasr_loss_scratch_bytes() of the call's dims.  The one place where
    that scratch is allocated: tests/test_workspace_bounds_gpu.py replaces this function to put the scratch between guards (keep
    it a function of its own)"""
    return torch.empty(nbytes // 4, dtype=torch.float32, device=dev)


def _loss_grad(d0: Dims, shape, dev) -> torch.Tensor:
    """A fresh buffer for the image gradient a fused loss writes.  The forward stores a sample's own pixels only, and the
    Gaussian-stationary backward kernels load up to seven rows past a window's last row in their last trip and switch them off by
    a factor of exactly 0 (bwd_block, splat_bwd_sweep.h): below a sample shorter than its slot those rows are padding nobody
    wrote, and a NaN left there by whoever had the memory before makes 0 * NaN.  So a canvas WITH such padding starts as zeros;
    every other shape -- one image, a batch of crops of whole 16-row tiles -- has none and stays uninitialised."""
    pad = d0.__dict__.get("_loss_pad")
    if pad is None:
        pad = d0.__dict__["_loss_pad"] = d0.batch > 1 and any(d0.sample_hw[2 * b] < d0.slot for b in range(d0.batch))
    return (torch.zeros if pad else torch.empty)(shape, dtype=torch.float32, device=dev)


def forward_loss(p: Plan, target: torch.Tensor, kind: int, norm: int = 0, weight: float = 1.0, eps: float = 1e-12,
                 chw: bool = False, grad_chw: bool = False, want_grad: bool = True, want_image: bool = False, flags: int = 0,
                 grad: Optional[torch.Tensor] = None, scratch: Optional[torch.Tensor] = None):
    """gsasr_splat_forward_loss on plan `p`: the forward kernel `forward(p, ..., flags=flags)` runs, ending in the fused pixel
    loss against `target` -- `[rows, W, 3]`, or with `chw` planar `[3, rows, W]` (canvas: `[B*slot, W, 3]` / `[B, 3, any rows >=
    every h_b, W]`).  Returns (loss `[1 + B]`, the image gradient -- interleaved, or with `grad_chw` planar, what `backward`
    with GSASR_FLAG_CHW_GRAD reads -- or None, the image in the target's layout or None).  `grad`: write the gradient into the
    caller's buffer of that shape instead of a fresh one; `scratch`: likewise the partial sums (fp32, gsasr_loss_scratch_bytes)."""
    d0 = p.dims
    B = d0.batch if d0.batch > 1 else 1
    rows, dev = d0.row1 - d0.row0, p.device
    _chk(target, "target")
    if chw:
        trows = _loss_target(target, d0)
    else:
        trows = 0
        if tuple(target.shape) != (rows, d0.w, 3):
            raise RuntimeError(f"target has shape {tuple(target.shape)}, expected [{rows}, {d0.w}, 3]")
    d = _dims_with(p, FLAG_OVERWRITE_IMAGE | (FLAG_CHW_IMAGE if chw else 0) | (FLAG_CHW_GRAD if grad_chw else 0) |
                   (flags & (FLAG_FWD_WIDE | FLAG_FWD_NARROW)))
    per = d0.slot if d0.batch > 1 else rows
    planar, hwc = ((B, 3, per, d0.w), (rows, d0.w, 3)) if d0.batch > 1 else ((3, rows, d0.w), (rows, d0.w, 3))
    with _on(dev):
        if grad is not None:
            if _chk(grad, "grad") == 0 or tuple(grad.shape) != (planar if grad_chw else hwc) or grad.device != dev:
                raise RuntimeError(f"grad has shape {tuple(grad.shape)}, expected {planar if grad_chw else hwc}")
        elif want_grad:
            grad = _loss_grad(d0, planar if grad_chw else hwc, dev)
        img = torch.empty(planar if chw else hwc, dtype=torch.float32, device=dev) if want_image else None
        loss = torch.empty(1 + B, dtype=torch.float32, device=dev)
        if scratch is None:
            scratch = _loss_scratch(d0, dev)
        elif _chk(scratch, "scratch") == 0 or 4 * scratch.numel() < lib().gsasr_loss_scratch_bytes(ctypes.byref(d0)) or scratch.device != dev:
            raise RuntimeError("scratch is smaller than gsasr_loss_scratch_bytes()")
        desc = Loss(int(kind), int(norm), float(weight), float(eps), target.data_ptr(), trows, None if grad is None else grad.data_ptr(),
                    loss.data_ptr(), None if img is None else img.data_ptr(), scratch.data_ptr())
        check(lib().gsasr_splat_forward_loss(ctypes.byref(d), None if p.view is None else _vref(p.view), p.workspace.data_ptr(),
                                             p.workspace.numel(), ctypes.byref(desc), _stream(dev)), "gsasr_splat_forward_loss")
    return loss, grad, img


def _step_loss(shape, pp: int, src, target: torch.Tensor, kind: int, norm: int, weight: float, eps: float, want_image: bool, dev):
    """prologue + plan + forward ending in the fused pixel loss, for an image or a canvas `shape` (an entry of `_SHAPES`).
    Returns (loss `[1 + B]` = total and per sample, the image gradient in the layout the plan's backward reads or None on a
    forward-only plan, the planar image or None, the plan)."""
    with _on(dev):
        stream = _stream(dev)
        d0 = shape[0][0]
        trows = _loss_target(target, d0)
        if target.device != dev:
            raise RuntimeError("target must be on the Gaussians' device")
        nscratch = d0.__dict__.get("_loss_scratch")
        if nscratch is None:
            nscratch = d0.__dict__["_loss_scratch"] = int(lib().gsasr_loss_scratch_bytes(ctypes.byref(d0)))
            if nscratch == 0:
                check(-1, "gsasr_loss_scratch_bytes")
        d, ws, pool_key, parity = _acquire(shape, dev, stream)
        B = d.batch if d.batch > 1 else 1
        planar = (B, 3, d.slot, d.w) if d.batch > 1 else (3, d.h, d.w)
        grad = None
        if not (d.flags & FLAG_FORWARD_ONLY):
            hwc = (B, d.slot, d.w, 3) if d.batch > 1 else (d.h, d.w, 3)
            grad = _loss_grad(d0, planar if d.flags & FLAG_CHW_GRAD else hwc, dev)
        loss = torch.empty(1 + B, dtype=torch.float32, device=dev)
        scratch = _loss_scratch_of(nscratch, dev)
        img = torch.empty(planar, dtype=torch.float32, device=dev) if want_image else None
        desc = Loss(int(kind), int(norm), float(weight), float(eps), target.data_ptr(), trows, None if grad is None else grad.data_ptr(),
                    loss.data_ptr(), None if img is None else img.data_ptr(), scratch.data_ptr())
        step, sm = (src[0], (None, 0, 0.0, None)) if len(src) == 1 else (None, src)
        v = d.__dict__.get("_view")
        check(lib().gsasr_step_forward_loss(pp, step, *sm, ctypes.byref(d), None if v is None else _vref(v), ws.data_ptr(), shape[1],
                                            ctypes.byref(desc), stream), "gsasr_step_forward_loss")
    return loss, grad, img, Plan(d, ws, dev, pool_key, parity)


def step_forward_loss(gs_parameters: torch.Tensor, step: Optional[torch.Tensor], h: int, w: int, dmax: Optional[float],
                      target: torch.Tensor, kind: int, norm: int = 0, weight: float = 1.0, eps: float = 1e-12, extra_flags: int = 0,
                      scale_modify: Optional[torch.Tensor] = None, default_step_size: float = 1.2, view=None, want_image: bool = False):
    """`step_forward` ending in the fused pixel loss against `target` `[3,h,w]` (fp32, planar) instead of the image: raw
    `gs_parameters[N,9]` -> (loss `[2]` = {L, L_0}, d L / d image for `step_backward` -- planar `[3,h,w]` when `extra_flags`
    carry FLAG_CHW_GRAD, else `[h,w,3]`; None with FLAG_FORWARD_ONLY --, the image `[3,h,w]` if `want_image` else None, the plan).
    `kind` / `norm`: `LOSS_KINDS` / `LOSS_NORMS`.  `view`: as for `step_forward`; target and loss are then the window's."""
    pp, src = _step_args(gs_parameters, step, scale_modify, default_step_size)
    shape = _image_shape(_STEP_BYTES, gs_parameters.shape[0], int(h), int(w), dmax,
                         FLAG_OVERWRITE_IMAGE | FLAG_CHW_IMAGE | int(extra_flags), view=view)
    return _step_loss(shape, pp, src, target, kind, norm, weight, eps, want_image, gs_parameters.device)


def batch_forward_loss(gs_parameters: torch.Tensor, steps: Optional[torch.Tensor], sizes, dmax: Optional[float], target: torch.Tensor,
                       kind: int, norm: int = 0, weight: float = 1.0, eps: float = 1e-12, extra_flags: int = 0,
                       scale_modify: Optional[torch.Tensor] = None, default_step_size: float = 1.2, views=None, want_image: bool = False):
    """`batch_forward` ending in the fused pixel loss: `target` `[B,3,rows,w_max]` (any `rows` >= every sample's height, read in
    place) -> (loss `[1 + B]` = {L, L_0 .. L_{B-1}}, d L / d image for `batch_backward` -- `[B,3,slot,w_max]` with
    FLAG_CHW_GRAD, else `[B,slot,w_max,3]`; only the samples' own pixels are written --, the images `[B,3,slot,w_max]` or None,
    the plan)."""
    pp, src = _step_args(gs_parameters, steps, scale_modify, default_step_size, sizes)
    shape = _canvas_shape(gs_parameters.shape[1], sizes, dmax, FLAG_OVERWRITE_IMAGE | FLAG_CHW_IMAGE | int(extra_flags), views)
    return _step_loss(shape, pp, src, target, kind, norm, weight, eps, want_image, gs_parameters.device)


# ---- SSIM loss of a stored image (include/gsasr_splat.h: gsasr_ssim) -----------------------------------------
def make_ssim(batch: int, rows: int, w: int, sizes=None, target_rows: int = 0, grad_rows: int = 0, weight: float = 1.0,
              flags: int = 0) -> Ssim:
    """a gsasr_ssim descriptor without pointers; `sizes`: the (h_b, w_b) of every sample, None = all rows x w"""
    d = Ssim(int(batch), int(rows), int(w), int(target_rows), int(grad_rows))
    d.weight, d.flags = float(weight), int(flags)
    if sizes is not None:
        if len(sizes) != batch:
            raise RuntimeError("sizes must hold one (h, w) per sample")
        d._hw = (ctypes.c_int * (2 * batch))(*[int(v) for hw in sizes for v in hw])     # kept alive by the descriptor
        d.sample_hw = ctypes.cast(d._hw, ctypes.POINTER(ctypes.c_int))
    return d


def ssim_loss(img: torch.Tensor, target: torch.Tensor, sizes=None, weight: float = 1.0, want_grad: bool = True,
              grad: Optional[torch.Tensor] = None, hwc: bool = False, accumulate: bool = False,
              scratch: Optional[torch.Tensor] = None):
    """gsasr_ssim_loss: `img` planar `[B,3,rows,W]` (or `[3,rows,W]`), `target` `[B,3,any rows >= every h_b,W]`, `sizes` the
    samples' own (h_b, w_b) -> (loss `[1 + B]` = {L, L_0 .. L_{B-1}}, d L / d img or None).  The gradient is planar
    `[B,3,grad_rows,W]`, or with `hwc` interleaved `[B,grad_rows,W,3]`; `grad`: the caller's buffer of that layout (any
    grad_rows >= every h_b), stored into or -- `accumulate` -- added to, on the samples' own pixels only.  `scratch`: a
    caller's fp32 buffer of gsasr_ssim_scratch_bytes."""
    _chk(img, "img")
    _chk(target, "target")
    if img.dim() not in (3, 4) or target.dim() != img.dim() or img.shape[-3] != 3 or target.shape[-3] != 3:
        raise RuntimeError(f"img {tuple(img.shape)} and target {tuple(target.shape)} must both be [B,3,rows,W] or [3,rows,W]")
    B = img.shape[0] if img.dim() == 4 else 1
    rows, w, dev = int(img.shape[-2]), int(img.shape[-1]), img.device
    if target.shape[-1] != w or (target.dim() == 4 and target.shape[0] != B) or target.device != dev:
        raise RuntimeError(f"target has shape {tuple(target.shape)}, expected [{B}, 3, *, {w}] on the image's device")
    flags = (SSIM_GRAD_HWC if hwc else 0) | (SSIM_ACCUMULATE if accumulate else 0)
    d = make_ssim(B, rows, w, sizes, int(target.shape[-2]), 0, weight, flags)
    with _on(dev):
        if grad is not None:
            _chk(grad, "grad")
            lead = () if img.dim() == 3 and grad.dim() == 3 else (B,)
            grows = int(grad.shape[-3] if hwc else grad.shape[-2])
            if tuple(grad.shape) != lead + ((grows, w, 3) if hwc else (3, grows, w)) or grad.device != dev:
                raise RuntimeError(f"grad has shape {tuple(grad.shape)}, expected {'[B,rows,W,3]' if hwc else '[B,3,rows,W]'}")
            d.grad_rows = grows
        elif want_grad:
            if accumulate:
                raise RuntimeError("accumulate needs the gradient buffer to add to")
            lead = (B,) if img.dim() == 4 else ()
            grad = torch.empty(lead + ((rows, w, 3) if hwc else (3, rows, w)), dtype=torch.float32, device=dev)
        d.img, d.target, d.grad_img = img.data_ptr(), target.data_ptr(), None if grad is None else grad.data_ptr()
        n = int(lib().gsasr_ssim_scratch_bytes(ctypes.byref(d)))
        if n == 0:
            check(-1, "gsasr_ssim_scratch_bytes")
        if scratch is None:
            scratch = torch.empty(n // 4, dtype=torch.float32, device=dev)
        elif _chk(scratch, "scratch") == 0 or 4 * scratch.numel() < n or scratch.device != dev:
            raise RuntimeError("scratch is smaller than gsasr_ssim_scratch_bytes()")
        loss = torch.empty(1 + B, dtype=torch.float32, device=dev)
        d.loss, d.scratch = loss.data_ptr(), scratch.data_ptr()
        check(lib().gsasr_ssim_loss(ctypes.byref(d), _stream(dev)), "gsasr_ssim_loss")
    return loss, grad


# ---- the decoder's window attention (include/gsasr_splat.h: gsasr_window_attn) ----------------------------------
def make_window_attn(windows: int, heads: int, nq: int, nk: int, head_dim: int, table_rows: int, scale: float, bf16: bool = False):
    """a gsasr_window_attn (`bf16`: gsasr_window_attn_bf16) descriptor without pointers"""
    d = (WindowAttnBf16 if bf16 else WindowAttn)(int(windows), int(heads), int(nq), int(nk), int(head_dim), int(table_rows))
    d.scale, d.flags = float(scale), 0
    return d


def _chk_act(t: torch.Tensor, name: str, bf16: bool) -> int:
    """`_chk` of an activation: fp32, or bf16 for the bf16 entry points"""
    if not bf16:
        return _chk(t, name)
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.is_contiguous() and t.dtype == torch.bfloat16):
        raise RuntimeError(f"{name} must be a contiguous bfloat16 CUDA tensor")
    return t.data_ptr()


def _own_scratch(scratch: torch.Tensor, n: int, dev, sizer: str) -> int:
    """a caller's scratch for a call that needs `n` bytes (the export `sizer`): a contiguous uint8 CUDA tensor of at least `n`
    bytes on `dev`, 256-byte aligned -> its address"""
    if not (isinstance(scratch, torch.Tensor) and scratch.is_cuda and scratch.dtype == torch.uint8 and scratch.is_contiguous()
            and scratch.device == dev):
        raise RuntimeError("scratch must be a contiguous uint8 CUDA tensor on the call's device")
    if scratch.numel() < n:
        raise RuntimeError(f"scratch is smaller than {sizer}()")
    if scratch.data_ptr() % 256:
        raise RuntimeError("scratch must be 256-byte aligned")
    return scratch.data_ptr()


def make_window_attn_rope(windows: int, heads: int, nq: int, nk: int, head_dim: int, angle_rows: int, scale: float, bf16: bool = False):
    """a gsasr_window_attn_rope (`bf16`: gsasr_window_attn_rope_bf16) descriptor without pointers"""
    d = (WindowAttnRopeBf16 if bf16 else WindowAttnRope)(int(windows), int(heads), int(nq), int(nk), int(head_dim), int(angle_rows))
    d.scale, d.flags = float(scale), 0
    return d


# (rope, bf16) -> the family's entry points
_ATTN_FNS = {(rope, bf16): {what: f"gsasr_window_attn{'_rope' if rope else ''}{'_bf16' if bf16 else ''}_{what}" for what in ("forward", "backward", "scratch_bytes")}
             for rope in (False, True) for bf16 in (False, True)}


def _attn_desc(q, k, v, side, rope: bool, scale: float):
    """the descriptor of a call with q, k, v and `side` (the bias table `[T,H]`, or with `rope` the angles `[H,N,d/2]`) filled in,
    and the names of its entry points; bf16 activations (`q`'s dtype) select the bf16 family"""
    bf16 = q.dtype == torch.bfloat16
    for t, name in ((q, "q"), (k, "k"), (v, "v")):
        _chk_act(t, name, bf16)
    if rope:
        heads = int(side.shape[0])
        d = make_window_attn_rope(q.shape[0], heads, q.shape[1], k.shape[1], q.shape[2] // heads, side.shape[1], scale, bf16)
        d.angles = _chk(side, "angles")
    else:
        heads = int(side.shape[1])
        d = make_window_attn(q.shape[0], heads, q.shape[1], k.shape[1], q.shape[2] // heads, side.shape[0], scale, bf16)
        d.table = _chk(side, "bias_table")
    d.q, d.k, d.v = q.data_ptr(), k.data_ptr(), v.data_ptr()
    return d, _ATTN_FNS[rope, bf16]


def _attn_forward(d, fns, q, want_stats: bool):
    """`out` and (if wanted) the rows' log-sum-exp allocated and the forward called -> (out, stats or None)"""
    dev = q.device
    with _on(dev):
        out = torch.empty_like(q)
        stats = torch.empty(d.windows, d.heads, d.nq, dtype=torch.float32, device=dev) if want_stats else None
        d.out, d.stats = out.data_ptr(), None if stats is None else stats.data_ptr()
        check(getattr(lib(), fns["forward"])(ctypes.byref(d), _stream(dev)), fns["forward"])
    return out, stats


def _attn_backward(d, fns, q, out, stats, grad_out, scratch=None, **grads):
    """out, stats and grad_out checked, the gradient pointers set (`grads`: field -> tensor or None), the scratch asked for
    (0: the descriptor's error is raised) and allocated (or the caller's `scratch`, a uint8 tensor, taken), the backward called"""
    bf16 = q.dtype == torch.bfloat16
    _chk_act(out, "out", bf16), _chk(stats, "stats"), _chk_act(grad_out, "grad_out", bf16)
    if out.shape != q.shape or grad_out.shape != q.shape or tuple(stats.shape) != (d.windows, d.heads, d.nq):
        raise RuntimeError("out / grad_out must have q's shape and stats [W,H,nq]")
    dev = q.device
    with _on(dev):
        d.out, d.stats, d.grad_out = out.data_ptr(), stats.data_ptr(), grad_out.data_ptr()
        for field, g in grads.items():
            setattr(d, field, None if g is None else g.data_ptr())
        n = int(getattr(lib(), fns["scratch_bytes"])(ctypes.byref(d)))
        if n == 0:
            check(-1, fns["scratch_bytes"])
        if scratch is None:
            scratch = torch.empty(n // 4, dtype=torch.float32, device=dev)
            d.scratch = scratch.data_ptr()
        else:
            d.scratch = _own_scratch(scratch, n, dev, fns["scratch_bytes"])
        check(getattr(lib(), fns["backward"])(ctypes.byref(d), _stream(dev)), fns["backward"])


def _attn_index(d, index):
    if index.dtype != torch.int32 or not index.is_cuda or not index.is_contiguous():
        raise RuntimeError("bias_index must be a contiguous int32 CUDA tensor")
    d.index = index.data_ptr()


def window_attn_forward(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, table: torch.Tensor, index: torch.Tensor, scale: float,
                        want_stats: bool = True):
    """gsasr_window_attn_forward: `q` `[W,nq,H*d]`, `k`, `v` `[W,nk,H*d]`, `table` `[T,H]` fp32 contiguous, `index` int32
    `[nq,nk]` (validated by the caller) -> (out `[W,nq,H*d]`, the rows' log-sum-exp `[W,H,nq]` or None).  bf16 `q`, `k`, `v`:
    gsasr_window_attn_bf16_forward, `out` bf16"""
    d, fns = _attn_desc(q, k, v, table, False, scale)
    _attn_index(d, index)
    return _attn_forward(d, fns, q, want_stats)


def window_attn_backward(q, k, v, table, index, scale: float, out, stats, grad_out, need=(True, True, True, True), scratch=None):
    """gsasr_window_attn_backward (bf16 activations: gsasr_window_attn_bf16_backward) -> (g_q, g_k, g_v, g_table), None where
    `need` is False.  `scratch`: the caller's uint8 tensor of gsasr_window_attn[_bf16]_scratch_bytes()"""
    d, fns = _attn_desc(q, k, v, table, False, scale)
    _attn_index(d, index)
    grads = [torch.empty_like(t) if n else None for t, n in zip((q, k, v, table), need)]
    _attn_backward(d, fns, q, out, stats, grad_out, scratch, **dict(zip(("g_q", "g_k", "g_v", "g_table"), grads)))
    return tuple(grads)


# ---- the biased window attention with a mask and packed q, k, v (include/gsasr_splat.h: gsasr_window_attn_masked) ----
def make_window_attn_masked(windows: int, heads: int, nq: int, nk: int, head_dim: int, table_rows: int, scale: float, bf16: bool = False,
                            mask_windows: int = 0, pitches=(0, 0, 0), grad_pitches=(0, 0, 0)):
    """a gsasr_window_attn_masked (`bf16`: gsasr_window_attn_masked_bf16) descriptor without pointers"""
    d = (WindowAttnMaskedBf16 if bf16 else WindowAttnMasked)(int(windows), int(heads), int(nq), int(nk), int(head_dim), int(table_rows))
    d.scale, d.flags, d.mask_windows = float(scale), 0, int(mask_windows)
    d.pitch_q, d.pitch_k, d.pitch_v = (int(p) for p in pitches)
    d.pitch_gq, d.pitch_gk, d.pitch_gv = (int(p) for p in grad_pitches)
    return d


_MASKED_FNS = {bf16: {what: f"gsasr_window_attn_masked{'_bf16' if bf16 else ''}_{what}" for what in ("forward", "backward", "scratch_bytes")}
               for bf16 in (False, True)}


def _rows_view(t: torch.Tensor, name: str, bf16: bool) -> int:
    """the row pitch (elements) of an activation `[W,n,C]` that may be a column block of a wider contiguous tensor"""
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == (torch.bfloat16 if bf16 else torch.float32)):
        raise RuntimeError(f"{name} must be a {'bfloat16' if bf16 else 'float32'} CUDA tensor")
    W, n, C = t.shape
    pitch = t.stride(1) if n > 1 else (t.stride(0) if W > 1 else C)
    if t.stride(2) != 1 or pitch < C or (W > 1 and t.stride(0) != n * pitch):
        raise RuntimeError(f"{name} must be [W,n,C] with unit column stride and one row pitch (strides {tuple(t.stride())})")
    return int(pitch)


def _masked_desc(q, k, v, table, index, mask, scale: float):
    """the gsasr_window_attn_masked descriptor of a call: q, k, v `[W,n,C]` each contiguous or a column block of a packed tensor
    (their row pitches go into the descriptor), `mask` fp32 `[nW,nq,nk]` contiguous or None"""
    bf16 = q.dtype == torch.bfloat16
    pitches = tuple(_rows_view(t, name, bf16) for t, name in ((q, "q"), (k, "k"), (v, "v")))
    heads = int(table.shape[1])
    d = make_window_attn_masked(q.shape[0], heads, q.shape[1], k.shape[1], q.shape[2] // heads, table.shape[0], scale, bf16, pitches=pitches)
    d.table = _chk(table, "bias_table")
    d.q, d.k, d.v = q.data_ptr(), k.data_ptr(), v.data_ptr()
    _attn_index(d, index)
    if mask is not None:
        d.mask, d.mask_windows = _chk(mask, "mask", (d.nq, d.nk)), int(mask.shape[0])
    return d, _MASKED_FNS[bf16]


def window_attn_masked_forward(q, k, v, table, index, mask, scale: float, want_stats: bool = True):
    """gsasr_window_attn_masked_forward (bf16 `q`, `k`, `v`: _masked_bf16_forward) -> (out `[W,nq,C]` contiguous, the rows'
    log-sum-exp or None).  `q`, `k`, `v` may be column blocks of one packed tensor: they are read in place"""
    d, fns = _masked_desc(q, k, v, table, index, mask, scale)
    dev = q.device
    with _on(dev):
        out = torch.empty(q.shape, dtype=q.dtype, device=dev)
        stats = torch.empty(d.windows, d.heads, d.nq, dtype=torch.float32, device=dev) if want_stats else None
        d.out, d.stats = out.data_ptr(), None if stats is None else stats.data_ptr()
        check(getattr(lib(), fns["forward"])(ctypes.byref(d), _stream(dev)), fns["forward"])
    return out, stats


def window_attn_masked_backward(q, k, v, table, index, mask, scale: float, out, stats, grad_out, need=(True, True, True, True), packed=False,
                                grads=None, scratch=None):
    """gsasr_window_attn_masked_backward -> (g_q, g_k, g_v, g_table), None where `need` is False.  `packed`: g_q, g_k, g_v are the
    column blocks of ONE `[W,n,3C]` tensor, written in place through the gradient pitches (all three are then computed).
    `grads`: the caller's own (g_q, g_k, g_v), each of its input's shape and dtype, contiguous or a view with unit column stride
    and one row pitch (which goes into the descriptor), or None where none is wanted: written in place and returned; only
    `need[3]` is then looked at.  `scratch`: the caller's uint8 tensor of gsasr_window_attn_masked[_bf16]_scratch_bytes()"""
    d, fns = _masked_desc(q, k, v, table, index, mask, scale)
    C = int(q.shape[2])
    if grads is not None:
        if packed:
            raise RuntimeError("`grads` and `packed` exclude each other")
        grads = list(grads)
        if len(grads) != 3:
            raise RuntimeError("`grads` must be (g_q, g_k, g_v), None where none is wanted")
        for field, g, t in zip(("gq", "gk", "gv"), grads, (q, k, v)):
            if g is None:
                continue
            pitch = _rows_view(g, "g_" + field[1], q.dtype == torch.bfloat16)
            if g.shape != t.shape or g.device != t.device:
                raise RuntimeError(f"g_{field[1]} must have {field[1]}'s shape {tuple(t.shape)} on its device (got {tuple(g.shape)})")
            setattr(d, "pitch_" + field, pitch)
    elif packed:
        if k.shape != q.shape:
            raise RuntimeError("a packed gradient needs nq == nk")
        whole = torch.empty(q.shape[0], q.shape[1], 3 * C, dtype=q.dtype, device=q.device)
        grads = [whole[..., :C], whole[..., C:2 * C], whole[..., 2 * C:]]
        d.pitch_gq = d.pitch_gk = d.pitch_gv = 3 * C
    else:
        grads = [torch.empty(t.shape, dtype=t.dtype, device=t.device) if n else None for t, n in zip((q, k, v), need)]
    g_table = torch.empty_like(table) if need[3] else None
    _attn_backward(d, fns, out, out, stats, grad_out, scratch, g_q=grads[0], g_k=grads[1], g_v=grads[2], g_table=g_table)
    return (whole, g_table) if packed else (*grads, g_table)


# ---- the decoder's window attention with a rotary embedding (include/gsasr_splat.h: gsasr_window_attn_rope) -----
def window_attn_rope_forward(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, angles: torch.Tensor, scale: float, want_stats: bool = True):
    """gsasr_window_attn_rope_forward: `q` `[W,nq,H*d]`, `k`, `v` `[W,nk,H*d]`, `angles` `[H,N,d/2]` fp32 contiguous ->
    (out `[W,nq,H*d]`, the rows' log-sum-exp `[W,H,nq]` or None, the (cos, sin) table `[H,N,d/2,2]` the backward reads).  bf16
    `q`, `k`, `v`: gsasr_window_attn_rope_bf16_forward, `out` bf16"""
    d, fns = _attn_desc(q, k, v, angles, True, scale)
    cossin = torch.empty(*angles.shape, 2, dtype=torch.float32, device=q.device)
    d.cossin = cossin.data_ptr()
    return (*_attn_forward(d, fns, q, want_stats), cossin)


def window_attn_rope_backward(q, k, v, angles, scale: float, out, stats, cossin, grad_out, need=(True, True, True, True), scratch=None):
    """gsasr_window_attn_rope_backward -> (g_q, g_k, g_v, g_angles), None where `need` is False (the angle gradient is formed
    from g_q and g_k: both are computed for it, and dropped here when not needed themselves).  `scratch`: the caller's uint8
    tensor of gsasr_window_attn_rope[_bf16]_scratch_bytes()"""
    d, fns = _attn_desc(q, k, v, angles, True, scale)
    d.cossin = _chk(cossin, "cossin")
    if tuple(cossin.shape) != (*angles.shape, 2):
        raise RuntimeError("out / grad_out must have q's shape, stats [W,H,nq] and cossin angles' shape + [2]")
    make = (need[0] or need[3], need[1] or need[3], need[2], need[3])
    grads = [torch.empty_like(t) if n else None for t, n in zip((q, k, v, angles), make)]
    _attn_backward(d, fns, q, out, stats, grad_out, scratch, **dict(zip(("g_q", "g_k", "g_v", "g_angles"), grads)))
    return tuple(g if n else None for g, n in zip(grads, need))


# ---- validation metrics of an 8-bit picture (include/gsasr_splat.h: gsasr_metrics) -----------------------------
def make_metrics(batch: int, h: int, w: int, sizes=None, crop_border: int = 0, flags: int = METRIC_PSNR | METRIC_SSIM,
                 img_pitch: Optional[int] = None, img_stride: Optional[int] = None, ref_pitch: Optional[int] = None,
                 ref_stride: Optional[int] = None) -> Metrics:
    """a gsasr_metrics descriptor without pointers (dense pitches and strides unless given); `sizes`: the (h_b, w_b) of every
    sample, None = all h x w"""
    d = Metrics(int(batch), int(h), int(w))
    d.img_pitch = 3 * int(w) if img_pitch is None else int(img_pitch)
    d.ref_pitch = 3 * int(w) if ref_pitch is None else int(ref_pitch)
    d.img_stride = int(h) * d.img_pitch if img_stride is None else int(img_stride)
    d.ref_stride = int(h) * d.ref_pitch if ref_stride is None else int(ref_stride)
    d.crop_border, d.flags = int(crop_border), int(flags)
    if sizes is not None:
        if len(sizes) != batch:
            raise RuntimeError("sizes must hold one (h, w) per sample")
        d._hw = (ctypes.c_int * (2 * batch))(*[int(v) for hw in sizes for v in hw])     # kept alive by the descriptor
        d.sample_hw = ctypes.cast(d._hw, ctypes.POINTER(ctypes.c_int))
    return d


def _u8_picture(t: torch.Tensor, name: str):
    """a uint8 CUDA `[h,w,3]` or `[B,h,w,3]` tensor whose innermost `[w,3]` is dense and whose row and sample strides are not
    negative -> (pointer, pitch, stride) in bytes"""
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.uint8:
        raise RuntimeError(f"{name} must be a uint8 CUDA tensor")
    if t.dim() not in (3, 4) or t.shape[-1] != 3:
        raise RuntimeError(f"{name} has shape {tuple(t.shape)}, expected [h,w,3] or [B,h,w,3]")
    st = t.stride()
    dense = st[-1] == 1 and (st[-2] == 3 or t.shape[-2] == 1)              # (the stride of an extent of 1 is never used)
    rows_apart = st[-3] >= 3 * t.shape[-2] or t.shape[-3] == 1
    if not dense or not rows_apart or (t.dim() == 4 and st[0] < 0):
        raise RuntimeError(f"{name} has strides {st}: the innermost [w,3] must be dense and rows at least 3 * w bytes apart")
    return t.data_ptr(), (st[-3] if t.shape[-3] > 1 else 3 * t.shape[-2]), (st[0] if t.dim() == 4 else 0)


def image_metrics(img: torch.Tensor, ref: torch.Tensor, sizes=None, crop_border: int = 0, y_channel: bool = False, bgr: bool = False,
                  psnr: bool = True, ssim: bool = True, out: Optional[torch.Tensor] = None,
                  scratch: Optional[torch.Tensor] = None) -> torch.Tensor:
    """gsasr_image_metrics: `img`, `ref` uint8 `[h,w,3]` or `[B,H,W,3]` (windows of larger tensors are taken through their
    strides), `sizes` the samples' own (h_b, w_b) -> float64 `[B,2]` = {psnr, ssim} per sample on the device, no
    synchronisation.  A metric that is not asked for leaves its column as it is (`out`: the caller's tensor; else zeros).
    `scratch`: the caller's uint8 tensor of gsasr_metrics_scratch_bytes()."""
    pi, ip, istr = _u8_picture(img, "img")
    pr, rp, rstr = _u8_picture(ref, "ref")
    if img.shape != ref.shape or img.device != ref.device:
        raise RuntimeError(f"img {tuple(img.shape)} and ref {tuple(ref.shape)} must have the same shape and device")
    B = img.shape[0] if img.dim() == 4 else 1
    h, w, dev = int(img.shape[-3]), int(img.shape[-2]), img.device
    flags = (METRIC_PSNR if psnr else 0) | (METRIC_SSIM if ssim else 0) | (METRIC_Y if y_channel else 0) | (METRIC_BGR if bgr else 0)
    d = make_metrics(B, h, w, sizes, crop_border, flags, ip, istr, rp, rstr)
    n = int(lib().gsasr_metrics_scratch_bytes(ctypes.byref(d)))
    if n == 0:
        check(-1, "gsasr_metrics_scratch_bytes")
    with _on(dev):
        if out is None:
            out = torch.empty(B, 2, dtype=torch.float64, device=dev) if psnr and ssim else torch.zeros(B, 2, dtype=torch.float64, device=dev)
        elif not (out.is_cuda and out.dtype == torch.float64 and out.is_contiguous() and tuple(out.shape) == (B, 2) and out.device == dev):
            raise RuntimeError(f"out must be a contiguous float64 [{B}, 2] tensor on the pictures' device")
        if scratch is None:
            scratch = torch.empty(n // 8, dtype=torch.float64, device=dev)
            ps = scratch.data_ptr()
        else:
            ps = _own_scratch(scratch, n, dev, "gsasr_metrics_scratch_bytes")
        d.img, d.ref, d.out, d.scratch = pi, pr, out.data_ptr(), ps
        check(lib().gsasr_image_metrics(ctypes.byref(d), _stream(dev)), "gsasr_image_metrics")
    return out


# ---- bicubic imresize (include/gsasr_splat.h: gsasr_resize) ------------------------------------------------------
def make_resize(batch: int, channels: int, in_h: int, in_w: int, out_h: int, out_w: int, scales, sizes=None, flags: int = 0) -> Resize:
    """a gsasr_resize descriptor without pointers, dense pitches and strides; `scales`: one (scale_h, scale_w) for all samples or
    one per sample; `sizes`: the (h_b, w_b) of every sample, None = all in_h x in_w"""
    d = Resize(int(batch), int(channels), int(in_h), int(in_w))
    d.out_h, d.out_w = int(out_h), int(out_w)
    d.in_pitch, d.out_pitch = 4 * int(in_w), 4 * int(out_w)
    d.in_plane, d.out_plane = int(in_h) * d.in_pitch, int(out_h) * d.out_pitch
    d.in_stride, d.out_stride = int(channels) * d.in_plane, int(channels) * d.out_plane
    flat = [float(v) for v in scales] if not isinstance(scales[0], (tuple, list)) else [float(v) for sc in scales for v in sc]
    if len(flat) == 2:
        flags |= RESIZE_SHARED_SCALE
    elif len(flat) != 2 * batch:
        raise RuntimeError("scales must hold one (scale_h, scale_w) pair, or one per sample")
    d._sc = (ctypes.c_double * len(flat))(*flat)      # kept alive by the descriptor
    d.scales = ctypes.cast(d._sc, ctypes.POINTER(ctypes.c_double))
    if sizes is not None:
        if len(sizes) != batch:
            raise RuntimeError("sizes must hold one (h, w) per sample")
        d._hw = (ctypes.c_int * (2 * batch))(*[int(v) for hw in sizes for v in hw])
        d.sample_hw = ctypes.cast(d._hw, ctypes.POINTER(ctypes.c_int))
    d.flags = int(flags)
    return d


def _planar(t: torch.Tensor, name: str):
    """an fp32 CUDA `[B,C,h,w]` tensor whose rows are dense and whose strides are not negative -> (pointer, pitch, plane, stride) in bytes"""
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32 or t.dim() != 4:
        raise RuntimeError(f"{name} must be a float32 CUDA tensor [B,C,h,w]")
    st = t.stride()
    if (st[3] != 1 and t.shape[3] > 1) or (st[2] < t.shape[3] and t.shape[2] > 1) or st[0] < 0 or st[1] < 0:
        raise RuntimeError(f"{name} has strides {st}: rows must be dense and at least w elements apart")
    return t.data_ptr(), 4 * (st[2] if t.shape[2] > 1 else t.shape[3]), 4 * st[1], 4 * st[0]


def imresize(x: torch.Tensor, out: torch.Tensor, scales, sizes=None, antialiasing: bool = True, backward: bool = False,
             accumulate: bool = False, scratch: Optional[torch.Tensor] = None) -> torch.Tensor:
    """gsasr_imresize: `x` fp32 `[B,C,H,W]` -> `out` `[B,C,out_h,out_w]` (windows of larger tensors are taken through their
    strides); `scales`: (scale_h, scale_w), or one pair per sample; `sizes`: the samples' own (h_b, w_b) in their H x W slot.
    `backward`: gsasr_imresize_backward -- `out` is read as grad_out and `x` written (`accumulate`: added to) as grad_in, on the
    samples' own pixels only.  Returns the tensor written.  On the current stream; scratch from torch unless given."""
    px, d_in = _planar(x, "x"), None
    po = _planar(out, "out")
    if x.shape[:2] != out.shape[:2] or x.device != out.device:
        raise RuntimeError(f"x {tuple(x.shape)} and out {tuple(out.shape)} must agree on [B,C] and the device")
    B, C, H, W = (int(v) for v in x.shape)
    dev = x.device
    flags = (0 if antialiasing else RESIZE_NO_ANTIALIAS) | (RESIZE_ACCUMULATE if accumulate else 0)
    d = make_resize(B, C, H, W, int(out.shape[2]), int(out.shape[3]), scales, sizes, flags)
    d.in_pitch, d.in_plane, d.in_stride = px[1:]
    d.out_pitch, d.out_plane, d.out_stride = po[1:]
    n = int(lib().gsasr_resize_scratch_bytes(ctypes.byref(d)))
    if n == 0:
        check(-1, "gsasr_resize_scratch_bytes")
    with _on(dev):
        if scratch is None:
            scratch = torch.empty(n // 4, dtype=torch.float32, device=dev)
        elif _chk(scratch, "scratch") == 0 or 4 * scratch.numel() < n or scratch.device != dev:
            raise RuntimeError("scratch is smaller than gsasr_resize_scratch_bytes()")
        d.inp, d.out, d.scratch = px[0], po[0], scratch.data_ptr()
        if backward:
            check(lib().gsasr_imresize_backward(ctypes.byref(d), _stream(dev)), "gsasr_imresize_backward")
        else:
            check(lib().gsasr_imresize(ctypes.byref(d), _stream(dev)), "gsasr_imresize")
    return x if backward else out


# ---- training batches from decoded images (include/gsasr_splat.h: gsasr_batch) -----------------------------------
def make_batch_desc(srcs, src_hw, windows, aug=None, gt_hw=(0, 0), lr_hw=(0, 0), flags: int = 0) -> Batch:
    """a gsasr_batch descriptor without gt / lq / scratch: `srcs` device addresses, `src_hw` (h, w) and `windows`
    (y0, x0, gh, gw) per sample, `aug` one byte of BATCH_HFLIP | _VFLIP | _TRANSPOSE per sample or None"""
    n = len(srcs)
    if len(src_hw) != n or len(windows) != n or (aug is not None and len(aug) != n):
        raise RuntimeError("one source, (h, w), window and augmentation per sample")
    d = Batch(n)
    # (NumPy packs the host arrays in one conversion each; the descriptor keeps them alive)
    d._src = np.array([int(p) if p else 0 for p in srcs] or [0], dtype=np.uint64)
    d._hw = np.ascontiguousarray(np.array(src_hw if n else [(0, 0)], dtype=np.int32).reshape(-1, 2))
    d._win = np.ascontiguousarray(np.array(windows if n else [(0, 0, 0, 0)], dtype=np.int32).reshape(-1, 4))
    d.src = ctypes.cast(d._src.ctypes.data, ctypes.POINTER(ctypes.c_void_p))
    d.src_hw = ctypes.cast(d._hw.ctypes.data, ctypes.POINTER(ctypes.c_int))
    d.window = ctypes.cast(d._win.ctypes.data, ctypes.POINTER(ctypes.c_int))
    if aug is not None:
        d._aug = np.array(list(aug) or [0], dtype=np.uint8)
        d.aug = ctypes.cast(d._aug.ctypes.data, ctypes.POINTER(ctypes.c_ubyte))
    d.gt_h, d.gt_w = int(gt_hw[0]), int(gt_hw[1])
    d.lr_h, d.lr_w = int(lr_hw[0]), int(lr_hw[1])
    d.flags = int(flags)
    return d


def _sources(images):
    """uint8 CUDA tensors `[h,w,3]`, contiguous, on one device -> (device, addresses, sizes)"""
    dev = images[0].device
    for t in images:
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.uint8 and t.dim() == 3 and t.shape[2] == 3
                and t.is_contiguous() and t.device == dev):
            raise RuntimeError("images must be contiguous uint8 CUDA tensors [h,w,3] on one device")
    return dev, [t.data_ptr() for t in images], [(int(t.shape[0]), int(t.shape[1])) for t in images]


def batch_make(images, windows, aug, gt: Optional[torch.Tensor], lq: torch.Tensor, bgr: bool = True, antialiasing: bool = True,
               scratch: Optional[torch.Tensor] = None):
    """gsasr_batch_make: windows of the uint8 `images` -> `gt` fp32 `[B,3,Gh,Gw]` (augmented, zero-padded; None: not made) and
    `lq` fp32 `[B,3,lh,lw]` (bicubic LR of the un-augmented window, then augmented), both written.  On the current stream;
    scratch (a uint8 tensor of gsasr_batch_scratch_bytes()) from torch unless given."""
    dev, ptrs, hw = _sources(images)
    return _batch_make(dev, ptrs, hw, windows, aug, gt, lq, bgr, antialiasing, scratch)


def _batch_make(dev, ptrs, hw, windows, aug, gt, lq, bgr=True, antialiasing=True, scratch=None):
    """`batch_make` on sources that are already checked: their device, addresses and (h, w)"""
    B = len(ptrs)
    pg, pl = None if gt is None else _chk(gt, "gt"), _chk(lq, "lq")
    if lq.dim() != 4 or tuple(lq.shape[:2]) != (B, 3) or lq.device != dev:
        raise RuntimeError(f"lq {tuple(lq.shape)} must be [{B},3,h,w] on the images' device")
    if gt is not None and (gt.dim() != 4 or tuple(gt.shape[:2]) != (B, 3) or gt.device != dev):
        raise RuntimeError(f"gt {tuple(gt.shape)} must be [{B},3,h,w] on the images' device")
    flags = (BATCH_BGR if bgr else 0) | (0 if antialiasing else BATCH_NO_ANTIALIAS)
    gt_hw = gt.shape[2:] if gt is not None else (max(max(wd[2], wd[3]) for wd in windows),) * 2     # (any slot that holds the samples)
    d = make_batch_desc(ptrs, hw, windows, aug, gt_hw, lq.shape[2:], flags)
    n = int(lib().gsasr_batch_scratch_bytes(ctypes.byref(d)))
    if n == 0:
        check(-1, "gsasr_batch_scratch_bytes")
    with _on(dev):
        if scratch is None:
            scratch = torch.empty(n, dtype=torch.uint8, device=dev)
        elif not (isinstance(scratch, torch.Tensor) and scratch.is_cuda and scratch.dtype == torch.uint8 and scratch.is_contiguous()
                  and scratch.numel() >= n and scratch.device == dev):
            raise RuntimeError("scratch must be a contiguous uint8 tensor of at least gsasr_batch_scratch_bytes() on the images' device")
        d.gt, d.lq, d.scratch = pg, pl, scratch.data_ptr()
        check(lib().gsasr_batch_make(ctypes.byref(d), _stream(dev)), "gsasr_batch_make")
    return gt, lq


def batch_pick(images, windows, aug, points: torch.Tensor, out: torch.Tensor, bgr: bool = True) -> torch.Tensor:
    """gsasr_batch_pick: `out` fp32 `[B,3,S]` = the augmented windows at the int32 `points` `[B,S,2]` = (row, column)"""
    dev, ptrs, hw = _sources(images)
    return _batch_pick(dev, ptrs, hw, windows, aug, points, out, bgr)


def _batch_pick(dev, ptrs, hw, windows, aug, points, out, bgr=True):
    """`batch_pick` on sources that are already checked"""
    B = len(ptrs)
    if not (isinstance(points, torch.Tensor) and points.is_cuda and points.dtype == torch.int32 and points.is_contiguous()
            and points.dim() == 3 and points.shape[0] == B and points.shape[2] == 2 and points.device == dev):
        raise RuntimeError(f"points must be a contiguous int32 tensor [{B},S,2] on the images' device")
    S = int(points.shape[1])
    if _chk(out, "out") == 0 or tuple(out.shape) != (B, 3, S) or out.device != dev:
        raise RuntimeError(f"out must be a contiguous float32 tensor [{B},3,{S}] on the images' device")
    d = make_batch_desc(ptrs, hw, windows, aug, flags=BATCH_BGR if bgr else 0)
    with _on(dev):
        check(lib().gsasr_batch_pick(ctypes.byref(d), points.data_ptr(), S, out.data_ptr(), _stream(dev)), "gsasr_batch_pick")
    return out


# ---- sampled pixels ----------------------------------------------------------------
def _points(points: torch.Tensor, batch: int, device) -> Tuple[torch.Tensor, int]:
    """`[S,2]` (one image) or `[B,S,2]` (batched canvas) integer (row, column) pairs -> contiguous int32 on `device`."""
    if not (isinstance(points, torch.Tensor) and not points.dtype.is_floating_point and points.dtype != torch.bool
            and points.shape[-1:] == (2,) and points.dim() == (3 if batch > 1 else 2)
            and (batch <= 1 or points.shape[0] == batch)):
        raise RuntimeError("points must be an integer tensor [S,2] (or [B,S,2] for a batched canvas)")
    return points.to(device=device, dtype=torch.int32).contiguous(), int(points.shape[-2])


def _query_points(points: torch.Tensor, batch: int, device) -> Tuple[torch.Tensor, int]:
    """`[S,2]` (one image) or `[B,S,2]` (batched canvas) floating-point (r, c) pairs -> contiguous float32 on `device`."""
    if not (isinstance(points, torch.Tensor) and points.dtype.is_floating_point
            and points.shape[-1:] == (2,) and points.dim() == (3 if batch > 1 else 2)
            and (batch <= 1 or points.shape[0] == batch)):
        raise RuntimeError("query points must be a floating-point tensor [S,2] (or [B,S,2] for a batched canvas)")
    return points.detach().to(device=device, dtype=torch.float32).contiguous(), int(points.shape[-2])


def _fresh_ws(nbytes: int, dev) -> torch.Tensor:
    """a plan workspace that is not pooled (the sampled and query step forms).  The one place where it is allocated:
    tests/test_workspace_bounds_gpu.py replaces this function to put the workspace between guards (keep it a function of its own)"""
    return torch.empty(nbytes, dtype=torch.uint8, device=dev)


def _sample_ws(d: Dims, n_points: int, dev) -> torch.Tensor:
    nbytes = lib().gsasr_sample_workspace_bytes(ctypes.byref(d), n_points)
    if nbytes == 0:
        check(-1, "gsasr_sample_workspace_bytes")
    return torch.empty(nbytes, dtype=torch.uint8, device=dev)


def sample_forward(p: Plan, points: torch.Tensor, _query: bool = False, sample_ws: Optional[torch.Tensor] = None):
    """values of the splat at `points` only: `[3,S]` (`[B,3,S]` on a batched canvas) + the state for `sample_backward`.
    `sample_ws`: the caller's uint8 tensor of gsasr_sample_workspace_bytes(), which the state then carries to the backward."""
    B = max(int(p.dims.batch), 1)
    pts, n = (_query_points if _query else _points)(points, B, p.device)
    name = "gsasr_splat_query_forward" if _query else "gsasr_splat_sample_forward"
    with _on(p.device):
        if sample_ws is None:
            sws = _sample_ws(p.dims, n, p.device)
        else:
            sws = sample_ws
            need = int(lib().gsasr_sample_workspace_bytes(ctypes.byref(p.dims), n))
            if need == 0:
                check(-1, "gsasr_sample_workspace_bytes")
            _own_scratch(sws, need, p.device, "gsasr_sample_workspace_bytes")
        out = torch.empty((B, 3, n) if B > 1 else (3, n), dtype=torch.float32, device=p.device)
        check(getattr(lib(), name)(ctypes.byref(p.dims), p.workspace.data_ptr(), p.workspace.numel(),
                                   pts.data_ptr(), n, out.data_ptr(), sws.data_ptr(), sws.numel(),
                                   _stream(p.device)), name)
    return out, (pts, n, sws)


def query_forward(p: Plan, points: torch.Tensor, sample_ws: Optional[torch.Tensor] = None):
    """values of the splat at fractional pixel positions: `points` float `[S,2]` (r, c) on the image's own grid (`[B,S,2]` on a
    batched canvas) -> `[3,S]` (`[B,3,S]`) + the state for `query_backward`.  `p`: a plan made with `flags=FLAG_CONTINUOUS`."""
    return sample_forward(p, points, _query=True, sample_ws=sample_ws)


def query_backward(p: Plan, state, sigmas, coords, colors, grad_out, g_sigmas, g_coords, g_colors,
                   overwrite: bool = False, resort: bool = False) -> None:
    """g_* (+)= gradient of sum(grad_out * query_forward(...)) w.r.t. the Gaussians; `state` is what `query_forward` returned."""
    sample_backward(p, state, sigmas, coords, colors, grad_out, g_sigmas, g_coords, g_colors, overwrite, resort, _query=True)


def sample_backward(p: Plan, state, sigmas, coords, colors, grad_out, g_sigmas, g_coords, g_colors,
                    overwrite: bool = False, resort: bool = False, _query: bool = False) -> None:
    """g_* (+)= gradient of sum(grad_out * sample_forward(...)); `state` is what `sample_forward` returned."""
    pts, n, sws = state
    B = max(int(p.dims.batch), 1)
    ptrs = [_chk(sigmas, "sigmas", (3,)), _chk(coords, "coords", (2,)), _chk(colors, "colors", (3,)),
            _chk(grad_out, "grad_out", (3, n)), _chk(g_sigmas, "grads_sigmas", (3,)),
            _chk(g_coords, "grads_coords", (2,)), _chk(g_colors, "grads_colors", (3,))]
    if grad_out.numel() != B * 3 * n:
        raise RuntimeError("grad_out does not match the points")
    d = _dims_with(p, FLAG_OVERWRITE_GRADS if overwrite else 0)
    name = "gsasr_splat_query_backward" if _query else "gsasr_splat_sample_backward"
    with _on(p.device):
        check(getattr(lib(), name)(*ptrs, ctypes.byref(d), p.workspace.data_ptr(), p.workspace.numel(),
                                   pts.data_ptr() if resort else None, n, sws.data_ptr(), sws.numel(),
                                   _stream(p.device)), name)


def step_sample_forward(gs_parameters: torch.Tensor, step: Optional[torch.Tensor], h: int, w: int, dmax: Optional[float],
                        points: torch.Tensor, scale_modify: Optional[torch.Tensor] = None, default_step_size: float = 1.2):
    """prologue + plan + sampled forward in ONE call: raw `gs_parameters[N,9]` -> `[3,S]` (step size as in `step_forward`)."""
    pp, src = _step_args(gs_parameters, step, scale_modify, default_step_size)
    shape = _image_shape(_STEP_BYTES, gs_parameters.shape[0], int(h), int(w), dmax, 0)
    return _step_sampled(shape, pp, src, points, gs_parameters.device)


def batch_sample_forward(gs_parameters: torch.Tensor, steps: torch.Tensor, sizes, dmax: Optional[float],
                         points: torch.Tensor):
    """the same for a whole batch: `gs_parameters` [B,N,9], `points` [B,S,2] on each sample's own grid -> `[B,3,S]`."""
    pp, src = _step_args(gs_parameters, steps, None, 1.2, sizes)
    return _step_sampled(_canvas_shape(gs_parameters.shape[1], sizes, dmax, 0), pp, src, points, gs_parameters.device)


def step_query_forward(gs_parameters: torch.Tensor, step: Optional[torch.Tensor], h: int, w: int, dmax: Optional[float],
                       points: torch.Tensor, scale_modify: Optional[torch.Tensor] = None, default_step_size: float = 1.2):
    """`step_sample_forward` at fractional pixel positions: `points` float `[S,2]` (r, c) -> `[3,S]` (the library plans with
    GSASR_FLAG_CONTINUOUS itself)."""
    pp, src = _step_args(gs_parameters, step, scale_modify, default_step_size)
    shape = _image_shape(_STEP_BYTES, gs_parameters.shape[0], int(h), int(w), dmax, 0)
    return _step_sampled(shape, pp, src, points, gs_parameters.device, _STEP_QUERY)


def batch_query_forward(gs_parameters: torch.Tensor, steps: torch.Tensor, sizes, dmax: Optional[float],
                        points: torch.Tensor):
    """the same for a whole batch: `gs_parameters` [B,N,9], `points` float [B,S,2] on each sample's own grid -> `[B,3,S]`."""
    pp, src = _step_args(gs_parameters, steps, None, 1.2, sizes)
    return _step_sampled(_canvas_shape(gs_parameters.shape[1], sizes, dmax, 0), pp, src, points, gs_parameters.device, _STEP_QUERY)


def _step_sampled(shape, pp: int, src, points: torch.Tensor, dev, names=None):
    """prologue + plan + sampled forward (`_step_planar`'s sibling; these plans take a fresh workspace each)"""
    d, nbytes = shape[0][0], shape[1]
    B = max(int(d.batch), 1)
    names = names or _STEP_SAMPLE
    pts, n = (_query_points if names is _STEP_QUERY else _points)(points, B, dev)
    with _on(dev):
        ws = _fresh_ws(nbytes, dev)
        sws = _sample_ws(d, n, dev)
        out = torch.empty((B, 3, n) if B > 1 else (3, n), dtype=torch.float32, device=dev)
        _step_call(names, pp, src, d, ws, nbytes, pts.data_ptr(), n, out.data_ptr(), sws.data_ptr(), sws.numel(), _stream(dev))
    return out, Plan(d, ws, dev), (pts, n, sws)


def step_query_backward(p: Plan, state, gs_parameters: torch.Tensor, step: torch.Tensor, grad_out: torch.Tensor) -> torch.Tensor:
    """query backward + prologue backward in ONE call (`step_sample_backward`'s twin for `step_query_forward` / `batch_query_forward`)"""
    return step_sample_backward(p, state, gs_parameters, step, grad_out, _name="gsasr_step_query_backward")


def step_sample_backward(p: Plan, state, gs_parameters: torch.Tensor, step: torch.Tensor,
                         grad_out: torch.Tensor, _name: str = "gsasr_step_sample_backward") -> torch.Tensor:
    """sampled backward + prologue backward in ONE call; returns d/d gs_parameters (`[N,9]` or `[B,N,9]`)."""
    pts, n, sws = state
    pp = _chk(gs_parameters, "gs_parameters", (9,))
    ps = None if step is None else _chk(step, "step_size")      # None: the step sizes the forward's prologue used
    pg = _chk(grad_out, "grad_out", (3, n))
    if grad_out.numel() != max(int(p.dims.batch), 1) * 3 * n:
        raise RuntimeError("grad_out does not match the points")
    with _on(p.device):
        gp = torch.empty_like(gs_parameters)
        check(getattr(lib(), _name)(pp, ps, pg, gp.data_ptr(), ctypes.byref(p.dims), p.workspace.data_ptr(),
                                    p.workspace.numel(), None, n, sws.data_ptr(), sws.numel(),
                                    _stream(p.device)), _name)
    return gp


def query_backward_points(p: Plan, state, grad_out: torch.Tensor, resort: bool = False,
                          _name: str = "gsasr_splat_query_backward_points") -> torch.Tensor:
    """gradient of sum(grad_out * query_forward(...)) w.r.t. the POSITIONS: float32 `[S,2]` (`[B,S,2]`) of (d/dr, d/dc), every row
    written (a point outside the domain: zeros).  `state` is what `query_forward` returned; `p` may be a FLAG_FORWARD_ONLY plan."""
    pts, n, sws = state
    B = max(int(p.dims.batch), 1)
    pg = _chk(grad_out, "grad_out", (3, n))
    if grad_out.numel() != B * 3 * n:
        raise RuntimeError("grad_out does not match the points")
    with _on(p.device):
        gpts = torch.empty((B, n, 2) if B > 1 else (n, 2), dtype=torch.float32, device=p.device)
        check(getattr(lib(), _name)(ctypes.byref(p.dims), p.workspace.data_ptr(), p.workspace.numel(), pg,
                                    pts.data_ptr() if resort else None, n, gpts.data_ptr(), sws.data_ptr(), sws.numel(),
                                    _stream(p.device)), _name)
    return gpts


def step_query_backward_points(p: Plan, state, grad_out: torch.Tensor) -> torch.Tensor:
    """`query_backward_points` on the plan of `step_query_forward` / `batch_query_forward` (needs no gs_parameters)"""
    return query_backward_points(p, state, grad_out, _name="gsasr_step_query_backward_points")


def set_default_cutoff(tau: float) -> None:
    """tau > 0: skip exponent < -tau; tau < 0: never skip; 0 restores the adaptive default ln(N/1e-5)."""
    lib().gsasr_set_default_cutoff(float(tau))


def get_default_cutoff() -> float:
    return float(lib().gsasr_get_default_cutoff())


def plan_cutoff(p: Plan) -> Tuple[float, int]:
    """(tau, K) the windows of plan `p` were built with: for the bounded op under the adaptive default tau is data-derived,
    ln(K / 1e-5) with K = the plan's own bound on how many dmax boxes cover one pixel (include/gsasr_splat.h); K = 0
    otherwise.  Synchronises the stream: for reports and tests."""
    tau, k = ctypes.c_float(0.0), ctypes.c_uint(0)
    with _on(p.device):
        check(lib().gsasr_plan_cutoff(ctypes.byref(p.dims), p.workspace.data_ptr(), p.workspace.numel(), _stream(p.device),
                                      ctypes.byref(tau), ctypes.byref(k)), "gsasr_plan_cutoff")
    return float(tau.value), int(k.value)


def resolve_cutoff(cutoff: float, s: int) -> float:
    """tau a plan with `cutoff` (0 = process default) over `s` Gaussians uses."""
    return float(lib().gsasr_resolve_cutoff(float(cutoff), int(s)))


# ---- kernel choices registered per shape (include/gsasr_splat.h: gsasr_set_kernel_choice; gsasr_amd/tune.py measures them) ----
CHOICE_FLAGS = FLAG_FWD_WIDE | FLAG_FWD_NARROW | FLAG_BWD_TILE | FLAG_BWD_GAUSSIAN | FLAG_BWD_HOME


_N_CHOICES = 0      # registrations made through this module since the last clear (0 = the fused host path skips its lookup)


def kernel_choices_registered() -> bool:
    return _N_CHOICES > 0


def set_kernel_choice(shape: Dims, flags: int, list_cap: int = 0) -> None:
    """Register the kernel choice for plans of `shape` (a Dims as `make_dims` / `make_batch_dims` builds them; only its shape
    fields and FLAG_FORWARD_ONLY are read).  Later calls without an explicit choice of their own follow it."""
    global _N_CHOICES
    check(lib().gsasr_set_kernel_choice(ctypes.byref(shape), int(flags), int(list_cap)), "gsasr_set_kernel_choice")
    _N_CHOICES += 1
    _SHAPES.clear()      # workspace sizes follow the registered choice


def get_kernel_choice(shape: Dims) -> Optional[Tuple[int, int]]:
    f, c = ctypes.c_uint(0), ctypes.c_int(0)
    if not lib().gsasr_get_kernel_choice(ctypes.byref(shape), ctypes.byref(f), ctypes.byref(c)):
        return None
    return int(f.value), int(c.value)


def clear_kernel_choices() -> None:
    global _N_CHOICES
    lib().gsasr_clear_kernel_choices()
    _N_CHOICES = 0
    _SHAPES.clear()
