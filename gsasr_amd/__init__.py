"""gsasr_amd -- MI355X-native 2D Gaussian-splatting rasterizer for GSASR (the one hot path of
ChrisDud0257/GSASR, behind the reference's own autograd/operator surface).

    from gsasr_amd.gaussian_splatting import generate_2D_gaussian_splatting_step   # utils/gaussian_splatting.py
    from gsasr_amd.gs_cuda_dmax.gswrapper import GSCUDA, gaussiansplatting_render  # utils/gs_cuda_dmax/gswrapper.py
    from gsasr_amd.gs_cuda.gswrapper import GSCUDA                                 # utils/gs_cuda/gswrapper.py
    import gsasr_amd.gscuda                                                        # pybind module `gscuda`
    from gsasr_amd.shard import splat_band                                         # multi-GPU row-band shard
    from gsasr_amd import ssim_loss                                                # cri_ssim (SSIMLoss) as one HIP call
    from gsasr_amd import image_metrics, calculate_psnr, calculate_ssim            # val.metrics of the 8-bit picture, on the GPU

    from gsasr_amd import imresize, imresize_new, imresize_batch                   # MATLAB bicubic degradation, batched, differentiable
    from gsasr_amd import make_batch, draw_batch                                   # the dataset's crop / LR / augment / pad, one call on uint8 images
    from gsasr_amd import window_attention, use_hip_attention                      # the Fea2GS decoder's window attention, fused
    from gsasr_amd import window_attention_qkv                                     # ... of a Swin layer: packed qkv, a mask per window
    from gsasr_amd import window_attention_rope                                    # ... of the RoPE decoder (Fea2GS_ROPE_AMP)
    from gsasr_amd import window_attention_bf16_torch, window_attention_rope_bf16_torch   # the contracts of their compute="bf16" mode

The compute lives in gsasr_amd/csrc/splat_{plan,forward,backward,backward_home,step,sampled,shard,ssim,metrics,resize,data,attn,api}.hip (hand-written HIP
for gfx950; csrc/gsasr_splat.hip is the same code as one translation unit for the micro-benchmark) behind the C ABI of
include/gsasr_splat.h; Python only moves pointers.  Build with `python -m gsasr_amd.build`.
"""
__version__ = "0.1.0"


def __getattr__(name):      # (lazily: importing the package alone does not import torch)
    if name == "ssim_loss":
        from .ssim import ssim_loss
        return ssim_loss
    if name in ("image_metrics", "calculate_psnr", "calculate_ssim"):
        from . import metrics
        return getattr(metrics, name)
    if name in ("imresize", "imresize_new", "imresize_batch"):
        from . import resize
        return getattr(resize, name)
    if name in ("make_batch", "draw_batch"):
        from . import data
        return getattr(data, name)
    if name in ("window_attention", "window_attention_rope", "use_hip_attention", "window_attention_bf16_torch",
                "window_attention_rope_bf16_torch", "window_attention_qkv", "window_attention_qkv_torch"):
        from . import attention
        return getattr(attention, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
