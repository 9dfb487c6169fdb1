/*
 * gsasr_splat.h -- C ABI of the MI355X-native 2D Gaussian-splatting rasterizer (libgsasr_splat.so).
 *
 * This is the drop-in boundary for GSASR's rasterizer path.  Every entry point takes plain device
 * pointers, sizes and a HIP stream; there are no torch types.  What each one replaces in the
 * reference (paths relative to the reference tree):
 *
 *   gsasr_gs_render            <- _gs_render            utils/gs_cuda/gs.h:1-10       (gs.cu:64-79)
 *   gsasr_gs_render_backward   <- _gs_render_backward   utils/gs_cuda/gs.h:12-24      (gs.cu:180-198)
 *   gsasr_gs_render_dmax       <- _gs_render            utils/gs_cuda_dmax/gs.h:1-11  (gs.cu:67-83)
 *   gsasr_gs_render_backward_dmax <- _gs_render_backward utils/gs_cuda_dmax/gs.h:13-26 (gs.cu:167-186)
 *
 * i.e. exactly what utils/gs_cuda{,_dmax}/gswrapper.cpp:9-71 binds through pybind11 (`gs_render`,
 * `gs_render_backward`).  The four functions keep the reference argument order and meaning
 * (fp32, contiguous, `rendered_img` accumulated into, dmax-backward `+=` into caller-zeroed
 * outputs, unbounded backward overwrites) and add: the stream to launch on (the reference uses the
 * null stream) and an int status instead of void.
 *
 * The plan API below them is what the PyTorch host code actually uses: it exposes the binning
 * workspace so that forward and backward of one autograd node share it, and the [row0,row1) row
 * band for the multi-GPU HR-tile shard.  INTEGRATION.md shows the reference-side
 * binding.
 *
 * Conventions: all pointers are device pointers valid on the current HIP device (the one exception is the small
 * host array gsasr_dims.sample_hw of a batched canvas); `stream` is a
 * hipStream_t passed as void* (NULL = default stream); calls only enqueue work (no host sync);
 * return 0 on success or a negative gsasr_status / positive hipError_t, with a thread-local message
 * available from gsasr_last_error().  c must be 3 (the reference forward hard-codes stride 3,
 * gs_cuda/gs.cu:58, gs_cuda_dmax/gs.cu:29-31).  h, w >= 2 (the grid is 2*i/(n-1)-1).
 */
#ifndef GSASR_SPLAT_H
#define GSASR_SPLAT_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* the library is built with -fvisibility=hidden: these entry points are everything it exports */
#if defined(__GNUC__) || defined(__clang__)
#define GSASR_API __attribute__((visibility("default")))
#else
#define GSASR_API
#endif

#define GSASR_SPLAT_ABI_VERSION 7 /* 7: GSASR_FLAG_BWD_HOME; 2: gsasr_dims gained batch / slot / sample_hw; 3: grad_rows, the backward flags; 4: the _sm step entry points, step_size = NULL in the step backwards; 5: gsasr_dims.list_cap (tile lists); 6: the kernel-choice registry */

enum gsasr_status {
    GSASR_OK = 0,
    GSASR_ERR_ARG = -1,        /* bad dims / null pointer / c != 3 */
    GSASR_ERR_WORKSPACE = -2,  /* workspace too small or misaligned */
    GSASR_ERR_PLAN = -3        /* workspace does not hold a plan for these dims: the library keeps what each plan decided
                                  about its workspace's layout (slots, tile lists) per workspace address, losslessly, and a
                                  forward / backward on an address it holds no plan of this shape for is refused -- never
                                  laid out from the kernel choice registered at the time of the call.  Re-plan. */
};

/* flags */
#define GSASR_FLAG_OVERWRITE_IMAGE 2u /* forward STORES the splat (img need not be initialised) instead of
                                         accumulating into it; saves the caller's memset and a 12 B/px read */
#define GSASR_FLAG_CHW_IMAGE 8u       /* forward writes img as planar [3, row1-row0, w] (the layout the host API
                                         returns, utils/gaussian_splatting.py:129) instead of [row1-row0, w, 3] */
#define GSASR_FLAG_OVERWRITE_GRADS 4u /* backward STORES the gradients (outputs need not be zeroed) instead
                                         of adding into them */
#define GSASR_FLAG_STRIDE8 16u        /* sigmas/coords/colors AND g_sigmas/g_coords/g_colors are columns of packed
                                         [s,8] records {sx,sy,rho,x,y,r,g,b}: element k of Gaussian i is at
                                         ptr[8*i+k].  Pass base, base+3, base+5 of one array; this is the wire
                                         format of the multi-GPU exchange, so nothing is repacked around it */

#define GSASR_FLAG_CHW_GRAD 32u       /* backward reads grad_img as planar [3, row1-row0, w] (what autograd hands back for the
                                         planar image of GSASR_FLAG_CHW_IMAGE; batched canvas: [B, 3, grad_rows, w]) instead
                                         of [row1-row0, w, 3]: no permute pass in front of the backward.  Tile backward only */
#define GSASR_FLAG_FORWARD_ONLY 64u   /* the plan will not be used by a backward (inference): the workspace carries no backward
                                         records, constants, accumulators, slots or gradient scratch (about half the bytes per
                                         Gaussian) and the plan does not write them; a backward on it is GSASR_ERR_PLAN */
#define GSASR_FLAG_BWD_GAUSSIAN 128u  /* backward kernel choice (default: the library picks): Gaussian-stationary
                                         (one wave per Gaussian sweeping its window through L1/L2) ...              */
#define GSASR_FLAG_BWD_TILE 256u      /* ... or tile-stationary (one workgroup per 32x16-px tile, grad_img staged once
                                         in LDS, deterministic partial-gradient slots + gather).  Set it on the dims the
                                         PLAN is made with: the workspace then carries the slots (32 * 8 or 16 bytes per
                                         Gaussian) and the per-quadrant ellipse spans.  Whether a workspace carries slots
                                         is the PLAN's decision (the library remembers it per workspace): a backward that
                                         asks for this kernel on a plan without slots runs the Gaussian-stationary kernel
                                         instead (with GSASR_FLAG_CHW_GRAD: the atomic variant below) -- never reads slots
                                         that were not written */
#define GSASR_FLAG_BWD_ATOMIC 512u    /* tile-stationary with ONE fp32 atomic set per (tile, Gaussian) instead of the
                                         slots (the measured alternative of DESIGN.md 3c; order-dependent rounding)  */
#define GSASR_FLAG_BWD_HOME 32768u    /* home-tile backward (ABI 7): a workgroup owns the Gaussians BINNED in its tile of plan cells, stages
                                         the tile + a 16-px halo of grad_img once in LDS and finishes each of its Gaussians itself
                                         (items of 8 x 8 px per lane, added in LDS, one write per Gaussian): no slots, no gather, no
                                         atomics, deterministic.  Needs nothing from the plan beyond what the Gaussian-stationary
                                         kernel reads; a Gaussian whose window does not fit the region is swept by a whole wave
                                         (that kernel's code), so any input stays correct.  Interleaved [rows, w, 3] gradients:
                                         with GSASR_FLAG_CHW_GRAD gsasr_splat_backward returns GSASR_ERR_ARG, as it does
                                         when this kernel or the Gaussian-stationary one is the shape's registered choice
                                         and the plan has no slots (the step backwards interleave a planar gradient first
                                         and run the chosen kernel on it).
                                         The default of whole images and batched canvases denser than one Gaussian per two pixels on
                                         at least 1024 tiles of 32 x 16 px (1024^2 at GSASR's 16 per LR pixel: -8..-9% against the
                                         Gaussian-stationary kernel) */
#define GSASR_FLAG_COUNTERS_CLEAN 1024u /* plan: the caller keeps this workspace between plans and promises that the
                                         per-cell counters of the parity given by GSASR_FLAG_PARITY are zero: the plan
                                         skips its memset launch.  Every plan zeroes the OTHER parity's counters on the
                                         side (in its first kernel), so a workspace that was used with parity p is clean
                                         for parity 1-p: alternate the bit plan by plan.  (First use of a workspace: leave
                                         CLEAN off.) */
#define GSASR_FLAG_PARITY 2048u        /* which of the two counter arrays this plan counts in */
#define GSASR_FLAG_CUTOFF_CAP 4096u    /* bounded op with an explicit dims.cutoff: treat it as an UPPER bound -- classes and dead set
                                         use it as given, the windows the data-derived tau' <= cutoff (gsasr_plan_cutoff).  For
                                         callers that must name the conservative tau themselves (the row-band exchange: the
                                         selection of halo Gaussians and the neighbour's plan have to agree on it) */
#define GSASR_FLAG_FWD_WIDE 8192u      /* forward kernel choice (default: the library picks by scale factor and image size): 16 x 16
                                         sub-tiles, four pixels per lane (scale factors from x5 up) ... */
#define GSASR_FLAG_FWD_NARROW 16384u   /* ... or 8 x 16 sub-tiles, two pixels per lane.  Read by gsasr_splat_forward only (the plan
                                         is the same).  _WIDE forces the 16 x 16 kernel on ANY single image (tests, A/B runs),
                                         a batched canvas ignores it; _NARROW leaves the choice among the 8 x 16 kernels to the
                                         image size.  Same sums in a different order: results agree to fp32 rounding */
#define GSASR_FLAG_CONTINUOUS 65536u   /* plan for queries BETWEEN the pixel centres (gsasr_splat_query_*, below): every Gaussian's
                                         window is widened by one pixel on each side before it is found empty or clipped, so
                                         that a point within half a pixel of a pixel centre finds every Gaussian whose support
                                         holds it -- a plain plan drops a Gaussian whose support lies between the centres.
                                         Such a plan serves the query and the sampled-pixel entry points only: it carries no
                                         tile lists and no slots (laid out as with list_cap < 0), looks up no registered kernel
                                         choice, and the image forwards / backwards on it are GSASR_ERR_PLAN.  With a
                                         kernel-choice flag, list_cap > 0, a row band or a view: GSASR_ERR_ARG / a workspace
                                         size of 0.  Part of what the plan IS: every call on the workspace passes it too */

typedef struct gsasr_dims {
    int s;        /* number of Gaussians                                              */
    int h, w;     /* FULL HR grid (pixel centres at 2*i/(n-1)-1, gs.cu:27-28)          */
    int c;        /* channels, must be 3                                              */
    float dmax;   /* < 0: unbounded (gs_cuda);  >= 0: |dx|,|dy| <= dmax box (gs_cuda_dmax) */
    int row0, row1; /* HR rows [row0,row1) owned by this call; 0,h for a single GPU   */
    float cutoff; /* support cutoff tau: a Gaussian is skipped for an 8x8 pixel tile when its
                     exponent is < -tau everywhere on it (|d| > sigma*sqrt(2 tau)).
                     0 -> process default (adaptive, see below); < 0 -> never skip
                     (every in-box term is summed, as the reference does).                */
    unsigned flags;
    /* Batched canvas (the reference splats a training batch sample by sample,
     * basicsr/models/gsasr_model.py:191-233).  All three zero = one image.  With batch = B > 1 the s Gaussians
     * are B samples of s/B each (sample-major) and the "image" is a canvas of B slots stacked vertically:
     * h = B * slot rows (slot a multiple of 16), w columns, row0 = 0, row1 = h.  Sample b has its OWN pixel grid
     * of sample_hw[2b] x sample_hw[2b+1] pixels (each <= slot x w; pixel centres 2i/(n-1)-1 of that size, so every
     * sample is computed exactly as a single-image call would) in the top-left corner of slot b; the rest of
     * the slot is padding (stored as 0 with GSASR_FLAG_OVERWRITE_IMAGE, like the reference's F.pad).  Image
     * layouts: [B*slot, w, 3], or with GSASR_FLAG_CHW_IMAGE [B, 3, slot, w].  Not combinable with row bands. */
    int batch;
    int slot;
    const int *sample_hw; /* HOST array [2*batch]: (h_b, w_b) per sample, read during the call */
    int grad_rows;        /* batched canvas + GSASR_FLAG_CHW_GRAD: rows per plane of grad_img [B, 3, grad_rows, w]
                             (>= every h_b; 0 = slot), so that the [B,3,Hmax,Wmax] gradient autograd returns is read in place */
    int list_cap;         /* tile lists (ABI 5): the plan appends every Gaussian of the normal class to the hit list of each
                             32 x 16-px (wide forward: 32 x 32) tile its ellipse reaches, and the forward renders from those
                             lists instead of searching the cells around each tile.  0 = the library decides: lists for
                             DENSE plans (at least one Gaussian per four pixels -- GSASR's 16 per LR pixel up to x8 -- where
                             they save ~5% of a step), sized four times what GSASR-shaped Gaussians fill, and the search
                             kernels elsewhere (at one Gaussian per LR pixel the plan's list atomics cost more than the
                             search); > 0 = lists with this many entries per tile (rounded up to 64) on any image; < 0 = no
                             lists.  A tile whose list overflows is rendered by the search: same image, only slower.  Part of
                             the workspace layout: pass the same value to every call on a plan */
} gsasr_dims;

#define GSASR_MAX_BATCH 64

/* Default tau is ADAPTIVE and keeps the sum of the skipped terms on any pixel below
 * GSASR_SPLAT_DEFAULT_EPS * max|colour| for ANY input: a bound RELATIVE to the colour scale.  After the host prologue
 * (sigmoid * alpha) colours are <= 1 and the bound is 1e-5 absolute -- an order below the 1e-4 parity tolerance and at the
 * level of fp32 summation noise; the raw op accepts any float as a colour, and there the bound scales with it exactly as the
 * fp32 rounding of the sum itself does (tests/test_hip_parity.py::test_raw_op_colours_far_above_one).  Gradients lose the
 * same tail: relative error ~ tau * exp(-tau) < 1e-7.
 *   conservative   tau = ln(s / eps), clamped to [16, 104]: every skipped term is < exp(-tau) times its colour and at most s
 *                  terms can be skipped on one pixel.  Classes, the dead set and the halo selection of the multi-GPU exchange
 *                  use it.  (s = 65 536 -> 22.6; s = 2^20 -> 25.4.)
 *   data-derived   the WINDOWS are built with tau' = ln(K / budget) <= tau, where K bounds the live Gaussians that can lose
 *                  a non-negligible term on one pixel and is counted on the device from the plan's own cell histogram:
 *                  (largest cell count) x (cells that can hold such a Gaussian) + (large class), the cells being the
 *                  smaller of (a) those a dmax box around a pixel touches (bounded op: utils/gs_cuda_dmax/gs.cu:41-50, only
 *                  a Gaussian whose box covers the pixel adds anything) and (b) those within the class' largest support of
 *                  the pixel (both ops); `budget` is eps minus exp(-tau) for every term of the geometric tail of everything
 *                  farther and for every dead Gaussian whose tails the op would still add to these rows.  Config
 *                  2: K = 336, tau' = 17.3; x8 (config 4): K = 392, tau' = 17.5.  gsasr_plan_cutoff reports both;
 *                  gsasr_amd/csrc/gsasr_splat.hip (adapt_kcut) has the derivation, tests/test_adaptive_cutoff.py the checks
 *                  incl. adversarial inputs (everything stacked on one spot: K ~ s, tau' = tau).
 * A fixed tau can be set per call (dims.cutoff) or per process (gsasr_set_default_cutoff / environment
 * GSASR_SPLAT_CUTOFF) and is used as given (GSASR_FLAG_CUTOFF_CAP: as an upper bound for the data-derived one):
 * tau = 104 (GSASR_SPLAT_EXACT_CUTOFF) skips only terms for which fp32 expf() in the
 * reference returns exactly +0 (exp(-104) < 2^-150), i.e. it sums the same set of non-zero terms as the
 * reference; tau < 0 never skips. */
#define GSASR_SPLAT_DEFAULT_EPS 1e-5f
#define GSASR_SPLAT_EXACT_CUTOFF 104.0f
/* The BACKWARD's own cutoff under the adaptive default (round 6).  The forward's tau' grows with K because the skipped terms of
 * up to K Gaussians add up on ONE pixel (GSASR's 16 Gaussians per LR pixel: K ~ 7 000, tau' = 20.4).  A Gaussian's gradient is a
 * sum over ITS OWN pixels only -- nothing accumulates across Gaussians -- so its window needs no more than the tau at which the
 * integrals themselves are complete: outside the ellipse {exponent >= -tau} lies exp(-tau) of a Gaussian's mass,
 * (2 / sqrt(pi)) sqrt(tau) exp(-tau) of its first and (1 + tau) exp(-tau) of its second moments (the d/dmu, d/dsigma, d/drho
 * integrands): 1.1e-7, 5e-7 and 1.9e-6 at tau = 16 -- the LOWEST value the data-derived tau' of the forward ever takes (sparse
 * plans), i.e. the per-Gaussian gradient accuracy every plan with few Gaussians per pixel has always had.  The
 * Gaussian-stationary and home-tile backward sweep the window of min(tau', GSASR_SPLAT_GRAD_TAU), whatever K is.  (14.3 --
 * "complete to 1e-5" -- was measured first: another 6% on the backward, and on stacked Gaussians 1.3e-5 of the tensor's
 * max-abs on d/dmu, whose odd integrand leaves a signed value far below the unsigned mass the truncation is relative to: no
 * margin under the per-Gaussian parity bar.)  Whole images and batched canvases only (a row band's share of a gradient may be
 * all tail); an explicit cutoff (dims.cutoff, GSASR_SPLAT_CUTOFF) is used as given by both directions. */
#define GSASR_SPLAT_GRAD_TAU 16.0f

GSASR_API int gsasr_abi_version(void);
GSASR_API const char *gsasr_last_error(void);

/* Bytes of scratch the plan needs for these dims (0 on bad dims). 256-byte aligned base required. */
GSASR_API size_t gsasr_splat_workspace_bytes(const gsasr_dims *dims);

/* Bytes of ONE of the workspace's two counter arrays for these dims (0 on bad dims): the per-cell counters, the extent groups
 * and the dead-class counter lines that GSASR_FLAG_COUNTERS_CLEAN speaks of.  The plan header (256 bytes) is followed by the
 * array of parity 0 and then by that of GSASR_FLAG_PARITY.  Read-only; for callers that keep workspaces between plans and want
 * to check, or clear, the array the next plan will count in. */
GSASR_API size_t gsasr_splat_counter_bytes(const gsasr_dims *dims);

/* Bin the Gaussians for [row0,row1) into `workspace` (classify -> scan -> scatter -> pack). */
GSASR_API int gsasr_splat_plan(const float *sigmas /*[s,3]*/, const float *coords /*[s,2]*/,
                     const float *colors /*[s,3]*/, const gsasr_dims *dims, void *workspace,
                     size_t workspace_bytes, void *stream);

/* img[row1-row0, w, 3] += splat (= splat with GSASR_FLAG_OVERWRITE_IMAGE).  `workspace` must hold the
 * plan of the same inputs and dims. */
GSASR_API int gsasr_splat_forward(const gsasr_dims *dims, const void *workspace, size_t workspace_bytes,
                        float *img, void *stream);

/* 8-bit image output (inference: what every caller of the reference does to the float image straight away --
 * x[:, :, :gt_h, :gt_w] -> clamp(0, 1) -> HWC -> (x * 255).round().astype(uint8), basicsr/utils/img_util.py:73-96 -- fused
 * into the forward's store).  Per pixel (Y, X) of the full grid and channel k, with v the finished fp32 sum:
 *     out[(Y - row0) * pitch + 3 * X + (swap ? 2 - k : k)] = (unsigned char) rintf(fminf(fmaxf(v, 0), 1) * 255)
 * for Y < crop_rows and X < crop_cols only (the top-left crop_rows x crop_cols of the grid, 1 <= crop_* <= h, w); no other
 * byte of `out` is touched, row padding (pitch > 3 * crop_cols bytes) included.  Rounding is half-to-even like numpy's
 * .round(); a NaN sum gives 0.  Always a store, always interleaved: GSASR_FLAG_OVERWRITE_IMAGE / _CHW_IMAGE of dims.flags
 * are ignored; everything else (row bands: `out` points at the band's first row; kernel-choice flags, registered choices,
 * list_cap, GSASR_FLAG_FORWARD_ONLY plans) is as in gsasr_splat_forward -- both run the same kernel for the same dims.
 * Batched canvas: out is [batch, crop_rows, crop_cols, 3] (sample stride crop_rows * pitch, crop_rows <= slot); sample b
 * writes its own grid's pixels and 0 in the part of its rectangle beyond h_b x w_b.
 * GSASR_ERR_ARG: crop_* < 1 or larger than the grid, pitch < 3 * crop_cols, null out, unknown u8_flags. */
#define GSASR_U8_SWAP_RB 1u   /* write b,g,r (what cv2.imwrite / tensor2img(rgb2bgr=True) want) */
GSASR_API int gsasr_splat_forward_u8(const gsasr_dims *dims, const void *workspace, size_t workspace_bytes,
                                     unsigned char *out, int crop_rows, int crop_cols, size_t pitch,
                                     unsigned u8_flags, void *stream);

/* g_* += d(sum(grad_img*img))/d{sigmas,coords,colors} over rows [row0,row1).  Outputs must be
 * zero-initialised by the caller when a plain gradient is wanted (the reference wrapper does
 * torch.zeros_like, gs_cuda_dmax/gswrapper.py:40-42), unless GSASR_FLAG_OVERWRITE_GRADS is set. */
GSASR_API int gsasr_splat_backward(const float *sigmas, const float *coords, const float *colors,
                         const float *grad_img /*[row1-row0, w, 3]*/, float *g_sigmas,
                         float *g_coords, float *g_colors, const gsasr_dims *dims,
                         const void *workspace, size_t workspace_bytes, void *stream);

/* Fused host prologue of the path: raw decoder output gs_parameters[n,9] =
 * [sigma_x, sigma_y, rho, alpha, r, g, b, mu_x, mu_y] -> the kernel-frame tensors handed to the splat,
 * i.e. the activations of utils/gaussian_splatting.py:174-180 followed by the conversion of :121-123
 * (x/y swap of the sigmas, align-corners fix of the means, colour * alpha) in ONE kernel instead of ~15
 * elementwise launches.  `step_size` points at one float in DEVICE memory (default_step_size / scale, which
 * the reference holds as a 0-dim tensor), so no host sync is needed.  The backward applies the chain rule
 * and overwrites g_parameters[n,9]. */
GSASR_API int gsasr_prologue_forward(const float *gs_parameters, const float *step_size, int n, int h, int w,
                           float *sigmas, float *coords, float *colors, void *stream);
GSASR_API int gsasr_prologue_backward(const float *gs_parameters, const float *step_size, int n, int h, int w,
                            const float *g_sigmas, const float *g_coords, const float *g_colors,
                            float *g_parameters, void *stream);

/* The whole host-API step in one call each way (what generate_2D_gaussian_splatting_step enqueues):
 * prologue + plan + forward, and splat-backward + prologue-backward.  The workspace additionally holds the
 * kernel-frame tensors and their gradients (gsasr_step_workspace_bytes >= gsasr_splat_workspace_bytes).
 * Forward honours dims.flags (OVERWRITE_IMAGE, CHW_IMAGE); backward always stores g_parameters[n,9] and
 * reads grad_img as [row1-row0, w, 3], or with GSASR_FLAG_CHW_GRAD as planar [3, row1-row0, w] (batched canvas:
 * [B, 3, grad_rows, w], grad_rows >= every sample's height).  step_size = NULL in the backward: the step sizes the
 * forward's prologue used (kept in the workspace) -- the counterpart of the _sm forward below.
 *
 * gsasr_step_forward_sm: the reference's `scale_modify` calling convention (utils/gaussian_splatting.py:166-171:
 * `assert scale_modify[0] == scale_modify[1]`, step = default_step_size / scale_modify[0]) evaluated on the DEVICE by the
 * plan's first kernel.  scale_modify = device floats, sample b's pair at scale_modify[b * sm_stride + {0, 1}]
 * (sm_stride >= 2; one image: b = 0).  mismatch = device int[2] or NULL: set to {1 + b, bits of scale_modify[b][0]} when
 * a pair differs and never cleared here -- the caller reads it when convenient (no host synchronisation per call). */
GSASR_API size_t gsasr_step_workspace_bytes(const gsasr_dims *dims);
GSASR_API int gsasr_step_forward(const float *gs_parameters, const float *step_size, const gsasr_dims *dims, void *workspace,
                       size_t workspace_bytes, float *img, void *stream);
GSASR_API int gsasr_step_forward_sm(const float *gs_parameters, const float *scale_modify, int sm_stride, float default_step_size,
                          int *mismatch, const gsasr_dims *dims, void *workspace, size_t workspace_bytes, float *img,
                          void *stream);
/* gsasr_step_forward / gsasr_step_forward_sm ending in gsasr_splat_forward_u8 instead of the float forward */
GSASR_API int gsasr_step_forward_u8(const float *gs_parameters, const float *step_size, const gsasr_dims *dims, void *workspace,
                          size_t workspace_bytes, unsigned char *out, int crop_rows, int crop_cols, size_t pitch,
                          unsigned u8_flags, void *stream);
GSASR_API int gsasr_step_forward_sm_u8(const float *gs_parameters, const float *scale_modify, int sm_stride,
                             float default_step_size, int *mismatch, const gsasr_dims *dims, void *workspace,
                             size_t workspace_bytes, unsigned char *out, int crop_rows, int crop_cols, size_t pitch,
                             unsigned u8_flags, void *stream);
GSASR_API int gsasr_step_backward(const float *gs_parameters, const float *step_size, const float *grad_img,
                        float *g_parameters, const gsasr_dims *dims, void *workspace, size_t workspace_bytes,
                        void *stream);

/* A rectangular window of the HR grid.  GSASR is arbitrary-scale: the reference's demo offers scale factors up to x30, and a
 * caller who looks at part of such a grid should pay for that part.  The `_view` entry points render -- and differentiate
 * through -- the dims.h x dims.w pixels whose first one is pixel (y0, x0) of a full_h x full_w grid:
 *
 *   dims      the WINDOW as one whole image: h, w >= 2 its size, row0 = 0, row1 = h, batch = 0; s, dmax, cutoff, flags,
 *             list_cap as always.  Image, gradient and 8-bit layouts, GSASR_FLAG_OVERWRITE_* / CHW_* / STRIDE8 /
 *             FORWARD_ONLY, the kernel-choice flags, crop / pitch / swap of the 8-bit store: those of a whole image of
 *             the window's size.
 *   view      the grid it is cut from, 2 <= full_h, full_w <= 32767, and its origin: 0 <= y0, y0 + h <= full_h, likewise
 *             columns.  Anything else (a row band, a window that leaves the grid) is GSASR_ERR_ARG / a workspace size
 *             of 0, before anything is enqueued.  view = NULL: the plain entry point.  (A batched canvas: below.)
 *
 * Output pixel (i, j) IS pixel (y0 + i, x0 + j) of the full grid: the same float coordinates
 * ((float)(2.0 * (x0 + j) / (full_w - 1) - 1.0)), the same dmax box test, the same cutoff rules; the step forms run the host
 * prologue for the full grid's size.  The dmax box in pixels and the adaptive cutoff's cell counts follow the full grid's
 * scale, everything the workspace sizes the window.  The plan still classifies all s Gaussians (those whose support misses
 * the window are dead to it); forward and backward touch the window only.  The backward is the gradient of
 * sum(grad_img * window), and -- a window being a band of its grid -- sweeps the forward's windows like a row band's does
 * (no GSASR_SPLAT_GRAD_TAU: a Gaussian's share inside the window may be all tail).
 * The view belongs to the plan: forward / backward with another view, or none, on that workspace is GSASR_ERR_PLAN.  The
 * kernel-choice rules see the Gaussians the window can expect, s * (h * w) / (full_h * full_w), not s; choices registered
 * with gsasr_set_kernel_choice are keyed on whole-image shapes and are not looked up for a window (explicit flags in the
 * dims hold as always).  A view that is the whole grid (y0 = x0 = 0, full = dims) is the plain call, bit for bit.
 *
 * One window per sample of a batched canvas: with dims.batch = B > 1 (a whole canvas as always: h = B * slot, row0 = 0,
 * row1 = h, s a multiple of B) `view` addresses B gsasr_views, one per sample in order, and dims.sample_hw[b] is the size of
 * window b: at least 2 x 2, at most slot x dims.w, inside its own grid (0 <= y0_b, y0_b + h_b <= full_h_b, likewise columns;
 * 2 <= full_h_b, full_w_b <= 32767).  Everything above holds per sample: pixel (i, j) of slot b is pixel (y0_b + i, x0_b + j)
 * of sample b rendered alone on its full grid, the step forms run the prologue (and its chain rule) with each sample's full
 * grid and step size, the backward is the gradient of a loss that looks at the windows only, the padding of a slot is zero
 * under GSASR_FLAG_OVERWRITE_IMAGE and never read by the backward.  The adaptive cutoff counts with the largest full grid's
 * dmax box (an upper bound for every sample).  All B views are part of the plan's identity (another set, or none, is
 * GSASR_ERR_PLAN); when every view is its sample's whole grid the call is the plain batched one, bit for bit.  Row bands and
 * GSASR_FLAG_CONTINUOUS stay GSASR_ERR_ARG.  The workspace carries the table of views behind everything else: a plan
 * without views has the bytes and offsets it always had.  The kernel-choice rules judge the canvas with the Gaussians its
 * windows can expect, sum_b (s / B) * h_b w_b / (full_h_b full_w_b). */
typedef struct gsasr_view {
    int full_h, full_w;   /* the grid the window is cut from: pixel (Y, X) of it sits at 2*X/(full_w-1)-1, 2*Y/(full_h-1)-1 */
    int y0, x0;           /* the window's first row / column on that grid; its size is dims.h x dims.w               */
} gsasr_view;
GSASR_API size_t gsasr_splat_workspace_bytes_view(const gsasr_dims *dims, const gsasr_view *view);
GSASR_API size_t gsasr_step_workspace_bytes_view(const gsasr_dims *dims, const gsasr_view *view);
GSASR_API int gsasr_splat_plan_view(const float *sigmas, const float *coords, const float *colors, const gsasr_dims *dims,
                          const gsasr_view *view, void *workspace, size_t workspace_bytes, void *stream);
GSASR_API int gsasr_splat_forward_view(const gsasr_dims *dims, const gsasr_view *view, const void *workspace,
                             size_t workspace_bytes, float *img, void *stream);
GSASR_API int gsasr_splat_forward_u8_view(const gsasr_dims *dims, const gsasr_view *view, const void *workspace,
                                size_t workspace_bytes, unsigned char *out, int crop_rows, int crop_cols, size_t pitch,
                                unsigned u8_flags, void *stream);
GSASR_API int gsasr_splat_backward_view(const float *sigmas, const float *coords, const float *colors, const float *grad_img,
                              float *g_sigmas, float *g_coords, float *g_colors, const gsasr_dims *dims,
                              const gsasr_view *view, const void *workspace, size_t workspace_bytes, void *stream);
/* (step_size / scale_modify: of the FULL grid's scale factor, as for the whole image) */
GSASR_API int gsasr_step_forward_view(const float *gs_parameters, const float *step_size, const gsasr_dims *dims,
                            const gsasr_view *view, void *workspace, size_t workspace_bytes, float *img, void *stream);
GSASR_API int gsasr_step_forward_sm_view(const float *gs_parameters, const float *scale_modify, int sm_stride,
                               float default_step_size, int *mismatch, const gsasr_dims *dims, const gsasr_view *view,
                               void *workspace, size_t workspace_bytes, float *img, void *stream);
GSASR_API int gsasr_step_forward_u8_view(const float *gs_parameters, const float *step_size, const gsasr_dims *dims,
                               const gsasr_view *view, void *workspace, size_t workspace_bytes, unsigned char *out,
                               int crop_rows, int crop_cols, size_t pitch, unsigned u8_flags, void *stream);
GSASR_API int gsasr_step_forward_sm_u8_view(const float *gs_parameters, const float *scale_modify, int sm_stride,
                                  float default_step_size, int *mismatch, const gsasr_dims *dims, const gsasr_view *view,
                                  void *workspace, size_t workspace_bytes, unsigned char *out, int crop_rows,
                                  int crop_cols, size_t pitch, unsigned u8_flags, void *stream);
GSASR_API int gsasr_step_backward_view(const float *gs_parameters, const float *step_size, const float *grad_img,
                             float *g_parameters, const gsasr_dims *dims, const gsasr_view *view, void *workspace,
                             size_t workspace_bytes, void *stream);

/* Pixel loss fused into the forward's store (training: what basicsr/models/gsasr_model.py:191-237 does with a rendered batch --
 * per sample, slice output and ground truth to gt_size[i], cri_pix(b_output, b_gt) with reduction='mean' times loss_weight
 * (L1Loss / MSELoss / CharbonnierLoss, basicsr/losses/basic_loss.py:14-25), summed over the samples and divided by b).  The
 * forward kernels hold the finished pixel in registers: they load the target pixel, form d = v - t and write dL/dimg and one
 * partial sum of phi(d) per sub-tile; a small kernel adds the partials of each sample in a fixed order, in double.  No image is
 * written or read back, no float atomics, no memset; two calls on one plan give the same bits wherever the forward gives the
 * same pixels (the search kernels add a pixel's terms in an order that follows wave timing: where Gaussians overlap, the pixels'
 * last bits, and then the loss's and the gradient's, may differ between two calls).
 *
 *   kind                    phi(d)             phi'(d)
 *   GSASR_LOSS_L1           |d|                (d > 0) - (d < 0): 0 at d == 0, torch's convention
 *   GSASR_LOSS_MSE          d * d              2 d
 *   GSASR_LOSS_CHARBONNIER  sqrt(d * d + eps)  d / sqrt(d * d + eps)
 *
 * Sample b (one image: b = 0, B = 1) has its own grid of h_b x w_b pixels, over which -- three channels each --
 *   GSASR_LOSS_MEAN   c_b = weight / (3 h_b w_b B) (one fp32 division by the integer product),  L_b = weight / (3 h_b w_b) * sum phi,
 *                     L = (1 / B) sum_b L_b
 *   GSASR_LOSS_SUM    c_b = weight,  L_b = weight * sum phi,  L = sum_b L_b
 *   grad_img[pixel, k] = c_b * phi'(d) on the sample's own pixels; the padding of a slot is not written.  No backward takes a
 *                     term from it, but the Gaussian-stationary kernels LOAD up to seven rows below a window's last row and
 *                     multiply them by exactly 0: the rows below a sample shorter than its slot must hold finite values (zero
 *                     the buffer once; a NaN left there turns into a NaN gradient)
 *   loss[0] = L, loss[1 + b] = L_b
 * Plain IEEE arithmetic, no special handling of NaN or Inf: a NaN pixel or target makes its sample's loss NaN; its gradient is
 * NaN for MSE and Charbonnier and 0 for L1 (both comparisons are false).
 *
 *   target       device fp32 in the layout the image flags of dims describe: [rows, w, 3] (canvas: [B * slot, w, 3]), or with
 *                GSASR_FLAG_CHW_IMAGE planar [3, target_rows, w] (canvas: [B, 3, target_rows, w]): only a sample's own pixels are read
 *   target_rows  rows per plane of a planar target, >= every h_b; 0 = h (canvas: slot).  The counterpart of dims.grad_rows: the
 *                padded [B, 3, Hmax, Wmax] ground truth of a training batch is read in place
 *   grad_img     written in the layout the BACKWARD on these dims reads: [rows, w, 3] (canvas: [B * slot, w, 3]), or with
 *                GSASR_FLAG_CHW_GRAD planar [3, h, w] (canvas: [B, 3, dims.grad_rows, w]).  NULL: the value only (a validation
 *                loss on a GSASR_FLAG_FORWARD_ONLY plan)
 *   loss         device float[1 + max(1, batch)]
 *   img          NULL, or the float image, stored as well exactly as gsasr_splat_forward would (dims.flags)
 *   scratch      gsasr_loss_scratch_bytes(dims) bytes, 4-byte aligned: the partial sums (every one is written before it is read)
 *
 * view: NULL = the plain call, else as for gsasr_splat_forward_view / gsasr_step_forward_view (one per sample of a canvas); the
 * loss is then that of the windows.  The forward kernel is the one gsasr_splat_forward runs for the same dims.  The backward is
 * gsasr_splat_backward[_view] / gsasr_step_backward[_view] on grad_img; an upstream d/dL other than 1 multiplies its result.
 * GSASR_ERR_ARG before anything is enqueued: a row band, unknown kind / normalisation, null target / loss / scratch, eps < 0,
 * 0 < target_rows < a sample's height.  A GSASR_FLAG_CONTINUOUS plan: GSASR_ERR_PLAN, like every image forward.
 * gsasr_step_forward_loss: prologue + plan + this forward; the step size is `step_size` (device floats, as gsasr_step_forward) or,
 * with step_size = NULL, formed from scale_modify / sm_stride / default_step_size / mismatch as by gsasr_step_forward_sm. */
#define GSASR_LOSS_L1 0
#define GSASR_LOSS_MSE 1
#define GSASR_LOSS_CHARBONNIER 2
#define GSASR_LOSS_MEAN 0
#define GSASR_LOSS_SUM 1
typedef struct gsasr_loss {
    int kind;             /* GSASR_LOSS_L1 / _MSE / _CHARBONNIER */
    int normalisation;    /* GSASR_LOSS_MEAN / _SUM */
    float weight;         /* loss_weight */
    float eps;            /* Charbonnier only (basic_loss.py:24 defaults to 1e-12) */
    const float *target;
    int target_rows;
    float *grad_img;
    float *loss;
    float *img;
    void *scratch;
} gsasr_loss;
GSASR_API size_t gsasr_loss_scratch_bytes(const gsasr_dims *dims);   /* 0 on bad dims */
GSASR_API int gsasr_splat_forward_loss(const gsasr_dims *dims, const gsasr_view *view, const void *workspace, size_t workspace_bytes,
                             const gsasr_loss *loss, void *stream);
GSASR_API int gsasr_step_forward_loss(const float *gs_parameters, const float *step_size, const float *scale_modify, int sm_stride,
                            float default_step_size, int *mismatch, const gsasr_dims *dims, const gsasr_view *view,
                            void *workspace, size_t workspace_bytes, const gsasr_loss *loss, void *stream);

/* SSIM loss of a rendered batch (training: the other half of l_total = l_pix + l_ssim, basicsr/models/gsasr_model.py:213-242 --
 * cri_ssim = SSIMLoss, basicsr/losses/basic_loss.py:256-264: loss_weight * (1 - pytorch_msssim.ssim(x, y, data_range=1)) per sample,
 * summed over the samples and divided by b).  It needs the image, so it is a call of its own behind a forward that stored one
 * (GSASR_FLAG_CHW_IMAGE; gsasr_loss.img), and it can ADD its gradient to the one the fused pixel loss wrote: one backward serves
 * both terms.  No float atomics, no memset, no allocation, no host synchronisation; two calls give the same bits.
 *
 *   window  g[i] = exp(-(i - 5)^2 / (2 * 1.5^2)) / sum, i = 0..10, applied along rows and columns per channel in "valid" mode: sample
 *           b (h_b x w_b pixels) has a map of 3 x (h_b - 10) x (w_b - 10) values
 *   mu1 = g*x, mu2 = g*y, s1 = g*(x^2) - mu1^2, s2 = g*(y^2) - mu2^2, s12 = g*(xy) - mu1 mu2,  C1 = 0.01^2, C2 = 0.03^2
 *   A1 = 2 mu1 mu2 + C1, A2 = 2 s12 + C2, B1 = mu1^2 + mu2^2 + C1, B2 = s1 + s2 + C2,  map = (A1 / B1) (A2 / B2)  (not clamped)
 *   L_b = weight * (1 - mean(map)),  L = (1 / B) sum_b L_b;  loss[0] = L, loss[1 + b] = L_b
 *   d map / d s1 = -A1 A2 / (B1 B2^2),  d map / d s12 = 2 A1 / (B1 B2),
 *   d map / d mu1 = 2 mu2 A2 / (B1 B2) - 2 mu1 A1 A2 / (B1^2 B2) - 2 mu1 d map / d s1 - mu2 d map / d s12
 *   grad_img = c_b [ gT*(d map / d mu1) + 2 x gT*(d map / d s1) + y gT*(d map / d s12) ],  c_b = -weight / (3 (h_b - 10) (w_b - 10) B)
 *           (gT*: the transposed correlation with the same window, the map taken as zero outside its valid pixels)
 * Plain IEEE fp32 arithmetic, the tiles' sums of 1 - map added in double: a NaN pixel makes the map NaN within its 11 x 11 reach, and its sample's loss.
 * (The kernels evaluate the formulas on x - cx, y - cy, cx and cy the sample's centre pixel of the channel -- the same quantities
 * with less cancellation where the images are flat; a NaN or Inf there reaches every value of that sample's channel.)
 *
 *   img        planar [batch, 3, rows, w], as GSASR_FLAG_CHW_IMAGE stores it (one image: batch = 1, [3, rows, w])
 *   target     planar [batch, 3, target_rows, w], read in place (target_rows = 0: rows; the padded ground truth may have more rows)
 *   sample_hw  HOST array [2 * batch] of (h_b, w_b), read during the call, as gsasr_dims.sample_hw; NULL: every sample is rows x w.
 *              Only a sample's own pixels are read, of img and of target
 *   grad_img   NULL: the value only.  Else d L / d img, planar [batch, 3, grad_rows, w] (what a backward with GSASR_FLAG_CHW_GRAD
 *              reads), or with GSASR_SSIM_GRAD_HWC interleaved [batch * grad_rows, w, 3] (grad_rows = 0: rows).  The samples' own
 *              pixels are stored -- with GSASR_SSIM_ACCUMULATE added to what is there --, the padding is never touched
 *   loss       device float[1 + batch]
 *   scratch    gsasr_ssim_scratch_bytes(descriptor) bytes, 4-byte aligned: the tiles' partial sums and, when grad_img is not NULL,
 *              the three derivative maps (36 bytes per pixel of img).  Every word is written before it is read
 * GSASR_ERR_ARG before anything is enqueued: null img / target / loss / scratch, batch outside 1..GSASR_MAX_BATCH, rows or w
 * outside 11..32767, a sample smaller than 11 in either extent or larger than rows x w, 0 < target_rows or 0 < grad_rows below a
 * sample's height, unknown flag bits. */
#define GSASR_SSIM_GRAD_HWC 1u   /* grad_img interleaved [batch * grad_rows, w, 3]; else planar [batch, 3, grad_rows, w] */
#define GSASR_SSIM_ACCUMULATE 2u /* grad_img += ...; else the samples' own pixels are stored, padding untouched */
typedef struct gsasr_ssim {
    int batch, rows, w;
    int target_rows;      /* 0 = rows */
    int grad_rows;        /* 0 = rows */
    const int *sample_hw; /* HOST array [2*batch], or NULL */
    float weight;         /* loss_weight */
    unsigned flags;       /* GSASR_SSIM_* */
    const float *img, *target;
    float *grad_img;
    float *loss;
    void *scratch;
} gsasr_ssim;
GSASR_API size_t gsasr_ssim_scratch_bytes(const gsasr_ssim *ssim);   /* 0 on bad arguments (the pointers other than grad_img are not looked at) */
GSASR_API int gsasr_ssim_loss(const gsasr_ssim *ssim, void *stream);

/* Validation metrics of an 8-bit picture (inference / validation: what basicsr/models/gsasr_model.py:483-488 asks of every
 * validation image -- basicsr/metrics/psnr_ssim.py calculate_psnr (12-48) and calculate_ssim (85-128, 170-198) with crop_border and
 * test_y_channel (metric_util.py:32-45, color_util.py:38-68)), computed where the 8-bit forward stored the picture.  No float
 * atomics, no memset, no allocation, no host synchronisation; two calls on the same inputs give the same bits.
 *
 *   img, ref   uint8, interleaved [h, w, 3], rows img_pitch / ref_pitch bytes apart (>= 3 * w; any alignment), sample b at
 *              img + b * img_stride / ref + b * ref_stride bytes: either may be a window of a larger picture.  Bytes outside the
 *              3 * w_b bytes of a sample's h_b rows are never read
 *   sample_hw  HOST array [2 * batch] of (h_b, w_b), read during the call: sample b is the top-left h_b x w_b pixels of its
 *              h x w slot; NULL: every sample is h x w
 *   crop_border = cb >= 0: both metrics look at rows [cb, h_b - cb) and columns [cb, w_b - cb) only (img[cb:-cb, cb:-cb]; 0: no
 *              crop), hc x wc pixels
 *   values     RGB mode: the bytes as numbers 0..255, three channels (their order does not matter).  GSASR_METRIC_Y: one channel,
 *              with r, g, b the pixel's bytes (in memory r, g, b; with GSASR_METRIC_BGR b, g, r -- as GSASR_U8_SWAP_RB stores):
 *                x = float32(v) / 255f per channel;  y64 = 24.966 b + 128.553 g + 65.481 r + 16.0 in double (products and sums
 *                rounded one by one, left to right);  y32 = float32(y64 / 255.0);  Y = float32(y32 * 255f), widened to double
 *   PSNR       mse = mean over the cropped pixels and the channels of (a - b)^2 -- in RGB mode the sum is an exact integer --,
 *              psnr = 10 log10(255^2 / mse), +inf when mse == 0
 *   SSIM       per channel: window g (x) g, g[i] = exp(-(i - 5)^2 / (2 * 1.5^2)) / sum, i = 0..10 (cv2.getGaussianKernel(11, 1.5);
 *              applied along rows, then columns), "valid" mode over a, b, a^2, b^2, ab: a (hc - 10) x (wc - 10) map;
 *              C1 = (0.01 * 255)^2, C2 = (0.03 * 255)^2, mu1 = g*a, mu2 = g*b, s1 = g*(a^2) - mu1^2, s2 = g*(b^2) - mu2^2,
 *              s12 = g*(ab) - mu1 mu2,  map = (2 mu1 mu2 + C1)(2 s12 + C2) / ((mu1^2 + mu2^2 + C1)(s1 + s2 + C2));
 *              ssim = mean of the map over its pixels and the channels.  All of it in double
 *   out        device double [batch][2]: out[2 b] = psnr, out[2 b + 1] = ssim of sample b; a metric that was not asked for
 *              (flags) is left untouched
 *   scratch    gsasr_metrics_scratch_bytes(descriptor) bytes, 8-byte aligned: the tiles' partial sums.  Every word that is read
 *              was written by the same call
 * GSASR_ERR_ARG before anything is enqueued: a null descriptor, null img / ref / out / scratch, a pitch below 3 * w, batch outside
 * 1..GSASR_MAX_BATCH, h or w outside 1..32767, a sample larger than h x w, neither GSASR_METRIC_PSNR nor GSASR_METRIC_SSIM, unknown
 * flag bits, crop_border < 0, hc < 1 or wc < 1, and with GSASR_METRIC_SSIM hc < 11 or wc < 11 (the reference would return the
 * mean of an empty map). */
#define GSASR_METRIC_PSNR 1u
#define GSASR_METRIC_SSIM 2u
#define GSASR_METRIC_Y 4u     /* test_y_channel: the metrics of the Y channel (one channel) */
#define GSASR_METRIC_BGR 8u   /* the bytes of a pixel are b, g, r (matters in Y mode only) */
typedef struct gsasr_metrics {
    int batch, h, w;      /* the canvas: batch slots of h x w pixels */
    const int *sample_hw; /* HOST array [2*batch], or NULL */
    const unsigned char *img;
    size_t img_pitch, img_stride;   /* bytes between rows / between samples */
    const unsigned char *ref;
    size_t ref_pitch, ref_stride;
    int crop_border;
    unsigned flags;       /* GSASR_METRIC_* */
    double *out;          /* device [batch][2] */
    void *scratch;
} gsasr_metrics;
GSASR_API size_t gsasr_metrics_scratch_bytes(const gsasr_metrics *metrics);   /* 0 on bad arguments (img, ref, out and scratch are not looked at) */
GSASR_API int gsasr_image_metrics(const gsasr_metrics *metrics, void *stream);

/* MATLAB-compatible bicubic imresize and its adjoint (the degradation that defines the task: basicsr/utils/matlab_functions.py
 * imresize / imresize_new, which basicsr/data/continuous_bicubic_downsample_dataset.py:70-72 applies to every GT crop), batched,
 * on planar fp32 images.  No float atomics, no memset, no allocation, no host synchronisation: a call can be captured, and two
 * calls on the same inputs give the same bits.
 *
 *   per axis   input length n, output length m, scale s: kw = 4 / s when s < 1 and antialiasing is on, else 4; p = ceil(kw) + 2
 *              taps.  Output o = 1..m (1-based): u = o / s + 0.5 (1 - 1 / s), left = floor(u - kw / 2), taps k = left .. left + p - 1
 *              with raw weight s cubic((u - k) s) in the antialiased-shrink case, else cubic(u - k);
 *              cubic(x) = 1.5|x|^3 - 2.5|x|^2 + 1 (|x| <= 1), -0.5|x|^3 + 2.5|x|^2 - 4|x| + 2 (1 < |x| <= 2), 0 beyond.  The p
 *              weights are divided by their sum.  u and the weights are computed in double and rounded once to float.
 *   edges      a tap outside the input reads the symmetric extension, mirrored once: 0-based k < 0 -> -1 - k, k >= n -> 2n - 1 - k.
 *              A tap with a non-zero weight that is still outside after one reflection is an argument error (the reference's
 *              symmetric copy fails on such a call too)
 *   order      rows (H) first, then columns (W); the intermediate [out_h, w_b] is fp32, each pass one fp32 dot product per
 *              output in tap order
 *   sizes      out_h, out_w are the caller's and shared by all samples: the formulas run for o = 1..out.  The reference's sizes
 *              are ceil(n s) (imresize) and Python's round(n s) (imresize_new); the library does not compare
 *   batch      1..GSASR_MAX_BATCH samples of `channels` >= 1 planes each (batch * channels <= 65535)
 *   in_h, in_w the input slot, 1..32767 each (so are out_h, out_w)
 *   sample_hw  HOST array [2 * batch] of (h_b, w_b), read during the call: sample b is the top-left h_b x w_b pixels of its
 *              slot; NULL: every sample is in_h x in_w.  Pixels of a slot outside h_b x w_b are never read, and the backward
 *              leaves them untouched (a caller that wants zeros there clears the buffer first)
 *   scales     HOST array of doubles, read during the call: [2 * batch] = (scale_h, scale_w) of sample b, or with
 *              GSASR_RESIZE_SHARED_SCALE [2], one pair for every sample.  Each finite and > 0
 *   in, out    fp32 planar; pixel (y, x) of channel c of sample b at byte b * stride + c * plane + y * pitch + 4 x.  Pitches, plane
 *              and sample strides are multiples of 4 bytes, the pitch at least the row (4 * in_w, 4 * out_w); the pointers 4-byte
 *              aligned: either tensor may be a window of a larger one
 *   flags      GSASR_RESIZE_NO_ANTIALIAS: antialiasing=False; GSASR_RESIZE_SHARED_SCALE: above; GSASR_RESIZE_ACCUMULATE (backward
 *              only; an argument error in the forward): grad_in += ..., else stored
 *   scratch    gsasr_resize_scratch_bytes(descriptor) bytes, 16-byte aligned: the weight tables and the row-pass intermediate.
 *              Every word that is read was written by the same call
 *   backward   gsasr_imresize_backward reads `out` as grad_out [batch, channels, out_h, out_w] and writes `in` (const cast away)
 *              as grad_in = A^T grad_out on the h_b x w_b pixels of every sample, A being the forward's linear map with the
 *              same float weights; gather form, fixed order
 * GSASR_ERR_ARG before anything is enqueued: a null descriptor, null in / out / scratch / scales, batch outside
 * 1..GSASR_MAX_BATCH, channels < 1 or batch * channels > 65535, in_h / in_w / out_h / out_w outside 1..32767, a sample with
 * no pixel or larger than its slot, a pitch below the row, a pitch / plane / stride that is no multiple of 4, a misaligned
 * pointer, a scale that is not finite and > 0, unknown flag bits, GSASR_RESIZE_ACCUMULATE in the forward, and the reflection
 * condition above (e.g. 26 pixels at s = 1/16). */
#define GSASR_RESIZE_NO_ANTIALIAS 1u
#define GSASR_RESIZE_ACCUMULATE 2u     /* backward: grad_in += ... ; else stored */
#define GSASR_RESIZE_SHARED_SCALE 4u   /* scales holds one (scale_h, scale_w) pair for all samples */
typedef struct gsasr_resize {
    int batch, channels;
    int in_h, in_w;          /* the input slot */
    const int *sample_hw;    /* HOST array [2*batch], or NULL */
    const double *scales;    /* HOST array [2*batch], or [2] with GSASR_RESIZE_SHARED_SCALE */
    int out_h, out_w;        /* every sample's output size */
    const float *in;         /* backward: grad_in, written */
    size_t in_pitch, in_plane, in_stride;      /* bytes between rows / channels / samples */
    float *out;              /* backward: grad_out, read */
    size_t out_pitch, out_plane, out_stride;
    unsigned flags;          /* GSASR_RESIZE_* */
    void *scratch;
} gsasr_resize;
GSASR_API size_t gsasr_resize_scratch_bytes(const gsasr_resize *resize);   /* 0 on bad arguments (sample_hw and scales are read; in, out and scratch are not looked at) */
GSASR_API int gsasr_imresize(const gsasr_resize *resize, void *stream);
GSASR_API int gsasr_imresize_backward(const gsasr_resize *resize, void *stream);

/* Training batches from decoded images (what basicsr/data/continuous_bicubic_downsample_dataset.py:46-111 does per sample on the
 * host, and the DataLoader's collation): `batch` windows of `batch` 8-bit images resident on the device become, in one call, the
 * float tensors a training step reads.  New entry points of ABI 7; no existing one changed.
 *
 *   sources    src: HOST array [batch] of DEVICE pointers to dense uint8 images [h, w, 3] (any byte alignment; the same image may
 *              serve several samples); src_hw: HOST array [2 * batch] of (h, w), 1..32767 each.  Nothing outside an image's
 *              h * w * 3 bytes is read
 *   window     HOST array [4 * batch] of (y0, x0, gh, gw): sample b is rows y0 .. y0 + gh - 1, columns x0 .. x0 + gw - 1 of
 *              its image; inside the image, at least one pixel
 *   value      (float)byte / 255.0f, one correctly rounded division.  With GSASR_BATCH_BGR a pixel's bytes are b, g, r and
 *              the planes come out r, g, b (the reference's img2tensor(bgr2rgb=True)); without it the planes keep the bytes' order
 *   aug        HOST array [batch] of GSASR_BATCH_HFLIP | _VFLIP | _TRANSPOSE, or NULL for none.  The order is
 *              basicsr/data/transforms.py:119-133's: horizontal flip, vertical flip, transposition -- pixel (r, c) of a transposed
 *              sample is row c, column r of the flipped window, and the sample's extent is gw x gh
 *   gt         fp32 [batch, 3, gt_h, gt_w], dense: the augmented sample in the top-left corner of its slot, every other pixel
 *              of the slot written as 0 (the reference's F.pad to gt_size_max; no memset is launched).  NULL: only lq is made
 *              (the sampled-pixel batch, whose GT comes from gsasr_batch_pick); gt_h x gt_w must hold the samples all the same
 *   lq         fp32 [batch, 3, lr_h, lr_w], dense: gsasr_imresize of the UN-augmented float window with scales lr_h / gh,
 *              lr_w / gw, then the same flips / transposition (resize first, augment second: the reference's order; a transposed
 *              sample needs lr_h == lr_w)
 *   flags      GSASR_BATCH_BGR: above; GSASR_BATCH_NO_ANTIALIAS: the resize's antialiasing=False
 *   scratch    gsasr_batch_scratch_bytes(descriptor) bytes, 256-byte aligned: the planar float windows, the un-augmented LR
 *              images and the resize's own scratch.  Every word that is read was written by the same call
 *   pick       gsasr_batch_pick writes out [batch, 3, n_points] = the augmented sample at the integer points
 *              [batch, n_points, 2] = (row, column) (device int32), read straight from the bytes: the float GT is not made.  The
 *              points follow the sampled-pixel entry points' rule: a negative index wraps once, a point that is still out of the
 *              sample's extent yields 0.  It reads src, src_hw, window, aug and GSASR_BATCH_BGR of the descriptor only
 * All host arrays are read during the call.  The calls only enqueue work on `stream`: no allocation, no host synchronisation,
 * and two calls on the same inputs give the same bits.  A call reads host arrays and, as a rule, new pointers on every step:
 * it is not meant to be captured into a graph (a replay would repeat the windows and pointers of the capture).
 * GSASR_ERR_ARG before anything is enqueued: a null descriptor; batch outside 1..GSASR_MAX_BATCH; a null src / src_hw / window
 * array, source image, lq or scratch (pick: points or out); gt, lq, points or out not 4-byte aligned, scratch not 256-byte
 * aligned; a source h or w, gt_h, gt_w, lr_h or lr_w outside 1..32767; a window outside its source, or with no pixel; a GT slot
 * smaller than a sample's extent; a transposed sample with lr_h != lr_w; unknown flag or augmentation bits; n_points outside
 * 1..2^24; and everything gsasr_imresize refuses on these windows, the reflection condition included (a 9-pixel window to
 * lr 1 is one). */
#define GSASR_BATCH_HFLIP 1u           /* aug bits */
#define GSASR_BATCH_VFLIP 2u
#define GSASR_BATCH_TRANSPOSE 4u
#define GSASR_BATCH_BGR 1u             /* flags */
#define GSASR_BATCH_NO_ANTIALIAS 2u
typedef struct gsasr_batch {
    int batch;
    const unsigned char *const *src;   /* HOST array [batch] of device pointers */
    const int *src_hw;                 /* HOST array [2*batch] */
    const int *window;                 /* HOST array [4*batch]: y0, x0, gh, gw */
    const unsigned char *aug;          /* HOST array [batch] of GSASR_BATCH_HFLIP | _VFLIP | _TRANSPOSE, or NULL */
    int gt_h, gt_w;                    /* the GT slot */
    float *gt;
    int lr_h, lr_w;
    float *lq;
    unsigned flags;                    /* GSASR_BATCH_BGR | GSASR_BATCH_NO_ANTIALIAS */
    void *scratch;
} gsasr_batch;
GSASR_API size_t gsasr_batch_scratch_bytes(const gsasr_batch *batch);   /* 0 on bad arguments (the host arrays are read; gt, lq and scratch are not looked at) */
GSASR_API int gsasr_batch_make(const gsasr_batch *batch, void *stream);
GSASR_API int gsasr_batch_pick(const gsasr_batch *batch, const int *points, int n_points, float *out, void *stream);

/* Window attention with a relative-position bias: the core of every layer of GSASR's Fea2GS decoder (WindowCrossAttn and
 * GSSelfAttn, utils/fea2gs.py:162-194, 321-350), fused -- no [windows, heads, nq, nk] score tensor and no head split / merge copy
 * ever touches memory.  For window w and head h, with x[w, :, h] the columns h * head_dim .. (h + 1) * head_dim - 1 of x:
 *
 *   S = scale q[w, :, h] k[w, :, h]^T + B_h,  B_h[i, j] = table[index[i, j], h],  P = softmax over j of S,  out[w, :, h] = P v[w, :, h]
 *   stats[w, h, i] = log sum_j exp(S[i, j])                                   (the row statistic a backward recomputes P from)
 *   backward, given grad_out = d L / d out:  delta_i = sum_c grad_out[i, c] out[i, c],  dP = grad_out v^T,  dS = P o (dP - delta),
 *   g_v = P^T grad_out,  g_q = scale dS k,  g_k = scale dS^T q,  g_table[t, h] = sum over w and all (i, j) with index[i, j] = t of dS[i, j]
 *
 * fp32 throughout: the products run on the exact-fp32 matrix instruction (a k-ordered chain of fmaf), the softmax sees the
 * whole row at once (one maximum, one sum; no online rescaling).  out, g_q, g_k and g_v are written once by the workgroup that
 * owns the (window, head) -- no atomics, two calls give the same bits.  g_table is binned with float adds in LDS whose order is
 * not fixed (above 4096 table rows: with global adds in double, rounded once): its last bits may differ between two calls; a
 * row that no (i, j) uses is exactly 0.  Nothing is read on the host and
 * everything is enqueued on `stream`: the calls can be captured into a graph.
 *
 *   q, out, grad_out, g_q   [windows, nq, heads * head_dim], contiguous;  k, v, g_k, g_v   [windows, nk, heads * head_dim]
 *   table, g_table          [table_rows, heads];  index   int [nq, nk] with 0 <= index < table_rows -- NOT checked here (the
 *                           kernels read table[index]): the caller validates it, as gsasr_amd.window_attention does once per tensor
 *   stats                   float [windows, heads, nq]; forward: NULL = not stored; backward: what the forward stored
 *   g_q, g_k, g_v, g_table  each NULL = not wanted (its work is skipped where that saves a kernel)
 *   scratch                 gsasr_window_attn_scratch_bytes(descriptor) bytes, 256-byte aligned, for the backward when g_table is set
 *                           (set g_table before asking): per-workgroup partial tables, every word written before it is read
 *                           (above 4096 table rows: the table's sums in double, zeroed by the call)
 * GSASR_ERR_ARG before anything is enqueued: windows, heads or table_rows below 1, nq or nk outside 1..256, head_dim outside
 * 1..32, flags other than 0, a NaN scale, a null pointer among those the call needs. */
typedef struct gsasr_window_attn {
    int windows, heads, nq, nk, head_dim, table_rows;
    float scale;
    unsigned flags;       /* 0 (none defined) */
    const float *q, *k, *v, *table;
    const int *index;
    float *out;           /* written by the forward, read by the backward */
    float *stats;
    const float *grad_out;
    float *g_q, *g_k, *g_v, *g_table;
    void *scratch;
} gsasr_window_attn;
GSASR_API size_t gsasr_window_attn_scratch_bytes(const gsasr_window_attn *attn);   /* 0 on bad arguments (only g_table among the pointers is looked at) */
GSASR_API int gsasr_window_attn_forward(const gsasr_window_attn *attn, void *stream);
GSASR_API int gsasr_window_attn_backward(const gsasr_window_attn *attn, void *stream);

/* Window attention with a 2-D rotary embedding: the core of every layer of the Fea2GS_ROPE_AMP decoder (WindowCrossAttn and
 * GSSelfAttn of utils/fea2gsropeamp.py: rotation of q and k by learned angles, then bias-free scaled-dot-product attention),
 * fused like the biased one above -- same layouts, same kernels' geometry, no table and no index.  For window w, head h, with
 * x[w, n, h] the head's columns of token n read as head_dim / 2 complex numbers (column 2 j + i column 2 j + 1):
 *
 *   R(x)[w, n, h, j] = x[w, n, h, j] (cos t + i sin t),  t = angles[h, n, j]       (query i uses row i, key j row j of angles)
 *   S = scale R(q)[w, :, h] R(k)[w, :, h]^T (rotate, then scale),  P = softmax over the keys of S,  out[w, :, h] = P v[w, :, h]
 *   stats[w, h, i] = log sum_j exp(S[i, j]);   cossin[h, n, j] = (cos t, sin t), the accurate sincosf, written by the forward
 *   backward, given grad_out: delta, dP, dS as above;  g_v = P^T grad_out,  g_q = conj-rotation of scale dS R(k),
 *   g_k = conj-rotation of scale dS^T R(q)   (a rotation is unitary: the gradient of the un-rotated input is the gradient of the
 *   rotated one times cos t - i sin t),
 *   g_angles[h, n, j] = sum_w Im(conj(q) g_q)[w, n, h, j] [n < nq] + sum_w Im(conj(k) g_k)[w, n, h, j] [n < nk],
 *   Im(conj(x) g) = x_re g_im - x_im g_re, of the UN-rotated inputs and their gradients.
 *
 * fp32 throughout.  out, g_q, g_k, g_v and g_angles are each written once and two calls give the same bits: g_angles is added
 * in a fixed order (window by window inside a slice of windows, then slice by slice), without atomics; its rows past
 * max(nq, nk) are exactly 0.  Nothing is read on the host and everything is enqueued on `stream`.
 *
 *   q, k, v, out, stats, grad_out, g_q, g_k, g_v   as in gsasr_window_attn; q, k, g_q, g_k and cossin 8-byte aligned
 *   angles, g_angles   [heads, angle_rows, head_dim / 2], angle_rows >= max(nq, nk)
 *   cossin             float [heads, angle_rows, head_dim / 2, 2]: written by the forward, read by the backward (like stats)
 *   g_q, g_k, g_v, g_angles   each NULL = not wanted, but g_angles needs g_q AND g_k: it is formed from them
 *   scratch            gsasr_window_attn_rope_scratch_bytes(descriptor) bytes, 256-byte aligned, for the backward when g_angles
 *                      is set (set it before asking): the slices' partial sums, every word written before it is read
 * GSASR_ERR_ARG before anything is enqueued: windows or heads below 1, nq or nk outside 1..256, head_dim odd or outside 2..32,
 * angle_rows < max(nq, nk), flags other than 0, a NaN scale, a null or misaligned pointer among those the call needs, g_angles
 * without g_q or g_k. */
typedef struct gsasr_window_attn_rope {
    int windows, heads, nq, nk, head_dim, angle_rows;
    float scale;
    unsigned flags;       /* 0 (none defined) */
    const float *q, *k, *v, *angles;
    float *out;           /* written by the forward, read by the backward */
    float *stats;
    const float *grad_out;
    float *g_q, *g_k, *g_v, *g_angles;
    float *cossin;
    void *scratch;
} gsasr_window_attn_rope;
GSASR_API size_t gsasr_window_attn_rope_scratch_bytes(const gsasr_window_attn_rope *attn);   /* 0 on bad arguments (only g_angles among the pointers is looked at) */
GSASR_API int gsasr_window_attn_rope_forward(const gsasr_window_attn_rope *attn, void *stream);
GSASR_API int gsasr_window_attn_rope_backward(const gsasr_window_attn_rope *attn, void *stream);

/* The two window attentions with bf16 activations: what the decoder's Linears hand over under torch.autocast(dtype=bfloat16)
 * (the AMP and UltraPerformance models).  Same formulas, layouts, limits and entry points as gsasr_window_attn and
 * gsasr_window_attn_rope above; the descriptors have the same fields in the same order, with the eight activation pointers
 * typed gsasr_bf16 (a bf16 is the upper half of the fp32 with the same value).  The numerical contract:
 *
 *   q, k, v, out, grad_out, g_q, g_k, g_v   bf16 in memory;  table, angles, stats, cossin, g_table, g_angles   fp32, as above
 *   every product accumulates in fp32.  S = scale * (sum_c q[i, c] k[j, c]) (+ B_h[i, j], fp32, added to the finished score):
 *   `scale` multiplies the fp32 score SUM, never an operand before it is rounded.  The softmax sees the whole row in fp32: one
 *   maximum m, one sum l of the unrounded fp32 p = exp(S - m).  p is rounded to bf16 (nearest even) ONLY as the operand of
 *   P v:  out = (sum_j bf16(p_j) v_j) / l, rounded to bf16 once at the store;  stats = m + log l in fp32.
 *   Rotary variant: the rotation is evaluated in fp32 from the accurate cossin table, then R(q) and R(k) are rounded to bf16
 *   (the reference's apply_rotary_emb_single rotates x.float() and returns type_as(x)); the backward recomputes S from the
 *   same bf16-rounded rotated operands, so the statistic is of the forward's scores up to the fp32 summation order.
 *   Backward: dS, dP and delta stay fp32 (the products run on the exact-fp32 matrix instruction on the widened operands);
 *   delta is formed from the bf16 out that was stored; g_q, g_k, g_v are rounded to bf16 at the store; g_table and g_angles
 *   are accumulated and stored in fp32 as above (g_angles from the stored bf16 g_q, g_k).
 *   out, g_q, g_k, g_v and g_angles are written once by their owner, without atomics: two calls give the same bits.
 *
 * The forward runs on v_mfma_f32_16x16x32_bf16: one matrix instruction per 16 x 16 score tile.  Its loads are chosen by the
 * alignment of a head's slice: 16 bytes at a time when head_dim % 8 == 0 and q, k, v are 16-byte aligned, 4 bytes for an even
 * head_dim and 4-byte aligned q, k, v, else 2 bytes.
 * GSASR_ERR_ARG as for the fp32 descriptors; in addition an activation pointer the call needs that is not 2-byte aligned
 * (rotary variant: 4-byte, for the pair loads). */
typedef unsigned short gsasr_bf16;
typedef struct gsasr_window_attn_bf16 {
    int windows, heads, nq, nk, head_dim, table_rows;
    float scale;
    unsigned flags;       /* 0 (none defined) */
    const gsasr_bf16 *q, *k, *v;
    const float *table;
    const int *index;
    gsasr_bf16 *out;      /* written by the forward, read by the backward */
    float *stats;
    const gsasr_bf16 *grad_out;
    gsasr_bf16 *g_q, *g_k, *g_v;
    float *g_table;
    void *scratch;
} gsasr_window_attn_bf16;
GSASR_API size_t gsasr_window_attn_bf16_scratch_bytes(const gsasr_window_attn_bf16 *attn);   /* as gsasr_window_attn_scratch_bytes */
GSASR_API int gsasr_window_attn_bf16_forward(const gsasr_window_attn_bf16 *attn, void *stream);
GSASR_API int gsasr_window_attn_bf16_backward(const gsasr_window_attn_bf16 *attn, void *stream);

typedef struct gsasr_window_attn_rope_bf16 {
    int windows, heads, nq, nk, head_dim, angle_rows;
    float scale;
    unsigned flags;       /* 0 (none defined) */
    const gsasr_bf16 *q, *k, *v;
    const float *angles;
    gsasr_bf16 *out;      /* written by the forward, read by the backward */
    float *stats;
    const gsasr_bf16 *grad_out;
    gsasr_bf16 *g_q, *g_k, *g_v;
    float *g_angles;
    float *cossin;        /* 8-byte aligned */
    void *scratch;
} gsasr_window_attn_rope_bf16;
GSASR_API size_t gsasr_window_attn_rope_bf16_scratch_bytes(const gsasr_window_attn_rope_bf16 *attn);   /* as gsasr_window_attn_rope_scratch_bytes */
GSASR_API int gsasr_window_attn_rope_bf16_forward(const gsasr_window_attn_rope_bf16 *attn, void *stream);
GSASR_API int gsasr_window_attn_rope_bf16_backward(const gsasr_window_attn_rope_bf16 *attn, void *stream);

/* The biased window attention with an additive mask per window and q, k, v read in place from a packed tensor: the attention
 * of a Swin layer (SwinIR's WindowAttention, utils/swinir.py:226-257 -- one Linear writes [windows, n, 3 heads head_dim], every
 * second layer adds its shifted-window mask).  gsasr_window_attn's formulas, layouts, limits and guarantees, word for word
 * (exact softmax over the whole row, the log-sum-exp statistic, one owner per output row and no atomics for out, g_q, g_k, g_v,
 * the table gradient's two paths), with
 *
 *   S = (scale q[w, :, h] k[w, :, h]^T + B_h) + M_(w mod mask_windows)      in this order of fp32 additions (torch's)
 *
 *   mask           const float [mask_windows, nq, nk], fp32 for both element types; window w reads mask[w % mask_windows];
 *                  windows % mask_windows == 0.  mask == NULL with mask_windows == 0: no mask.  The entries must be finite --
 *                  NOT checked here, like the index (a row of -inf has no softmax).  The mask gets no gradient.
 *   pitch_q, pitch_k, pitch_v   elements between consecutive rows of q / k / v: row (w, i) of q starts at
 *                  q + (w nq + i) pitch_q, of k and v at k + (w nk + j) pitch_k and v + (w nk + j) pitch_v.  0 = heads * head_dim
 *                  (contiguous).  A packed qkv tensor [windows, n, 3 C], C = heads * head_dim: q = qkv, k = qkv + C,
 *                  v = qkv + 2 C, all three pitches 3 C.
 *   pitch_gq, pitch_gk, pitch_gv   the same for g_q, g_k, g_v (one [windows, n, 3 C] gradient is written in place).
 *                  out, grad_out and stats stay contiguous.
 *
 * The forward and both backward kernels form S by the same chain, mask included: the statistic is of the forward's bits.
 * gsasr_window_attn_masked_bf16 follows the bf16 contract above; the mask is added to the fp32 score sum after `scale` and the
 * bias.  Its forward chooses the load width from the base pointers AND the pitches (16 bytes: head_dim % 8 == 0, 16-byte aligned
 * q, k, v and pitches that are multiples of 8; 4 bytes: an even head_dim, 4-byte aligned q, k, v, even pitches; else 2 bytes;
 * a pitch counts elements, so every pitch keeps the 2-byte rule).  Mask rows are read 16 bytes at a time when nk % 4 == 0 and
 * mask is 16-byte aligned.
 * GSASR_ERR_ARG before anything is enqueued: what gsasr_window_attn (or _bf16) refuses; mask_windows < 0; windows not a
 * multiple of mask_windows; mask without mask_windows or mask_windows without mask; a non-zero pitch below heads * head_dim. */
typedef struct gsasr_window_attn_masked {
    int windows, heads, nq, nk, head_dim, table_rows;
    float scale;
    unsigned flags;       /* 0 (none defined) */
    const float *q, *k, *v, *table;
    const int *index;
    float *out;           /* written by the forward, read by the backward */
    float *stats;
    const float *grad_out;
    float *g_q, *g_k, *g_v, *g_table;
    void *scratch;
    const float *mask;
    int mask_windows;
    int pitch_q, pitch_k, pitch_v, pitch_gq, pitch_gk, pitch_gv;
} gsasr_window_attn_masked;
GSASR_API size_t gsasr_window_attn_masked_scratch_bytes(const gsasr_window_attn_masked *attn);   /* as gsasr_window_attn_scratch_bytes */
GSASR_API int gsasr_window_attn_masked_forward(const gsasr_window_attn_masked *attn, void *stream);
GSASR_API int gsasr_window_attn_masked_backward(const gsasr_window_attn_masked *attn, void *stream);

typedef struct gsasr_window_attn_masked_bf16 {
    int windows, heads, nq, nk, head_dim, table_rows;
    float scale;
    unsigned flags;       /* 0 (none defined) */
    const gsasr_bf16 *q, *k, *v;
    const float *table;
    const int *index;
    gsasr_bf16 *out;      /* written by the forward, read by the backward */
    float *stats;
    const gsasr_bf16 *grad_out;
    gsasr_bf16 *g_q, *g_k, *g_v;
    float *g_table;
    void *scratch;
    const float *mask;    /* fp32 */
    int mask_windows;
    int pitch_q, pitch_k, pitch_v, pitch_gq, pitch_gk, pitch_gv;
} gsasr_window_attn_masked_bf16;
GSASR_API size_t gsasr_window_attn_masked_bf16_scratch_bytes(const gsasr_window_attn_masked_bf16 *attn);   /* as gsasr_window_attn_scratch_bytes */
GSASR_API int gsasr_window_attn_masked_bf16_forward(const gsasr_window_attn_masked_bf16 *attn, void *stream);
GSASR_API int gsasr_window_attn_masked_bf16_backward(const gsasr_window_attn_masked_bf16 *attn, void *stream);

/* Sampled pixels.  With `sample_coords` the reference renders the whole [3,H,W] image and
 * then picks the S requested pixels out of it, one indexing op per point (utils/gaussian_splatting.py:214-216;
 * the points come from basicsr/data/continuous_bicubic_downsample_dataset.py:86-88).  These entry points evaluate
 * only those pixels: forward = the values out[3, n_points] at the points (one wave per point, its lanes spread over
 * the Gaussians binned within reach), backward = the gradient of sum(grad_out * out) (one wave per Gaussian, its
 * lanes spread over the points inside its window, found through a counting sort of the points).
 *
 *   points    device int32 [n_points, 2] = (row, column) on the image's own grid; negative values wrap once like
 *             Python indices; a point that is still out of range yields 0 and takes no part in the backward
 *             (the reference raises IndexError -- checking would cost a host synchronisation).  Repeated points
 *             are evaluated independently, as the reference's gather does.
 *   out / grad_out   [3, n_points], written (not accumulated).
 *   batched canvas (dims.batch = B): points [B, n_points, 2] on each sample's own grid, out [B, 3, n_points].
 *   workspace a plan of the same dims (gsasr_splat_plan, or the step entry point below); the whole image
 *             (row0 = 0, row1 = h).  Flags: OVERWRITE_GRADS / STRIDE8 as for gsasr_splat_backward.
 *   sample_ws scratch of gsasr_sample_workspace_bytes(dims, n_points) bytes, 256-byte aligned: the sorted points.
 *             The backward re-sorts `points`, or, given points = NULL, uses what the forward call left there.
 * The step variants fuse the host prologue exactly as gsasr_step_forward / gsasr_step_backward do. */
GSASR_API size_t gsasr_sample_workspace_bytes(const gsasr_dims *dims, int n_points);
GSASR_API int gsasr_splat_sample_forward(const gsasr_dims *dims, const void *workspace, size_t workspace_bytes, const int *points,
                               int n_points, float *out, void *sample_ws, size_t sample_ws_bytes, void *stream);
GSASR_API int gsasr_splat_sample_backward(const float *sigmas, const float *coords, const float *colors, const float *grad_out,
                                float *g_sigmas, float *g_coords, float *g_colors, const gsasr_dims *dims,
                                const void *workspace, size_t workspace_bytes, const int *points, int n_points,
                                void *sample_ws, size_t sample_ws_bytes, void *stream);
GSASR_API int gsasr_step_sample_forward(const float *gs_parameters, const float *step_size, const gsasr_dims *dims, void *workspace,
                              size_t workspace_bytes, const int *points, int n_points, float *out, void *sample_ws,
                              size_t sample_ws_bytes, void *stream);
GSASR_API int gsasr_step_sample_forward_sm(const float *gs_parameters, const float *scale_modify, int sm_stride,
                                 float default_step_size, int *mismatch, const gsasr_dims *dims, void *workspace,
                                 size_t workspace_bytes, const int *points, int n_points, float *out, void *sample_ws,
                                 size_t sample_ws_bytes, void *stream);
GSASR_API int gsasr_step_sample_backward(const float *gs_parameters, const float *step_size, const float *grad_out,
                               float *g_parameters, const gsasr_dims *dims, void *workspace, size_t workspace_bytes,
                               const int *points, int n_points, void *sample_ws, size_t sample_ws_bytes, void *stream);

/* Queries at fractional pixel positions: the set of Gaussians is a continuous image, evaluated anywhere on the closed grid
 * rectangle.  The five entry points mirror the sampled-pixel ones argument for argument, with float points:
 *
 *   points    device float32 [n_points, 2] = fractional pixel indices (r, c) on the image's own h x w grid (batched canvas:
 *             [B, n_points, 2] on sample b's own h_b x w_b).  The point sits at
 *                 px = (float)(2.0 * (double)c / (double)(w - 1) - 1.0),  py = (float)(2.0 * (double)r / (double)(h - 1) - 1.0)
 *             -- the pixel tables' own expression with a real index: integer-valued (r, c) give the tables' floats bit for
 *             bit, and the value there IS pixel (r, c).  The value at a point is the op's own sum at (px, py): same exponent,
 *             same |dx|, |dy| <= dmax test per term (bounded op), same cutoff rules and the same 1e-5 * max|colour| bound of
 *             the adaptive cutoff.  Domain: 0 <= r <= h - 1 and 0 <= c <= w - 1, both ends included; a point outside it or
 *             with a NaN / infinite component yields 0 and takes no part in the backward (no wrap-around).  Repeated points
 *             are independent outputs whose gradients add.
 *   workspace a plan made with GSASR_FLAG_CONTINUOUS (gsasr_splat_plan; the step forms set the flag and list_cap = -1
 *             themselves).  The plan-API forms on a workspace whose plan lacks the flag: GSASR_ERR_PLAN -- never a silently
 *             incomplete sum.  The integer sampled points may be evaluated on a continuous plan too (same terms).
 *   out, grad_out, sample_ws (gsasr_sample_workspace_bytes serves both kinds), points = NULL in the backward, flags, errors:
 *             as for the sampled pixels.
 * gsasr_*_query_backward is the gradient of sum(grad_out * out) with respect to the Gaussians; the gradient with respect to the
 * positions themselves is a call of its own, gsasr_*_query_backward_points below. */
GSASR_API int gsasr_splat_query_forward(const gsasr_dims *dims, const void *workspace, size_t workspace_bytes, const float *points,
                              int n_points, float *out, void *sample_ws, size_t sample_ws_bytes, void *stream);
GSASR_API int gsasr_splat_query_backward(const float *sigmas, const float *coords, const float *colors, const float *grad_out,
                               float *g_sigmas, float *g_coords, float *g_colors, const gsasr_dims *dims,
                               const void *workspace, size_t workspace_bytes, const float *points, int n_points,
                               void *sample_ws, size_t sample_ws_bytes, void *stream);
GSASR_API int gsasr_step_query_forward(const float *gs_parameters, const float *step_size, const gsasr_dims *dims, void *workspace,
                             size_t workspace_bytes, const float *points, int n_points, float *out, void *sample_ws,
                             size_t sample_ws_bytes, void *stream);
GSASR_API int gsasr_step_query_forward_sm(const float *gs_parameters, const float *scale_modify, int sm_stride,
                                float default_step_size, int *mismatch, const gsasr_dims *dims, void *workspace,
                                size_t workspace_bytes, const float *points, int n_points, float *out, void *sample_ws,
                                size_t sample_ws_bytes, void *stream);
GSASR_API int gsasr_step_query_backward(const float *gs_parameters, const float *step_size, const float *grad_out,
                              float *g_parameters, const gsasr_dims *dims, void *workspace, size_t workspace_bytes,
                              const float *points, int n_points, void *sample_ws, size_t sample_ws_bytes, void *stream);

/* Gradient of a query with respect to its POSITIONS: g_points[s] = d sum(grad_out * out) / d (r_s, c_s).  With, for point s at
 * (px, py) and Gaussian j, dx = px - x_j, dy = py - y_j, u = dx / sigma_x, v = dy / sigma_y, B = v - rho u,
 * t_sj = exp(-(u^2 + B^2 / (1 - rho^2)) / 2) (0 outside the dmax box, bounded op) and w_sj = sum_k grad_out[k, s] * colour[j, k]:
 *       g_px[s] = sum_j w_sj t_sj * -(u - rho B / (1 - rho^2)) / sigma_x        g_py[s] = sum_j w_sj t_sj * -B / ((1 - rho^2) sigma_y)
 *       g_points[s] = (g_py[s] * 2 / (h - 1), g_px[s] * 2 / (w - 1))            (d/dr, d/dc; h, w: the sample's own grid)
 * The sum runs over the terms the query forward sums (same cutoff rules).  It is the derivative almost everywhere: neither
 * the box test nor the float rounding of px, py is differentiated; a point on the edge of the closed domain gets the analytic
 * value (no projection); a point outside the domain or with a NaN / infinite component gets (0, 0); dead and non-finite
 * Gaussians contribute nothing; repeated points are independent rows.  One point-stationary kernel, no global atomics.
 *   workspace a GSASR_FLAG_CONTINUOUS plan (else GSASR_ERR_PLAN).  Only the forward's records are read: a plan made with
 *             GSASR_FLAG_FORWARD_ONLY is accepted, so positions can be fitted against frozen Gaussians on an inference plan.
 *   grad_out  device float32 [3, n_points] ([B, 3, n_points]), as for gsasr_splat_query_backward.
 *   points    as for the forward, or NULL: sample_ws still holds what the forward (or a backward) sorted.
 *   g_points  device float32 [n_points, 2] ([B, n_points, 2]); every row is WRITTEN, whatever GSASR_FLAG_OVERWRITE_GRADS says.
 *   sample_ws gsasr_sample_workspace_bytes(dims, n_points) bytes, 256-byte aligned (else GSASR_ERR_WORKSPACE).  The call
 *             gathers grad_out into it itself: it does not matter whether a Gaussian backward ran before.
 * n_points == 0: GSASR_OK, nothing touched; n_points < 0 or a null grad_out / g_points with n_points > 0: GSASR_ERR_ARG;
 * dims.s == 0: zeros.  The step form takes the dims and the workspace of gsasr_step_query_forward[_sm] (it sets list_cap = -1
 * and GSASR_FLAG_CONTINUOUS itself, as gsasr_step_query_backward does) and needs no gs_parameters. */
GSASR_API int gsasr_splat_query_backward_points(const gsasr_dims *dims, const void *workspace, size_t workspace_bytes,
                                      const float *grad_out, const float *points, int n_points, float *g_points,
                                      void *sample_ws, size_t sample_ws_bytes, void *stream);
GSASR_API int gsasr_step_query_backward_points(const gsasr_dims *dims, void *workspace, size_t workspace_bytes,
                                     const float *grad_out, const float *points, int n_points, float *g_points,
                                     void *sample_ws, size_t sample_ws_bytes, void *stream);

/* Reference-shaped launchers: the argument lists of `_gs_render` / `_gs_render_backward` in utils/gs_cuda/gs.h:4-24 and
 * utils/gs_cuda_dmax/gs.h:4-26 (+ the stream, + a status instead of void).  The reference's launchers take no workspace,
 * so these keep their plan scratch per (device, stream) between calls (allocated stream-ordered on first use, reused in
 * stream order, re-planned on every call -- a backward never trusts the plan of an earlier forward: the arrays may have
 * changed); gsasr_release_launcher_scratch() frees what they hold. */
GSASR_API int gsasr_release_launcher_scratch(void);
GSASR_API int gsasr_gs_render(const float *sigmas, const float *coords, const float *colors,
                    float *rendered_img, int s, int h, int w, int c, void *stream);
GSASR_API int gsasr_gs_render_backward(const float *sigmas, const float *coords, const float *colors,
                             const float *grads, float *grads_sigmas, float *grads_coords,
                             float *grads_colors, int s, int h, int w, int c, void *stream);
GSASR_API int gsasr_gs_render_dmax(const float *sigmas, const float *coords, const float *colors,
                         float *rendered_img, int s, int h, int w, int c, float dmax, void *stream);
GSASR_API int gsasr_gs_render_backward_dmax(const float *sigmas, const float *coords, const float *colors,
                                  const float *grads, float *grads_sigmas, float *grads_coords,
                                  float *grads_colors, int s, int h, int w, int c, float dmax,
                                  void *stream);

/* Row-band shard (one process per GPU): neighbour exchange of the Gaussians whose footprint
 * crosses an edge of this rank's band.  The reference has no counterpart (its rasterizer is rank-local,
 * basicsr/models/base_model.py:96-99); these two kernels are the device side of gsasr_amd/shard.py.
 *
 * gsasr_band_select: `packed` is this rank's [s,8] Gaussians, dims = FULL grid h,w with [row0,row1) the
 * rank's band, dmax/cutoff as for the plan (the footprint is the plan's own row window: box ∩ support).
 * Gaussians reaching rows < row0 are appended to up[cap,8] (+ their index to up_index[cap]), those reaching
 * rows >= row1 to down/down_index; unused slots are filled with NaN records, which every kernel of this
 * library treats as dead Gaussians.  counts[4] (device) = {n_up, n_down, n_far, 0}: n_up/n_down may exceed
 * `cap` (overflow: the excess was dropped -- the caller must check and re-run with a larger cap), n_far =
 * Gaussians reaching beyond the adjacent band (more than rows_above above row0 / rows_below below row1),
 * which a nearest-neighbour exchange cannot serve.  rows_above/rows_below = 0: no neighbour on that side.
 *
 * gsasr_band_merge: g_packed[index[j], :] += g_up[j, :] for j < min(n_up, cap), same for down: adds the
 * partial gradients a neighbour computed for the records it was sent. */
GSASR_API int gsasr_band_select(const float *packed, const gsasr_dims *dims, int rows_above, int rows_below, int cap,
                      float *up, float *down, int *up_index, int *down_index, int *counts, void *stream);
GSASR_API int gsasr_band_merge(float *g_packed, int s, const float *g_up, const float *g_down, const int *up_index,
                     const int *down_index, const int *counts, int cap, void *stream);

/* Process-wide default used when dims.cutoff == 0: 0 = adaptive (initial state), otherwise a fixed tau
 * (initially the value of the environment variable GSASR_SPLAT_CUTOFF if set).  gsasr_resolve_cutoff
 * returns the tau a plan with dims.cutoff = `cutoff` over `s` Gaussians uses. */
GSASR_API void gsasr_set_default_cutoff(float tau);
GSASR_API float gsasr_get_default_cutoff(void);
GSASR_API float gsasr_resolve_cutoff(float cutoff, int s);

/* The cutoff the windows of the plan in `workspace` were actually built with (synchronises `stream`; for reports and
 * tests): under the adaptive default the data-derived tau' described above, *k_box = its K (0 when the cutoff is not
 * data-derived: explicit tau without GSASR_FLAG_CUTOFF_CAP, GSASR_SPLAT_ADAPT=0). */
GSASR_API int gsasr_plan_cutoff(const gsasr_dims *dims, const void *workspace, size_t workspace_bytes, void *stream,
                                float *tau, unsigned *k_box);

/* Which forward kernel gsasr_splat_forward runs for these dims (flags included; no device work; for reports and tests):
 * the width of a wave's sub-tile in pixels -- 16 = the wide forward (16 x 16 sub-tiles, four pixels per lane: scale factors
 * from x5 up on single images of 2 Mpx and more, or GSASR_FLAG_FWD_WIDE), 8 = the 8 x 16 kernels.  < 0: invalid dims. */
GSASR_API int gsasr_forward_subtile_width(const gsasr_dims *dims);

/* Kernel choices registered per problem shape (round 5; gsasr_amd/tune.py measures and registers them).
 * The library picks its kernels -- 8 x 16 or 16 x 16 forward sub-tiles, Gaussian- or tile-stationary backward, tile lists or the
 * search -- from the SHAPE of the problem (pixels per Gaussian, image size): the window sizes that really decide live on the device,
 * and no entry point synchronises to read them.  On Gaussians much smaller or larger than "about one LR pixel" another
 * combination can be 5..45% faster (profiles/history/r05_policy_regret.txt).  A caller who knows better -- it timed the combinations on
 * its own data -- registers the choice once; every later plan / forward / backward whose dims match `shape` in {s, h, w, row0,
 * row1, batch, slot, dmax, cutoff, GSASR_FLAG_FORWARD_ONLY} and carry NO explicit choice of their own (flags below, list_cap != 0)
 * behaves as if it had been given
 *     flags    : any of GSASR_FLAG_FWD_WIDE | GSASR_FLAG_FWD_NARROW, GSASR_FLAG_BWD_TILE | GSASR_FLAG_BWD_GAUSSIAN
 *     list_cap : as gsasr_dims.list_cap (0 = the library's rule, > 0 entries per tile, < 0 no lists).
 * Results are the same sums in another order.  Register BEFORE sizing workspaces for the shape (gsasr_splat_workspace_bytes
 * follows the registered choice; a workspace sized earlier may be too small and is refused, never overrun).  A workspace that
 * has been planned keeps its plan's layout (slots, tile lists, the step scratch behind them) whatever is registered, switched or
 * cleared afterwards: only the kernel its calls pick may follow the new choice.  Process-wide,
 * thread-safe; at most 256 shapes (GSASR_ERR_ARG beyond, or on flags outside the four above). */
GSASR_API int gsasr_set_kernel_choice(const gsasr_dims *shape, unsigned flags, int list_cap);
/* 1 and the registered values if `shape` has a registered choice, else 0 */
GSASR_API int gsasr_get_kernel_choice(const gsasr_dims *shape, unsigned *flags, int *list_cap);
GSASR_API void gsasr_clear_kernel_choices(void);

#ifdef __cplusplus
}
#endif
#endif /* GSASR_SPLAT_H */
