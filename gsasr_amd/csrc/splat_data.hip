// splat_data.hip -- the dataset's per-sample work as one batched call: from decoded 8-bit images resident on the device to the
// collated tensors of a training step (basicsr/data/continuous_bicubic_downsample_dataset.py:46-111: crop, /255, bicubic LR,
// flips / transposition, BGR -> RGB, HWC -> CHW, zero padding or sampled pixels): gsasr_batch_make, gsasr_batch_pick (one
// translation unit of libgsasr_splat.so; include/gsasr_splat.h has the contract)
//
//   k_batch_crop   one workgroup per 32 x 32 pixels of a sample's GT slot.  The source pixels under the tile are a rectangle of
//                  the crop whichever the augmentation (rows and columns change places for a transposed sample).  The tile is
//                  written twice in whole row segments: augmented into the GT slot, zeros outside the sample's extent, and
//                  un-augmented into the planar crop the resize reads; each pixel's three bytes are read where they lie (96
//                  contiguous bytes per 32 lanes for an untransposed sample, 32 rows for a transposed one: the tile's 3 KB
//                  stay in L1 for the second pass).  Staging the rectangle in LDS as aligned dwords first, so that neither side
//                  walks a column, was built and measured no faster: this is the simpler form.
//   k_batch_d4     the same flips / transposition on the small planar LR images after the resize (resize first, augment
//                  second: the reference's order); one thread per output pixel.
//   k_batch_pick   the sampled GT: one thread per point, straight from the bytes through the same index map.
// Per-sample parameters travel by value (BatchArgs: 64 samples * 24 bytes, under the 4 KiB kernarg limit).  No memset, no
// allocation, no host synchronisation; every scratch word that is read was written by the same call.
#include "splat_common.h"

using namespace gsasr_detail;

namespace {

constexpr unsigned BT_AUG_KNOWN = GSASR_BATCH_HFLIP | GSASR_BATCH_VFLIP | GSASR_BATCH_TRANSPOSE;
constexpr unsigned BT_KNOWN = GSASR_BATCH_BGR | GSASR_BATCH_NO_ANTIALIAS;
constexpr int BT_TILE = 32;             // the tile of k_batch_crop, pixels each way

struct BatchSample {
    const unsigned char *src;           // the whole image [h, w, 3]
    unsigned short h, w, y0, x0, gh, gw, aug, pad;
};

struct BatchArgs {
    float *gt;                          // [batch, 3, gt_h, gt_w], or null
    float *crop;                        // [batch, 3, crop_h, crop_w], or null
    const int *points;                  // k_batch_pick: [batch, n_points, 2]
    float *picked;                      // k_batch_pick: [batch, 3, n_points]
    int batch, gt_h, gt_w, crop_h, crop_w, n_points;
    unsigned flags;
    BatchSample s[GSASR_MAX_BATCH];
};
static_assert(sizeof(BatchArgs) <= 2048, "BatchArgs travels by value: keep it well under the 4 KiB kernarg limit");

struct D4Args {
    const float *in;                    // [batch, 3, h, w]
    float *out;                         // [batch, 3, h, w] (a transposed sample needs h == w)
    int batch, h, w;
    unsigned char aug[GSASR_MAX_BATCH];
};

// pixel (r, c) of the augmented sample reads pixel (*cy, *cx) of the crop: horizontal flip, then vertical flip, then transposition
__device__ __forceinline__ void bt_source_of(int r, int c, unsigned aug, int gh, int gw, int *cy, int *cx)
{
    const int fr = (aug & GSASR_BATCH_TRANSPOSE) ? c : r, fc = (aug & GSASR_BATCH_TRANSPOSE) ? r : c;
    *cy = (aug & GSASR_BATCH_VFLIP) ? gh - 1 - fr : fr;
    *cx = (aug & GSASR_BATCH_HFLIP) ? gw - 1 - fc : fc;
}

__device__ __forceinline__ float bt_value(unsigned byte) { return (float)byte / 255.0f; }     // one correctly rounded division

__global__ __launch_bounds__(256) void k_batch_crop(BatchArgs A)
{
    const int b = blockIdx.z, tid = threadIdx.x;
    const BatchSample S = A.s[b];
    const int gh = S.gh, gw = S.gw;
    const unsigned aug = S.aug;
    const bool tr = (aug & GSASR_BATCH_TRANSPOSE) != 0u;
    const int eh = tr ? gw : gh, ew = tr ? gh : gw;     // the augmented sample's extent
    const int oy0 = blockIdx.y * BT_TILE, ox0 = blockIdx.x * BT_TILE;
    const int oy1 = min(oy0 + BT_TILE, eh), ox1 = min(ox0 + BT_TILE, ew);
    // the rectangle of the crop under the tile: rows [sy0, sy0 + nrows), columns [sx0, sx0 + ncols)
    int sy0 = 0, sx0 = 0, nrows = 0, ncols = 0;
    if (oy1 > oy0 && ox1 > ox0) {
        const int fr0 = tr ? ox0 : oy0, fr1 = tr ? ox1 : oy1, fc0 = tr ? oy0 : ox0, fc1 = tr ? oy1 : ox1;
        sy0 = (aug & GSASR_BATCH_VFLIP) ? gh - fr1 : fr0;  nrows = fr1 - fr0;
        sx0 = (aug & GSASR_BATCH_HFLIP) ? gw - fc1 : fc0;  ncols = fc1 - fc0;
    }
    const size_t pitch = 3 * (size_t)S.w;
    const unsigned char *first = S.src + (size_t)(S.y0 + sy0) * pitch + 3 * (size_t)(S.x0 + sx0);      // byte 0 of the rectangle
    // pixel (row, col) of the rectangle: its three bytes in the low 24 bits
    auto pixel = [&](int row, int col) -> unsigned {
        const unsigned char *q = first + (size_t)row * pitch + 3 * col;
        return (unsigned)q[0] | (unsigned)q[1] << 8 | (unsigned)q[2] << 16;
    };
    const bool bgr = (A.flags & GSASR_BATCH_BGR) != 0u;
    const int lx = tid & 31, ly0 = tid >> 5;
    // (a) the augmented GT, zeros outside the sample's extent
    float *__restrict__ gt = A.gt + (size_t)b * 3 * A.gt_h * A.gt_w;
    const size_t gplane = (size_t)A.gt_h * A.gt_w;
#pragma unroll
    for (int k = 0; k < BT_TILE / 8; ++k) {
        const int r = oy0 + ly0 + 8 * k, c = ox0 + lx;
        if (!A.gt || r >= A.gt_h || c >= A.gt_w) continue;
        float v0 = 0.f, v1 = 0.f, v2 = 0.f;
        if (r < eh && c < ew) {
            int cy, cx;
            bt_source_of(r, c, aug, gh, gw, &cy, &cx);
            const unsigned px = pixel(cy - sy0, cx - sx0);
            v0 = bt_value(px & 255u); v1 = bt_value((px >> 8) & 255u); v2 = bt_value((px >> 16) & 255u);
        }
        float *dst = gt + (size_t)r * A.gt_w + c;
        dst[0] = bgr ? v2 : v0; dst[gplane] = v1; dst[2 * gplane] = bgr ? v0 : v2;
    }
    // (b) the un-augmented crop, for the resize
    if (!A.crop) return;
    float *__restrict__ crop = A.crop + (size_t)b * 3 * A.crop_h * A.crop_w;
    const size_t cplane = (size_t)A.crop_h * A.crop_w;
#pragma unroll
    for (int k = 0; k < BT_TILE / 8; ++k) {
        const int row = ly0 + 8 * k;
        if (row >= nrows || lx >= ncols) continue;
        const unsigned px = pixel(row, lx);
        const float v0 = bt_value(px & 255u), v1 = bt_value((px >> 8) & 255u), v2 = bt_value((px >> 16) & 255u);
        float *dst = crop + (size_t)(sy0 + row) * A.crop_w + sx0 + lx;
        dst[0] = bgr ? v2 : v0; dst[cplane] = v1; dst[2 * cplane] = bgr ? v0 : v2;
    }
}

__global__ __launch_bounds__(256) void k_batch_d4(D4Args A)
{
    const int z = blockIdx.z, b = z / 3;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= A.h * A.w) return;
    const int r = i / A.w, c = i - r * A.w;
    int cy, cx;
    bt_source_of(r, c, A.aug[b], A.h, A.w, &cy, &cx);      // (a transposed sample is square: the host checked)
    const size_t plane = (size_t)z * A.h * A.w;
    A.out[plane + i] = A.in[plane + (size_t)cy * A.w + cx];
}

__global__ __launch_bounds__(256) void k_batch_pick(BatchArgs A)
{
    const int b = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    if (i >= A.n_points) return;
    const BatchSample S = A.s[b];
    const int gh = S.gh, gw = S.gw;
    const bool tr = (S.aug & GSASR_BATCH_TRANSPOSE) != 0u;
    const int eh = tr ? gw : gh, ew = tr ? gh : gw;
    const int *__restrict__ p = A.points + 2 * ((size_t)b * A.n_points + i);
    int r = p[0], c = p[1];
    if (r < 0) r += eh;     // Python's wrap-around of negative indices, once
    if (c < 0) c += ew;
    float v0 = 0.f, v1 = 0.f, v2 = 0.f;
    if (r >= 0 && r < eh && c >= 0 && c < ew) {
        int cy, cx;
        bt_source_of(r, c, S.aug, gh, gw, &cy, &cx);
        const unsigned char *px = S.src + ((size_t)(S.y0 + cy) * S.w + (size_t)(S.x0 + cx)) * 3;
        v0 = bt_value(px[0]); v1 = bt_value(px[1]); v2 = bt_value(px[2]);
    }
    const bool bgr = (A.flags & GSASR_BATCH_BGR) != 0u;
    float *dst = A.picked + (size_t)b * 3 * A.n_points + i;
    dst[0] = bgr ? v2 : v0; dst[A.n_points] = v1; dst[2 * (size_t)A.n_points] = bgr ? v0 : v2;
}

// the samples: sources, windows, augmentation bits (everything gsasr_batch_pick needs).  Sets the largest window.
int batch_samples_check(const gsasr_batch *d, BatchArgs *A, int *gh_max, int *gw_max)
{
    if (!d) return fail(GSASR_ERR_ARG, "null batch descriptor");
    if (d->batch < 1 || d->batch > GSASR_MAX_BATCH) return fail(GSASR_ERR_ARG, "batch must be 1..GSASR_MAX_BATCH");
    if (d->flags & ~BT_KNOWN) return fail(GSASR_ERR_ARG, "unknown flags (GSASR_BATCH_BGR, _NO_ANTIALIAS)");
    if (!d->src || !d->src_hw || !d->window) return fail(GSASR_ERR_ARG, "null src, src_hw or window array");
    *gh_max = *gw_max = 0;
    for (int b = 0; b < d->batch; ++b) {
        const int h = d->src_hw[2 * b], w = d->src_hw[2 * b + 1];
        const int y0 = d->window[4 * b], x0 = d->window[4 * b + 1], gh = d->window[4 * b + 2], gw = d->window[4 * b + 3];
        const unsigned aug = d->aug ? d->aug[b] : 0u;
        if (!d->src[b]) return fail(GSASR_ERR_ARG, "a null source image");
        if (h < 1 || w < 1 || h > 32767 || w > 32767) return fail(GSASR_ERR_ARG, "a source image's h, w must be 1..32767");
        if (gh < 1 || gw < 1) return fail(GSASR_ERR_ARG, "a window has no pixel");
        if (y0 < 0 || x0 < 0 || gh > h - y0 || gw > w - x0) return fail(GSASR_ERR_ARG, "a window lies outside its source image");
        if (aug & ~BT_AUG_KNOWN) return fail(GSASR_ERR_ARG, "unknown augmentation bits (GSASR_BATCH_HFLIP, _VFLIP, _TRANSPOSE)");
        *gh_max = gh > *gh_max ? gh : *gh_max;
        *gw_max = gw > *gw_max ? gw : *gw_max;
        A->s[b] = BatchSample{d->src[b], (unsigned short)h, (unsigned short)w, (unsigned short)y0, (unsigned short)x0,
                              (unsigned short)gh, (unsigned short)gw, (unsigned short)aug, 0};
    }
    A->batch = d->batch;
    A->flags = d->flags;
    return GSASR_OK;
}

struct BatchLayout { size_t off_lr, off_resize, total; };

// everything gsasr_batch_scratch_bytes depends on (the host arrays are read; gt, lq and scratch are not looked at).  Fills the
// resize's descriptor except for its pointers; `hw` and `scales` are the host arrays it reads during the call
int batch_geometry_check(const gsasr_batch *d, BatchArgs *A, gsasr_resize *R, int *hw, double *scales, BatchLayout *L)
{
    int gh_max, gw_max;
    if (int rc = batch_samples_check(d, A, &gh_max, &gw_max)) return rc;
    if (d->gt_h < 1 || d->gt_w < 1 || d->gt_h > 32767 || d->gt_w > 32767 || d->lr_h < 1 || d->lr_w < 1 || d->lr_h > 32767 || d->lr_w > 32767)
        return fail(GSASR_ERR_ARG, "need 1 <= gt_h, gt_w, lr_h, lr_w <= 32767");
    bool any = false;
    for (int b = 0; b < d->batch; ++b) {
        const BatchSample &S = A->s[b];
        const bool tr = (S.aug & GSASR_BATCH_TRANSPOSE) != 0u;
        if ((tr ? S.gw : S.gh) > d->gt_h || (tr ? S.gh : S.gw) > d->gt_w) return fail(GSASR_ERR_ARG, "the GT slot gt_h x gt_w is smaller than a sample");
        if (tr && d->lr_h != d->lr_w) return fail(GSASR_ERR_ARG, "a transposed sample needs lr_h == lr_w");
        any = any || S.aug != 0;
        hw[2 * b] = S.gh; hw[2 * b + 1] = S.gw;
        scales[2 * b] = (double)d->lr_h / (double)S.gh; scales[2 * b + 1] = (double)d->lr_w / (double)S.gw;
    }
    A->gt_h = d->gt_h; A->gt_w = d->gt_w; A->crop_h = gh_max; A->crop_w = gw_max;
    memset(R, 0, sizeof *R);
    R->batch = d->batch; R->channels = 3; R->in_h = gh_max; R->in_w = gw_max; R->sample_hw = hw; R->scales = scales;
    R->out_h = d->lr_h; R->out_w = d->lr_w;
    R->in_pitch = 4 * (size_t)gw_max; R->in_plane = R->in_pitch * gh_max; R->in_stride = 3 * R->in_plane;
    R->out_pitch = 4 * (size_t)d->lr_w; R->out_plane = R->out_pitch * d->lr_h; R->out_stride = 3 * R->out_plane;
    R->flags = (d->flags & GSASR_BATCH_NO_ANTIALIAS) ? GSASR_RESIZE_NO_ANTIALIAS : 0u;
    const size_t rz = gsasr_resize_scratch_bytes(R);        // the resize's own argument errors, the reflection condition among them
    if (rz == 0) return GSASR_ERR_ARG;                      // (its message stands)
    L->off_lr = align_up((size_t)d->batch * R->in_stride, 256);
    // the un-augmented LR images: only when a sample is augmented, else the resize writes lq itself
    L->off_resize = L->off_lr + (any ? align_up((size_t)d->batch * R->out_stride, 256) : 0);
    L->total = L->off_resize + align_up(rz, 256);
    return any ? 1 : GSASR_OK;
}

inline unsigned bt_div(int n, int d) { return (unsigned)((n + d - 1) / d); }

}  // namespace

extern "C" {

size_t gsasr_batch_scratch_bytes(const gsasr_batch *d)
{
    BatchArgs A;
    gsasr_resize R;
    int hw[2 * GSASR_MAX_BATCH];
    double scales[2 * GSASR_MAX_BATCH];
    BatchLayout L;
    if (batch_geometry_check(d, &A, &R, hw, scales, &L) < 0) return 0;
    return L.total;
}

int gsasr_batch_make(const gsasr_batch *d, void *stream)
{
    BatchArgs A;
    gsasr_resize R;
    int hw[2 * GSASR_MAX_BATCH];
    double scales[2 * GSASR_MAX_BATCH];
    BatchLayout L;
    const int any = batch_geometry_check(d, &A, &R, hw, scales, &L);
    if (any < 0) return any;
    if (!d->lq || !d->scratch) return fail(GSASR_ERR_ARG, "null lq or scratch pointer");
    if (((uintptr_t)d->gt | (uintptr_t)d->lq) & 3u) return fail(GSASR_ERR_ARG, "gt and lq must be 4-byte aligned");
    if ((uintptr_t)d->scratch & 255u) return fail(GSASR_ERR_ARG, "scratch must be 256-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    A.gt = d->gt;
    A.crop = (float *)d->scratch;
    A.points = nullptr; A.picked = nullptr; A.n_points = 0;
    hipLaunchKernelGGL(k_batch_crop, dim3(bt_div(A.gt_w, BT_TILE), bt_div(A.gt_h, BT_TILE), (unsigned)A.batch), dim3(256), 0, st, A);
    HIP_TRY(hipGetLastError());
    float *lr = any ? (float *)((char *)d->scratch + L.off_lr) : d->lq;
    R.in = A.crop; R.out = lr; R.scratch = (char *)d->scratch + L.off_resize;
    if (int rc = gsasr_imresize(&R, stream)) return rc;
    if (any) {
        D4Args D;
        D.in = lr; D.out = d->lq; D.batch = A.batch; D.h = d->lr_h; D.w = d->lr_w;
        for (int b = 0; b < A.batch; ++b) D.aug[b] = (unsigned char)A.s[b].aug;
        hipLaunchKernelGGL(k_batch_d4, dim3(bt_div(D.h * D.w, 256), 1, (unsigned)(3 * A.batch)), dim3(256), 0, st, D);
        HIP_TRY(hipGetLastError());
    }
    return GSASR_OK;
}

int gsasr_batch_pick(const gsasr_batch *d, const int *points, int n_points, float *out, void *stream)
{
    BatchArgs A;
    int gh_max, gw_max;
    if (int rc = batch_samples_check(d, &A, &gh_max, &gw_max)) return rc;
    if (n_points < 1 || n_points > (1 << 24)) return fail(GSASR_ERR_ARG, "n_points must be 1..2^24");
    if (!points || !out) return fail(GSASR_ERR_ARG, "null points or out pointer");
    if (((uintptr_t)points | (uintptr_t)out) & 3u) return fail(GSASR_ERR_ARG, "points and out must be 4-byte aligned");
    A.gt = nullptr; A.crop = nullptr; A.gt_h = A.gt_w = A.crop_h = A.crop_w = 0;
    A.points = points; A.picked = out; A.n_points = n_points;
    hipLaunchKernelGGL(k_batch_pick, dim3(bt_div(n_points, 256), (unsigned)A.batch), dim3(256), 0, (hipStream_t)stream, A);
    HIP_TRY(hipGetLastError());
    return GSASR_OK;
}

}  // extern "C"
