// splat_resize.hip -- MATLAB-compatible bicubic imresize (GSASR's degradation: basicsr/utils/matlab_functions.py imresize /
// imresize_new, called by the dataset on every GT crop) and its adjoint, batched, on planar fp32 images: gsasr_imresize,
// gsasr_imresize_backward (one translation unit of libgsasr_splat.so; include/gsasr_splat.h has the contract)
//
//   k_resize_weights   one thread per (sample, axis, output index): the first tap `left` and the p normalised weights of that
//                      output, computed in double from the formulas of the header and rounded once to float, into the tables
//                      both passes read.  Forward and backward build the same tables.
//   k_resize_rows      H pass: one wave per output row and 64 columns, four consecutive output rows per workgroup; the p input
//                      rows are read coalesced along w (neighbouring output rows share 3/4 of their taps: those reads meet in
//                      L1 / L2), the weights through the scalar unit (the row is wave-uniform).  Writes the intermediate
//                      [out_h, w_b] to scratch.
//   k_resize_cols      W pass: one workgroup per 32 intermediate rows x TOX output columns.  The stretch of the rows under the
//                      tile's taps is staged once, coalesced and already reflected, into LDS (32 x 256 floats, pitch 257: the 32
//                      rows of a half-wave fall on 32 banks) in chunks of 256 taps, so any tap count runs through the same code;
//                      lane = row, so an output column's weights are uniform over a half-wave.  The tile goes back through LDS
//                      to be stored in whole row segments.
//   k_resize_cols_adj  adjoint of the W pass in gather form: one thread per (row, input column x); the outputs whose window
//   k_resize_rows_adj  can hold x, -1-x or 2w-1-x are a short range around (k - c) s, walked in a fixed order, each checked
//                      against the table's `left`.  The H adjoint is the same over rows: the list is the row's, so a wave
//                      walks it once for 256 columns.  No atomics anywhere.
// Every scratch word that is read was written by the same call; no memset, no allocation, no host synchronisation.
#include "splat_common.h"

using namespace gsasr_detail;

namespace {

constexpr unsigned RZ_KNOWN = GSASR_RESIZE_NO_ANTIALIAS | GSASR_RESIZE_ACCUMULATE | GSASR_RESIZE_SHARED_SCALE;
constexpr int RZ_ROWS = 32;             // rows of a W-pass tile
constexpr int RZ_SPAN = 256;            // taps staged per chunk
constexpr int RZ_PITCH = RZ_SPAN + 1;
constexpr int RZ_TOX_MAX = 64;          // output columns of a W-pass tile (a multiple of 8, at most this)
constexpr double RZ_KW_MAX = 4.0 * 32767.0;     // a wider kernel cannot keep its taps within one reflection of 32767 pixels

struct ResizeArgs {
    const float *in;        // backward: grad_in (written)
    const float *out;       // backward: grad_out (read)
    float *tmp;             // [batch][channels][out_h][in_w]
    float *wt;              // [entries][pw]
    int *left;              // [entries]: 0-based first tap; entry of (b, axis, o) = b * (out_h + out_w) + axis * out_h + o
    size_t in_pitch, in_plane, in_stride, out_pitch, out_plane, out_stride;     // in floats
    int batch, channels, in_w, out_h, out_w, pw, tox;
    unsigned flags;
    unsigned short hw[2 * GSASR_MAX_BATCH];
    int p[2 * GSASR_MAX_BATCH];
    double scale[2 * GSASR_MAX_BATCH];
    double shift[2 * GSASR_MAX_BATCH];      // 0.5 (1 - 1 / scale)
};

__host__ __device__ inline double rz_cubic(double x)
{
    const double a = fabs(x), a2 = a * a, a3 = a2 * a;
    if (a <= 1.0) return 1.5 * a3 - 2.5 * a2 + 1.0;
    if (a <= 2.0) return -0.5 * a3 + 2.5 * a2 - 4.0 * a + 2.0;
    return 0.0;
}

// output o (0-based) of an axis with scale s: u (1-based input coordinate) and the 1-based first tap
__host__ __device__ inline void rz_window(int o, double s, double kw, double *u, double *left1)
{
    *u = (double)(o + 1) / s + 0.5 * (1.0 - 1.0 / s);
    *left1 = floor(*u - kw / 2.0);
}

__host__ __device__ inline double rz_raw(double u, double k1, double s, bool shrink)
{
    return shrink ? s * rz_cubic((u - k1) * s) : rz_cubic(u - k1);
}

__host__ __device__ inline int rz_reflect(int k, int n)
{
    const int r = k < 0 ? -1 - k : k >= n ? 2 * n - 1 - k : k;
    return r < 0 ? 0 : r >= n ? n - 1 : r;      // (a tap beyond one reflection has weight 0: the host checked)
}

__global__ __launch_bounds__(256) void k_resize_weights(ResizeArgs A)
{
    const int per = A.out_h + A.out_w, e = blockIdx.x * 256 + threadIdx.x;
    if (e >= A.batch * per) return;
    const int b = e / per, r = e - b * per, axis = r >= A.out_h, o = axis ? r - A.out_h : r;
    const double s = A.scale[2 * b + axis];
    const int p = A.p[2 * b + axis];
    const bool shrink = s < 1.0 && !(A.flags & GSASR_RESIZE_NO_ANTIALIAS);
    const double kw = shrink ? 4.0 / s : 4.0;
    double u, left1;
    rz_window(o, s, kw, &u, &left1);
    double sum = 0.0;
    for (int t = 0; t < p; ++t) sum += rz_raw(u, left1 + (double)t, s, shrink);
    float *w = A.wt + (size_t)e * A.pw;
    for (int t = 0; t < p; ++t) w[t] = (float)(rz_raw(u, left1 + (double)t, s, shrink) / sum);
    for (int t = p; t < A.pw; ++t) w[t] = 0.f;
    A.left[e] = (int)left1 - 1;
}

__global__ __launch_bounds__(256) void k_resize_rows(ResizeArgs A)
{
    const int z = blockIdx.z, b = z / A.channels, c = z - b * A.channels;
    const int h = A.hw[2 * b], w = A.hw[2 * b + 1], p = A.p[2 * b];
    const int x = blockIdx.x * 64 + (threadIdx.x & 63);
    const int oy = __builtin_amdgcn_readfirstlane(blockIdx.y * 4 + (threadIdx.x >> 6));
    if (oy >= A.out_h || x >= w) return;
    const int e = b * (A.out_h + A.out_w) + oy, l = A.left[e];
    const float *__restrict__ wt = A.wt + (size_t)e * A.pw;
    const float *__restrict__ src = A.in + (size_t)b * A.in_stride + (size_t)c * A.in_plane + x;
    float acc = 0.f;
    for (int t = 0; t < p; ++t) acc = fmaf(wt[t], src[(size_t)rz_reflect(l + t, h) * A.in_pitch], acc);
    A.tmp[((size_t)z * A.out_h + oy) * A.in_w + x] = acc;
}

__global__ __launch_bounds__(256) void k_resize_cols(ResizeArgs A)
{
    __shared__ float s_t[RZ_ROWS * RZ_PITCH];
    const int z = blockIdx.z, b = z / A.channels, c = z - b * A.channels, tid = threadIdx.x;
    const int w = A.hw[2 * b + 1], p = A.p[2 * b + 1];
    const int row = tid & 31, oxl = tid >> 5;
    const int oy0 = blockIdx.y * RZ_ROWS, ox0 = blockIdx.x * A.tox;
    const int nrows = min(RZ_ROWS, A.out_h - oy0), nx = min(A.tox, A.out_w - ox0);
    const int eb = b * (A.out_h + A.out_w) + A.out_h;
    const int kmin = A.left[eb + ox0], kmax = A.left[eb + ox0 + nx - 1] + p;
    const float *__restrict__ src = A.tmp + ((size_t)z * A.out_h + oy0) * A.in_w;
    float acc[RZ_TOX_MAX / 8];
#pragma unroll
    for (int j = 0; j < RZ_TOX_MAX / 8; ++j) acc[j] = 0.f;
    for (int c0 = kmin; c0 < kmax; c0 += RZ_SPAN) {
        const int n = min(RZ_SPAN, kmax - c0);
        for (int i = tid; i < RZ_ROWS * RZ_SPAN; i += 256) {
            const int r = i >> 8, j = i & (RZ_SPAN - 1);
            if (r < nrows && j < n) s_t[r * RZ_PITCH + j] = src[(size_t)r * A.in_w + rz_reflect(c0 + j, w)];
        }
        __syncthreads();
        if (row < nrows) {
#pragma unroll
            for (int j = 0; j < RZ_TOX_MAX / 8; ++j) {
                const int ox = oxl + 8 * j;
                if (ox >= nx) continue;
                const int l = A.left[eb + ox0 + ox];
                const float *__restrict__ wt = A.wt + (size_t)(eb + ox0 + ox) * A.pw;
                const int t0 = max(0, c0 - l), t1 = min(p, c0 + n - l);
                const float *sr = s_t + row * RZ_PITCH + (l - c0);
                for (int t = t0; t < t1; ++t) acc[j] = fmaf(wt[t], sr[t], acc[j]);
            }
        }
        __syncthreads();
    }
    // the tile back through LDS: stored in whole row segments
    constexpr int OP = RZ_TOX_MAX + 1;
#pragma unroll
    for (int j = 0; j < RZ_TOX_MAX / 8; ++j) s_t[row * OP + oxl + 8 * j] = acc[j];
    __syncthreads();
    float *dst = const_cast<float *>(A.out) + (size_t)b * A.out_stride + (size_t)c * A.out_plane + (size_t)oy0 * A.out_pitch + ox0;
    for (int i = tid; i < RZ_ROWS * RZ_TOX_MAX; i += 256) {
        const int r = i >> 6, xx = i & 63;
        if (r < nrows && xx < nx) dst[(size_t)r * A.out_pitch + xx] = s_t[r * OP + xx];
    }
}

// The outputs (0-based, clipped to [0, m)) whose window can hold tap k (0-based, any sign) with a non-zero weight:
// |u_o - k1| < kw / 2 with u_o = o1 / s + c, so |o1 - (k1 - c) s| < kw s / 2; one more on either side for the rounding.
__device__ __forceinline__ void rz_outputs_of(int k, double s, double shift, bool shrink, int m, int *lo, int *hi)
{
    const double oc = ((double)(k + 1) - shift) * s, half = shrink ? 2.0 : 2.0 * s;
    const double a = floor(oc - half) - 2.0, z = ceil(oc + half);        // 1-based o1 in [a + 1, z + 1] -> 0-based [a, z]
    *lo = a < 0.0 ? 0 : a > (double)m ? m : (int)a;
    *hi = z < -1.0 ? -1 : z >= (double)m ? m - 1 : (int)z;
}

// sum over the outputs o of an axis (n inputs, m outputs, table entries e0 .. e0 + m - 1) whose window holds input i directly or
// through one reflection, in a fixed order, of weight * g[o * gstride]
__device__ __forceinline__ float rz_gather(const ResizeArgs &A, int i, int n, int m, int e0, int p, double s, double shift, bool shrink,
                                           const float *__restrict__ g, size_t gstride)
{
    float acc = 0.f;
#pragma unroll
    for (int which = 0; which < 3; ++which) {
        const int k = which == 0 ? i : which == 1 ? -1 - i : 2 * n - 1 - i;
        int lo, hi;
        rz_outputs_of(k, s, shift, shrink, m, &lo, &hi);
        for (int o = lo; o <= hi; ++o) {
            const int t = k - A.left[e0 + o];
            if (t >= 0 && t < p) acc = fmaf(A.wt[(size_t)(e0 + o) * A.pw + t], g[(size_t)o * gstride], acc);
        }
    }
    return acc;
}

// gtmp[z, oy, x] = sum over ox of ww[ox][tap that reads x] * grad_out[z, oy, ox]
__global__ __launch_bounds__(256) void k_resize_cols_adj(ResizeArgs A)
{
    const int z = blockIdx.z, b = z / A.channels, c = z - b * A.channels;
    const int w = A.hw[2 * b + 1], p = A.p[2 * b + 1];
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), oy = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (oy >= A.out_h || x >= w) return;
    const double s = A.scale[2 * b + 1];
    const bool shrink = s < 1.0 && !(A.flags & GSASR_RESIZE_NO_ANTIALIAS);
    const float *__restrict__ g = A.out + (size_t)b * A.out_stride + (size_t)c * A.out_plane + (size_t)oy * A.out_pitch;
    A.tmp[((size_t)z * A.out_h + oy) * A.in_w + x] = rz_gather(A, x, w, A.out_w, b * (A.out_h + A.out_w) + A.out_h, p, s, A.shift[2 * b + 1], shrink, g, 1);
}

// grad_in[z, y, x] (+)= sum over oy of wh[oy][tap that reads y] * gtmp[z, oy, x]: the list of (oy, tap) belongs to the row, so a
// wave walks it once for 256 columns, four per lane
__global__ __launch_bounds__(256) void k_resize_rows_adj(ResizeArgs A)
{
    const int z = blockIdx.z, b = z / A.channels, c = z - b * A.channels;
    const int h = A.hw[2 * b], w = A.hw[2 * b + 1], p = A.p[2 * b];
    const int x0 = blockIdx.x * 256 + (threadIdx.x & 63);
    const int y = __builtin_amdgcn_readfirstlane(blockIdx.y * 4 + (threadIdx.x >> 6));
    if (y >= h || x0 >= w) return;
    const double s = A.scale[2 * b];
    const bool shrink = s < 1.0 && !(A.flags & GSASR_RESIZE_NO_ANTIALIAS);
    const int e0 = b * (A.out_h + A.out_w);
    const float *__restrict__ g = A.tmp + (size_t)z * A.out_h * A.in_w + x0;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int which = 0; which < 3; ++which) {
        const int k = which == 0 ? y : which == 1 ? -1 - y : 2 * h - 1 - y;
        int lo, hi;
        rz_outputs_of(k, s, A.shift[2 * b], shrink, A.out_h, &lo, &hi);
        for (int o = lo; o <= hi; ++o) {
            const int t = k - A.left[e0 + o];
            if (t < 0 || t >= p) continue;
            const float wgt = A.wt[(size_t)(e0 + o) * A.pw + t];
            const float *__restrict__ go = g + (size_t)o * A.in_w;
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (x0 + 64 * i < w) acc[i] = fmaf(wgt, go[64 * i], acc[i]);
        }
    }
    float *dst = const_cast<float *>(A.in) + (size_t)b * A.in_stride + (size_t)c * A.in_plane + (size_t)y * A.in_pitch + x0;
#pragma unroll
    for (int i = 0; i < 4; ++i)
        if (x0 + 64 * i < w) dst[64 * i] = (A.flags & GSASR_RESIZE_ACCUMULATE) ? dst[64 * i] + acc[i] : acc[i];
}

// one axis of one sample: n inputs, m outputs, scale s.  Sets *p; fails when a tap with a non-zero weight lies beyond one
// reflection (the taps reach furthest at the first and the last output: u grows with o)
int rz_axis_check(int n, int m, double s, bool antialias, int *p)
{
    if (!(s > 0.0) || !std::isfinite(s)) return fail(GSASR_ERR_ARG, "a scale is not a positive finite number");
    const bool shrink = s < 1.0 && antialias;
    const double kw = shrink ? 4.0 / s : 4.0;
    if (!(kw <= RZ_KW_MAX)) return fail(GSASR_ERR_ARG, "a tap with non-zero weight lies beyond one reflection of the input (scale too small for this length)");
    *p = (int)ceil(kw) + 2;
    for (int end = 0; end < 2; ++end) {
        double u, left1;
        rz_window(end ? m - 1 : 0, s, kw, &u, &left1);
        if (!(fabs(left1) < 1e9)) return fail(GSASR_ERR_ARG, "a tap with non-zero weight lies beyond one reflection of the input");
        int first = 0, last = *p - 1;
        while (first < *p && rz_raw(u, left1 + first, s, shrink) == 0.0) ++first;
        while (last >= 0 && rz_raw(u, left1 + last, s, shrink) == 0.0) --last;
        if (first > last) return fail(GSASR_ERR_ARG, "an output has no tap with a non-zero weight");
        // 0-based taps left1 - 1 + t must lie in [-n, 2n - 1]
        if (left1 - 1.0 + first < -(double)n || left1 - 1.0 + last > 2.0 * n - 1.0)
            return fail(GSASR_ERR_ARG, "a tap with non-zero weight lies beyond one reflection of the input (the reference's symmetric copy fails there too)");
    }
    return GSASR_OK;
}

// everything gsasr_resize_scratch_bytes depends on (the host arrays are read, the device pointers are not looked at)
int resize_geometry_check(const gsasr_resize *r, ResizeArgs *A)
{
    if (!r) return fail(GSASR_ERR_ARG, "null resize descriptor");
    if (r->batch < 1 || r->batch > GSASR_MAX_BATCH) return fail(GSASR_ERR_ARG, "batch must be 1..GSASR_MAX_BATCH");
    if (r->channels < 1 || r->channels > 65535 / r->batch) return fail(GSASR_ERR_ARG, "need channels >= 1 and batch * channels <= 65535");
    if (r->in_h < 1 || r->in_w < 1 || r->in_h > 32767 || r->in_w > 32767 || r->out_h < 1 || r->out_w < 1 || r->out_h > 32767 || r->out_w > 32767)
        return fail(GSASR_ERR_ARG, "need 1 <= in_h, in_w, out_h, out_w <= 32767");
    if (r->flags & ~RZ_KNOWN) return fail(GSASR_ERR_ARG, "unknown flags (GSASR_RESIZE_NO_ANTIALIAS, _ACCUMULATE, _SHARED_SCALE)");
    if (!r->scales) return fail(GSASR_ERR_ARG, "null scales");
    if (r->in_pitch < 4 * (size_t)r->in_w || r->out_pitch < 4 * (size_t)r->out_w) return fail(GSASR_ERR_ARG, "a pitch is below the row's bytes");
    if ((r->in_pitch | r->in_plane | r->in_stride | r->out_pitch | r->out_plane | r->out_stride) & 3u)
        return fail(GSASR_ERR_ARG, "pitches, plane and sample strides must be multiples of 4 bytes");
    int pw = 0;
    double smin = INFINITY;
    for (int b = 0; b < r->batch; ++b) {
        const int h = r->sample_hw ? r->sample_hw[2 * b] : r->in_h, w = r->sample_hw ? r->sample_hw[2 * b + 1] : r->in_w;
        if (h < 1 || w < 1) return fail(GSASR_ERR_ARG, "a sample has no pixel");
        if (h > r->in_h || w > r->in_w) return fail(GSASR_ERR_ARG, "a sample is larger than in_h x in_w");
        for (int axis = 0; axis < 2; ++axis) {
            const double s = r->scales[((r->flags & GSASR_RESIZE_SHARED_SCALE) ? 0 : 2 * b) + axis];
            int p;
            if (int rc = rz_axis_check(axis ? w : h, axis ? r->out_w : r->out_h, s, !(r->flags & GSASR_RESIZE_NO_ANTIALIAS), &p)) return rc;
            pw = p > pw ? p : pw;
            if (axis) smin = s < smin ? s : smin;
            if (A) { A->p[2 * b + axis] = p; A->scale[2 * b + axis] = s; A->shift[2 * b + axis] = 0.5 * (1.0 - 1.0 / s); }
        }
        if (A) { A->hw[2 * b] = (unsigned short)h; A->hw[2 * b + 1] = (unsigned short)w; }
    }
    if (A) {
        A->pw = pw;
        // the widest W-pass tile whose taps fit one staged chunk: p + (tox - 1) / s <= RZ_SPAN
        const double fit = pw < RZ_SPAN ? floor((double)(RZ_SPAN - pw) * smin) + 1.0 : 8.0;
        A->tox = fit >= RZ_TOX_MAX ? RZ_TOX_MAX : fit < 8.0 ? 8 : (int)fit / 8 * 8;
    }
    return GSASR_OK;
}

struct ResizeLayout { size_t off_wt, off_tmp, total; };

ResizeLayout resize_layout(const gsasr_resize *r, int pw)
{
    ResizeLayout L;
    const size_t entries = (size_t)r->batch * ((size_t)r->out_h + (size_t)r->out_w);
    L.off_wt = align_up(entries * sizeof(int), 256);
    L.off_tmp = L.off_wt + align_up(entries * (size_t)pw * sizeof(float), 256);
    L.total = L.off_tmp + align_up((size_t)r->batch * (size_t)r->channels * (size_t)r->out_h * (size_t)r->in_w * sizeof(float), 256);
    return L;
}

int resize_args(const gsasr_resize *r, ResizeArgs *A)
{
    if (int rc = resize_geometry_check(r, A)) return rc;
    if (!r->in || !r->out || !r->scratch) return fail(GSASR_ERR_ARG, "null in, out or scratch pointer");
    if (((uintptr_t)r->in | (uintptr_t)r->out) & 3u) return fail(GSASR_ERR_ARG, "in and out must be 4-byte aligned");
    if ((uintptr_t)r->scratch & 15u) return fail(GSASR_ERR_ARG, "scratch must be 16-byte aligned");
    const ResizeLayout L = resize_layout(r, A->pw);
    A->in = r->in; A->out = r->out;
    A->left = (int *)r->scratch;
    A->wt = (float *)((char *)r->scratch + L.off_wt);
    A->tmp = (float *)((char *)r->scratch + L.off_tmp);
    A->in_pitch = r->in_pitch / 4; A->in_plane = r->in_plane / 4; A->in_stride = r->in_stride / 4;
    A->out_pitch = r->out_pitch / 4; A->out_plane = r->out_plane / 4; A->out_stride = r->out_stride / 4;
    A->batch = r->batch; A->channels = r->channels; A->in_w = r->in_w; A->out_h = r->out_h; A->out_w = r->out_w;
    A->flags = r->flags;
    return GSASR_OK;
}

inline unsigned rz_div(int n, int d) { return (unsigned)((n + d - 1) / d); }

}  // namespace

extern "C" {

size_t gsasr_resize_scratch_bytes(const gsasr_resize *r)
{
    ResizeArgs A;
    if (resize_geometry_check(r, &A)) return 0;
    return resize_layout(r, A.pw).total;
}

int gsasr_imresize(const gsasr_resize *r, void *stream)
{
    ResizeArgs A;
    if (int rc = resize_args(r, &A)) return rc;
    if (r->flags & GSASR_RESIZE_ACCUMULATE) return fail(GSASR_ERR_ARG, "GSASR_RESIZE_ACCUMULATE belongs to gsasr_imresize_backward");
    hipStream_t st = (hipStream_t)stream;
    const dim3 block(256);
    const unsigned planes = (unsigned)(A.batch * A.channels);
    hipLaunchKernelGGL(k_resize_weights, dim3(rz_div(A.batch * (A.out_h + A.out_w), 256)), block, 0, st, A);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_resize_rows, dim3(rz_div(A.in_w, 64), rz_div(A.out_h, 4), planes), block, 0, st, A);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_resize_cols, dim3(rz_div(A.out_w, A.tox), rz_div(A.out_h, RZ_ROWS), planes), block, 0, st, A);
    HIP_TRY(hipGetLastError());
    return GSASR_OK;
}

int gsasr_imresize_backward(const gsasr_resize *r, void *stream)
{
    ResizeArgs A;
    if (int rc = resize_args(r, &A)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const dim3 block(256);
    const unsigned planes = (unsigned)(A.batch * A.channels);
    hipLaunchKernelGGL(k_resize_weights, dim3(rz_div(A.batch * (A.out_h + A.out_w), 256)), block, 0, st, A);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_resize_cols_adj, dim3(rz_div(A.in_w, 64), rz_div(A.out_h, 4), planes), block, 0, st, A);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_resize_rows_adj, dim3(rz_div(A.in_w, 256), rz_div(r->in_h, 4), planes), block, 0, st, A);
    HIP_TRY(hipGetLastError());
    return GSASR_OK;
}

}  // extern "C"
