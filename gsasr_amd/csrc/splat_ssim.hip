// splat_ssim.hip -- the SSIM loss of a rendered batch (GSASR's cri_ssim: basicsr/losses/basic_loss.py:256-264, i.e.
// loss_weight * (1 - pytorch_msssim.ssim(x, y, data_range=1))) and its gradient with respect to the image: gsasr_ssim_loss
// (one translation unit of libgsasr_splat.so; include/gsasr_splat.h has the formulas)
//
//   k_ssim_stats   one workgroup per (32 x 32 tile of the valid map, channel, sample): the 42 x 42 patches of x and y staged in
//                  LDS, the 11-tap window over the five products x, y, x^2, y^2, xy along the rows (into LDS), then along the
//                  columns (four map rows per lane, in registers), the map and -- for the gradient -- its derivatives with respect
//                  to mu1, s1 and s12 written to scratch; the tile's sum of 1 - map is one partial.
//   k_ssim_grad    one workgroup per 32 x 32 tile of the image: the window is symmetric, so the transposed ("full") stencil
//                  is the same two passes over the derivative maps padded with zeros; combined with x and y, scaled by c_b and
//                  stored or added into grad_img, planar or interleaved.
//   k_ssim_reduce  the partials of every sample added in a fixed order in double (the pattern of k_loss_reduce).
// Numerics: s = g*(x^2) - mu^2 cancels, and so does the gradient's mu-term against its x-term -- in a flat region, where the
// map is most sensitive (B2 small), to the last digits fp32 has.  Variances and covariance do not change when a constant is
// taken off x and y, so k_ssim_stats takes off a LOCAL one: the row pass forms the moments of every output about its own centre
// pixel, the column pass moves them to the pixel in the middle of the lane's rows before it weights them -- the squares that
// cancel are those of the image's variation within the window, not of its level.  For the gradient both kernels work on
// x - cx and y - cy, cx and cy being the sample's centre pixel of the channel, and d map / d mu1 is stored as the part that
// does not cancel,
//   D0 = 2 cs (mu2 - mu1) (mu2 (mu1 + mu2) + C1) / B1^2 - 2 (mu1 - cx) d map / d s1 - (mu2 - cy) d map / d s12,
//   grad = c_b [ gT*D0 + 2 (x - cx) gT*(d map / d s1) + (y - cy) gT*(d map / d s12) ]   (the same sums, regrouped).
// No float atomics, no memset: every scratch word that is read was written by this call, and two calls give the same bits.
#include "splat_common.h"

using namespace gsasr_detail;

namespace {

constexpr int SS_T = 32;            // tile side (map pixels in k_ssim_stats, image pixels in k_ssim_grad)
constexpr int SS_P = SS_T + 10;     // ... and of the patch under an 11-tap window
constexpr float SS_C1 = 0.01f * 0.01f, SS_C2 = 0.03f * 0.03f;

// g[i] = exp(-(i - 5)^2 / (2 * 1.5^2)) / sum, i = 0..10, by distance from the centre (computed in double, rounded once)
__device__ __forceinline__ constexpr float ss_g(int j)
{
    const int d = j < 5 ? 5 - j : j - 5;
    return d == 0 ? 2.660117249e-01f : d == 1 ? 2.130055377e-01f : d == 2 ? 1.093606895e-01f
         : d == 3 ? 3.600077213e-02f : d == 4 ? 7.598758135e-03f : 1.028380084e-03f;
}

struct SsimArgs {
    const float *img, *target;
    float *grad;        // null: value only
    float *part;        // [batch][3][tiles] sums of 1 - map
    float *dmap;        // [batch][3 channels][3 maps][rows * w]: D0 (above), d map / d s1, d map / d s12 on the valid pixels
    float *loss;
    int batch, rows, w, trows, grows;
    int ntx, ntiles;    // tiles of the valid map per row of tiles / in all (k_ssim_stats)
    int gtx;            // tiles of the image per row of tiles (k_ssim_grad)
    float weight;
    unsigned short hw[2 * GSASR_MAX_BATCH];     // (h_b, w_b)
};

// the window along the columns: lane (col, rg) owns rows 4 rg .. 4 rg + 3 of its column and reads rows 4 rg .. 4 rg + 13 of the
// row-filtered planes s_h[N][SS_P * SS_T] once each
template <int N>
__device__ __forceinline__ void ss_vertical(const float (*s_h)[SS_P * SS_T], int col, int rg, float (&acc)[N][4])
{
#pragma unroll
    for (int p = 0; p < N; ++p)
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[p][q] = 0.f;
#pragma unroll
    for (int k = 0; k < 14; ++k)
#pragma unroll
        for (int p = 0; p < N; ++p) {
            const float v = s_h[p][(rg * 4 + k) * SS_T + col];
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (k - q >= 0 && k - q < 11) acc[p][q] = fmaf(ss_g(k - q), v, acc[p][q]);
        }
}

template <bool GRAD>
__global__ __launch_bounds__(256) void k_ssim_stats(SsimArgs A)
{
    __shared__ float s_x[SS_P * SS_P], s_y[SS_P * SS_P];
    __shared__ float s_h[5][SS_P * SS_T];
    __shared__ float s_red[4];
    const int b = blockIdx.z, ch = blockIdx.y, tid = threadIdx.x;
    const int h = A.hw[2 * b], w = A.hw[2 * b + 1], vh = h - 10, vw = w - 10;
    const int ty0 = (int)(blockIdx.x / (unsigned)A.ntx) * SS_T, tx0 = (int)(blockIdx.x % (unsigned)A.ntx) * SS_T;
    float *part = A.part + ((size_t)b * 3 + ch) * A.ntiles + blockIdx.x;
    if (ty0 >= vh || tx0 >= vw) {       // a tile of the padding (the whole workgroup): its partial is still written
        if (tid == 0) *part = 0.f;
        return;
    }
    const float *__restrict__ x = A.img + ((size_t)b * 3 + ch) * A.rows * A.w;
    const float *__restrict__ y = A.target + ((size_t)b * 3 + ch) * A.trows * A.w;
    const float cx = x[(size_t)(h / 2) * A.w + w / 2], cy = y[(size_t)(h / 2) * A.w + w / 2];
    for (int i = tid; i < SS_P * SS_P; i += 256) {
        const int r = i / SS_P, c = i - r * SS_P;
        const int gy = ty0 + r, gx = tx0 + c;
        const bool in = gy < h && gx < w;       // the sample's own pixels only: padding is never read
        s_x[i] = in ? x[(size_t)gy * A.w + gx] - cx : 0.f;
        s_y[i] = in ? y[(size_t)gy * A.w + gx] - cy : 0.f;
    }
    __syncthreads();
    const int col = tid & 31, rg = tid >> 5;
    // along the rows, each output about ITS OWN centre pixel (ac, bc): moments of x - ac, y - bc (the local shift, above)
    for (int r = rg; r < SS_P; r += 8) {
        float m1 = 0.f, m2 = 0.f, xx = 0.f, yy = 0.f, xy = 0.f;
        const float ac = s_x[r * SS_P + col + 5], bc = s_y[r * SS_P + col + 5];
#pragma unroll
        for (int j = 0; j < 11; ++j) {
            const float a = s_x[r * SS_P + col + j] - ac, c = s_y[r * SS_P + col + j] - bc;
            const float ga = ss_g(j) * a, gc = ss_g(j) * c;
            m1 += ga; m2 += gc;
            xx = fmaf(ga, a, xx); yy = fmaf(gc, c, yy); xy = fmaf(ga, c, xy);
        }
        s_h[0][r * SS_T + col] = m1; s_h[1][r * SS_T + col] = m2;
        s_h[2][r * SS_T + col] = xx; s_h[3][r * SS_T + col] = yy; s_h[4][r * SS_T + col] = xy;
    }
    __syncthreads();
    // along the columns: every row's moments are moved to the lane's reference (a0, b0) -- the pixel in the middle of the 14 rows
    // it reads -- before they are weighted: E(x - a0) = E(x - ac) + (ac - a0), E(x - a0)^2 = E(x - ac)^2 + (ac - a0) (2 E(x - ac) +
    // (ac - a0)), E(x - a0)(y - b0) likewise (the taps sum to 1 - 1.4e-9).  All of it stays as small as the image is flat HERE.
    float acc[5][4];
#pragma unroll
    for (int p = 0; p < 5; ++p)
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[p][q] = 0.f;
    const float a0 = s_x[(rg * 4 + 7) * SS_P + col + 5], b0 = s_y[(rg * 4 + 7) * SS_P + col + 5];
#pragma unroll
    for (int k = 0; k < 14; ++k) {
        const int row = rg * 4 + k;
        const float da = s_x[row * SS_P + col + 5] - a0, db = s_y[row * SS_P + col + 5] - b0;
        const float h1 = s_h[0][row * SS_T + col], h2 = s_h[1][row * SS_T + col];
        float v[5];
        v[0] = h1 + da;
        v[1] = h2 + db;
        v[2] = fmaf(da, fmaf(2.f, h1, da), s_h[2][row * SS_T + col]);
        v[3] = fmaf(db, fmaf(2.f, h2, db), s_h[3][row * SS_T + col]);
        v[4] = fmaf(da, h2 + db, fmaf(db, h1, s_h[4][row * SS_T + col]));
#pragma unroll
        for (int p = 0; p < 5; ++p)
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (k - q >= 0 && k - q < 11) acc[p][q] = fmaf(ss_g(k - q), v[p], acc[p][q]);
    }
    float *__restrict__ dm = A.dmap + ((size_t)b * 3 + ch) * 3 * (size_t)A.rows * A.w;
    const size_t plane = (size_t)A.rows * A.w;
    const int ox = tx0 + col;
    float sum = 0.f;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int oy = ty0 + rg * 4 + q;
        if (oy >= vh || ox >= vw) continue;
        const float M1 = acc[0][q], M2 = acc[1][q];         // means of x - a0, y - b0 (a0, b0: values of x - cx, y - cy)
        const float s1 = acc[2][q] - M1 * M1, s2 = acc[3][q] - M2 * M2, s12 = acc[4][q] - M1 * M2;
        const float m1 = M1 + a0, m2 = M2 + b0;             // means of x - cx, y - cy
        const float mu1 = m1 + cx, mu2 = m2 + cy;
        const float A1 = 2.f * mu1 * mu2 + SS_C1, A2 = 2.f * s12 + SS_C2;
        const float B1 = mu1 * mu1 + mu2 * mu2 + SS_C1, B2 = s1 + s2 + SS_C2;
        const float l = A1 / B1, cs = A2 / B2;
        const float m = l * cs;
        sum += 1.f - m;     // (1 - map is what the loss averages: exact for map >= 0.5, and a sum without the ones that would hide it)
        if (GRAD) {
            const float ds1 = -m / B2, ds12 = 2.f * l / B2;
            const float d0 = 2.f * cs / (B1 * B1) * ((mu2 - mu1) * (mu2 * (mu1 + mu2) + SS_C1)) - 2.f * m1 * ds1 - m2 * ds12;
            const size_t o = (size_t)oy * A.w + ox;
            dm[o] = d0; dm[plane + o] = ds1; dm[2 * plane + o] = ds12;
        }
    }
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
    if ((tid & 63) == 0) s_red[tid >> 6] = sum;
    __syncthreads();
    if (tid == 0) *part = (s_red[0] + s_red[1]) + (s_red[2] + s_red[3]);
}

// HWC: grad_img interleaved [batch * grows, w, 3] -- the workgroup does the three channels in turn and each lane stores the
// three floats of its pixels; else planar [batch, 3, grows, w], one channel (blockIdx.y) per workgroup.  ACC: add into grad_img.
template <bool HWC, bool ACC>
__global__ __launch_bounds__(256) void k_ssim_grad(SsimArgs A)
{
    __shared__ float s_d[3][SS_P * SS_P];
    __shared__ float s_h[3][SS_P * SS_T];
    const int b = blockIdx.z, tid = threadIdx.x;
    const int h = A.hw[2 * b], w = A.hw[2 * b + 1], vh = h - 10, vw = w - 10;
    const int ty0 = (int)(blockIdx.x / (unsigned)A.gtx) * SS_T, tx0 = (int)(blockIdx.x % (unsigned)A.gtx) * SS_T;
    if (ty0 >= h || tx0 >= w) return;       // a tile of the padding: nothing is written there
    const float cb = -A.weight / (float)(3.0 * (double)vh * (double)vw * (double)A.batch);
    const size_t plane = (size_t)A.rows * A.w;
    const int col = tid & 31, rg = tid >> 5;
    const int px = tx0 + col;
    constexpr int NC = HWC ? 3 : 1;
    float out[NC][4];
#pragma unroll
    for (int k = 0; k < NC; ++k) {
        const int ch = HWC ? k : (int)blockIdx.y;
        const float *__restrict__ dm = A.dmap + ((size_t)b * 3 + ch) * 3 * plane;
        if (k > 0) __syncthreads();
        // patch (r, c) <- map (ty0 - 10 + r, tx0 - 10 + c), zero outside the valid map
        for (int i = tid; i < SS_P * SS_P; i += 256) {
            const int r = i / SS_P, c = i - r * SS_P;
            const int my = ty0 - 10 + r, mx = tx0 - 10 + c;
            const bool in = my >= 0 && my < vh && mx >= 0 && mx < vw;
            const size_t o = in ? (size_t)my * A.w + mx : 0;
            s_d[0][i] = in ? dm[o] : 0.f;
            s_d[1][i] = in ? dm[plane + o] : 0.f;
            s_d[2][i] = in ? dm[2 * plane + o] : 0.f;
        }
        __syncthreads();
        for (int r = rg; r < SS_P; r += 8) {
            float a0 = 0.f, a1 = 0.f, a2 = 0.f;
#pragma unroll
            for (int j = 0; j < 11; ++j) {
                a0 = fmaf(ss_g(j), s_d[0][r * SS_P + col + j], a0);
                a1 = fmaf(ss_g(j), s_d[1][r * SS_P + col + j], a1);
                a2 = fmaf(ss_g(j), s_d[2][r * SS_P + col + j], a2);
            }
            s_h[0][r * SS_T + col] = a0; s_h[1][r * SS_T + col] = a1; s_h[2][r * SS_T + col] = a2;
        }
        __syncthreads();
        float acc[3][4];
        ss_vertical<3>(s_h, col, rg, acc);
        const float *__restrict__ x = A.img + ((size_t)b * 3 + ch) * plane;
        const float *__restrict__ y = A.target + ((size_t)b * 3 + ch) * A.trows * A.w;
        const float cx = x[(size_t)(h / 2) * A.w + w / 2], cy = y[(size_t)(h / 2) * A.w + w / 2];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int py = ty0 + rg * 4 + q;
            out[k][q] = 0.f;
            if (py < h && px < w) {
                const float xv = x[(size_t)py * A.w + px] - cx, yv = y[(size_t)py * A.w + px] - cy;
                out[k][q] = cb * (acc[0][q] + 2.f * xv * acc[1][q] + yv * acc[2][q]);
            }
        }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int py = ty0 + rg * 4 + q;
        if (py >= h || px >= w) continue;       // the sample's own pixels only
        if (HWC) {
            float *__restrict__ g = A.grad + (((size_t)b * A.grows + py) * A.w + px) * 3;
#pragma unroll
            for (int k = 0; k < NC; ++k) g[k] = ACC ? g[k] + out[k][q] : out[k][q];
        } else {
            float *__restrict__ g = A.grad + (((size_t)b * 3 + blockIdx.y) * A.grows + py) * A.w + px;
            *g = ACC ? *g + out[0][q] : out[0][q];
        }
    }
}

// One workgroup: sample b is dealt to `wps` waves (16 / batch of them, at least one), each lane adds every (64 * wps)-th of
// the sample's 3 * tiles partials in double, a butterfly combines the lanes and the waves are added in order.
// L_b = weight * sum / (3 vh vw) (the partials are sums of 1 - map), L = (1 / B) sum_b L_b, formed in double and rounded once.
__global__ __launch_bounds__(1024) void k_ssim_reduce(SsimArgs A, int wps)
{
    __shared__ double s_sum[GSASR_MAX_BATCH * 16];
    __shared__ double s_lb[GSASR_MAX_BATCH];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int part = wv % wps, per_sample = 3 * A.ntiles;
    for (int b = wv / wps; b < A.batch; b += 16 / wps) {
        const float *__restrict__ src = A.part + (size_t)b * per_sample;
        double a = 0.0;
        for (int i = part * 64 + lane; i < per_sample; i += 64 * wps) a += (double)src[i];
        for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o);
        if (lane == 0) s_sum[b * wps + part] = a;
    }
    __syncthreads();
    if ((int)threadIdx.x < A.batch) {
        const int b = (int)threadIdx.x;
        double a = 0.0;
        for (int k = 0; k < wps; ++k) a += s_sum[b * wps + k];
        const double n = 3.0 * (double)(A.hw[2 * b] - 10) * (double)(A.hw[2 * b + 1] - 10);
        const double lb = (double)A.weight * (a / n);
        s_lb[b] = lb;
        A.loss[1 + b] = (float)lb;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double a = 0.0;
        for (int b = 0; b < A.batch; ++b) a += s_lb[b];
        A.loss[0] = (float)(a / (double)A.batch);
    }
}

// the geometry of a descriptor (everything gsasr_ssim_scratch_bytes depends on); fills hw[] with the samples' sizes
int ssim_geometry_check(const gsasr_ssim *s, unsigned short *hw)
{
    if (!s) return fail(GSASR_ERR_ARG, "null ssim descriptor");
    if (s->batch < 1 || s->batch > GSASR_MAX_BATCH) return fail(GSASR_ERR_ARG, "batch must be 1..GSASR_MAX_BATCH");
    if (s->rows < 11 || s->w < 11 || s->rows > 32767 || s->w > 32767) return fail(GSASR_ERR_ARG, "need 11 <= rows, w <= 32767 (the window has 11 taps)");
    if (s->target_rows < 0 || s->grad_rows < 0) return fail(GSASR_ERR_ARG, "negative target_rows or grad_rows");
    if (s->flags & ~(GSASR_SSIM_GRAD_HWC | GSASR_SSIM_ACCUMULATE)) return fail(GSASR_ERR_ARG, "unknown flags (GSASR_SSIM_GRAD_HWC, GSASR_SSIM_ACCUMULATE)");
    for (int b = 0; b < s->batch; ++b) {
        const int h = s->sample_hw ? s->sample_hw[2 * b] : s->rows, w = s->sample_hw ? s->sample_hw[2 * b + 1] : s->w;
        if (h < 11 || w < 11) return fail(GSASR_ERR_ARG, "a sample is smaller than the 11 x 11 window: no valid pixel");
        if (h > s->rows || w > s->w) return fail(GSASR_ERR_ARG, "a sample is larger than rows x w");
        if (s->target_rows > 0 && s->target_rows < h) return fail(GSASR_ERR_ARG, "target_rows is below a sample's height");
        if (s->grad_rows > 0 && s->grad_rows < h) return fail(GSASR_ERR_ARG, "grad_rows is below a sample's height");
        if (hw) { hw[2 * b] = (unsigned short)h; hw[2 * b + 1] = (unsigned short)w; }
    }
    return GSASR_OK;
}

inline int ss_tiles(int n) { return (n + SS_T - 1) / SS_T; }
inline size_t ss_part_bytes(const gsasr_ssim *s)
{
    return align_up((size_t)s->batch * 3 * (size_t)ss_tiles(s->w - 10) * (size_t)ss_tiles(s->rows - 10) * sizeof(float), 256);
}

}  // namespace

extern "C" {

size_t gsasr_ssim_scratch_bytes(const gsasr_ssim *s)
{
    if (ssim_geometry_check(s, nullptr)) return 0;
    // the partial sums, and -- when a gradient is asked for -- the three derivative maps of every channel
    return ss_part_bytes(s) + (s->grad_img ? (size_t)s->batch * 9 * (size_t)s->rows * (size_t)s->w * sizeof(float) : 0);
}

int gsasr_ssim_loss(const gsasr_ssim *s, void *stream)
{
    SsimArgs A;
    if (int rc = ssim_geometry_check(s, A.hw)) return rc;
    if (!s->img || !s->target || !s->loss || !s->scratch) return fail(GSASR_ERR_ARG, "null img, target, loss or scratch pointer");
    A.img = s->img; A.target = s->target; A.grad = s->grad_img; A.loss = s->loss;
    A.part = (float *)s->scratch;
    A.dmap = (float *)((char *)s->scratch + ss_part_bytes(s));
    A.batch = s->batch; A.rows = s->rows; A.w = s->w;
    A.trows = s->target_rows > 0 ? s->target_rows : s->rows;
    A.grows = s->grad_rows > 0 ? s->grad_rows : s->rows;
    A.ntx = ss_tiles(s->w - 10); A.ntiles = A.ntx * ss_tiles(s->rows - 10);
    A.gtx = ss_tiles(s->w);
    A.weight = s->weight;
    hipStream_t st = (hipStream_t)stream;
    const dim3 block(256), grid((unsigned)A.ntiles, 3, (unsigned)A.batch);
    if (A.grad) hipLaunchKernelGGL(k_ssim_stats<true>, grid, block, 0, st, A);
    else hipLaunchKernelGGL(k_ssim_stats<false>, grid, block, 0, st, A);
    HIP_TRY(hipGetLastError());
    if (A.grad) {
        const bool hwc = s->flags & GSASR_SSIM_GRAD_HWC, acc = s->flags & GSASR_SSIM_ACCUMULATE;
        const dim3 gg((unsigned)(A.gtx * ss_tiles(s->rows)), hwc ? 1 : 3, (unsigned)A.batch);
        if (hwc) { if (acc) hipLaunchKernelGGL((k_ssim_grad<true, true>), gg, block, 0, st, A);
                   else hipLaunchKernelGGL((k_ssim_grad<true, false>), gg, block, 0, st, A); }
        else { if (acc) hipLaunchKernelGGL((k_ssim_grad<false, true>), gg, block, 0, st, A);
               else hipLaunchKernelGGL((k_ssim_grad<false, false>), gg, block, 0, st, A); }
        HIP_TRY(hipGetLastError());
    }
    int wps = 1;
    while (wps * 2 * A.batch <= 16) wps *= 2;
    hipLaunchKernelGGL(k_ssim_reduce, dim3(1), dim3(1024), 0, st, A, wps);
    HIP_TRY(hipGetLastError());
    return GSASR_OK;
}

}  // extern "C"
