// splat_metrics.hip -- the validation metrics of an 8-bit picture against its 8-bit ground truth (GSASR's val.metrics:
// basicsr/metrics/psnr_ssim.py calculate_psnr / calculate_ssim, with crop_border and test_y_channel): gsasr_image_metrics
// (one translation unit of libgsasr_splat.so; include/gsasr_splat.h has the contract)
//
//   k_metric_stats<Y>  one workgroup per (32 x 32 tile of the CROPPED picture, channel, sample) -- in Y mode one channel.  The
//                      bytes under the tile's 42 x 42 patch are fetched once, as aligned dwords where a dword lies inside the
//                      row and as single bytes at the row's ends, into LDS; converted once to the values the metrics are
//                      defined on (the byte, or the reference's Y with its two roundings: exact in fp32 either way); the
//                      11-tap window over x, y, x^2, y^2, xy along the rows (into LDS), then along the columns (four map
//                      rows per lane, in registers); the tile's sum of the map and its sum of squared differences are the
//                      two partials.  The tiles cover the cropped picture, not the valid map: every pixel's squared difference
//                      is counted once, by the tile it lies in, and the map pixel (y, x) -- whose window starts at (y, x) --
//                      belongs to the same tile.  A tile of the last 10 rows or columns has pixels and no map.
//   k_metric_reduce    one workgroup per sample: its own tiles' partials added in double in an order that depends on the
//                      sample's extent alone (so a sample of a batch and the same picture alone give the same bits), then
//                      psnr = 10 log10(255^2 / mse) (+inf at mse = 0) and ssim = mean(map).
// Arithmetic: double.  Values reach 255^2 and s = g*(x^2) - mu^2 is compared with C2 = 58.5 to five decimals of the mean; in
// double the cancellation costs 1e-11 and no shift is needed.  The squared differences of RGB mode are integers: 32-bit within
// a workgroup (at most 1024 * 255^2 = 6.7e7), then doubles that hold integers below 2^53 exactly (32767^2 * 3 * 255^2 = 2.1e14).
// No float atomics, no memset: every scratch word that is read was written by this call, and two calls give the same bits.
#include "splat_common.h"

using namespace gsasr_detail;

namespace {

constexpr int MT_T = 32;                // tile side
constexpr int MT_P = MT_T + 10;         // ... and of the patch under an 11-tap window
constexpr int MT_RAW = 33;              // dwords that cover the 3 * 42 bytes of a patch row from any byte offset (3 + 126 + 3) / 4
constexpr double MT_C1 = (0.01 * 255) * (0.01 * 255), MT_C2 = (0.03 * 255) * (0.03 * 255);
constexpr unsigned MT_KNOWN = GSASR_METRIC_PSNR | GSASR_METRIC_SSIM | GSASR_METRIC_Y | GSASR_METRIC_BGR;

// g[i] = exp(-(i - 5)^2 / (2 * 1.5^2)) / sum, i = 0..10, by distance from the centre (cv2.getGaussianKernel(11, 1.5))
__device__ __forceinline__ constexpr double mt_g(int j)
{
    const int d = j < 5 ? 5 - j : j - 5;
    return d == 0 ? 0.26601172486179436 : d == 1 ? 0.2130055377112537 : d == 2 ? 0.10936068950970002
         : d == 3 ? 0.03600077212843083 : d == 4 ? 0.007598758135239185 : 0.00102838008447911;
}

struct MetricArgs {
    const unsigned char *img, *ref;
    size_t img_pitch, img_stride, ref_pitch, ref_stride;
    double *part;       // [batch][nch][ntiles][2]: the tile's sum of the map, its sum of squared differences
    double *out;        // [batch][2]
    int batch, cb, nch;
    int ntx, ntiles;    // tiles of the cropped canvas per row of tiles / in all
    unsigned flags;
    unsigned short hw[2 * GSASR_MAX_BATCH];     // (h_b, w_b), uncropped
};

__host__ __device__ inline int mt_tiles(int n) { return (n + MT_T - 1) / MT_T; }

// The bytes [xb0, xb0 + nbytes) of rows y0 .. y0 + nrows - 1 of a picture whose rows hold `rowbytes` bytes, `pitch` apart, into
// s_raw[row][MT_RAW] dwords: dword k of a row is the aligned dword at (address of the row's first wanted byte & ~3) + 4 k.  A
// dword that lies inside the row is one load; one that straddles either end of the row is put together from the bytes that
// belong to the row -- nothing outside a row's `rowbytes` bytes is read.
__device__ __forceinline__ void mt_stage_raw(const unsigned char *base, size_t pitch, int rowbytes, int y0, int nrows, int xb0, int nbytes,
                                             unsigned *s_raw, int tid)
{
    for (int i = tid; i < nrows * MT_RAW; i += 256) {
        const int r = i / MT_RAW, k = i - r * MT_RAW;
        const uintptr_t R0 = (uintptr_t)(base + (size_t)(y0 + r) * pitch), R1 = R0 + (uintptr_t)rowbytes;
        const uintptr_t p0 = R0 + (uintptr_t)xb0, p1 = p0 + (uintptr_t)nbytes;
        const uintptr_t a = (p0 & ~(uintptr_t)3) + 4u * (unsigned)k;
        unsigned v = 0u;
        if (a < p1) {
            if (a >= R0 && a + 4 <= R1) v = *(const unsigned *)a;
            else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (a + j >= R0 && a + j < R1) v |= (unsigned)*(const unsigned char *)(a + j) << (8 * j);
            }
        }
        s_raw[i] = v;
    }
}

// the reference's Y of one pixel (metric_util.py:32-45, color_util.py:38-68): float32(v) / 255f per channel, the weighted sum in
// double, one rounding to float32 after / 255.0 and one after * 255f
__device__ __forceinline__ float mt_y(unsigned r, unsigned g, unsigned b)
{
    const double xr = (double)__fdiv_rn((float)r, 255.f), xg = (double)__fdiv_rn((float)g, 255.f), xb = (double)__fdiv_rn((float)b, 255.f);
    const double y64 = __dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(24.966, xb), __dmul_rn(128.553, xg)), __dmul_rn(65.481, xr)), 16.0);
    return __fmul_rn((float)__ddiv_rn(y64, 255.0), 255.f);
}

template <bool Y>
__global__ __launch_bounds__(256) void k_metric_stats(MetricArgs A)
{
    __shared__ float s_x[MT_P * MT_P], s_y[MT_P * MT_P];
    __shared__ double s_h[5][MT_P * MT_T];      // (its first 2 * 42 * 33 dwords hold the raw bytes before the row pass)
    __shared__ double s_red[2][4];
    const int b = blockIdx.z, ch = blockIdx.y, tid = threadIdx.x;
    const int w = A.hw[2 * b + 1], hc = A.hw[2 * b] - 2 * A.cb, wc = w - 2 * A.cb;
    const int ty0 = (int)(blockIdx.x / (unsigned)A.ntx) * MT_T, tx0 = (int)(blockIdx.x % (unsigned)A.ntx) * MT_T;
    if (ty0 >= hc || tx0 >= wc) return;         // a tile of the canvas' padding (the whole workgroup): k_metric_reduce does not read it
    const int nrows = min(MT_P, hc - ty0), ncols = min(MT_P, wc - tx0);
    const unsigned char *pa = A.img + (size_t)b * A.img_stride, *pb = A.ref + (size_t)b * A.ref_stride;
    const int y0 = A.cb + ty0, xb0 = 3 * (A.cb + tx0);
    unsigned *s_rawa = (unsigned *)&s_h[0][0], *s_rawb = s_rawa + MT_P * MT_RAW;
    mt_stage_raw(pa, A.img_pitch, 3 * w, y0, nrows, xb0, 3 * ncols, s_rawa, tid);
    mt_stage_raw(pb, A.ref_pitch, 3 * w, y0, nrows, xb0, 3 * ncols, s_rawb, tid);
    __syncthreads();
    const bool bgr = A.flags & GSASR_METRIC_BGR;
    for (int i = tid; i < MT_P * MT_P; i += 256) {
        const int r = i / MT_P, c = i - r * MT_P;
        float va = 0.f, vb = 0.f;       // outside the cropped picture both are 0: no squared difference, and no map pixel reads them
        if (r < nrows && c < ncols) {
            const unsigned sa = (unsigned)(((uintptr_t)(pa + (size_t)(y0 + r) * A.img_pitch) + (uintptr_t)xb0) & 3u);
            const unsigned sb = (unsigned)(((uintptr_t)(pb + (size_t)(y0 + r) * A.ref_pitch) + (uintptr_t)xb0) & 3u);
            const unsigned char *qa = (const unsigned char *)(s_rawa + r * MT_RAW) + sa + 3 * c;
            const unsigned char *qb = (const unsigned char *)(s_rawb + r * MT_RAW) + sb + 3 * c;
            if (Y) {
                va = bgr ? mt_y(qa[2], qa[1], qa[0]) : mt_y(qa[0], qa[1], qa[2]);
                vb = bgr ? mt_y(qb[2], qb[1], qb[0]) : mt_y(qb[0], qb[1], qb[2]);
            } else {
                va = (float)qa[ch]; vb = (float)qb[ch];
            }
        }
        s_x[i] = va; s_y[i] = vb;
    }
    __syncthreads();
    const int col = tid & 31, rg = tid >> 5;
    // the squared differences of the tile's own 32 x 32 pixels (four rows per lane)
    double sse;
    if (Y) {
        sse = 0.0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const double d = (double)s_x[(rg * 4 + q) * MT_P + col] - (double)s_y[(rg * 4 + q) * MT_P + col];
            sse = fma(d, d, sse);
        }
        for (int o = 32; o > 0; o >>= 1) sse += __shfl_xor(sse, o);
    } else {
        unsigned e = 0u;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int d = (int)s_x[(rg * 4 + q) * MT_P + col] - (int)s_y[(rg * 4 + q) * MT_P + col];
            e += (unsigned)(d * d);
        }
        for (int o = 32; o > 0; o >>= 1) e += __shfl_xor(e, o);
        sse = (double)e;
    }
    double sum = 0.0;
    // (uniform in the workgroup: a tile of the last 10 rows or columns has no map pixel)
    if ((A.flags & GSASR_METRIC_SSIM) && ty0 < hc - 10 && tx0 < wc - 10) {
        for (int r = rg; r < MT_P; r += 8) {
            double m1 = 0.0, m2 = 0.0, xx = 0.0, yy = 0.0, xy = 0.0;
#pragma unroll
            for (int j = 0; j < 11; ++j) {
                const double a = (double)s_x[r * MT_P + col + j], c = (double)s_y[r * MT_P + col + j];
                const double ga = mt_g(j) * a, gc = mt_g(j) * c;
                m1 += ga; m2 += gc;
                xx = fma(ga, a, xx); yy = fma(gc, c, yy); xy = fma(ga, c, xy);
            }
            s_h[0][r * MT_T + col] = m1; s_h[1][r * MT_T + col] = m2;
            s_h[2][r * MT_T + col] = xx; s_h[3][r * MT_T + col] = yy; s_h[4][r * MT_T + col] = xy;
        }
        __syncthreads();
        double acc[5][4];
#pragma unroll
        for (int p = 0; p < 5; ++p)
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[p][q] = 0.0;
#pragma unroll
        for (int k = 0; k < 14; ++k)
#pragma unroll
            for (int p = 0; p < 5; ++p) {
                const double v = s_h[p][(rg * 4 + k) * MT_T + col];
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    if (k - q >= 0 && k - q < 11) acc[p][q] = fma(mt_g(k - q), v, acc[p][q]);
            }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (ty0 + rg * 4 + q >= hc - 10 || tx0 + col >= wc - 10) continue;
            // every product and sum rounded on its own: with equal pictures numerator and denominator are the same numbers
            const double mu1 = acc[0][q], mu2 = acc[1][q];
            const double m11 = __dmul_rn(mu1, mu1), m22 = __dmul_rn(mu2, mu2), m12 = __dmul_rn(mu1, mu2);
            const double s1 = __dsub_rn(acc[2][q], m11), s2 = __dsub_rn(acc[3][q], m22), s12 = __dsub_rn(acc[4][q], m12);
            const double num = __dmul_rn(__dadd_rn(__dmul_rn(2.0, m12), MT_C1), __dadd_rn(__dmul_rn(2.0, s12), MT_C2));
            const double den = __dmul_rn(__dadd_rn(__dadd_rn(m11, m22), MT_C1), __dadd_rn(__dadd_rn(s1, s2), MT_C2));
            sum += __ddiv_rn(num, den);
        }
        for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
    }
    if ((tid & 63) == 0) { s_red[0][tid >> 6] = sum; s_red[1][tid >> 6] = sse; }
    __syncthreads();
    if (tid == 0) {
        double *part = A.part + (((size_t)b * A.nch + ch) * A.ntiles + blockIdx.x) * 2;
        part[0] = (s_red[0][0] + s_red[0][1]) + (s_red[0][2] + s_red[0][3]);
        part[1] = (s_red[1][0] + s_red[1][1]) + (s_red[1][2] + s_red[1][3]);
    }
}

// One workgroup per sample.  Item i of the sample -- channel i / (its tiles), then its own tiles row by row -- goes to lane
// i mod 256; a butterfly combines the lanes and the four waves are added in order: the order is a function of the sample's
// cropped extent and of nothing else.
__global__ __launch_bounds__(256) void k_metric_reduce(MetricArgs A)
{
    __shared__ double s_red[2][4];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int hc = A.hw[2 * b] - 2 * A.cb, wc = A.hw[2 * b + 1] - 2 * A.cb;
    const int ntx = mt_tiles(wc), per = ntx * mt_tiles(hc), n = A.nch * per;
    double m = 0.0, e = 0.0;
    for (int i = tid; i < n; i += 256) {
        const int ch = i / per, t = i - ch * per, ty = t / ntx, tx = t - ty * ntx;
        const double *__restrict__ p = A.part + (((size_t)b * A.nch + ch) * A.ntiles + (size_t)ty * A.ntx + tx) * 2;
        m += p[0]; e += p[1];
    }
    for (int o = 32; o > 0; o >>= 1) { m += __shfl_xor(m, o); e += __shfl_xor(e, o); }
    if ((tid & 63) == 0) { s_red[0][tid >> 6] = m; s_red[1][tid >> 6] = e; }
    __syncthreads();
    if (tid == 0) {
        m = (s_red[0][0] + s_red[0][1]) + (s_red[0][2] + s_red[0][3]);
        e = (s_red[1][0] + s_red[1][1]) + (s_red[1][2] + s_red[1][3]);
        if (A.flags & GSASR_METRIC_PSNR) {
            const double mse = e / ((double)A.nch * (double)hc * (double)wc);
            A.out[2 * b] = mse == 0.0 ? (double)INFINITY : 10.0 * log10(255.0 * 255.0 / mse);
        }
        if (A.flags & GSASR_METRIC_SSIM) A.out[2 * b + 1] = m / ((double)A.nch * (double)(hc - 10) * (double)(wc - 10));
    }
}

// everything gsasr_metrics_scratch_bytes depends on (no pointer but sample_hw is looked at); fills hw[] with the samples' sizes
int metrics_geometry_check(const gsasr_metrics *m, unsigned short *hw)
{
    if (!m) return fail(GSASR_ERR_ARG, "null metrics descriptor");
    if (m->batch < 1 || m->batch > GSASR_MAX_BATCH) return fail(GSASR_ERR_ARG, "batch must be 1..GSASR_MAX_BATCH");
    if (m->h < 1 || m->w < 1 || m->h > 32767 || m->w > 32767) return fail(GSASR_ERR_ARG, "need 1 <= h, w <= 32767");
    if (m->flags & ~MT_KNOWN) return fail(GSASR_ERR_ARG, "unknown flags (GSASR_METRIC_PSNR, _SSIM, _Y, _BGR)");
    if (!(m->flags & (GSASR_METRIC_PSNR | GSASR_METRIC_SSIM))) return fail(GSASR_ERR_ARG, "no metric asked for (GSASR_METRIC_PSNR, GSASR_METRIC_SSIM)");
    if (m->crop_border < 0) return fail(GSASR_ERR_ARG, "negative crop_border");
    if (m->img_pitch < 3 * (size_t)m->w || m->ref_pitch < 3 * (size_t)m->w) return fail(GSASR_ERR_ARG, "a pitch is below 3 * w bytes");
    for (int b = 0; b < m->batch; ++b) {
        const int h = m->sample_hw ? m->sample_hw[2 * b] : m->h, w = m->sample_hw ? m->sample_hw[2 * b + 1] : m->w;
        if (h > m->h || w > m->w) return fail(GSASR_ERR_ARG, "a sample is larger than h x w");
        // (in 64 bits: crop_border is any int)
        const long long hc = (long long)h - 2 * (long long)m->crop_border, wc = (long long)w - 2 * (long long)m->crop_border;
        if (hc < 1 || wc < 1) return fail(GSASR_ERR_ARG, "crop_border leaves no pixel of a sample");
        if ((m->flags & GSASR_METRIC_SSIM) && (hc < 11 || wc < 11))
            return fail(GSASR_ERR_ARG, "a cropped sample is smaller than the 11 x 11 SSIM window: no valid pixel");
        if (hw) { hw[2 * b] = (unsigned short)h; hw[2 * b + 1] = (unsigned short)w; }
    }
    return GSASR_OK;
}

inline int mt_nch(const gsasr_metrics *m) { return (m->flags & GSASR_METRIC_Y) ? 1 : 3; }

}  // namespace

extern "C" {

size_t gsasr_metrics_scratch_bytes(const gsasr_metrics *m)
{
    if (metrics_geometry_check(m, nullptr)) return 0;
    const size_t tiles = (size_t)mt_tiles(m->w - 2 * m->crop_border) * (size_t)mt_tiles(m->h - 2 * m->crop_border);
    return align_up((size_t)m->batch * (size_t)mt_nch(m) * tiles * 2 * sizeof(double), 256);
}

int gsasr_image_metrics(const gsasr_metrics *m, void *stream)
{
    MetricArgs A;
    if (int rc = metrics_geometry_check(m, A.hw)) return rc;
    if (!m->img || !m->ref || !m->out || !m->scratch) return fail(GSASR_ERR_ARG, "null img, ref, out or scratch pointer");
    if ((uintptr_t)m->scratch & 7u) return fail(GSASR_ERR_ARG, "scratch must be 8-byte aligned");
    A.img = m->img; A.ref = m->ref;
    A.img_pitch = m->img_pitch; A.img_stride = m->img_stride; A.ref_pitch = m->ref_pitch; A.ref_stride = m->ref_stride;
    A.part = (double *)m->scratch; A.out = m->out;
    A.batch = m->batch; A.cb = m->crop_border; A.nch = mt_nch(m);
    A.ntx = mt_tiles(m->w - 2 * m->crop_border); A.ntiles = A.ntx * mt_tiles(m->h - 2 * m->crop_border);
    A.flags = m->flags;
    hipStream_t st = (hipStream_t)stream;
    const dim3 block(256), grid((unsigned)A.ntiles, (unsigned)A.nch, (unsigned)A.batch);
    if (m->flags & GSASR_METRIC_Y) hipLaunchKernelGGL(k_metric_stats<true>, grid, block, 0, st, A);
    else hipLaunchKernelGGL(k_metric_stats<false>, grid, block, 0, st, A);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_metric_reduce, dim3((unsigned)A.batch), block, 0, st, A);
    HIP_TRY(hipGetLastError());
    return GSASR_OK;
}

}  // extern "C"
