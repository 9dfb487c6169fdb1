/*
 * tests/c_abi/c_abi_metrics_check.c -- PSNR and SSIM of an 8-bit picture (gsasr_image_metrics) from plain C: no Python, no torch.
 *
 * A 45 x 77 picture and its ground truth in buffers with different pitches (neither a multiple of 4) and a base that is not
 * 4-byte aligned, crop_border 4, in RGB mode and on the Y channel of b, g, r bytes, against a double-precision host loop over
 * the formulas of include/gsasr_splat.h (the 11 x 11 window applied directly).  Bars: PSNR 1e-9 relative in RGB mode and
 * 5e-4 dB in Y mode, SSIM 5e-6.  Then the descriptor's argument errors.  Built and run by tests/test_metrics_gpu.py on the GPU box.
 */
#include <hip/hip_runtime_api.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "gsasr_splat.h"

#define CK(x)                                                                      \
    do {                                                                           \
        hipError_t e_ = (x);                                                       \
        if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 2; } \
    } while (0)
#define OK(x)                                                                      \
    do {                                                                           \
        int rc_ = (x);                                                             \
        if (rc_ != 0) { fprintf(stderr, "%s -> %d: %s\n", #x, rc_, gsasr_last_error()); return 3; } \
    } while (0)

enum { H = 45, W = 77, CB = 4, HC = H - 2 * CB, WC = W - 2 * CB, PA = 3 * W + 7, PB = 3 * W + 2, OFF = 5 };

static unsigned lcg_state = 12345u;
static unsigned lcg(void) { lcg_state = lcg_state * 1664525u + 1013904223u; return lcg_state >> 8; }

/* the value the metrics are defined on: channel k of the pixel, or (y) the reference's Y of its b, g, r bytes */
static double value(const unsigned char *px, int k, int y)
{
    if (!y) return (double)px[k];
    const float xb = (float)px[0] / 255.0f, xg = (float)px[1] / 255.0f, xr = (float)px[2] / 255.0f;
    volatile double t = 24.966 * (double)xb;
    volatile double u = 128.553 * (double)xg;
    volatile double v = 65.481 * (double)xr;
    const double y64 = ((t + u) + v) + 16.0;
    const float y32 = (float)(y64 / 255.0);
    volatile float out = y32 * 255.0f;
    return (double)out;
}

static void host_metrics(const unsigned char *a, const unsigned char *b, int y, double *psnr, double *ssim)
{
    const int nch = y ? 1 : 3;
    const double c1 = (0.01 * 255) * (0.01 * 255), c2 = (0.03 * 255) * (0.03 * 255);
    double g[11], gs = 0.0, sse = 0.0, map = 0.0;
    for (int i = 0; i < 11; ++i) { g[i] = exp(-(double)((i - 5) * (i - 5)) / (2.0 * 1.5 * 1.5)); gs += g[i]; }
    for (int i = 0; i < 11; ++i) g[i] /= gs;
    static double va[HC][WC], vb[HC][WC];
    for (int k = 0; k < nch; ++k) {
        for (int r = 0; r < HC; ++r)
            for (int c = 0; c < WC; ++c) {
                va[r][c] = value(a + (size_t)(CB + r) * PA + 3 * (CB + c), k, y);
                vb[r][c] = value(b + (size_t)(CB + r) * PB + 3 * (CB + c), k, y);
                sse += (va[r][c] - vb[r][c]) * (va[r][c] - vb[r][c]);
            }
        for (int r = 0; r + 10 < HC; ++r)
            for (int c = 0; c + 10 < WC; ++c) {
                double m1 = 0, m2 = 0, xx = 0, yy = 0, xy = 0;
                for (int i = 0; i < 11; ++i)
                    for (int j = 0; j < 11; ++j) {
                        const double wgt = g[i] * g[j], p = va[r + i][c + j], q = vb[r + i][c + j];
                        m1 += wgt * p; m2 += wgt * q; xx += wgt * p * p; yy += wgt * q * q; xy += wgt * p * q;
                    }
                const double s1 = xx - m1 * m1, s2 = yy - m2 * m2, s12 = xy - m1 * m2;
                map += ((2 * m1 * m2 + c1) * (2 * s12 + c2)) / ((m1 * m1 + m2 * m2 + c1) * (s1 + s2 + c2));
            }
    }
    const double mse = sse / ((double)nch * HC * WC);
    *psnr = mse == 0.0 ? INFINITY : 10.0 * log10(255.0 * 255.0 / mse);
    *ssim = map / ((double)nch * (HC - 10) * (WC - 10));
}

int main(void)
{
    const size_t na = OFF + (size_t)H * PA, nb = OFF + (size_t)H * PB;
    unsigned char *a = malloc(na), *b = malloc(nb);
    memset(a, 255, na); memset(b, 0, nb);
    for (int r = 0; r < H; ++r)
        for (int c = 0; c < 3 * W; ++c) {
            const int base = 128 + (int)(90.0 * sin(0.09 * (c / 3) + 0.13 * r + (c % 3))) + (int)(lcg() % 21u) - 10;
            const int noisy = base + (int)(lcg() % 9u) - 4;
            b[OFF + (size_t)r * PB + c] = (unsigned char)(base < 0 ? 0 : base > 255 ? 255 : base);
            a[OFF + (size_t)r * PA + c] = (unsigned char)(noisy < 0 ? 0 : noisy > 255 ? 255 : noisy);
        }
    unsigned char *d_a, *d_b;
    double *d_out;
    CK(hipMalloc((void **)&d_a, na)); CK(hipMalloc((void **)&d_b, nb)); CK(hipMalloc((void **)&d_out, 2 * sizeof(double)));
    CK(hipMemcpy(d_a, a, na, hipMemcpyHostToDevice)); CK(hipMemcpy(d_b, b, nb, hipMemcpyHostToDevice));
    hipStream_t st;
    CK(hipStreamCreate(&st));
    int bad = 0;
    gsasr_metrics m;
    memset(&m, 0, sizeof m);
    m.batch = 1; m.h = H; m.w = W;
    m.img = d_a + OFF; m.img_pitch = PA; m.img_stride = 0;
    m.ref = d_b + OFF; m.ref_pitch = PB; m.ref_stride = 0;
    m.crop_border = CB; m.out = d_out;
    for (int y = 0; y < 2; ++y) {
        m.flags = GSASR_METRIC_PSNR | GSASR_METRIC_SSIM | (y ? GSASR_METRIC_Y | GSASR_METRIC_BGR : 0u);
        const size_t bytes = gsasr_metrics_scratch_bytes(&m);
        const size_t least = (size_t)(y ? 1 : 3) * ((HC + 31) / 32) * ((WC + 31) / 32) * 2 * sizeof(double);
        if (bytes < least || bytes % 8) { printf("scratch bytes %zu (at least %zu expected)\n", bytes, least); bad = 1; }
        void *scratch;
        CK(hipMalloc(&scratch, bytes ? bytes : 8));
        m.scratch = scratch;
        double out[2] = {-1.0, -1.0}, psnr, ssim;
        OK(gsasr_image_metrics(&m, st));
        CK(hipStreamSynchronize(st));
        CK(hipMemcpy(out, d_out, sizeof out, hipMemcpyDeviceToHost));
        host_metrics(a + OFF, b + OFF, y, &psnr, &ssim);
        const double ep = fabs(out[0] - psnr), es = fabs(out[1] - ssim);
        printf("%s: psnr %.9f dB (host %.9f, error %.3e), ssim %.9f (host %.9f, error %.3e)\n", y ? "Y" : "RGB", out[0], psnr, ep, out[1], ssim, es);
        if (!(ep <= (y ? 5e-4 : 1e-9 * psnr)) || !(es <= 5e-6) || !(psnr > 20 && psnr < 48.13)) bad = 1;     /* (48.13 dB: an rms error of one level, which the Y bar assumes) */
        /* one metric alone leaves the other slot as it is */
        const double sentinel[2] = {-7.5, -7.5};
        CK(hipMemcpy(d_out, sentinel, sizeof sentinel, hipMemcpyHostToDevice));
        m.flags &= ~GSASR_METRIC_SSIM;
        OK(gsasr_image_metrics(&m, st));
        CK(hipStreamSynchronize(st));
        double one[2];
        CK(hipMemcpy(one, d_out, sizeof one, hipMemcpyDeviceToHost));
        if (one[0] != out[0] || one[1] != -7.5) { printf("PSNR alone: %g %g\n", one[0], one[1]); bad = 1; }
        CK(hipFree(scratch));
    }
    /* argument errors: status + message, nothing enqueued */
    m.flags = GSASR_METRIC_PSNR | GSASR_METRIC_SSIM;
    gsasr_metrics e = m;
    e.img_pitch = 3 * W - 1;
    if (gsasr_image_metrics(&e, st) != GSASR_ERR_ARG || gsasr_metrics_scratch_bytes(&e) != 0) { printf("short pitch accepted\n"); bad = 1; }
    e = m; e.flags = GSASR_METRIC_Y;
    if (gsasr_image_metrics(&e, st) != GSASR_ERR_ARG) { printf("no metric flag accepted\n"); bad = 1; }
    e = m; e.crop_border = 18;      /* 9 rows left */
    if (gsasr_image_metrics(&e, st) != GSASR_ERR_ARG) { printf("a 9-row region accepted for SSIM\n"); bad = 1; }
    e = m; e.out = NULL;
    if (gsasr_image_metrics(&e, st) != GSASR_ERR_ARG) { printf("null out accepted\n"); bad = 1; }
    if (gsasr_image_metrics(NULL, st) != GSASR_ERR_ARG || gsasr_metrics_scratch_bytes(NULL) != 0) { printf("null descriptor accepted\n"); bad = 1; }
    if (!strlen(gsasr_last_error())) { printf("no error message\n"); bad = 1; }
    if (gsasr_abi_version() != 7) { printf("ABI version changed\n"); bad = 1; }
    printf("%s\n", bad ? "C-ABI METRICS CHECK FAILED" : "C-ABI METRICS CHECK OK");
    return bad;
}
